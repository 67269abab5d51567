"""Griffin-Lim waveform synthesis (crank_amd.griffin_lim, crk_gl_run) on one MI355X: prints one JSON line and writes it to
profiles/griffin_lim_bench_line.json.

Shape: a batch of 64 utterances x 500 frames of 80-mel log-mels at fs 22050, hop 128, window 1024, 100 iterations.  Inputs
are seeded (smooth random log-mels).  Reported: ms per call over --reps timed calls after --warmup (HIP events around each
call: median, min, max) of the iteration alone (``griffin_lim_batch`` with the spectra and the initial phases already on the
device), of the mel inversion, and of ``mlfb2wav_batch`` end to end, which also draws the initial phases on the host
(numpy RandomState per utterance, exp, upload); frames / s; and as the baseline the CPU restatement tests/griffin_lim_ref.py
(numpy, float64, one thread of this host) on --cpu-utts of the utterances, scaled per utterance.  Per-kernel shares come from
a `rocprofv3 --kernel-trace --stats` run of this script's own (a child process, --profile-child; its summary is copied to
profiles/griffin_lim_kernel_stats.csv).  --no-profile skips that run, --cpu-utts 0 the baseline.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, HOP, WIN, N_MELS, FMIN, FMAX = 22050, 128, 1024, 80, 80, 7600


def inputs(utts, frames):
    rng = np.random.default_rng(0)
    out = []
    for _ in range(utts):
        a = np.cumsum(np.cumsum(rng.standard_normal((frames + 8, N_MELS + 8)), 0), 1)
        a = (a[8:, 8:] - a[:-8, 8:] - a[8:, :-8] + a[:-8, :-8]) / 64.0
        out.append(-2.0 + 0.8 * a)
    return out


def kernel_shares(stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    return {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                            "share": round(float(r["Percentage"]) / 100.0, 4)}
            for r in rows if "gl_" in r["Name"]}


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-utts", type=int, default=1)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true", help="the run under rocprofv3: calls only, no output")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_griffin_lim needs the MI355X"
    from crank_amd.griffin_lim import GriffinLim
    from tests import griffin_lim_ref as R

    mlfbs = inputs(args.utts, args.frames)
    gl = GriffinLim(FS, N_MELS, 1024, WIN, HOP, FMIN, FMAX)
    dm = [torch.as_tensor(m, device="cuda") for m in mlfbs]
    lens = [args.frames] * args.utts
    S = gl.linear_spectrum_batch(dm)
    ang = gl.initial_angles(lens, 0)
    run = lambda: gl.griffin_lim_batch(S, args.iters, angles=ang)  # noqa: E731
    for _ in range(args.warmup):
        ys = run()
    torch.cuda.synchronize()
    if args.profile_child:
        for _ in range(2):
            gl.linear_spectrum_batch(dm)
            run()
        torch.cuda.synchronize()
        return
    F = args.utts * args.frames
    ys, t_iter = timed(run, args.reps)
    _, t_lin = timed(lambda: gl.linear_spectrum_batch(dm), args.reps)
    t0 = time.perf_counter()
    gl.initial_angles(lens, 0)
    torch.cuda.synchronize()
    host_phase_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    e2e = gl.mlfb2wav_batch(dm, args.iters, seed=0)
    torch.cuda.synchronize()
    e2e_s = time.perf_counter() - t0
    res = {"metric": "griffin_lim", "utts": args.utts, "frames": args.frames, "fs": FS, "hop": HOP, "win_length": WIN,
           "n_mels": N_MELS, "n_iters": args.iters, "reps": args.reps, "launches_per_call": args.iters + 2,
           "iteration": dict(t_iter, frames_per_s=round(F / t_iter["ms_median"] * 1e3),
                             us_per_iteration=round(t_iter["ms_median"] * 1e3 / max(args.iters, 1), 1)),
           "linear_spectrum": t_lin, "host_initial_phases_s": round(host_phase_s, 3),
           "mlfb2wav_batch_end_to_end_s": round(e2e_s, 3),
           "end_to_end_equals_iteration_bits": bool(all(torch.equal(a, b) for a, b in zip(ys, e2e))),
           "workspace_bytes": gl.workspace_bytes(args.utts, F, F - args.utts),
           "finite": bool(all(torch.isfinite(y).all() for y in ys))}
    if args.cpu_utts > 0:
        k = args.cpu_utts
        pinv = gl.pinv_basis()
        t0 = time.perf_counter()
        ref = [R.mlfb2wav(mlfbs[i], pinv, HOP, WIN, args.iters, i) for i in range(k)]
        cpu_s = time.perf_counter() - t0
        err = max(R.rel_l2(ys[i].cpu().numpy(), ref[i]) for i in range(k))
        res.update({"cpu_restatement_utts": k, "cpu_restatement_s_per_utt": round(cpu_s / k, 3),
                    "cpu_restatement_s_batch_estimate": round(cpu_s / k * args.utts, 1),
                    "speedup_vs_cpu_restatement": round(cpu_s / k * args.utts / (t_iter["ms_median"] / 1e3)),
                    "speedup_end_to_end_vs_cpu_restatement": round(cpu_s / k * args.utts / e2e_s),
                    "max_rel_l2_vs_cpu_restatement": err})
    if not args.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="gl_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", "--utts", str(args.utts), "--frames", str(args.frames),
               "--iters", str(args.iters)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode == 0 and found:
            out = os.path.join(ROOT, "profiles", "griffin_lim_kernel_stats.csv")
            shutil.copyfile(found[0], out)
            res["kernels"] = kernel_shares(out)
            res["kernel_stats"] = "profiles/griffin_lim_kernel_stats.csv (3 warm-up and 2 further calls, one mel inversion each)"
        else:
            res["kernels"] = f"rocprofv3 run failed (exit {p.returncode})"
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "griffin_lim_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
