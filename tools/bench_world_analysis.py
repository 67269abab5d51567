"""WORLD spectral analysis (crk_wana_mcep: low cut, CheapTrick, mel-cepstrum) on one MI355X: prints one JSON line and
writes it to profiles/world_analysis_bench_line.json.

Shape: a batch of 64 utterances x 500 frames at fs 22050, 35 mel-cepstral coefficients (alpha 0.455), at shiftms 5 and
10.  Inputs are seeded (harmonic signal over a noise floor, F0 around 140 Hz with 20 % unvoiced frames).  Reported per
shift: ms per call over --reps timed calls after --warmup (HIP events around each call: median, min, max), frames / s,
and as the baseline the CPU restatement tests/world_analysis_ref.py (numpy, float64, one thread of this host) on
--cpu-utts of the utterances, scaled per utterance.  Per-kernel shares come from a `rocprofv3 --kernel-trace --stats` run
of this script's own (a child process, --profile-child; its summary is copied to
profiles/world_analysis_kernel_stats.csv).  --no-profile skips that run, --cpu-utts 0 the baseline.
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

FS, DIM, ALPHA = 22050, 34, 0.455


def inputs(utts, frames, shiftms):
    rng = np.random.default_rng(0)
    n = int(frames * shiftms * FS / 1000)
    t = np.arange(n) / FS
    waves, f0s = [], []
    for _ in range(utts):
        y = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * 140.0 * h * t + rng.uniform(0, 6.28)) for h in range(1, 9))
        waves.append(y + 0.1 * rng.standard_normal(n))
        f = 140.0 + rng.uniform(-20, 20, frames)
        f[rng.uniform(size=frames) < 0.2] = 0.0
        f0s.append(f)
    return waves, f0s


def kernel_shares(stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    return {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                            "share": round(float(r["Percentage"]) / 100.0, 4)}
            for r in rows if "wana_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-utts", type=int, default=1)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true", help="the run under rocprofv3: calls only, no output")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_world_analysis needs the MI355X"
    from crank_amd.world import WorldAnalyzer
    from tests import world_analysis_ref as A

    res = {"metric": "world_analysis_mcep", "utts": args.utts, "frames": args.frames, "fs": FS, "order1": DIM + 1,
           "alpha": ALPHA, "low_cut": 70, "reps": args.reps, "shifts": {}}
    for shiftms in (5.0, 10.0):
        waves, f0s = inputs(args.utts, args.frames, shiftms)
        an = WorldAnalyzer(FS, 1024, shiftms)
        dw = [torch.as_tensor(w, device="cuda") for w in waves]
        df = [torch.as_tensor(f, device="cuda") for f in f0s]
        for _ in range(args.warmup):
            mcs = an.mcep_batch(dw, df, DIM, ALPHA, low_cut=70)
        torch.cuda.synchronize()
        if args.profile_child:
            for _ in range(5):
                an.mcep_batch(dw, df, DIM, ALPHA, low_cut=70)
            torch.cuda.synchronize()
            continue
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            mcs = an.mcep_batch(dw, df, DIM, ALPHA, low_cut=70)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        F = args.utts * args.frames
        r = {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
             "frames_per_s": round(F / med * 1e3), "finite": bool(all(torch.isfinite(m).all() for m in mcs))}
        if args.cpu_utts > 0:
            k = args.cpu_utts
            A.noise(A.n_draws(f0s[0], FS, shiftms))  # the randn table is made once per process, outside the timing
            t0 = time.perf_counter()
            ref = [A.analyze_mcep(waves[i], f0s[i], FS, 1024, shiftms, DIM, ALPHA) for i in range(k)]
            cpu_s = time.perf_counter() - t0
            err = max(float(np.abs(mcs[i].cpu().numpy() - ref[i]).max()) for i in range(k))
            r.update({"cpu_restatement_utts": k, "cpu_restatement_s_per_utt": round(cpu_s / k, 3),
                      "cpu_restatement_s_batch_estimate": round(cpu_s / k * args.utts, 1),
                      "speedup_vs_cpu_restatement": round(cpu_s / k * args.utts / (med / 1e3)),
                      "max_abs_mcep_diff_vs_cpu_restatement": err})
        res["shifts"][f"{shiftms:g}"] = r
    if args.profile_child:
        return
    if not args.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="wana_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", "--utts", str(args.utts), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode == 0 and found:
            out = os.path.join(ROOT, "profiles", "world_analysis_kernel_stats.csv")
            shutil.copyfile(found[0], out)
            res["kernels"] = kernel_shares(out)
            res["kernel_stats"] = "profiles/world_analysis_kernel_stats.csv (3 warm-up and 5 further calls per shift, both shifts)"
        else:
            res["kernels"] = f"rocprofv3 run failed (exit {p.returncode})"
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "world_analysis_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
