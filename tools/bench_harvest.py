"""Harvest F0 estimation (crank_amd.world.HarvestF0, crk_f0_harvest) on one MI355X: prints one JSON line and writes it to
profiles/harvest_bench_line.json.

Shape: 64 utterances x 5 s at fs 22050, search range 40 - 700 Hz, shiftms 5 (171 channels, decimation by 3).  Inputs are
seeded: eight harmonics of a slowly moving F0 with unvoiced (noise-only) stretches.  Reported: ms per ``harvest_batch`` call
over --reps timed calls after --warmup (HIP events around each call: median, min, max; the call includes the host-side
layout tables and their upload), utterance-seconds per second, and as the baseline the CPU restatement
tests/harvest_ref.py (numpy, float64, one thread of this host) on one utterance.  Per-kernel shares come from a
`rocprofv3 --kernel-trace --stats` run of this script's own (a child process, --profile-child; its summary is copied to
profiles/harvest_kernel_stats.csv).  --no-profile skips that run, --cpu-utts 0 the baseline.
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

FS, SHIFTMS, MINF0, MAXF0 = 22050, 5, 40, 700


def inputs(utts, seconds):
    rng = np.random.default_rng(0)
    n = int(seconds * FS)
    t = np.arange(n) / FS
    out = []
    for _ in range(utts):
        f = rng.uniform(90, 260) * (1.0 + 0.15 * np.sin(2 * np.pi * rng.uniform(0.3, 1.5) * t + rng.uniform(0, 6.28)))
        ph = 2 * np.pi * np.cumsum(f) / FS
        y = sum(rng.uniform(0.05, 0.3) * np.sin(h * ph + rng.uniform(0, 6.28)) for h in range(1, 9))
        voiced = np.sin(2 * np.pi * rng.uniform(0.4, 0.9) * t + rng.uniform(0, 6.28)) > -0.5
        out.append(y * voiced + 1e-3 * rng.standard_normal(n))
    return out


def kernel_shares(stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    return {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                            "share": round(float(r["Percentage"]) / 100.0, 4)}
            for r in rows if "f0_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-utts", type=int, default=1)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true", help="the run under rocprofv3: calls only, no output")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_harvest needs the MI355X"
    from crank_amd.world import HarvestF0
    from tests import harvest_ref as R

    waves = inputs(args.utts, args.seconds)
    dev = [torch.as_tensor(w, device="cuda") for w in waves]
    lo, hi = [MINF0] * args.utts, [MAXF0] * args.utts
    hf = HarvestF0(FS, SHIFTMS, "cuda")
    run = lambda: hf.harvest_batch(dev, lo, hi)  # noqa: E731
    for _ in range(args.warmup):
        f0s = run()
    torch.cuda.synchronize()
    if args.profile_child:
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        return
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f0s = run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    L = hf._layout([len(w) for w in waves], lo, hi)
    res = {"metric": "harvest_f0", "utts": args.utts, "seconds_per_utt": args.seconds, "fs": FS, "shiftms": SHIFTMS,
           "minf0": MINF0, "maxf0": MAXF0, "channels": int(L["C"] // args.utts), "decimation": hf.r, "reps": args.reps,
           "warmup": args.warmup, "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
           "utterance_seconds_per_s": round(args.utts * args.seconds / med * 1e3, 1),
           "voiced_share": round(float(np.mean([float((f > 0).double().mean()) for f in f0s])), 3),
           "workspace_bytes": int(hf._ws.numel()), "event_bytes": int(L["E"]) * 8,
           "finite": bool(all(torch.isfinite(f).all() for f in f0s))}
    if args.cpu_utts > 0:
        k = args.cpu_utts
        t0 = time.perf_counter()
        ref = [R.harvest(waves[i], FS, MINF0, MAXF0, SHIFTMS) for i in range(k)]
        cpu_s = time.perf_counter() - t0
        got = [f0s[i].cpu().numpy() for i in range(k)]
        both = [(g != 0) & (r != 0) for g, r in zip(got, ref)]
        res.update({"cpu_restatement_utts": k, "cpu_restatement_s_per_utt": round(cpu_s / k, 2),
                    "cpu_restatement_s_batch_estimate": round(cpu_s / k * args.utts, 1),
                    "speedup_vs_cpu_restatement": round(cpu_s / k * args.utts / (med / 1e3)),
                    "voicing_differs_frames": int(sum(np.sum((g != 0) != (r != 0)) for g, r in zip(got, ref))),
                    "max_rel_f0_vs_cpu_restatement": float(max(np.max(np.abs(g[m] / r[m] - 1.0)) for g, r, m in
                                                               zip(got, ref, both) if m.any()))})
    if not args.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="f0_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", "--utts", str(args.utts), "--seconds", str(args.seconds)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode == 0 and found:
            out = os.path.join(ROOT, "profiles", "harvest_kernel_stats.csv")
            shutil.copyfile(found[0], out)
            res["kernels"] = kernel_shares(out)
            res["kernel_stats"] = "profiles/harvest_kernel_stats.csv (3 warm-up and 2 further calls)"
        else:
            res["kernels"] = f"rocprofv3 run failed (exit {p.returncode})"
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "harvest_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
