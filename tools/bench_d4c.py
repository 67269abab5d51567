"""D4C aperiodicity (crk_wana_d4c: low cut, Love Train, general body, table / coding) on one MI355X: prints one JSON line
and writes it to profiles/d4c_bench_line.json.

Shape: a batch of 64 utterances x 500 frames at shiftms 5, fs 22050 and 24000 (2 and 3 coded bands).  Inputs are seeded
(harmonic signal over a noise floor, F0 around 140 Hz with 20 % unvoiced frames; every voiced frame passes the Love
Train).  Reported per rate for ``codeap_batch`` and ``d4c_batch``, both with the low cut: ms per call over --reps timed
calls after --warmup (HIP events around each call: median, min, max), frames / s, and next to it the CPU restatement
tests/d4c_ref.py (numpy, float64, one thread of this host) on --cpu-utts of the utterances, per utterance.  There is no
earlier implementation to compare with.  Per-kernel shares come from a `rocprofv3 --kernel-trace --stats` run of this
script's own (a child process, --profile-child; its summary is copied to profiles/d4c_kernel_stats.csv).  --no-profile
skips that run, --cpu-utts 0 the restatement, --out-dir names another directory than profiles/.
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

SHIFTMS = 5.0


def inputs(utts, frames, fs):
    rng = np.random.default_rng(0)
    n = int(frames * SHIFTMS * fs / 1000)
    t = np.arange(n) / fs
    waves, f0s = [], []
    for _ in range(utts):
        y = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * 140.0 * h * t + rng.uniform(0, 6.28)) for h in range(1, 9))
        waves.append(y + 0.02 * rng.standard_normal(n))
        f = 140.0 + rng.uniform(-20, 20, frames)
        f[rng.uniform(size=frames) < 0.2] = 0.0
        f0s.append(f)
    return waves, f0s


def kernel_shares(stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    return {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                            "share": round(float(r["Percentage"]) / 100.0, 4)}
            for r in rows if "d4c_" in r["Name"] or "wana_" in r["Name"]}


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-utts", type=int, default=1)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--profile-child", action="store_true", help="the run under rocprofv3: calls only, no output")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_d4c needs the MI355X"
    from crank_amd.world import WorldAnalyzer
    from tests import d4c_ref as D

    res = {"metric": "world_d4c", "utts": args.utts, "frames": args.frames, "shiftms": SHIFTMS, "low_cut": 70,
           "reps": args.reps, "rates": {}}
    for fs in (22050, 24000):
        waves, f0s = inputs(args.utts, args.frames, fs)
        an = WorldAnalyzer(fs, 1024, SHIFTMS)
        dw = [torch.as_tensor(w, device="cuda") for w in waves]
        df = [torch.as_tensor(f, device="cuda") for f in f0s]
        calls = {"codeap_batch": lambda: an.codeap_batch(dw, df, low_cut=70), "d4c_batch": lambda: an.d4c_batch(dw, df, low_cut=70)}
        r = {}
        for name, fn in calls.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            if args.profile_child:
                continue
            ms, out = timed(fn, args.reps)
            med = float(np.median(ms))
            r[name] = {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                       "frames_per_s": round(args.utts * args.frames / med * 1e3),
                       "finite": bool(all(torch.isfinite(o).all() for o in out))}
            if name == "codeap_batch":
                caps = out
        if args.profile_child:
            continue
        if args.cpu_utts > 0:
            from tests import world_analysis_ref as A

            k = args.cpu_utts
            # the randn table is made once per process, outside the timing: what the longest of the utterances can draw
            D.noise(max(D.general_offsets(sh, f != 0)[1] for f in f0s[:k] for sh in [D.frame_shapes(f, fs, SHIFTMS)]))
            t0 = time.perf_counter()
            ref = [D.codeap(A.low_cut_filter(np.array(waves[i], dtype=np.float32), fs, 70), f0s[i], fs, SHIFTMS) for i in range(k)]
            cpu_s = time.perf_counter() - t0
            r["cpu_restatement"] = {"utts": k, "s_per_utt": round(cpu_s / k, 3),
                                    "max_abs_cap_diff_db": max(float(np.abs(caps[i].cpu().numpy() - ref[i]).max()) for i in range(k))}
        res["rates"][str(fs)] = r
    if args.profile_child:
        return
    os.makedirs(args.out_dir, exist_ok=True)
    if not args.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="d4c_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", "--utts", str(args.utts), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode == 0 and found:
            out = os.path.join(args.out_dir, "d4c_kernel_stats.csv")
            shutil.copyfile(found[0], out)
            res["kernels"] = kernel_shares(out)
            res["kernel_stats"] = "profiles/d4c_kernel_stats.csv (3 warm-up calls of codeap_batch and of d4c_batch per rate)"
        else:
            res["kernels"] = f"rocprofv3 run failed (exit {p.returncode})"
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    with open(os.path.join(args.out_dir, "d4c_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
