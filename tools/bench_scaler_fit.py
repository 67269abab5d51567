"""Scaler fitting (crank_amd.bin.extract_statistics.fit_scalers; crk_scaler_moments, crk_scaler_merge) on one MI355X:
prints one JSON line and writes it to profiles/scaler_fit_bench_line.json.

Shape: a VCC2020-sized synthetic corpus, 14 speakers x 67 utterances x about 500 frames (seeded, 400 - 600), ``mlfb``
80-dim plus ``lcf0``, held in a FeatureStore on the device.  Reported: ms per ``fit_scalers`` call over --reps timed calls
after --warmup (wall clock around a synchronised call: it includes packing, four launches, the status check and the
download), and sklearn's ``partial_fit`` loop over the same utterances on this host when sklearn imports (the reference's
stage 2 without its HDF5 reads).  Per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script's
own (a child process, --profile-child; its summary is copied to profiles/scaler_fit_kernel_stats.csv): the moments
kernel against its byte floor (the corpus read twice from HBM, or once if the second pass hits cache, at the 6.3 TB/s a
float4 copy reaches), the merge kernel as latency per utterance of its sequential walk.  There is no target time: the
parent commit has no stage 2.  --no-profile skips the profiled run, --no-sklearn the baseline.
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

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy); the spec is 8e12
MLFB_DIM = 80


def corpus(speakers, utts, frames):
    """(host {file: {ext: ndarray}}, scp) of the synthetic corpus, in file order speaker by speaker."""
    rng = np.random.default_rng(0)
    data, feats, spk2utt = {}, {}, {}
    mu, sd = rng.uniform(-4.0, 0.0, MLFB_DIM), rng.uniform(0.3, 1.5, MLFB_DIM)
    for s in range(speakers):
        spk = f"SPK{s:02d}"
        spk2utt[spk] = []
        for u in range(utts):
            n = int(rng.integers(int(0.8 * frames), int(1.2 * frames) + 1))
            f = f"/feats/train/{spk}/E{u:04d}.h5"
            uid = f"{spk}_E{u:04d}"
            feats[uid] = f
            spk2utt[spk].append(uid)
            data[f] = {"mlfb": (rng.standard_normal((n, MLFB_DIM)) * sd + mu).astype(np.float32),
                       "lcf0": (rng.uniform(4.5, 5.5) + 0.3 * rng.standard_normal(n)).astype(np.float32)}
    return data, {"feats": feats, "spkrs": list(spk2utt), "spk2utt": spk2utt}


def kernel_times(stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    return {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                            "min_us": round(float(r.get("MinNs", "nan")) / 1e3, 2)}
            for r in rows if "scaler_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=14)
    ap.add_argument("--utts", type=int, default=67)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true", help="the run under rocprofv3: calls only, no output")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scaler_fit needs the MI355X"
    from crank_amd.bin.extract_statistics import fit_scalers
    from crank_amd.feature import FeatureStore

    data, scp = corpus(args.speakers, args.utts, args.frames)
    conf = {"feature": {"fs": 8000, "window_types": ["hann"]}}  # mlfb and lcf0, as the issue's corpus
    store = FeatureStore("cuda")
    for f, d in data.items():
        for k, v in d.items():
            store.put(f, k, v)
    run = lambda: fit_scalers(store, scp, conf)  # noqa: E731
    for _ in range(args.warmup):
        scaler = run()
    torch.cuda.synchronize()
    if args.profile_child:
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        return
    ms = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scaler = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    U = len(data)
    F = sum(d["lcf0"].shape[0] for d in data.values())
    mlfb_bytes, lcf0_bytes = F * MLFB_DIM * 4, F * 4
    res = {"metric": "scaler_fit", "speakers": args.speakers, "utts": U, "frames": F, "mlfb_dim": MLFB_DIM, "reps": args.reps,
           "warmup": args.warmup, "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
           "corpus_MB": round((mlfb_bytes + lcf0_bytes) / 1e6, 1), "scalers": len(scaler),
           "n_samples_seen": int(scaler["mlfb"].n_samples_seen_)}
    if not args.no_sklearn:
        try:
            from sklearn.preprocessing import StandardScaler
        except ImportError:
            StandardScaler = None
        if StandardScaler is not None:
            files = list(scp["feats"].values())
            t0 = time.perf_counter()
            ref = {}
            for ext in ("mlfb", "lcf0"):
                ref[ext] = StandardScaler()
                for f in files:
                    a = data[f][ext]
                    ref[ext].partial_fit(a[:, None] if a.ndim == 1 else a)
            for spk in scp["spkrs"]:
                ref[spk] = StandardScaler()
                for uid in scp["spk2utt"][spk]:
                    ref[spk].partial_fit(data[scp["feats"][uid]]["lcf0"][:, None])
            cpu_ms = (time.perf_counter() - t0) * 1e3
            rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))  # noqa: E731
            res.update({"sklearn_partial_fit_ms": round(cpu_ms, 1), "speedup_vs_sklearn": round(cpu_ms / med, 1),
                        "max_rel_mean_vs_sklearn": rel(scaler["mlfb"].mean_, ref["mlfb"].mean_),
                        "max_rel_var_vs_sklearn": rel(scaler["mlfb"].var_, ref["mlfb"].var_),
                        "max_rel_spk_lcf0_var_vs_sklearn": max(rel(scaler[s]["lcf0"].var_, ref[s].var_) for s in scp["spkrs"])})
    if not args.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="scaler_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", "--speakers", str(args.speakers), "--utts", str(args.utts),
               "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=200)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode == 0 and found:
            out = os.path.join(ROOT, "profiles", "scaler_fit_kernel_stats.csv")
            shutil.copyfile(found[0], out)
            k = kernel_times(out)
            res["kernels"] = k
            res["kernel_stats"] = "profiles/scaler_fit_kernel_stats.csv (3 warm-up and 2 further calls; each kernel runs for mlfb and lcf0)"
            # the 80-column launch is the slow half of the two moments launches and sets their maximum; the vector
            # kernel only ever runs on mlfb here
            vec = [v for n, v in k.items() if "moments" in n and "true" in n]
            if vec:
                us = vec[0]["avg_us"]
                res["moments_mlfb_us"] = us
                res["moments_mlfb_floor_us_2x"] = round(2 * mlfb_bytes / HBM_BYTES_PER_S * 1e6, 2)
                res["moments_mlfb_floor_us_1x"] = round(mlfb_bytes / HBM_BYTES_PER_S * 1e6, 2)
                res["moments_mlfb_GBps_of_corpus_bytes"] = round(mlfb_bytes / us / 1e3, 1)
            mrg = [v for n, v in k.items() if "merge" in n]
            if mrg:
                res["merge_avg_us"] = mrg[0]["avg_us"]
                res["merge_ns_per_utterance"] = round(mrg[0]["avg_us"] * 1e3 / U, 1)
        else:
            res["kernels"] = f"rocprofv3 run failed (exit {p.returncode})"
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "scaler_fit_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
