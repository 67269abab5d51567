"""The speaker histograms (crank_amd.histogram.SpeakerHistograms, crk_hist_accumulate) on one MI355X: prints one JSON
line and writes it to profiles/histogram_bench_line.json.

Two figures.
- ``add``: 2 speakers x 32 utterances x 5 s at fs 22050, search range 50 - 500 Hz, shiftms 5: one call's worth of audio
  (320 s), so low cut, Harvest, CheapTrick, the normalised power and the two histogram launches once each.  Inputs are
  those of tools/bench_harvest.py, scaled to the int16 range and cast to float32 as a WAV delivers them.  ms per ``add``
  over --reps timed calls after --warmup (HIP events around each call; the call includes the host-side tables and uploads).
- the histogram launch alone at corpus size: 467 723 values (the frame count of tools/bench_scaler_fit.py's corpus) in
  938 utterances of 14 groups, an F0-like contour (unvoiced zeros, voiced values around the speaker's mean).  Reported per
  launch: HIP events around --chain back-to-back launches, divided by their number (what a launch costs the stream when
  nothing waits for it), and its byte floor 8 N bytes over the copy rate.

Per-kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script's own (a child process,
--profile-child; its summary is copied to profiles/histogram_kernel_stats.csv and the histogram kernel's dispatches are
split by shape from the trace).  --no-profile skips that run.
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, SHIFTMS, MINF0, MAXF0 = 22050, 5, 50, 500
CORPUS_VALUES, CORPUS_GROUPS, CORPUS_UTTS = 467723, 14, 938
COPY_TBPS = 6.3  # what a float4 copy reaches
CHILD_ADDS, CHILD_LAUNCHES = 2, 20


def waves_by_speaker(speakers, utts, seconds):
    from tools.bench_harvest import inputs

    ys = inputs(speakers * utts, seconds)
    pcm = [np.round(y / np.abs(y).max() * 20000.0).astype(np.int16).astype(np.float32) for y in ys]
    return {f"S{s:02d}": pcm[s * utts:(s + 1) * utts] for s in range(speakers)}


def corpus_contour():
    """(x float64 [467 723], lens, groups): 938 utterances of about 400 - 600 values, speaker by speaker."""
    rng = np.random.default_rng(0)
    lens = rng.integers(400, 601, CORPUS_UTTS)
    diff = CORPUS_VALUES - int(lens.sum())
    np.add.at(lens, np.arange(abs(diff)) % CORPUS_UTTS, np.sign(diff))  # spread the remainder: the total is the corpus's
    assert int(lens.sum()) == CORPUS_VALUES and lens.min() > 0
    groups = np.repeat(np.arange(CORPUS_GROUPS), CORPUS_UTTS // CORPUS_GROUPS)
    mean = rng.uniform(90, 260, CORPUS_GROUPS)
    x = np.concatenate([np.where(rng.uniform(size=n) < 0.6, rng.normal(mean[g], 25.0, n), 0.0) for n, g in zip(lens, groups)])
    return x, [int(n) for n in lens], [int(g) for g in groups]


def hist_dispatches(trace_csv):
    """Durations in us of the histogram kernel's dispatches, in start order."""
    rows = [r for r in csv.DictReader(open(trace_csv)) if "hist_accumulate" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]


def stats_rows(stats_csv):
    rows = list(csv.DictReader(open(stats_csv)))
    return {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                            "share": round(float(r["Percentage"]) / 100.0, 5)}
            for r in rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=2)
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=500, help="back-to-back launches per timed window of the launch alone")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true", help="the run under rocprofv3: calls only, no output")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_histogram needs the MI355X"
    from crank_amd.histogram import Histogram, HistogramCall, SpeakerHistograms

    waves = waves_by_speaker(args.speakers, args.utts, args.seconds)
    hist = SpeakerHistograms(minf0=MINF0, maxf0=MAXF0)
    x, lens, groups = corpus_contour()
    xd = torch.as_tensor(x, device="cuda")
    alone = Histogram(40, 700, 200, CORPUS_GROUPS)
    call = HistogramCall(lens, groups)
    if args.profile_child:  # every add first, then every corpus-sized launch: the trace is split by position
        for _ in range(args.warmup + CHILD_ADDS):
            hist.add(waves, FS)
        torch.cuda.synchronize()
        for _ in range(args.warmup + CHILD_LAUNCHES):
            alone.launch(xd, call)
        torch.cuda.synchronize()
        return
    for _ in range(args.warmup):
        hist.add(waves, FS)
        assert alone.launch(xd, call) == 0
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hist.add(waves, FS)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    us = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.chain):
            alone.launch(xd, call)
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / args.chain)
    # the tables are numpy's after all those calls: every launch added the same counts
    n_alone = args.warmup + args.reps * args.chain
    want = np.stack([np.histogram(np.concatenate([x[s:s + n] for s, n, g in zip(np.cumsum([0] + lens[:-1]), lens, groups) if g == k]),
                                  bins=200, range=(40, 700))[0] for k in range(CORPUS_GROUPS)])
    res_tables = hist.result()
    n_utts = args.speakers * args.utts
    med = float(np.median(ms))
    res = {"metric": "speaker_histograms", "speakers": args.speakers, "utts_per_speaker": args.utts,
           "seconds_per_utt": args.seconds, "fs": FS, "shiftms": SHIFTMS, "minf0": MINF0, "maxf0": MAXF0, "reps": args.reps,
           "warmup": args.warmup, "add_ms_median": round(med, 3), "add_ms_min": round(min(ms), 3),
           "add_ms_max": round(max(ms), 3), "utterance_seconds_per_s": round(n_utts * args.seconds / med * 1e3, 1),
           "frames_per_add": int(sum(r["n_frames"] for r in res_tables.values()) // (args.warmup + args.reps)),
           "f0_kept_share": round(float(sum(r["f0"][0].sum() for r in res_tables.values())) /
                                  float(sum(r["n_frames"] for r in res_tables.values())), 3),
           "corpus_values": CORPUS_VALUES, "corpus_groups": CORPUS_GROUPS, "corpus_utts": CORPUS_UTTS, "chain": args.chain,
           "launch_us_median": round(float(np.median(us)), 3), "launch_us_min": round(min(us), 3),
           "launch_us_max": round(max(us), 3),
           "byte_floor_us": round(8.0 * CORPUS_VALUES / (COPY_TBPS * 1e12) * 1e6, 3),
           "corpus_counts_equal_numpy": bool(np.array_equal(alone.counts.cpu().numpy(), n_alone * want))}
    if not args.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="hist_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--profile-child", "--speakers", str(args.speakers), "--utts", str(args.utts),
               "--seconds", str(args.seconds), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode == 0 and stats and trace:
            out = os.path.join(ROOT, "profiles", "histogram_kernel_stats.csv")
            shutil.copyfile(stats[0], out)
            rows = stats_rows(out)
            adds = args.warmup + CHILD_ADDS
            durs = hist_dispatches(trace[0])
            assert len(durs) == 2 * adds + args.warmup + CHILD_LAUNCHES, len(durs)
            in_add, at_corpus = durs[:2 * adds], durs[2 * adds + args.warmup:]
            total_us = sum(r["calls"] * r["avg_us"] for r in rows.values())
            corpus_us = sum(durs[2 * adds:])
            res["kernel_stats"] = (f"profiles/histogram_kernel_stats.csv ({adds} add calls, and {args.warmup + CHILD_LAUNCHES} "
                                   "corpus-sized histogram launches)")
            res["hist_kernel_us_in_add"] = {"launches": len(in_add), "median": round(float(np.median(in_add)), 2),
                                            "min": round(min(in_add), 2), "max": round(max(in_add), 2)}
            res["hist_kernel_us_at_corpus_size"] = {"launches": len(at_corpus), "median": round(float(np.median(at_corpus)), 2),
                                                    "min": round(min(at_corpus), 2), "max": round(max(at_corpus), 2)}
            res["kernel_ms_per_add"] = round((total_us - corpus_us) / adds / 1e3, 3)
            res["hist_share_of_add_kernel_time"] = round(2 * float(np.median(in_add)) / ((total_us - corpus_us) / adds), 6)
            res["hist_share_of_add_call"] = round(2 * float(np.median(in_add)) / (med * 1e3), 6)
            res["kernels_us_per_add"] = {k: round(r["calls"] * r["avg_us"] / adds, 1) for k, r in rows.items()
                                         if "hist_accumulate" not in k and r["calls"] * r["avg_us"] / adds >= 100.0}
        else:
            res["kernels"] = f"rocprofv3 run failed (exit {p.returncode}): {p.stdout.decode(errors='replace')[-400:]}"
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "histogram_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
