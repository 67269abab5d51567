"""Streaming WORLD synthesis (crank_amd.world.StreamingWorldSynthesizer, crk_wsyn_stream_push) on one MI355X:
milliseconds per push for S concurrent streams in steady lock-step at 16 kHz, shiftms 5, 25 coefficients, 1 band - pushes
of 16 rows per stream (80 ms of signal; five launches, six with rmcep), with and without power modification.

Beside it, measured in the same process, what the parent offers for the same number of frames: one
``WorldSynthesizer.synthesis_batch`` call on S utterances of 16 frames (with its host-side checks, its allocations and its
one read-back of the pulse count).

Every number is the median over --reps pushes after --warmup, each timed from the host with a synchronisation either
side.  Real time needs one 80 ms push per 80 ms.  No time is a gate.  Prints one JSON line and writes it to
profiles/wsyn_stream_bench_line.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, SHIFTMS, ORDER1, ALPHA = 16000, 5.0, 25, 0.41
PUSH_MS, ROWS = 80, 16


def rows_of(S, T):
    """Per stream T frames of seeded cepstra on a slow voiced glide with an unvoiced run every 64 frames."""
    from tests.world_inputs import with_f0

    rng = np.random.default_rng(0)
    out = []
    for s in range(S):
        f0 = np.linspace(110.0 + 3 * (s % 40), 150.0 + 3 * (s % 40), T)
        f0[(np.arange(T) + 7 * s) % 64 < 6] = 0.0
        out.append(with_f0(rng, f0, ORDER1, 1))
    return [torch.from_numpy(np.stack([u[k] for u in out])).cuda() for k in range(4)]


def timed(fn, n):
    ms = []
    for i in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsyn_stream_bench_line.json"))
    a = ap.parse_args()
    from crank_amd.world import WorldSynthesizer, synthesis_capacities

    ws = WorldSynthesizer(FS, 1024, SHIFTMS, ALPHA)
    caps = synthesis_capacities(FS, SHIFTMS, ROWS, 1000.0)
    rows = []
    for S in a.streams:
        pushes = a.warmup + a.reps
        f0, mc, cap, rmc = rows_of(S, ROWS * (pushes + 5))
        res = dict(S=S)
        for pm in (False, True):
            sw = ws.streaming(S, ROWS, ORDER1, power_mod=pm, max_utt_samples=80 * ROWS * (pushes + 6))
            assert sw.capacities == caps
            out = sw.empty_outputs()
            at = [0]

            def push(i):
                k = slice(at[0] * ROWS, (at[0] + 1) * ROWS)
                sw.push(f0[:, k].contiguous(), mc[:, k].contiguous(), cap[:, k].contiguous(),
                        rmc[:, k].contiguous() if pm else None, out=out)
                at[0] += 1

            for _ in range(4):  # past the first pushes: every push lets about 1280 samples leave
                push(0)
            ms = timed(push, pushes)[a.warmup:]
            assert min(out["n_samples"].tolist()) > 0
            sw.status()
            key = "push_rmcep_ms" if pm else "push_ms"
            res[key] = round(float(np.median(ms)), 3)
            res[key + "_min"] = round(float(np.min(ms)), 3)
            res["state_bytes"] = sw.state_bytes()
            # the parent's way for the same number of frames: one offline call on S utterances of 16 frames
            lists = [[t[s, :ROWS].clone() for s in range(S)] for t in (f0, mc, cap, rmc)]
            base = timed(lambda i: ws.synthesis_batch(lists[0], lists[1], lists[2], lists[3] if pm else None), pushes)[a.warmup:]
            res["offline_call_rmcep_ms" if pm else "offline_call_ms"] = round(float(np.median(base)), 3)
        res["real_time_factor"] = round(res["push_rmcep_ms"] / PUSH_MS, 4)
        rows.append(res)
    line = dict(metric="wsyn_stream", fs=FS, shiftms=SHIFTMS, order1=ORDER1, bands=1, push_ms=PUSH_MS, rows_per_push=ROWS,
                capacities=caps, reps=a.reps, warmup=a.warmup, timing="host clock, synchronised either side of a push",
                device=torch.cuda.get_device_name(0), results=rows)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
