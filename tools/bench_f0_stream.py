"""Streaming F0 (crank_amd.world.StreamingF0, crk_f0_stream_push) on one MI355X: milliseconds per push for S concurrent
streams in lock-step at 16 kHz, 70 - 400 Hz, the 5 ms grid, the defaults 300 / 100 / 80 ms and the low cut - a push of
10 ms that completes no block (one launch) and a push of 80 ms that completes one (one round: window, Harvest, finish,
commit), both in the steady state behind the stream's first 480 ms, where the rounds' tables are one cached entry.

Beside it, measured in the same process, what a caller can do without it for one block: the windows sliced with torch
from a float64 history the caller keeps, ``HarvestF0(fs, 5).harvest_batch`` on them, ``continuous_f0_batch`` and
``crk_decode_f0`` (no low cut; the whole window's frames, of which the caller then keeps the block's).

Every number is the median over --reps pushes after --warmup, each timed from the host with a synchronisation either
side (a push cannot be captured in a graph, so what a caller waits for includes its launches).  Real time needs one
80 ms push per 80 ms.  Prints one JSON line and writes it to profiles/f0_stream_bench_line.json.
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

FS, SHIFTMS, LO, HI = 16000, 5, 70, 400
N_SPK = 4


def signal(S, seconds):
    """Eight harmonics of a slow glide per stream on a noise floor: voiced throughout."""
    rng = np.random.default_rng(0)
    n = int(seconds * FS)
    out = np.empty((S, n), np.float32)
    for s in range(S):
        f = np.linspace(110.0 + 3 * (s % 40), 150.0 + 3 * (s % 40), n)
        ph = 2 * np.pi * np.cumsum(f) / FS
        out[s] = sum(rng.uniform(0.05, 0.3) * np.sin(h * ph + rng.uniform(0, 6.28)) for h in range(1, 9)) + 1e-3 * rng.standard_normal(n)
    return out


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
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f0_stream_bench_line.json"))
    a = ap.parse_args()
    from crank_amd import _lib
    from crank_amd._lib import check, stream_ptr
    from crank_amd.world import HarvestF0, StreamingF0, continuous_f0_batch

    mean = torch.tensor([4.9, 5.3, 4.6, 5.1], dtype=torch.float64, device="cuda")
    std = torch.tensor([0.21, 0.17, 0.3, 0.25], dtype=torch.float64, device="cuda")
    block, small = 80 * FS // 1000, 10 * FS // 1000
    rows = []
    for S in a.streams:
        pushes = a.warmup + a.reps
        x = torch.from_numpy(signal(S, 0.5 + 0.08 * (2 * pushes + 2))).cuda()
        org = torch.arange(S, dtype=torch.int32, device="cuda") % N_SPK
        cv = (org + 1) % N_SPK
        sf = StreamingF0(FS, [LO] * S, [HI] * S, mean, std, block, shiftms=SHIFTMS, lcf0_scaler=(5.0, 0.3))
        out = sf.empty_outputs(S)
        at = [0]

        def push(c):
            sf.push(x[:, at[0]:at[0] + c].contiguous(), org, cv, out=out)
            at[0] += c

        for _ in range(7):  # past the first 480 ms: every window has its full length
            push(block)
        ready = timed(lambda i: push(block), pushes)[a.warmup:]
        assert int(out["n_frames"][0]) == block * 1000 // FS // SHIFTMS and len(sf._rounds) <= 7
        # 10 ms pushes: 7 of 8 complete no block; those are the idle ones
        idle, per = [], []
        for _ in range(8 * (a.reps // 4)):
            ms = timed(lambda i: push(small), 1)[0]
            (idle if int(out["n_frames"][0]) == 0 else per).append(ms)
        sf.status()

        # the caller's way, one block: windows of 480 ms from a float64 history, whole-window Harvest on the 5 ms grid
        hv = HarvestF0(FS, SHIFTMS)
        hist = x.double()
        W = (300 + 80 + 100) * FS // 1000
        T = int(1000.0 * W / FS / SHIFTMS) + 1
        cvl = torch.empty(S, T, dtype=torch.float64, device="cuda")
        nrm = torch.empty(S, T, dtype=torch.float64, device="cuda")

        def caller(i):
            lo = (i % 4) * block
            f0s = hv.harvest_batch([hist[s, lo:lo + W] for s in range(S)], [LO] * S, [HI] * S)
            res = continuous_f0_batch(f0s)
            lcf0 = torch.stack([r[3] for r in res]).float()
            uv = torch.stack([r[0] for r in res])
            check(_lib.lib().crk_decode_f0(lcf0.data_ptr(), uv.data_ptr(), S, T, org.data_ptr(), cv.data_ptr(), 0.0, 1.0, 0,
                                           mean.data_ptr(), std.data_ptr(), cvl.data_ptr(), 0, nrm.data_ptr(), stream_ptr()),
                  "crk_decode_f0")

        base = timed(caller, pushes)[a.warmup:]
        rows.append(dict(S=S, push_no_block_ms=round(float(np.median(idle)), 3), push_one_block_ms=round(float(np.median(ready)), 3),
                         push_one_block_ms_min=round(float(np.min(ready)), 3), push_10ms_with_block_ms=round(float(np.median(per)), 3),
                         caller_block_ms=round(float(np.median(base)), 3),
                         real_time_factor=round(float(np.median(ready)) / 80.0, 4), state_bytes=sf.state_bytes,
                         max_frames=sf.max_frames))
    line = dict(metric="f0_stream", fs=FS, shiftms=SHIFTMS, minf0=LO, maxf0=HI, back_ms=300, ahead_ms=100, block_ms=80,
                low_cut=70, reps=a.reps, warmup=a.warmup, timing="host clock, synchronised either side of a push",
                device=torch.cuda.get_device_name(0), results=rows)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
