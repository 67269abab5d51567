"""Streaming CheapTrick / mel-cepstrum analysis (crank_amd.world.StreamingMcep, crk_wana_stream_push) on one MI355X:
milliseconds per push for S concurrent streams in steady lock-step at 16 kHz, shiftms 5, dim 24 with the low cut - pushes
of 80 ms of samples and their 16 F0 rows, each of which lets 16 frames per stream leave (four launches).

Beside it, measured in the same process, what the parent offers for the same frames: one ``WorldAnalyzer.mcep_batch``
call on S utterances of 16 frames (low cut, offsets, CheapTrick, mcep, with its host-side checks and allocations).

Every number is the median over --reps pushes after --warmup, each timed from the host with a synchronisation either
side.  Real time needs one 80 ms push per 80 ms.  Prints one JSON line and writes it to
profiles/wana_stream_bench_line.json.
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

FS, SHIFTMS, DIM, ALPHA, LOW_CUT = 16000, 5.0, 24, 0.41, 70
PUSH_MS, ROWS = 80, 16


def signal(S, n):
    """Eight harmonics of a slow glide per stream on a noise floor, and the glide as the F0 contour."""
    rng = np.random.default_rng(0)
    hop = int(FS * SHIFTMS / 1000)
    out = np.empty((S, n), np.float32)
    f0 = np.empty((S, -(-n // hop)))
    for s in range(S):
        f = np.linspace(110.0 + 3 * (s % 40), 150.0 + 3 * (s % 40), n)
        ph = 2 * np.pi * np.cumsum(f) / FS
        out[s] = sum(rng.uniform(0.05, 0.3) * np.sin(h * ph + rng.uniform(0, 6.28)) for h in range(1, 9)) + 1e-2 * rng.standard_normal(n)
        f0[s] = f[::hop]
    return out, f0


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wana_stream_bench_line.json"))
    a = ap.parse_args()
    from crank_amd.world import WorldAnalyzer, analysis_capacities

    C = PUSH_MS * FS // 1000
    wa = WorldAnalyzer(FS, shiftms=SHIFTMS)
    rows = []
    for S in a.streams:
        pushes = a.warmup + a.reps
        xs, f0s = signal(S, C * (pushes + 9))
        x, f0 = torch.from_numpy(xs).cuda(), torch.from_numpy(f0s).cuda()
        ring, queue = analysis_capacities(FS, SHIFTMS, 0.0, C, ROWS)
        sm = wa.streaming(S, C, ROWS, dim=DIM, alpha=ALPHA, low_cut=LOW_CUT, max_utt_frames=ROWS * (pushes + 10))
        assert (sm.ring_capacity, sm.f0_capacity) == (ring, queue)
        out = sm.empty_outputs(S)
        at = [0]

        def push(i):
            k = at[0]
            sm.push(x[:, k * C:(k + 1) * C].contiguous(), f0[:, k * ROWS:(k + 1) * ROWS].contiguous(), out=out)
            at[0] += 1

        for _ in range(8):  # past the first 512 samples: every push lets 16 frames leave
            push(0)
        ms = timed(push, pushes)[a.warmup:]
        assert out["n_frames"].tolist() == [ROWS] * S
        sm.status()

        # the parent's way for the same frames: one offline call on S utterances of 16 frames
        waves = [x[s, :C].clone() for s in range(S)]
        conts = [f0[s, :ROWS].clone() for s in range(S)]
        base = timed(lambda i: wa.mcep_batch(waves, conts, DIM, ALPHA, LOW_CUT), pushes)[a.warmup:]
        rows.append(dict(S=S, push_ms=round(float(np.median(ms)), 3), push_ms_min=round(float(np.min(ms)), 3),
                         offline_call_ms=round(float(np.median(base)), 3),
                         real_time_factor=round(float(np.median(ms)) / PUSH_MS, 4), state_bytes=sm.state_bytes,
                         max_frames=sm.max_frames, ring_capacity=ring, f0_capacity=queue))
    line = dict(metric="wana_stream", fs=FS, shiftms=SHIFTMS, dim=DIM, low_cut=LOW_CUT, push_ms=PUSH_MS, frames_per_push=ROWS,
                reps=a.reps, warmup=a.warmup, timing="host clock, synchronised either side of a push",
                device=torch.cuda.get_device_name(0), results=rows)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
