"""Streaming log-mel front end (crank_amd.net.module.mlfb.StreamingLogMel, crk_logmel_stream_push) on one MI355X:
microseconds per push for S concurrent streams x C new samples per push at the recipe's framing (22 050 Hz, n_fft 1024 or --fft-size,
hop 128, 80 mels, centred, with a scaler), each push replayed from a HIP graph captured on static buffers.

Beside it, measured in the same process, what a caller does without it: a device-side tail of n_fft - hop samples per
stream, concatenated with the chunk, ``ops.logmel(center=False)`` on the result (C / hop frames), the tail replaced - once
replayed from a graph like the push, once eager.  (That caller still has to mirror the start and the end of every
utterance by hand; the steady state measured here has neither.)

Every number is the median over --reps timed repetitions after --warmup (HIP events; a repetition is --burst calls between
one pair of events).  Real-time factor: push time / (C / fs); below 1 the S streams keep up with their speakers.  Prints one
JSON line per (S, C) and writes the table to profiles/logmel_stream_bench_mi355x.txt.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, HOP, N_MELS = 22050, 128, 80


class Scaler:
    """Statistics of the magnitude the recipe's scaler holds (log10 mel energies around -4 +- 1)."""

    def __init__(self):
        rs = np.random.RandomState(0)
        self.mean_ = -4.0 + 0.5 * rs.standard_normal(N_MELS)
        self.var_ = rs.uniform(0.5, 1.5, N_MELS)


def timed(fn, warmup, reps, burst=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / burst)
    return float(np.median(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--chunks", type=int, nargs="+", default=[128, 512, 2048, 8192])
    ap.add_argument("--fft-size", type=int, default=1024, help="1024: ls_frame1024_kernel; another power of two: ls_frame_kernel")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logmel_stream_bench_mi355x.txt"))
    args = ap.parse_args()
    n_fft = args.fft_size
    assert torch.cuda.is_available(), "bench_logmel_stream needs the MI355X"
    from crank_amd import ops
    from crank_amd.net.module.mlfb import LogMelFilterBankLayer

    layer = LogMelFilterBankLayer(fs=FS, hop_size=HOP, fft_size=n_fft, n_mels=N_MELS, fmin=80, fmax=7600, center=True,
                                  scaler=Scaler())
    gen = torch.Generator("cuda").manual_seed(1)
    rows, lines = [], []
    for S in args.streams:
        sl = layer.streaming(S, max(args.chunks))
        for C in args.chunks:
            x = 0.1 * torch.randn(S, C, device="cuda", generator=gen)
            out = sl.empty_outputs(S)
            sl.reset()
            sl.push(x, out=out)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sl.push(x, out=out)
            push_us = timed(graph.replay, args.warmup, args.reps, args.burst)
            frames = int(out["n_frames"][0])  # the steady state: C / hop frames per push when hop divides C
            # the sliding-window call
            tail = 0.1 * torch.randn(S, n_fft - HOP, device="cuda", generator=gen)
            T = 1 + (n_fft - HOP + C - n_fft) // HOP

            def slide():
                buf = torch.cat([tail, x], 1)
                feats = ops.logmel(buf, T, n_fft, HOP, layer.win_length, layer.window, layer.mel_basis, layer.eps, layer.mean,
                                   layer.std, center=False)
                tail.copy_(buf[:, C:])
                return feats

            slide()
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                slide()
            slide_graph_us = timed(g2.replay, args.warmup, args.reps, args.burst)
            slide_eager_us = timed(slide, args.warmup, args.reps, args.burst)
            res = {"metric": "logmel_stream_push", "streams": S, "samples": C, "frames": frames, "push_us": round(push_us, 1),
                   "real_time_factor": round(push_us / (C / FS * 1e6), 6), "slide_graph_us": round(slide_graph_us, 1),
                   "slide_eager_us": round(slide_eager_us, 1), "ratio_graph": round(slide_graph_us / push_us, 2),
                   "ratio_eager": round(slide_eager_us / push_us, 2), "reps": args.reps, "burst": args.burst,
                   "state_bytes": sl.state_bytes}
            print(json.dumps(res), flush=True)
            rows.append(res)
            del graph, g2
    lines.append(f"streaming log-mel push (HIP graph replay) vs tail + chunk -> ops.logmel(center=False) (graph replay / eager), "
                 f"{FS} Hz, n_fft {n_fft}, hop {HOP}, {N_MELS} mels, centred, scaler; median of {args.reps} x {args.burst}")
    lines.append(f"{'S':>4} {'C':>5} {'frames':>6} {'push us':>9} {'RTF':>9} {'slide graph us':>15} {'x':>6} {'slide eager us':>15} {'x':>6}")
    for r in rows:
        lines.append(f"{r['streams']:>4} {r['samples']:>5} {r['frames']:>6} {r['push_us']:>9.1f} {r['real_time_factor']:>9.6f} "
                     f"{r['slide_graph_us']:>15.1f} {r['ratio_graph']:>6.2f} {r['slide_eager_us']:>15.1f} {r['ratio_eager']:>6.2f}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
