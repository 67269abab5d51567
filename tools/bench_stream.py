"""Streaming conversion (crank_amd.stream.StreamingConverter, crk_stream_push) on one MI355X: microseconds per push and
pushes per second for S concurrent streams x C new frames per push, on the default configuration with ``causal: true``,
each push replayed from a HIP graph captured on static buffers.

Beside it, measured in the same process, the only way to get the same frames without the carried state: the offline
``VQVAE2.forward`` under ``no_grad`` on the last R + C frames of every stream (R = the receptive chain, 132 frames for the
default shapes), of which the last C are kept - eager, as ``trainer.eval`` calls it, in bf16x3 (the arithmetic whose codes
agree with streaming's) and in plain bf16 (the fastest the package has).

Every number is the median over --reps timed repetitions after --warmup (HIP events; a streaming repetition is --burst
replays between one pair of events).  Real-time factor: push time / (C x 5.8 ms), the recipe's hop; below 1 the S streams
keep up with their speakers.  Prints one JSON line per (S, C) and writes the table to profiles/stream_bench_mi355x.txt.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP_MS = 5.8
N_SPK = 14


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
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench_mi355x.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stream needs the MI355X"
    from crank_amd import ops
    from crank_amd.net.module.vqvae2 import VQVAE2
    from crank_amd.stream import StreamingConverter, receptive_chain
    from crank_amd.utils import load_yaml

    conf = load_yaml(None, causal=True)
    torch.manual_seed(0)
    G = VQVAE2(conf, spkr_size=N_SPK).eval()
    with torch.no_grad():
        for q in G.quantizers:
            q.weight.normal_()
    G.touch()
    reach = receptive_chain(conf)
    gen = torch.Generator("cuda").manual_seed(1)
    rows, lines = [], []
    for S in args.streams:
        conv = StreamingConverter(G, S, max(args.chunks))
        for C in args.chunks:
            feats = torch.randn(S, C, conf["input_size"], device="cuda", generator=gen)
            lcf0 = torch.randn(S, C, 1, device="cuda", generator=gen)
            uv = (torch.rand(S, C, 1, device="cuda", generator=gen) < 0.7).float()
            spk = torch.randint(0, N_SPK, (S,), device="cuda", generator=gen)
            out = conv.empty_outputs(S, C)
            conv.push(feats, lcf0, uv, spk, out=out)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                conv.push(feats, lcf0, uv, spk, out=out)
            push_us = timed(graph.replay, args.warmup, args.reps, args.burst)
            # the recompute path: the whole receptive chain again for every push
            x = torch.randn(S, reach + C, conf["input_size"], device="cuda", generator=gen)
            dec_h = torch.cat([torch.randn(S, reach + C, 1, device="cuda", generator=gen),
                               (torch.rand(S, reach + C, 1, device="cuda", generator=gen) < 0.7).float()], -1)
            h = spk[:, None].expand(S, reach + C).contiguous()
            rec = {}
            for mode in ("bf16x3", "bf16"):
                ops.set_precision(mode)
                try:
                    def forward():
                        with torch.no_grad():
                            return G(x, None, dec_h, spkrvec=h, use_ema=False)["decoded"][:, reach:]
                    rec[mode] = timed(forward, args.warmup, args.reps)
                finally:
                    ops.set_precision("bf16")
            res = {"metric": "stream_push", "streams": S, "chunk": C, "push_us": round(push_us, 1),
                   "pushes_per_s": round(1e6 / push_us, 1), "frames_per_s": round(S * C * 1e6 / push_us),
                   "real_time_factor": round(push_us / (C * HOP_MS * 1e3), 5),
                   "recompute_frames": reach + C, "recompute_bf16x3_us": round(rec["bf16x3"], 1),
                   "recompute_bf16_us": round(rec["bf16"], 1), "ratio_bf16x3": round(rec["bf16x3"] / push_us, 2),
                   "ratio_bf16": round(rec["bf16"] / push_us, 2), "reps": args.reps, "burst": args.burst,
                   "state_bytes": conv.state_bytes}
            print(json.dumps(res), flush=True)
            rows.append(res)
    lines.append(f"streaming push (HIP graph replay) vs recompute of {reach} + C frames (eager VQVAE2.forward, no_grad), default "
                 f"causal configuration, median of {args.reps}, hop {HOP_MS} ms")
    lines.append(f"{'S':>4} {'C':>3} {'push us':>10} {'pushes/s':>10} {'frames/s':>10} {'RTF':>9} {'recompute bf16x3 us':>20} "
                 f"{'x':>7} {'recompute bf16 us':>18} {'x':>7}")
    for r in rows:
        lines.append(f"{r['streams']:>4} {r['chunk']:>3} {r['push_us']:>10.1f} {r['pushes_per_s']:>10.1f} {r['frames_per_s']:>10d} "
                     f"{r['real_time_factor']:>9.5f} {r['recompute_bf16x3_us']:>20.1f} {r['ratio_bf16x3']:>7.2f} "
                     f"{r['recompute_bf16_us']:>18.1f} {r['ratio_bf16']:>7.2f}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
