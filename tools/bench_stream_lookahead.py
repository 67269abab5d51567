"""Look-ahead streaming conversion (crank_amd.stream.LookaheadConverter, crk_lstream_push) on one MI355X: microseconds per
push for S concurrent streams x C new frames per push on the default configuration (``causal: false``, look-ahead 66
frames), in steady state (every stream further into its utterance than the look-ahead), each push replayed from a HIP graph
captured on static buffers.  Also one end push: C frames and the 66-slot flush of an utterance that starts and ends in it.

Beside it, measured in the same process on the same tree:
  * the causal push of tools/bench_stream.py at the same shapes (the same stacks built with ``causal: true``);
  * the only way to get the same frames without the carried state: the offline ``VQVAE2.forward`` under ``no_grad`` on a
    window of 2 LA + C frames per stream, of which C are kept - eager, in bf16x3 and in plain bf16.

Every number is the median over --reps timed repetitions after --warmup (HIP events; a streaming repetition is --burst
replays between one pair of events).  Prints one JSON line per (S, C) and writes the table to
profiles/stream_lookahead_bench_mi355x.txt.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_stream import HOP_MS, N_SPK, timed  # noqa: E402


def generator(conf):
    from crank_amd.net.module.vqvae2 import VQVAE2

    torch.manual_seed(0)
    G = VQVAE2(conf, spkr_size=N_SPK).eval()
    with torch.no_grad():
        for q in G.quantizers:
            q.weight.normal_()
    G.touch()
    return G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_lookahead_bench_mi355x.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stream_lookahead needs the MI355X"
    from crank_amd import ops
    from crank_amd.stream import LookaheadConverter, StreamingConverter, lookahead_frames
    from crank_amd.utils import load_yaml

    conf = load_yaml(None)
    assert not conf["causal"]
    G, Gc = generator(conf), generator(load_yaml(None, causal=True))
    la = lookahead_frames(conf)
    gen = torch.Generator("cuda").manual_seed(1)
    rows = []
    for S in args.streams:
        conv, causal = LookaheadConverter(G, S, max(args.chunks)), StreamingConverter(Gc, S, max(args.chunks))
        for C in args.chunks:
            feats = torch.randn(S, C, conf["input_size"], device="cuda", generator=gen)
            lcf0 = torch.randn(S, C, 1, device="cuda", generator=gen)
            uv = (torch.rand(S, C, 1, device="cuda", generator=gen) < 0.7).float()
            spk = torch.randint(0, N_SPK, (S,), device="cuda", generator=gen)
            end = torch.zeros(S, dtype=torch.int32, device="cuda")
            out = conv.empty_outputs(S)
            conv.reset()
            for _ in range(la // C + 2):  # past the look-ahead: every push emits C frames from here on
                conv.push(feats, lcf0, uv, spk, end=end, out=out)
            torch.cuda.synchronize()
            assert out["n_out"].tolist() == [C] * S
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                conv.push(feats, lcf0, uv, spk, end=end, out=out)
            push_us = timed(graph.replay, args.warmup, args.reps, args.burst)
            # an utterance that starts and ends in one push: C + LA slots
            conv.reset()
            end.fill_(1)
            graph_end = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_end):
                conv.push(feats, lcf0, uv, spk, end=end, out=out)
            end_us = timed(graph_end.replay, args.warmup, args.reps, args.burst)
            assert out["n_out"].tolist() == [C] * S and out["first"].tolist() == [0] * S
            conv.reset()
            # the causal push at the same shapes
            cout = causal.empty_outputs(S, C)
            causal.push(feats, lcf0, uv, spk, out=cout)
            torch.cuda.synchronize()
            graph_c = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_c):
                causal.push(feats, lcf0, uv, spk, out=cout)
            causal_us = timed(graph_c.replay, args.warmup, args.reps, args.burst)
            # the recompute path: LA frames of context on both sides again for every push
            W = 2 * la + C
            x = torch.randn(S, W, conf["input_size"], device="cuda", generator=gen)
            dec_h = torch.cat([torch.randn(S, W, 1, device="cuda", generator=gen),
                               (torch.rand(S, W, 1, device="cuda", generator=gen) < 0.7).float()], -1)
            h = spk[:, None].expand(S, W).contiguous()
            rec = {}
            for mode in ("bf16x3", "bf16"):
                ops.set_precision(mode)
                try:
                    def forward():
                        with torch.no_grad():
                            return G(x, None, dec_h, spkrvec=h, use_ema=False)["decoded"][:, la: la + C]
                    rec[mode] = timed(forward, args.warmup, args.reps)
                finally:
                    ops.set_precision("bf16")
            res = {"metric": "stream_lookahead_push", "streams": S, "chunk": C, "lookahead": la, "push_us": round(push_us, 1),
                   "causal_push_us": round(causal_us, 1), "vs_causal": round(push_us / causal_us, 3),
                   "end_push_us": round(end_us, 1), "end_us_per_slot": round(end_us / (C + la), 2),
                   "push_us_per_slot": round(push_us / C, 2), "frames_per_s": round(S * C * 1e6 / push_us),
                   "real_time_factor": round(push_us / (C * HOP_MS * 1e3), 5), "recompute_frames": W,
                   "recompute_bf16x3_us": round(rec["bf16x3"], 1), "recompute_bf16_us": round(rec["bf16"], 1),
                   "ratio_bf16x3": round(rec["bf16x3"] / push_us, 2), "ratio_bf16": round(rec["bf16"] / push_us, 2),
                   "reps": args.reps, "burst": args.burst, "state_bytes_per_stream": conv.state_bytes // S,
                   "causal_state_bytes_per_stream": causal.state_bytes // S}
            print(json.dumps(res), flush=True)
            rows.append(res)
    lines = [f"look-ahead streaming push (HIP graph replay, steady state, look-ahead {la} frames) vs the causal push at the same "
             f"shapes and vs recompute of 2 x {la} + C frames (eager VQVAE2.forward, no_grad), default configuration, median "
             f"of {args.reps}, hop {HOP_MS} ms; state per stream {rows[0]['state_bytes_per_stream']} bytes (causal "
             f"{rows[0]['causal_state_bytes_per_stream']})",
             f"{'S':>4} {'C':>3} {'push us':>10} {'causal us':>10} {'x causal':>9} {'end push us':>12} {'RTF':>9} "
             f"{'recompute bf16x3 us':>20} {'x':>7} {'recompute bf16 us':>18} {'x':>7}"]
    for r in rows:
        lines.append(f"{r['streams']:>4} {r['chunk']:>3} {r['push_us']:>10.1f} {r['causal_push_us']:>10.1f} {r['vs_causal']:>9.3f} "
                     f"{r['end_push_us']:>12.1f} {r['real_time_factor']:>9.5f} {r['recompute_bf16x3_us']:>20.1f} "
                     f"{r['ratio_bf16x3']:>7.2f} {r['recompute_bf16_us']:>18.1f} {r['ratio_bf16']:>7.2f}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
