"""Streaming vocoding (crank_amd.vocoder.StreamingVocoder, crk_voc_stream_push) on one MI355X: milliseconds per push for S
concurrent streams x C new frames per push, on the published generator configuration (30 layers / 3 stacks, 80 mel
channels, hop 256) with random weights, in steady state (every stream far enough into its utterance that every layer
computes C frames per push).  Each push is replayed from a HIP graph captured on static buffers; the eager push (the
Python call and its 3 + 4 + 30 launches) is timed beside it.

Beside it, measured in the same process, what the package offered before: ``inference_batch`` on a window of
2 * LA + C frames per stream (LA = 16), eager, of which C frames are kept.

Every number is the median over --reps timed repetitions after --warmup (HIP events; a repetition is --burst calls
between one pair of events), with the 10th and 90th percentile of the repetitions beside the streaming figure.  Share of
real time: push time / (C * hop / 24 kHz); below 1 the S streams keep up with their speakers.  Prints one JSON line per
cell and writes the table to profiles/voc_stream_bench_mi355x.txt.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 24000.0


def random_vocoder(params=None, seed=0, device="cuda"):
    """A ParallelWaveGANVocoder with random folded weights of the right shapes (fan-in scaled, so values stay finite)."""
    from crank_amd.vocoder import ParallelWaveGANVocoder, expected_keys, generator_params

    p = generator_params({"generator_params": params or {}})
    aux, K = p["aux_channels"], 2 * p["aux_context_window"] + 1
    scales = p["upsample_params"]["upsample_scales"]
    gen = torch.Generator().manual_seed(seed)
    shapes = {"first_conv.": (64, 1, 1), "upsample_net.conv_in.": (aux, aux, K), "last_conv_layers.1.": (64, 64, 1),
              "last_conv_layers.3.": (1, 64, 1)}
    for i, s in enumerate(scales):
        shapes[f"upsample_net.upsample.up_layers.{2 * i + 1}."] = (1, 1, 1, 2 * s + 1)
    for l in range(p["layers"]):
        shapes[f"conv_layers.{l}.conv."] = (128, 64, 3)
        shapes[f"conv_layers.{l}.conv1x1_aux."] = (128, aux, 1)
        shapes[f"conv_layers.{l}.conv1x1_out."] = (64, 64, 1)
        shapes[f"conv_layers.{l}.conv1x1_skip."] = (64, 64, 1)
    weights = {}
    for prefix, has_bias in expected_keys(p):
        shape = shapes[prefix]
        fan_in = int(np.prod(shape[1:]))
        w = torch.randn(shape, generator=gen) / np.sqrt(fan_in)
        weights[prefix] = (w, torch.randn(shape[0], generator=gen) * 0.1 if has_bias else None)
    return ParallelWaveGANVocoder(p, weights, int(np.prod(scales)), device=device)


def timed(fn, warmup, reps, burst=1):
    """(median, 10th percentile, 90th percentile) of ms per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / burst)
    return float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--precisions", nargs="+", default=["bf16", "bf16x3"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voc_stream_bench_mi355x.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voc_stream needs the MI355X"
    from crank_amd import ops

    voc = random_vocoder()
    H, A = voc.hop_size, voc.aux_channels
    gen = torch.Generator("cuda").manual_seed(1)
    rows = []
    for prec in args.precisions:
        ops.set_precision(prec)
        for S in args.streams:
            sv = voc.streaming(S, max(args.chunks))
            LA = sv.lookahead
            for C in args.chunks:
                c = torch.randn(S, C, A, device="cuda", generator=gen)
                x = torch.randn(S, C * H, device="cuda", generator=gen)
                out = sv.empty_outputs(S, C)
                sv.reset()
                for _ in range(LA // C + 4):  # into steady state: every layer computes C frames per push from here on
                    sv.push(c, x, out=out)
                torch.cuda.synchronize()
                assert out["n_out"].tolist() == [C * H] * S
                eager = timed(lambda: sv.push(c, x, out=out), args.warmup, args.reps, args.burst)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    sv.push(c, x, out=out)
                push = timed(graph.replay, args.warmup, args.reps, args.burst)
                assert out["n_out"].tolist() == [C * H] * S
                # what the package offered before: the offline vocoder on a window of 2 LA + C frames per stream
                W = 2 * LA + C
                cs = [torch.randn(W, A, device="cuda", generator=gen) for _ in range(S)]
                xs = [torch.randn(W * H, device="cuda", generator=gen) for _ in range(S)]
                voc.reserve(S, S * W)
                window = timed(lambda: voc.inference_batch(cs, xs), args.warmup, args.reps, max(1, args.burst // 4))
                real_ms = C * H / FS * 1e3
                res = {"metric": "voc_stream_push", "precision": prec, "streams": S, "chunk": C,
                       "push_ms": round(push[0], 4), "push_ms_p10": round(push[1], 4), "push_ms_p90": round(push[2], 4),
                       "eager_push_ms": round(eager[0], 4), "window_frames": W, "window_ms": round(window[0], 4),
                       "window_ms_p10": round(window[1], 4), "window_ms_p90": round(window[2], 4),
                       "window_over_push": round(window[0] / push[0], 2), "share_of_real_time": round(push[0] / real_ms, 4),
                       "window_share_of_real_time": round(window[0] / real_ms, 4), "reps": args.reps, "burst": args.burst,
                       "state_bytes": sv.state_bytes, "launches": 3 + len(voc.scales) + voc.params["layers"]}
                print(json.dumps(res), flush=True)
                rows.append(res)
    ops.set_precision("bf16")
    lines = [f"streaming vocoder push (HIP graph replay; eager beside it) vs inference_batch on a window of 2 LA + C frames per "
             f"stream (eager), published generator shapes, hop {H}, {FS / 1e3:g} kHz, median of {args.reps} x {args.burst} calls "
             "[10th .. 90th percentile]",
             f"{'prec':>7} {'S':>3} {'C':>2} {'push ms':>9} {'[p10':>8} {'p90]':>8} {'eager ms':>9} {'of real time':>13} "
             f"{'window ms':>10} {'[p10':>8} {'p90]':>8} {'of real time':>13} {'window / push':>14} {'state MiB':>10}"]
    for r in rows:
        lines.append(f"{r['precision']:>7} {r['streams']:>3} {r['chunk']:>2} {r['push_ms']:>9.4f} {r['push_ms_p10']:>8.4f} "
                     f"{r['push_ms_p90']:>8.4f} {r['eager_push_ms']:>9.4f} {r['share_of_real_time']:>13.4f} "
                     f"{r['window_ms']:>10.4f} {r['window_ms_p10']:>8.4f} {r['window_ms_p90']:>8.4f} "
                     f"{r['window_share_of_real_time']:>13.4f} {r['window_over_push']:>14.2f} {r['state_bytes'] / 2**20:>10.1f}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
