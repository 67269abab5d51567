"""Parallel WaveGAN vocoder inference (crk_voc_forward) on one MI355X: prints one JSON line.

Shapes: a batch of 64 utterances x 500 frames at hop 128 (upsample_scales [4, 4, 8], 4.1 M samples) and a single
500-frame utterance; the default generator (30 layers / 3 stacks, aux 80, window 2) with random weights.  Per shape:
ms per call (HIP events, warm-up excluded), samples/s, the real-time factor at 22.05 kHz, the executed MFLOP per
sample and its fraction of the dense bf16 MFMA peak (2.5 PFLOP/s), and the same generator composed in torch on the
same GPU (the test-side restatement, fp32, MIOpen convolutions, the 64 equal-length utterances as one padded batch) as
the baseline.  --no-torch skips the baseline (profiling runs).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16 = 2.5e15
SR = 22050


def executed_mflop_per_sample(layers, aux, precise):
    auxp = (aux + 15) // 16 * 16
    mfma = layers * ((3 * 64 + auxp) * 128 + 128 * 64) + 64 * 64  # MACs per sample on the matrix cores
    return 2 * mfma * (3 if precise else 1) / 1e6


def time_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vocoder needs the MI355X"
    from crank_amd import ops
    from crank_amd.vocoder import ParallelWaveGANVocoder
    from tests.pwg_vocoder_ref import checkpoint_of, random_generator

    params = dict(upsample_params={"upsample_scales": [4, 4, 8]})
    hop, layers, aux = 128, 30, 80
    g = random_generator(0, **params)
    voc = ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(g), {"generator_params": params, "hop_size": hop},
                                                 device="cuda")
    g.remove_weight_norm()
    g = g.cuda()
    prec = ops.get_precision()
    precise = prec in ("bf16x3", "bf16x3f")
    res = {"metric": "pwg_vocoder_inference", "precision": prec, "hop": hop, "layers": layers}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for tag, B, T in (("batch64x500", 64, 500), ("single500", 1, 500)):
        cs = [torch.randn(T, aux, device="cuda", generator=gen) for _ in range(B)]
        xs = [torch.randn(T * hop, device="cuda", generator=gen) for _ in range(B)]
        voc.reserve(B, B * T)
        ms = time_ms(lambda: voc.inference_batch(cs, xs), args.warmup, args.reps)
        n = B * T * hop
        mf = executed_mflop_per_sample(layers, aux, precise)
        r = {"ms": round(ms, 3), "samples": n, "samples_per_s": round(n / ms * 1e3), "rtf_22k": round(ms / 1e3 / (n / SR), 6),
             "mflop_per_sample": round(mf, 4), "frac_bf16_peak": round(mf * 1e6 * n / (ms / 1e3) / PEAK_BF16, 4)}
        if not args.no_torch:
            c = torch.stack(cs).transpose(1, 2)
            c = torch.nn.ReplicationPad1d(g.aux_context_window)(c)
            x = torch.stack(xs).unsqueeze(1)

            def torch_fwd():
                with torch.no_grad():
                    return g(x, c)

            tms = time_ms(torch_fwd, 1, max(1, args.reps // 2))
            r["torch_ms"] = round(tms, 3)
            r["speedup_vs_torch"] = round(tms / ms, 2)
            with torch.no_grad():
                y_t = torch_fwd().reshape(B, -1)
            ops.set_precision("bf16x3")
            try:
                y = torch.stack(voc.inference_batch(cs, xs))
            finally:
                ops.set_precision(prec)
            r["bf16x3_rel_l2_vs_torch"] = float((y - y_t).norm() / y_t.norm())
            del c, x, y_t
            torch.cuda.empty_cache()
        res[tag] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
