"""WORLD synthesis for mcep models (crk_world_synthesis) on one MI355X: prints one JSON line.

Shape: a batch of 64 utterances x 500 frames at fs 22050, shiftms 10, 35 mel-cepstral coefficients (alpha 0.455) and 2
coded aperiodicity bands, with power modification (rmcep given, as the reference's eval stage does when use_mcep_0th is
false).  Inputs are seeded (tests/world_inputs.py).  Reported: ms per call (HIP events, warm-up excluded), output
samples/s, the real-time factor, the batch's pulse count, and as the baseline the CPU restatement
tests/world_synth_ref.py (numpy, float64, one thread of this host) on --cpu-utts of the utterances, scaled per
utterance.  --cpu-utts 0 skips the baseline (profiling runs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS, SHIFTMS, ORDER1, ALPHA = 22050, 10.0, 35, 0.455


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-utts", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_world needs the MI355X"
    from crank_amd.world import WorldSynthesizer
    from tests import world_synth_ref as R
    from tests.world_inputs import utterance

    rng = np.random.default_rng(0)
    ins = [utterance(rng, args.frames, ORDER1, R.n_bands(FS)) for _ in range(args.utts)]
    f0s, mcs, caps, rms = (list(x) for x in zip(*ins))
    syn = WorldSynthesizer(FS, 1024, SHIFTMS, ALPHA)
    dev = [[torch.as_tensor(a, device="cuda") for a in xs] for xs in (f0s, mcs, caps, rms)]

    def call():
        return syn.synthesis_batch(*dev)

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        ys = call()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.reps
    n = sum(int(y.numel()) for y in ys)
    res = {"metric": "world_synthesis", "utts": args.utts, "frames": args.frames, "fs": FS, "shiftms": SHIFTMS,
           "order1": ORDER1, "bands": R.n_bands(FS), "rmcep": True, "ms": round(ms, 3), "samples": n,
           "samples_per_s": round(n / ms * 1e3), "rtf": round(ms / 1e3 / (n / FS), 7), "pulses": syn.last_pulse_count,
           "finite": bool(all(torch.isfinite(y).all() for y in ys))}
    if args.cpu_utts > 0:
        k = args.cpu_utts
        t0 = time.perf_counter()
        ref = [R.synthesis(f0s[i], mcs[i], caps[i], rms[i], FS, 1024, SHIFTMS, ALPHA) for i in range(k)]
        cpu_s = time.perf_counter() - t0
        err = max(float(np.linalg.norm(ys[i].cpu().numpy() - ref[i]) / np.linalg.norm(ref[i])) for i in range(k))
        res.update({"cpu_restatement_utts": k, "cpu_restatement_s_per_utt": round(cpu_s / k, 3),
                    "cpu_restatement_s_batch_estimate": round(cpu_s / k * args.utts, 1),
                    "speedup_vs_cpu_restatement": round(cpu_s / k * args.utts / (ms / 1e3)),
                    "rel_l2_vs_cpu_restatement": err})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
