"""SHA-256 digests of ``ParallelWaveGANVocoder.inference_batch`` on fixed seeded inputs: the published generator shapes
and a small one (6 layers / 2 stacks, hop 30, 8 aux channels), random weights, in bf16 and bf16x3, each on a single
utterance and on a ragged batch.  Run once per library (``CRANK_AMD_LIB`` selects another build of libcrank_hip.so) and
compare: a change that only moves the offline kernels' code must leave every digest as it was.

  python tools/voc_digest.py --out before.txt          # on the old library
  python tools/voc_digest.py --out after.txt --compare before.txt --table profiles/voc_offline_digests.txt
"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {
    "published 30/3 [4,4,4,4] aux 80": None,
    "small 6/2 [5,6] aux 8 win 1": dict(layers=6, stacks=2, aux_channels=8, aux_context_window=1,
                                       upsample_params={"upsample_scales": [5, 6]}),
}
BATCHES = {"single 23": [23], "ragged 1,3,17,40": [1, 3, 17, 40]}


def digests():
    from bench_voc_stream import random_vocoder
    from crank_amd import ops

    rows = []
    for name, params in CASES.items():
        voc = random_vocoder(params, seed=7)
        for bname, lens in BATCHES.items():
            gen = torch.Generator().manual_seed(13)
            cs = [torch.randn(T, voc.aux_channels, generator=gen).cuda() for T in lens]
            xs = [torch.randn(T * voc.hop_size, generator=gen).cuda() for T in lens]
            for prec in ("bf16", "bf16x3"):
                ops.set_precision(prec)
                try:
                    ys = voc.inference_batch(cs, xs)
                finally:
                    ops.set_precision("bf16")
                torch.cuda.synchronize()
                for T, y in zip(lens, ys):
                    assert bool(torch.isfinite(y).all())
                    rows.append((f"{name} | {bname} | {prec} | utterance of {T}", hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare")
    ap.add_argument("--table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "voc_digest needs the MI355X"
    rows = digests()
    with open(args.out, "w") as f:
        f.writelines(f"{k}\t{d}\n" for k, d in rows)
    if args.compare:
        before = dict(line.rstrip("\n").split("\t") for line in open(args.compare))
        lines = ["inference_batch waveform digests (sha256 of the fp32 samples), parent library | this tree", ""]
        changed = 0
        for k, d in rows:
            same = before.get(k) == d
            changed += not same
            lines.append(f"{k:<75} {before.get(k, '-')[:16]} {d[:16]} {'same' if same else 'DIFFERENT'}")
        lines.append("")
        lines.append(f"{len(rows)} outputs, {changed} changed")
        print("\n".join(lines))
        if args.table:
            with open(args.table, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
