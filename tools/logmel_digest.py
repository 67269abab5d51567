"""SHA-256 digests of the log-mel front end on fixed inputs, to show that a change which only moves the kernels' code left
every output bit as it was:
  * ``offline``: the offline call on every case of tests/logmel_cases.cases() as the GPU tests run it;
  * ``offline wave0``: its n_fft 1024 cases through the radix-2 kernel (CRK_LOGMEL_WAVE=0, in a fresh child process);
  * ``stream``: every name of tests/logmel_stream_ref.NAMES streamed under its mixed schedule, the frames below n_frames;
  * ``recipe``: the use_raw benchmark shape of tools/prof_logmel.py (64 x 65 023 samples -> 500 frames x 80).
Run once per library (``CRANK_AMD_LIB`` selects another build of libcrank_hip.so) and compare:

  python tools/logmel_digest.py --out before.txt          # on the old library
  python tools/logmel_digest.py --out after.txt --compare before.txt --table profiles/logmel_one_body_digests.txt
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def offline(names):
    from tests import test_gpu_logmel_shapes as G

    return [sha(G.run_case(G.BY[n], G.sig(n))) for n in names]


def digests():
    from tests import logmel_cases as C

    cs = C.cases()
    n1024 = [c["name"] for c in cs if c["n_fft"] == 1024]
    # the child first: this process has not touched the GPU yet
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--names"] + n1024, check=True, stdout=subprocess.PIPE,
                           text=True, env=dict(os.environ, CRK_LOGMEL_WAVE="0")).stdout.split()
    assert len(child) == len(n1024), child
    rows = [(f"offline wave0 | {n}", d) for n, d in zip(n1024, child)]

    import torch

    from crank_amd.net.module.mlfb import LogMelFilterBankLayer
    from tests import logmel_stream_ref as R
    from tests import test_gpu_logmel_stream as S

    names = [c["name"] for c in cs]
    rows = [(f"offline | {n}", d) for n, d in zip(names, offline(names))] + rows
    rows += [(f"stream mixed | {n}", sha(S.streamed(n))) for n in R.NAMES]
    B, hop, nfft, T = 64, 128, 1024, 500  # tools/prof_logmel.py
    layer = LogMelFilterBankLayer(fs=22050, hop_size=hop, fft_size=nfft, win_length=nfft, window="hann", center=False,
                                  n_mels=80, fmin=80, fmax=7600, device="cuda")
    x = (0.1 * torch.randn(B, (T - 1) * hop + nfft - 1 + 128, generator=torch.Generator().manual_seed(0))).cuda()
    y = layer(x)
    assert y.shape == (B, T, 80)
    rows.append(("recipe | 64 x 65023 -> 500 x 80", sha(y.cpu().numpy())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare")
    ap.add_argument("--table")
    ap.add_argument("--names", nargs="+", help="(the child) print the offline digests of these cases")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "logmel_digest needs the MI355X"
    if args.names:
        print("\n".join(offline(args.names)))
        return
    rows = digests()
    with open(args.out, "w") as f:
        f.writelines(f"{k}\t{d}\n" for k, d in rows)
    if args.compare:
        before = dict(line.rstrip("\n").split("\t") for line in open(args.compare))
        lines = ["log-mel digests (sha256 of the fp32 output), parent library | this tree", ""]
        changed = 0
        for k, d in rows:
            same = before.get(k) == d
            changed += not same
            lines.append(f"{k:<50} {before.get(k, '-')[:16]} {d[:16]} {'same' if same else 'DIFFERENT'}")
        lines += ["", f"{len(rows)} outputs, {changed} changed"]
        print("\n".join(lines))
        if args.table:
            with open(args.table, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
