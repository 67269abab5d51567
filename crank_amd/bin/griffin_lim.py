"""The reference's ``crank/bin/griffin_lim.py`` as one process on the MI355X: every log-mel feature file in --rootdir
becomes ``<stem>.wav`` (16-bit PCM) in --outdir through Griffin-Lim (crank_amd.griffin_lim), all of them as one ragged
batch instead of one joblib worker per file.

Reads ``*.npy`` (frames, mels; de-normalised, as stage 5 writes them and bin/pwg_decode.py reads them) and, when h5py
imports, ``*.h5`` with a ``feats`` dataset as the reference does.  The ``feature:`` block of --conf gives fs, mlfb_dim,
fftl, win_length, hop_size, fmin and fmax; --n_iters defaults to its ``n_iteration``.  Utterance i (in sorted file order)
starts from the phases of ``numpy.random.RandomState(seed + i)``.  A file with non-finite values is logged and skipped, as
the reference skips what librosa refuses.  (The reference builds its output names as ``Path / str + str``, a TypeError;
that is not reproduced.)
"""
import argparse
import logging
import os
import sys
from pathlib import Path

import numpy as np


def get_parser():
    p = argparse.ArgumentParser(description="Convert log-mel filter banks to waveforms with Griffin-Lim (HIP kernels)")
    p.add_argument("--conf", required=True, type=str, help="configuration file")
    p.add_argument("--rootdir", required=True, type=str, help="directory of *.npy / *.h5 feature files")
    p.add_argument("--outdir", required=True, type=str, help="directory for the wavs")
    p.add_argument("--n_iters", default=None, type=int, help="Griffin-Lim iterations (default: feature.n_iteration)")
    p.add_argument("--seed", default=0, type=int, help="seed of the initial phases")
    return p


def feature_files(rootdir):
    files = sorted(Path(rootdir).glob("*.npy"))
    try:
        import h5py  # noqa: F401
    except ImportError:
        return files
    return sorted(files + list(Path(rootdir).glob("*.h5")))


def read_feature(path):
    if Path(path).suffix == ".h5":
        import h5py

        with h5py.File(str(path), "r") as f:
            return np.asarray(f["feats"][()], np.float64)
    return np.asarray(np.load(path), np.float64)


def wav_name(outdir, feat_path):
    return Path(outdir) / (Path(feat_path).stem + ".wav")


def main(argv=None):
    args = get_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, stream=sys.stdout,
                        format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    from crank_amd.griffin_lim import GriffinLim
    from crank_amd.utils import load_yaml
    from crank_amd.world import write_pcm16

    fc = load_yaml(args.conf)["feature"]
    files = feature_files(args.rootdir)
    if not files:
        raise SystemExit(f"no *.npy or *.h5 features in {args.rootdir}")
    n_iters = fc.get("n_iteration", 100) if args.n_iters is None else args.n_iters
    gl = GriffinLim(fc["fs"], fc["mlfb_dim"], fc["fftl"], fc["win_length"], fc["hop_size"], fc["fmin"], fc["fmax"])
    names, feats = [], []
    for f in files:
        x = read_feature(f)
        if not np.isfinite(x).all():
            logging.info("ERROR: GriffinLim for {}".format(wav_name(args.outdir, f)))
            continue
        names.append(wav_name(args.outdir, f))
        feats.append(x)
    os.makedirs(args.outdir, exist_ok=True)
    if feats:
        for path, y in zip(names, gl.mlfb2wav_batch(feats, n_iters, args.seed)):
            write_pcm16(path, y.cpu().numpy(), fc["fs"])
    print(f"wrote {len(names)} wavs to {args.outdir}")


if __name__ == "__main__":
    main()
