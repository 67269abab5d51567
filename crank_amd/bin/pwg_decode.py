"""Recipe stage 6 with the Parallel WaveGAN vocoder on the MI355X (egs/vaevc/template/run.sh:173-241, voc=PWG):
``parallel-wavegan-normalize`` + ``parallel-wavegan-decode`` in one process.

Reads every ``*.npy`` log-mel (frames, mels; de-normalised, as stage 5 writes them) in --featdir, normalises it with
the vocoder's --stats, decodes all of them as one ragged batch and writes ``<stem>_gen.wav`` (16-bit PCM, clipped to
[-1, 1) like soundfile's PCM_16) into --outdir.
"""
import argparse
import glob
import os

import numpy as np


def get_parser():
    p = argparse.ArgumentParser(description="Parallel WaveGAN decoding of log-mel features (HIP kernels)")
    p.add_argument("--checkpoint", required=True, type=str, help="vocoder checkpoint (.pkl)")
    p.add_argument("--config", required=True, type=str, help="vocoder config.yml")
    p.add_argument("--stats", required=True, type=str, help="vocoder statistics (stats.npy or stats.h5)")
    p.add_argument("--featdir", required=True, type=str, help="directory of *.npy log-mel features")
    p.add_argument("--outdir", required=True, type=str, help="directory for the wavs")
    p.add_argument("--seed", default=0, type=int, help="seed of the noise input")
    return p


def feature_files(featdir):
    return sorted(glob.glob(os.path.join(featdir, "*.npy")))


def wav_name(outdir, feat_path):
    return os.path.join(outdir, os.path.splitext(os.path.basename(feat_path))[0] + "_gen.wav")


def to_pcm16(y):
    y = np.clip(np.asarray(y, np.float64), -1.0, 1.0 - 1.0 / 32768)
    return np.round(y * 32768).astype(np.int16)


def main(argv=None):
    args = get_parser().parse_args(argv)
    from scipy.io import wavfile

    from crank_amd.vocoder import ParallelWaveGANVocoder

    files = feature_files(args.featdir)
    if not files:
        raise SystemExit(f"no *.npy features in {args.featdir}")
    voc = ParallelWaveGANVocoder.from_checkpoint(args.checkpoint, args.config, stats=args.stats)
    voc.manual_seed(args.seed)
    feats = [voc.normalize(np.load(f)) for f in files]
    wavs = voc.inference_batch(feats)
    os.makedirs(args.outdir, exist_ok=True)
    sr = int(voc.sampling_rate or 22050)
    for f, y in zip(files, wavs):
        wavfile.write(wav_name(args.outdir, f), sr, to_pcm16(y.cpu().numpy()))
    print(f"wrote {len(files)} wavs to {args.outdir}")


if __name__ == "__main__":
    main()
