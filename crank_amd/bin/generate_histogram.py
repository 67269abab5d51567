"""The reference's ``crank/bin/generate_histogram.py`` (recipe "stage 1: initialization") on the MI355X: per speaker the
F0 histogram over (40, 700) Hz and the frame-power histogram over (-70, 20) dB of all its WAVs, 200 bins each, from which
the user reads ``minf0``, ``maxf0`` and ``npow`` for ``conf/spkr.yml``.

    python -m crank_amd.bin.generate_histogram [--n_jobs N] [--spkr S] wav_dir figure_dir

Speakers are the sub-directories of ``wav_dir``; a speaker is skipped when either of its figures exists
(generate_histogram.py:113).  The reference analyses one file per joblib worker with sprocket and pyworld and hands the
stacked contours to ``plt.hist``; here every remaining speaker goes through one ``crank_amd.histogram.SpeakerHistograms``
(analysis and binning on the device) and the figures are drawn from the downloaded counts:
``plt.hist(edges[:-1], bins=edges, weights=density)`` draws the patches ``plt.hist(data, bins=200, range=...,
density=True)`` draws.  Next to the two PNGs of a speaker goes ``<spkr>_histogram.npz`` with the counts themselves.
"""
import argparse
import logging
from pathlib import Path

import numpy as np

FIGURES = {  # generate_histogram.py:129-146
    "f0": dict(suffix="_f0histogram.png", step=50, xlabel="Fundamental frequency [Hz]"),
    "npow": dict(suffix="_npowhistogram.png", step=10, xlabel="Frame power [dB]"),
}


def speakers_of(wav_dir, spkr=None):
    """The speaker labels: the sub-directories of ``wav_dir``, sorted; ``spkr`` alone when given."""
    if spkr is not None:
        return [spkr]
    return sorted(p.name for p in Path(wav_dir).iterdir() if p.is_dir())


def wav_files(wav_dir, spkr):
    return sorted((Path(wav_dir) / spkr).glob("*.wav"))


def figure_paths(figure_dir, spkr):
    """{"f0": png, "npow": png, "npz": npz} of one speaker."""
    d = Path(figure_dir)
    out = {k: d / (spkr + v["suffix"]) for k, v in FIGURES.items()}
    out["npz"] = d / (spkr + "_histogram.npz")
    return out


def pending(wav_dir, figure_dir, spkr=None):
    """The speakers still to do: those with neither figure (the reference's rule)."""
    todo = []
    for s in speakers_of(wav_dir, spkr):
        paths = figure_paths(figure_dir, s)
        if paths["f0"].exists() or paths["npow"].exists():
            logging.info("Histogram of {} exists: skipped".format(s))
        else:
            todo.append(s)
    return todo


def pyplot():
    """matplotlib.pyplot on the Agg backend, or None (logged) when matplotlib does not import."""
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        logging.warning("matplotlib does not import: only the .npz files are written")
        return None
    return plt


def write_figure(plt, counts, edges, figure_path, step, xlabel):
    """``create_histogram`` (generate_histogram.py:31-74) from counts: the same patches, labels and ticks."""
    from crank_amd.histogram import density_of

    counts, edges = np.asarray(counts), np.asarray(edges, np.float64)
    weights = density_of(counts, edges) if counts.sum() > 0 else np.zeros(len(counts))
    plt.hist(edges[:-1], bins=edges, weights=weights, histtype="stepfilled")
    plt.xlabel(xlabel)
    plt.ylabel("Probability")
    plt.xticks(np.arange(edges[0], edges[-1], step))
    Path(figure_path).parent.mkdir(parents=True, exist_ok=True)
    plt.savefig(str(figure_path))
    plt.close()


def write_speaker(figure_dir, spkr, res, plt):
    """The .npz and, with matplotlib, the two figures of one speaker; ``res``: its entry of ``result()``."""
    paths = figure_paths(figure_dir, spkr)
    paths["npz"].parent.mkdir(parents=True, exist_ok=True)
    np.savez(str(paths["npz"]), f0_counts=res["f0"][0], f0_edges=res["f0"][1], npow_counts=res["npow"][0],
             npow_edges=res["npow"][1], n_frames=np.int64(res["n_frames"]), n_files=np.int64(res["n_files"]))
    if plt is not None:
        for key, fig in FIGURES.items():
            write_figure(plt, res[key][0], res[key][1], paths[key], fig["step"], fig["xlabel"])


def histograms_of(wav_dir, spkrs, hist):
    """Every WAV of ``spkrs`` through ``hist`` (a SpeakerHistograms), in speaker and file order.  Files are handed over
    whenever a call's worth of audio of one sampling rate has been read, so the corpus never lies in host memory whole."""
    from crank_amd.utils import read_wav

    held, held_fs, seconds = {}, None, 0.0
    for spkr in spkrs:
        files = wav_files(wav_dir, spkr)
        if not files:
            logging.warning("{}: no WAV file".format(spkr))
        for f in files:
            fs, x = read_wav(f)
            if held and (fs != held_fs or seconds >= hist.max_seconds):
                hist.add(held, held_fs)
                held, seconds = {}, 0.0
            held.setdefault(spkr, []).append(x)
            held_fs, seconds = fs, seconds + len(x) / fs
    if held:
        hist.add(held, held_fs)
    return hist.result()


def get_parser():
    parser = argparse.ArgumentParser(description="Create histogram for speaker-dependent configure")
    parser.add_argument("--n_jobs", type=int, default=-1, help="# of CPUs (unused: one process drives the GPU)")
    parser.add_argument("--spkr", type=str, default=None, help="Label of a speaker")
    parser.add_argument("wav_dir", type=str, help="Directory of wav file")
    parser.add_argument("figure_dir", type=str, help="Directory for figure output")
    return parser


def main(argv=None):
    args = get_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    from crank_amd.histogram import SpeakerHistograms

    todo = pending(args.wav_dir, args.figure_dir, args.spkr)
    if not todo:
        return
    plt = pyplot()
    result = histograms_of(args.wav_dir, todo, SpeakerHistograms())
    for spkr in todo:
        if spkr not in result:
            continue
        logging.info("Histogram generation for {}: {} files, {} frames".format(spkr, result[spkr]["n_files"],
                                                                                result[spkr]["n_frames"]))
        write_speaker(args.figure_dir, spkr, result[spkr], plt)


if __name__ == "__main__":
    main()
