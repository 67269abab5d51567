"""The reference's ``crank/bin/extract_statistics.py`` (recipe stage 2) on the MI355X: the speaker-independent scalers of
``mlfb``, ``lcf0``, ``mcep`` (fs != 8000) and ``mlfb_<window>``, and every speaker's ``lcf0`` scaler, written to
``<featdir>/<label>/scaler.pkl``.

The reference calls ``StandardScaler.partial_fit`` once per utterance in file order, per scaler.  Here every feature is
packed once on the device and fitted by two launches (crank_amd.scaler): the per-utterance moments, then sklearn's merge
walked in the same file order - one group of all utterances for a speaker-independent scaler, one group per speaker in
the same launch for ``lcf0``.  Given the same per-utterance moments the merge is sklearn's bit for bit; the moments differ
from numpy's in summation order only.

``fit_scalers`` takes the reader ``BaseDataset`` takes: a ``crank_amd.feature.FeatureStore`` (the features never leave
the device) or any ``reader(h5f, ext) -> ndarray``; ``None`` reads HDF5 with h5py.  A NaN or infinite value, an empty
utterance and a speaker without utterances raise ValueError (sklearn's ``nansum`` branch is not offered).
"""
import argparse
import logging
from pathlib import Path

import numpy as np
import torch

from crank_amd.scaler import FittedScaler, ScalerFit, make_scaler  # noqa: F401  (FittedScaler: where pickles find it)


def scaler_feats(conf):
    """extract_statistics.py:61-68."""
    feats = ["mlfb", "lcf0"]
    if conf["feature"]["fs"] != 8000:
        feats.append("mcep")
    for win_type in conf["feature"]["window_types"]:
        if win_type != "hann":
            feats += [f"mlfb_{win_type}"]
    return feats


def _read(reader, files, ext):
    """Every utterance's (frames, D) block of ``ext`` as the reader returns it, checked on the host as far as the host
    can see: shapes, and the values of what arrives as an ndarray."""
    parts = []
    for f in files:
        a = reader(str(f), ext=ext)
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a)
        a = a[:, None] if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] < 1:
            raise ValueError(f"{f}: {ext} has shape {tuple(a.shape)}: an utterance needs at least one frame")
        if parts and a.shape[1] != parts[0].shape[1]:
            raise ValueError(f"{f}: {ext} has {a.shape[1]} dimensions, {files[0]} has {parts[0].shape[1]}")
        if not isinstance(a, torch.Tensor) and not np.isfinite(a).all():
            raise ValueError(f"{f}: {ext} holds a NaN or an infinite value: it cannot be fitted")
        parts.append(a)
    return parts


def fit_scalers(store_or_reader, scp, conf, device="cuda"):
    """The dict the reference pickles: ``scaler[ext]`` and ``scaler[spkr]["lcf0"]``.  ``scp``: one phase's lists as
    ``open_scpdir`` returns them, with ``feats`` filled ({utterance id: feature file}, in file order)."""
    if store_or_reader is None:
        from crank_amd.net.trainer.dataset import read_feature as store_or_reader
    reader = store_or_reader
    uids = list(scp["feats"])
    files = [scp["feats"][u] for u in uids]
    if not files:
        raise ValueError("no utterance to fit")
    index = {u: i for i, u in enumerate(uids)}
    spk_groups = []
    for spkr in scp["spkrs"]:
        members = [index[u] for u in scp["spk2utt"].get(spkr, [])]
        if not members:
            raise ValueError(f"speaker {spkr} has no utterance: its lcf0 scaler cannot be fitted")
        spk_groups.append(members)
    everything = list(range(len(files)))
    dev = torch.device(device)
    scaler = {}
    for ext in scaler_feats(conf):
        # the reference's stage 1 writes mcep only for fs > 16000 (feature.py:92) while its stage 2 asks for it whenever
        # fs != 8000, and stops there at 16 kHz; a store that was never given mcep is fitted without it
        if ext == "mcep" and hasattr(reader, "has") and not reader.has(files[0], ext):
            logging.info("no mcep in the feature store: its scaler is not fitted")
            continue
        parts = _read(reader, files, ext)
        lens = [int(p.shape[0]) for p in parts]
        fit = ScalerFit(lens, parts[0].shape[1], dev)
        if isinstance(parts[0], torch.Tensor):  # a feature store: packed where it lies
            x = torch.cat([p.to(device=dev, dtype=torch.float32) for p in parts]).contiguous()
        else:
            x = torch.as_tensor(np.ascontiguousarray(np.concatenate(parts), dtype=np.float32), device=dev)
        fit.moments(x)
        groups = [everything] + (spk_groups if ext == "lcf0" else [])
        mean, var, count = (t.cpu().numpy() for t in fit.merge(groups))
        scaler[ext] = make_scaler(mean[0], var[0], count[0])
        logging.info("# of samples for {}: {}".format(ext, scaler[ext].n_samples_seen_))
        if ext == "lcf0":
            for g, spkr in enumerate(scp["spkrs"], 1):
                scaler[spkr] = {"lcf0": make_scaler(mean[g], var[g], count[g])}
                logging.info("# of samples {} of {}: {} samples".format("lcf0", spkr, scaler[spkr]["lcf0"].n_samples_seen_))
    return scaler


def get_parser():
    parser = argparse.ArgumentParser(description="Extract feature statistics")
    parser.add_argument("--n_jobs", type=int, default=-1, help="# of CPUs (unused: one process drives the GPU)")
    parser.add_argument("--phase", type=str, default=None, help="phase")
    parser.add_argument("--conf", type=str, help="ymal file for network parameters")
    parser.add_argument("--scpdir", type=str, help="scp directory")
    parser.add_argument("--featdir", type=str, help="output feature directory")
    return parser


def main(argv=None):
    args = get_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    import joblib

    from crank_amd.feature import FeatureStore
    from crank_amd.utils import load_yaml, open_featsscp, open_scpdir

    conf = load_yaml(args.conf)
    scp = open_scpdir(Path(args.scpdir) / args.phase)
    featdir = Path(args.featdir) / conf["feature"]["label"]
    scp["feats"] = open_featsscp(featdir / args.phase / "feats.scp")
    # features a FeatureStore saved lie next to where feats.scp points (.npz, and .h5 with h5py); else plain HDF5
    store = FeatureStore.load(featdir / args.phase)
    reader = store if len(store) and all(f in store for f in scp["feats"].values()) else None
    scaler = fit_scalers(reader, scp, conf)
    pklf = featdir / "scaler.pkl"
    joblib.dump(scaler, str(pklf))
    logging.info("Save scaler to {}".format(pklf))


if __name__ == "__main__":
    main()
