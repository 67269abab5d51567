"""Stage 1 of the recipe on the device: waveforms in, the features ``BaseDataset`` reads out, kept in HBM.

``Feature`` mirrors the reference's ``crank/feature/feature.py``: ``analyze_batch`` runs the stage-1 kernels the package
already has - log-mel (net/module/mlfb.py), low cut, Harvest, ``convert_continuos_f0`` with ``lf0`` / ``lcf0``,
CheapTrick, ``sp2mc``, ``npow``, D4C coded aperiodicity with its ``ccap`` / ``cap_uv`` (world.py) - over a ragged batch
of utterances and files the results in a ``FeatureStore`` under the names the reference gives its HDF5 datasets.  It adds
no arithmetic of its own: every key is what the entry point it wraps returns, as float32 (``_save_hdf5``,
feature.py:59-65, stores float64 as float32).

``cap``, ``ccap`` and ``cap_uv`` are filed under the reference's own condition for ``mcep`` (fftl not 256, fs above
16 kHz) at the rates the D4C kernels take (up to 24052 Hz; above, the store has ``mcep`` without ``cap``, as before);
``ap`` only with ``keep_ap=True`` (nothing in the package reads it).  Not produced: ``spc`` and the
``synth_flag`` outputs (analysis-synthesis and Griffin-Lim wavs, plots).

``FeatureStore`` is the reference's directory of ``.h5`` files held on the device: ``{utterance: {name: tensor}}``, callable
as the ``reader(h5f, ext)`` that ``BaseDataset`` and ``fit_scalers`` take, so that a corpus goes from waveforms to the
first training step without visiting the host.
"""
from pathlib import Path

import numpy as np
import torch

from crank_amd._ragged import require_gpu

APERIODICITY = ("ap", "cap", "ccap", "cap_uv")
EPS = 1e-10


def utt_key(path):
    """``.../<speaker>/<utterance>.<suffix>`` or ``<speaker>/<utterance>`` -> ``<speaker>/<utterance>``: the label the
    reference forms from an HDF5 path (dataset.py:80-82), under which the store keeps an utterance."""
    p = Path(str(path))
    stem = p.stem if p.suffix in (".h5", ".npz", ".wav") else p.name
    return f"{p.parent.name}/{stem}" if p.parent.name else stem


class FeatureStore:
    """``{utterance: {name: device tensor}}``.  An utterance is addressed by any path that ends in
    ``<speaker>/<utterance>.h5`` (or by ``<speaker>/<utterance>`` itself), so the paths of a ``feats.scp`` work whichever
    directory they name."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.feats = {}

    def put(self, path, name, value):
        if isinstance(value, torch.Tensor):
            t = value.detach().to(self.device)
        else:
            t = torch.as_tensor(np.ascontiguousarray(value), device=self.device)
        self.feats.setdefault(utt_key(path), {})[name] = t

    def __call__(self, h5f, ext="mlfb"):
        key = utt_key(h5f)
        if key not in self.feats:
            raise KeyError(f"the feature store holds no utterance {key!r} (asked for {h5f})")
        if ext not in self.feats[key]:
            why = " (D4C aperiodicity is not implemented: ap, cap, ccap and cap_uv are not produced)" if ext in APERIODICITY else ""
            raise KeyError(f"utterance {key!r} has no feature {ext!r}{why}")
        return self.feats[key][ext]

    def has(self, path, ext):
        return ext in self.feats.get(utt_key(path), {})

    def __contains__(self, path):
        return utt_key(path) in self.feats

    def __len__(self):
        return len(self.feats)

    def keys(self):
        return list(self.feats)

    def save(self, dirname):
        """One ``<dir>/<speaker>/<utterance>.npz`` per utterance with the reference's dataset names, and the same as
        ``.h5`` when h5py imports."""
        try:
            import h5py
        except ImportError:
            h5py = None
        for key, feats in self.feats.items():
            path = Path(dirname) / key
            path.parent.mkdir(parents=True, exist_ok=True)
            host = {k: v.cpu().numpy() for k, v in feats.items()}
            np.savez(str(path) + ".npz", **host)
            if h5py is not None:
                with h5py.File(str(path) + ".h5", "w") as fp:
                    for k, v in host.items():
                        fp.create_dataset(k, data=v)

    @classmethod
    def load(cls, dirname, device="cuda"):
        """The store ``save`` wrote to ``dirname``: its ``.npz`` files and, when h5py imports, ``.h5`` files without one."""
        store = cls(device)
        root = Path(dirname)
        for f in sorted(root.glob("**/*.npz")):
            with np.load(f) as z:
                for k in z.files:
                    store.put(f, k, z[k])
        try:
            import h5py
        except ImportError:
            return store
        for f in sorted(root.glob("**/*.h5")):
            if f not in store:
                with h5py.File(str(f), "r") as fp:
                    for k in fp:
                        store.put(f, k, fp[k][()])
        return store


def mlfb_name(win_type):
    return "mlfb" if win_type == "hann" else f"mlfb_{win_type}"


class Feature:
    """``Feature(conf["feature"])``: the reference's extractor for a batch of utterances.  ``analyze_batch`` takes what
    the reference reads from disk - each waveform as ``soundfile.read`` returns it, its label ``<speaker>/<utterance>`` and
    its speaker's ``{"minf0": .., "maxf0": ..}`` - and returns the ``FeatureStore`` it filled."""

    def __init__(self, conf, device="cuda", keep_ap=False):
        from crank_amd.net.module.mlfb import LogMelFilterBankLayer
        from crank_amd.world import D4C_FS_MAX, D4C_FS_MIN, WorldAnalyzer, check_d4c_fs

        self.conf = conf
        self.keep_ap = bool(keep_ap)
        self.device = torch.device(device)
        windows = list(conf["window_types"])
        assert "hann" in windows  # feature.py:171
        for w in windows:
            if not hasattr(torch, f"{w}_window"):
                raise NotImplementedError(f"window type {w!r}: the log-mel layer takes torch's fixed windows (hann, hamming, ...)")
        require_gpu(self.device, "feature extraction")
        self.mlfb = {
            mlfb_name(w): LogMelFilterBankLayer(fs=conf["fs"], hop_size=conf["hop_size"], fft_size=conf["fftl"],
                                                win_length=conf["win_length"], window=w, center=True, n_mels=conf["mlfb_dim"],
                                                fmin=conf["fmin"], fmax=conf["fmax"], eps=EPS, device=self.device)
            for w in windows
        }
        self.world = WorldAnalyzer(conf["fs"], conf["fftl"], conf["shiftms"], self.device)
        self.with_mcep = conf["fftl"] != 256 and conf["fs"] > 16000  # feature.py:92
        # 44.1 / 48 kHz recipes keep what they got before D4C: mcep and npow, no cap (the store's KeyError says so)
        self.with_cap = self.with_mcep and D4C_FS_MIN <= conf["fs"] <= D4C_FS_MAX
        if self.keep_ap:
            check_d4c_fs(conf["fs"])

    def analyze_batch(self, waves, flbls, spkr_confs, store=None):
        from crank_amd.world import cap_postprocess_batch, continuous_f0_batch

        if not (len(waves) == len(flbls) == len(spkr_confs)) or len(waves) < 1:
            raise ValueError("waves, flbls and spkr_confs must be lists of the same non-zero length")
        dev = self.device
        store = FeatureStore(dev) if store is None else store
        f32 = lambda t: t.to(torch.float32)  # noqa: E731
        raws = [f32(w.detach().to(dev)) if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w, np.float32), device=dev)
                for w in waves]
        raws = [r.reshape(-1) for r in raws]
        for lbl, r in zip(flbls, raws):
            store.put(lbl, "raw", r)
            for name, layer in self.mlfb.items():
                store.put(lbl, name, layer(r[None])[0])
        minf0s = [float(c["minf0"]) for c in spkr_confs]
        maxf0s = [float(c["maxf0"]) for c in spkr_confs]
        f0s, sps = self.world.analyze_batch(raws, minf0s, maxf0s, low_cut=70)
        # the reference's convert_continuos_f0 fills the ends of the contour it is given in place, so the "f0" it saves
        # is the filled one
        for lbl, (uv, cf0, lf0, lcf0, filled) in zip(flbls, continuous_f0_batch(f0s, dev, return_filled=True)):
            for name, t in (("f0", filled), ("uv", uv), ("cf0", cf0), ("lf0", lf0), ("lcf0", lcf0)):
                store.put(lbl, name, f32(t))
        if self.with_mcep:
            mceps = self.world.mcep_batch(raws, f0s, dim=self.conf["mcep_dim"], alpha=self.conf["mcep_alpha"], low_cut=70)
            for lbl, mc, npow in zip(flbls, mceps, self.world.npow_of_sp_batch(sps)):
                store.put(lbl, "mcep", f32(mc))
                store.put(lbl, "npow", f32(npow))
        if self.with_cap:
            # feature.py:98-107: the coded aperiodicity with its maxima zeroed, its continuous form and its mask
            caps = self.world.codeap_batch(raws, f0s, low_cut=70)
            for lbl, (cap, ccap, cap_uv) in zip(flbls, cap_postprocess_batch(caps, dev)):
                for name, t in (("cap", cap), ("ccap", ccap), ("cap_uv", cap_uv)):
                    store.put(lbl, name, f32(t))
        if self.keep_ap:
            for lbl, ap in zip(flbls, self.world.d4c_batch(raws, f0s, low_cut=70)):
                store.put(lbl, "ap", f32(ap))
        return store
