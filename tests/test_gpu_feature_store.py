"""From waveforms to a collated batch without the host: ``Feature.analyze_batch`` -> ``fit_scalers`` ->
``BaseDataset(reader=store)`` on 2 speakers x 2 short harmonic utterances at 16 kHz.

* every key of the store is what the entry point it wraps returns, called directly (as float32);
* a dataset packed from the store's tensors assembles, bit for bit, what a dataset packed through a numpy reader over the
  downloaded features assembles, with the same fitted scalers;
* ``FeatureStore.save`` / ``load`` round-trips; an mcep-typed dataset says that D4C's ``cap`` is what it lacks.
"""
import functools

import numpy as np
import pytest
import torch

from tests.harvest_cases import _harmonics

pytestmark = pytest.mark.gpu

FS = 16000
FEATURE = dict(label="mlfb", fs=FS, fftl=1024, win_length=1024, hop_size=80, window_types=["hann", "hamming"], fmin=80,
               fmax=7600, mlfb_dim=80, n_iteration=100, shiftms=5, mcep_dim=34, mcep_alpha=0.41)
SPKR_CONF = {"SF1": {"minf0": 120, "maxf0": 400}, "TM1": {"minf0": 70, "maxf0": 300}}
UTTS = [("SF1", "E1", 0.30, 221.0), ("TM1", "E1", 0.50, 103.0), ("SF1", "E2", 0.43, 247.0), ("TM1", "E2", 0.36, 131.0)]
KEYS = ["raw", "mlfb", "mlfb_hamming", "f0", "uv", "cf0", "lf0", "lcf0"]


def _h5(spk, utt):
    return f"/feats/mlfb/train/{spk}/{utt}.h5"


@functools.lru_cache(maxsize=None)
def corpus():
    """(waves float64 in [-1, 1], labels, store, fitted scalers, scp of the dataset, scp of the fit)."""
    from crank_amd.bin.extract_statistics import fit_scalers
    from crank_amd.feature import Feature

    rng = np.random.default_rng(77)
    waves = []
    for _, _, sec, f0 in UTTS:
        n = int(sec * FS) + 3
        waves.append(_harmonics(rng, np.linspace(f0, 1.1 * f0, n), FS))
    flbls = [f"{s}/{u}" for s, u, _, _ in UTTS]
    store = Feature(FEATURE, "cuda").analyze_batch(waves, flbls, [SPKR_CONF[s] for s, *_ in UTTS])
    feats = {f"{s}_{u}": _h5(s, u) for s, u, _, _ in UTTS}
    fit_scp = {"feats": feats, "spkrs": ["SF1", "TM1"],
               "spk2utt": {sp: [f"{s}_{u}" for s, u, _, _ in UTTS if s == sp] for sp in ("SF1", "TM1")}}
    conf = {"feature": FEATURE}
    scaler = fit_scalers(store, fit_scp, conf)
    scp = {"train": {"feats": feats, "spkrs": ["SF1", "TM1"]}}
    return waves, flbls, store, scaler, scp, fit_scp


def test_every_store_key_is_the_entry_point_it_wraps():
    from crank_amd.net.module.mlfb import logmelfilterbank
    from crank_amd.world import WorldAnalyzer, continuous_f0_batch

    waves, flbls, store, *_ = corpus()
    raws = [np.asarray(w, np.float32) for w in waves]
    f0s, _ = WorldAnalyzer(FS, 1024, 5, "cuda").analyze_batch(raws, [SPKR_CONF[s]["minf0"] for s, *_ in UTTS],
                                                             [SPKR_CONF[s]["maxf0"] for s, *_ in UTTS], low_cut=70)
    cont = continuous_f0_batch(f0s, "cuda", return_filled=True)
    for i, lbl in enumerate(flbls):
        got = {k: store(lbl, ext=k) for k in KEYS}
        assert sorted(store.feats[lbl]) == sorted(KEYS)  # no mcep / npow at 16 kHz, never ap / cap
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in got.values())
        assert np.array_equal(got["raw"].cpu().numpy(), raws[i])
        for win, name in (("hann", "mlfb"), ("hamming", "mlfb_hamming")):
            ref = logmelfilterbank(raws[i], FS, fft_size=1024, hop_size=80, win_length=1024, window=win, num_mels=80, fmin=80,
                                   fmax=7600, eps=1e-10)
            assert np.array_equal(got[name].cpu().numpy(), ref), name
        uv, cf0, lf0, lcf0, filled = cont[i]
        for name, ref in (("f0", filled), ("uv", uv), ("cf0", cf0), ("lf0", lf0), ("lcf0", lcf0)):
            assert torch.equal(got[name], ref.to(torch.float32)), name
        T = 1 + raws[i].size // 80
        assert got["mlfb"].shape == (T, 80) and got["lcf0"].shape == (T,) and bool(got["uv"].any())


def test_fitted_scalers_are_the_reference_dict():
    *_, store, scaler, scp, fit_scp = corpus()
    assert sorted(scaler) == ["SF1", "TM1", "lcf0", "mlfb", "mlfb_hamming"]
    rows = np.concatenate([store(f, ext="mlfb").cpu().numpy() for f in fit_scp["feats"].values()]).astype(np.float64)
    N = rows.shape[0]
    assert scaler["mlfb"].n_samples_seen_ == N and scaler["mlfb"].mean_.shape == (80,)
    # float64 numpy on the same rows, each within the worst-case summation bound of the other
    assert np.all(np.abs(scaler["mlfb"].mean_ - rows.mean(0)) <= 2 * N * 2.0**-53 * np.abs(rows).mean(0))
    assert np.all(np.abs(scaler["mlfb"].var_ - rows.var(0)) <= 2 * N * 2.0**-53 * (rows.var(0) + rows.mean(0) ** 2))
    n_sf1 = sum(store(_h5(s, u), ext="lcf0").shape[0] for s, u, _, _ in UTTS if s == "SF1")
    assert scaler["SF1"]["lcf0"].n_samples_seen_ == n_sf1 and scaler["SF1"]["lcf0"].mean_[0] > scaler["TM1"]["lcf0"].mean_[0]


@pytest.mark.parametrize("use_raw", [False, True])
def test_dataset_from_the_store_equals_dataset_from_a_numpy_reader_bitwise(use_raw):
    from crank_amd.net.trainer.dataset import BaseDataset

    *_, store, scaler, scp, _ = corpus()
    conf = {"batch_len": 80, "input_feat_type": "mlfb", "output_feat_type": "mlfb", "use_raw": use_raw, "ignore_scaler": [],
            "use_mcep_0th": False, "spec_augment": False, "feature": FEATURE}
    calls = []

    def host_reader(h5f, ext="mlfb"):
        calls.append(ext)
        return store(h5f, ext=ext).cpu().numpy()

    on_device = BaseDataset(conf, scp, scaler, phase="train", reader=store)
    through_host = BaseDataset(conf, scp, scaler, phase="train", reader=host_reader)
    assert calls and on_device.lens == through_host.lens and max(on_device.lens) > 80 > min(on_device.lens)
    for k in on_device.packed:
        assert torch.equal(on_device.packed[k], through_host.packed[k]), k
    draws = [("TM1", 0), ("SF1", 13), ("TM1", 0), ("SF1", 0)]
    a, b = on_device.assemble([0, 1, 2, 3], draws=draws), through_host.assemble([0, 1, 2, 3], draws=draws)
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b) and ("raw" in a) == use_raw
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert v.dtype == b[k].dtype and torch.equal(v, b[k]), k
        else:
            assert v == b[k], k
    assert a["flbl"] == ["SF1/E1", "TM1/E1", "SF1/E2", "TM1/E2"]


def test_store_round_trips_through_save_and_load(tmp_path):
    from crank_amd.feature import FeatureStore

    *_, store, scaler, scp, fit_scp = corpus()
    store.save(tmp_path)
    back = FeatureStore.load(tmp_path, "cuda")
    assert sorted(back.keys()) == sorted(store.keys())
    for lbl in store.keys():
        assert sorted(back.feats[lbl]) == sorted(store.feats[lbl])
        for k, t in store.feats[lbl].items():
            r = back(str(tmp_path / (lbl + ".h5")), ext=k)
            assert r.dtype == t.dtype and r.device == t.device and torch.equal(r, t), (lbl, k)


def test_an_mcep_dataset_over_the_store_says_that_cap_is_missing():
    from crank_amd.feature import FeatureStore
    from crank_amd.net.trainer.dataset import BaseDataset

    *_, store, scaler, scp, _ = corpus()
    with_mcep = FeatureStore("cuda")
    for lbl, feats in store.feats.items():
        for k, t in feats.items():
            with_mcep.put(lbl, k, t)
        with_mcep.put(lbl, "mcep", torch.zeros(feats["mlfb"].shape[0], 35, device="cuda"))
    conf = {"batch_len": 80, "input_feat_type": "mcep", "output_feat_type": "mcep", "use_raw": False,
            "ignore_scaler": ["mcep"], "use_mcep_0th": False, "spec_augment": False, "feature": FEATURE}
    with pytest.raises(KeyError, match="D4C aperiodicity is not implemented"):
        BaseDataset(conf, scp, scaler, phase="train", reader=with_mcep)


def test_main_writes_the_pickle_fit_scalers_returns(tmp_path):
    """The command line of the reference's stage 2 over a saved store: <featdir>/<label>/scaler.pkl holds the same dict."""
    import joblib
    import yaml

    from crank_amd.bin import extract_statistics

    *_, store, scaler, scp, fit_scp = corpus()
    featdir, scpdir = tmp_path / "feats", tmp_path / "scp" / "train"
    phase = featdir / "mlfb" / "train"
    store.save(phase)
    scpdir.mkdir(parents=True)
    (phase / "feats.scp").write_text("".join(f"{uid} {phase / utt}.h5\n" for uid, utt in
                                             zip(fit_scp["feats"], [f"{s}/{u}" for s, u, _, _ in UTTS])))
    (scpdir / "wav.scp").write_text("".join(f"{uid} /wav/{uid}.wav\n" for uid in fit_scp["feats"]))
    (scpdir / "utt2spk").write_text("".join(f"{uid} {uid.split('_')[0]}\n" for uid in fit_scp["feats"]))
    (scpdir / "spk2utt").write_text("".join(f"{s} {' '.join(u)}\n" for s, u in fit_scp["spk2utt"].items()))
    (tmp_path / "conf.yml").write_text(yaml.safe_dump({"feature": FEATURE}))
    extract_statistics.main(["--conf", str(tmp_path / "conf.yml"), "--scpdir", str(tmp_path / "scp"), "--featdir", str(featdir),
                             "--phase", "train"])
    got = joblib.load(featdir / "mlfb" / "scaler.pkl")
    assert sorted(got) == sorted(scaler)
    for k in ("mlfb", "mlfb_hamming", "lcf0"):
        for attr in ("mean_", "var_", "scale_"):
            assert np.array_equal(getattr(got[k], attr), getattr(scaler[k], attr)), (k, attr)
        assert got[k].n_samples_seen_ == scaler[k].n_samples_seen_
    for s in ("SF1", "TM1"):
        assert np.array_equal(got[s]["lcf0"].mean_, scaler[s]["lcf0"].mean_) and np.array_equal(got[s]["lcf0"].var_, scaler[s]["lcf0"].var_)
