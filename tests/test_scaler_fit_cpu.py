"""Scaler fitting, host side: the numpy mirror of the merge kernel against sklearn's recorded ``partial_fit`` results
(tests/golden/scaler_fit.npz), sklearn's ``scale_`` rule, the fixture against the bounds the GPU tests hold the kernels
to, and the argument checks of ``fit_scalers`` that need no device."""
import ctypes
import os

import numpy as np
import pytest

from tests import scaler_fit_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(b, g) for b in R.BLOCKS for g in R.GROUPS]


def _group_rows(b, g):
    parts = R.split(R.window(b))
    return np.concatenate([parts[u] for u in R.group_members(g)])


def test_fixture_has_the_shapes_the_issue_names():
    fx = R.fixture()
    assert sorted(R.LENS) == [1, 2, 63, 64, 65, 255, 256, 257, 700]
    assert [R.LENS[u] for u in R.group_members("C")] == [1]
    assert R.SPKS[:4] == ["A", "C", "B", "A"]  # interleaved
    for b, (ld, col0, D) in R.BLOCKS.items():
        assert fx[f"{b}_x"].dtype == np.float32 and fx[f"{b}_x"].shape == (sum(R.LENS), ld)
        assert fx[f"{b}_sum"].shape == fx[f"{b}_m2"].shape == (len(R.LENS), D)
        assert fx[f"{b}_n"].tolist() == R.LENS
    assert np.all(fx["d80_x"][:, R.CONST_COL] == -10.0) and np.all(fx["d80_x"][:, R.ZERO_COL] == 0.0)
    assert R.BLOCKS["win"][0] > R.BLOCKS["win"][2] and R.BLOCKS["win"][1] == 3


@pytest.mark.parametrize("b", list(R.BLOCKS))
def test_mirror_moments_are_the_recorded_ones(b):
    fx = R.fixture()
    for u, X in enumerate(R.split(np.ascontiguousarray(R.window(b)))):
        n, s, m2 = R.utt_moments(X)
        assert n == fx[f"{b}_n"][u] and np.array_equal(s, fx[f"{b}_sum"][u]) and np.array_equal(m2, fx[f"{b}_m2"][u])


@pytest.mark.parametrize("b,g", CASES)
def test_mirror_merge_equals_sklearn_bit_for_bit(b, g):
    fx = R.fixture()
    mem = R.group_members(g)
    mean, var, count = R.merge(fx[f"{b}_n"][mem], fx[f"{b}_sum"][mem], fx[f"{b}_m2"][mem])
    assert np.array_equal(mean, fx[f"{b}_{g}_mean"])
    assert np.array_equal(var, fx[f"{b}_{g}_var"])
    assert count == int(fx[f"{b}_{g}_count"]) == sum(R.LENS[u] for u in mem)


@pytest.mark.parametrize("b,g", CASES)
def test_scale_rule_equals_sklearn_on_every_column(b, g):
    from crank_amd.scaler import FittedScaler, make_scaler, scale_of

    fx = R.fixture()
    mean, var, n = fx[f"{b}_{g}_mean"], fx[f"{b}_{g}_var"], int(fx[f"{b}_{g}_count"])
    want = fx[f"{b}_{g}_scale"]
    assert np.array_equal(scale_of(mean, var, n), want)
    assert np.array_equal(R.scale_rule(mean, var, n), want)
    f = FittedScaler(mean, var, n)
    assert np.array_equal(f.scale_, want) and type(f.n_samples_seen_) is int and f.n_features_in_ == mean.size
    if b == "d80":
        assert want[R.CONST_COL] == 1.0 and want[R.ZERO_COL] == 1.0
    if g == "C":
        assert np.all(var == 0.0) and np.all(want == 1.0)
    s = make_scaler(mean, var, n)  # a real StandardScaler where sklearn imports
    X = _group_rows(b, g)[:5]
    assert np.array_equal(s.transform(X), f.transform(X)) and s.transform(X).dtype == np.float32
    assert np.array_equal(s.inverse_transform(X), f.inverse_transform(X))
    assert np.array_equal(s.scale_, want) and type(s.n_samples_seen_) is int


@pytest.mark.parametrize("b,g", CASES)
def test_sklearn_itself_lies_within_the_end_to_end_bounds(b, g):
    """What shows that the fixture obeys the bounds the kernels are held to: sklearn's own mean_ / var_ against the exact
    values.  Measured on this fixture: at most 4e-5 of the mean's bound and 1.2e-2 of the variance's."""
    fx = R.fixture()
    bm, bv = R.bounds_mean_var(_group_rows(b, g), fx[f"{b}_{g}_xmean"], fx[f"{b}_{g}_xvar"])
    em, ev = np.abs(fx[f"{b}_{g}_mean"] - fx[f"{b}_{g}_xmean"]), np.abs(fx[f"{b}_{g}_var"] - fx[f"{b}_{g}_xvar"])
    assert np.all(em <= bm), (em / bm).max()
    assert np.all(ev <= bv), (ev, bv)


@pytest.mark.parametrize("b", list(R.BLOCKS))
def test_recorded_moments_lie_within_the_moment_bounds(b):
    fx = R.fixture()
    for u, X in enumerate(R.split(R.window(b))):
        bs, b2 = R.bounds_moments(X, fx[f"{b}_xsum"][u])
        assert np.all(np.abs(fx[f"{b}_sum"][u] - fx[f"{b}_xsum"][u]) <= bs)
        assert np.all(np.abs(fx[f"{b}_m2"][u] - fx[f"{b}_xm2"][u]) <= b2)
    if b == "d80":
        assert np.all(fx["d80_m2"][:, [R.CONST_COL, R.ZERO_COL]] == 0.0) and np.all(fx["d80_xm2"][:, R.CONST_COL] == 0.0)


# ------------------------------------------------------------------------------------------------ fit_scalers' refusals
def _corpus(bad=None):
    rng = np.random.default_rng(3)
    feats, data = {}, {}
    for i, (spk, n) in enumerate([("A", 5), ("B", 7), ("A", 3)]):
        f = f"/feats/train/{spk}/u{i}.h5"
        feats[f"u{i}"] = f
        data[f] = {"mlfb": rng.standard_normal((n, 4)).astype(np.float32), "lcf0": rng.standard_normal(n).astype(np.float32)}
    scp = {"feats": feats, "spkrs": ["A", "B"], "spk2utt": {"A": ["u0", "u2"], "B": ["u1"]}}
    conf = {"feature": {"fs": 8000, "window_types": ["hann"]}}
    if bad == "nan":
        data["/feats/train/B/u1.h5"]["mlfb"][3, 2] = np.nan
    if bad == "empty":
        data["/feats/train/A/u2.h5"]["mlfb"] = np.zeros((0, 4), np.float32)
    if bad == "speaker":
        scp["spkrs"].append("C")
        scp["spk2utt"]["C"] = []
    return scp, conf, lambda h5f, ext: data[h5f][ext]


@pytest.mark.parametrize("bad,what", [("nan", "NaN"), ("empty", "at least one frame"), ("speaker", "speaker C has no utterance")])
def test_fit_scalers_refuses_what_sklearn_would_not_fit(bad, what):
    """Before anything is launched: these raise on a machine without a GPU too."""
    from crank_amd.bin.extract_statistics import fit_scalers

    scp, conf, reader = _corpus(bad)
    with pytest.raises(ValueError, match=what):
        fit_scalers(reader, scp, conf)


def test_scaler_feats_follow_the_reference():
    from crank_amd.bin.extract_statistics import scaler_feats

    assert scaler_feats({"feature": {"fs": 8000, "window_types": ["hann"]}}) == ["mlfb", "lcf0"]
    assert scaler_feats({"feature": {"fs": 22050, "window_types": ["hann", "hamming"]}}) == ["mlfb", "lcf0", "mcep", "mlfb_hamming"]


def test_feature_refuses_an_unsupported_window_and_the_store_names_d4c():
    import torch

    from crank_amd.feature import Feature, FeatureStore, utt_key

    conf = dict(fs=16000, fftl=1024, win_length=1024, hop_size=80, window_types=["hann", "itu-g"], fmin=80, fmax=7600,
                mlfb_dim=80, shiftms=5, mcep_dim=34, mcep_alpha=0.41)
    with pytest.raises(NotImplementedError, match="itu-g"):
        Feature(conf, device="cpu")
    assert utt_key("/a/b/SF1/E1.h5") == utt_key("SF1/E1") == utt_key("x/SF1/E1.npz") == "SF1/E1"
    store = FeatureStore("cpu")
    store.put("SF1/E1", "mlfb", torch.zeros(3, 2))
    assert store("/any/where/SF1/E1.h5", ext="mlfb").shape == (3, 2)
    with pytest.raises(KeyError, match="D4C aperiodicity is not implemented"):
        store("/any/where/SF1/E1.h5", ext="cap")


def test_store_saves_and_loads_on_the_host(tmp_path):
    import torch

    from crank_amd.feature import FeatureStore

    store = FeatureStore("cpu")
    store.put("SF1/E1", "mlfb", torch.arange(6, dtype=torch.float32).reshape(3, 2))
    store.put("SF1/E1", "uv", torch.ones(3))
    store.put("TM1/E2", "mlfb", torch.zeros(1, 2))
    store.save(tmp_path)
    assert (tmp_path / "SF1" / "E1.npz").exists()
    back = FeatureStore.load(tmp_path, "cpu")
    assert sorted(back.keys()) == sorted(store.keys())
    for k in store.keys():
        assert sorted(back.feats[k]) == sorted(store.feats[k])
        for name, t in store.feats[k].items():
            assert back.feats[k][name].dtype == t.dtype and torch.equal(back.feats[k][name], t)


def test_crk_scaler_entries_are_declared_bound_and_exported():
    from crank_amd import _lib

    names = {"crk_scaler_workspace_bytes", "crk_scaler_moments", "crk_scaler_merge"}
    assert names <= set(_lib.SIGNATURES)
    lib_path = os.path.join(REPO, "crank_amd", "libcrank_hip.so")
    assert os.path.exists(lib_path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, s) for s in names)
    # host-only entry: status per (utterance, 64-column tile), n, sum, m2, each rounded up to 256 bytes
    lib.crk_scaler_workspace_bytes.restype = ctypes.c_longlong
    lib.crk_scaler_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert lib.crk_scaler_workspace_bytes(9, 80) == up(9 * 2 * 4) + up(9 * 8) + 2 * up(9 * 80 * 8)
    assert lib.crk_scaler_workspace_bytes(0, 80) == -1 and lib.crk_scaler_workspace_bytes(9, 0) == -1
