"""crank_amd.world.WorldAnalyzer's D4C aperiodicity (csrc/d4c_kernels.hip, all float64) against the CPU restatement
tests/d4c_ref.py on the cases of tests/d4c_cases.py.  The bounds are 10 x the case's own two-FFT spread of the restatement
plus 1e-12 dB, derived on the CPU (test_d4c_cpu.py); no frame and no bin is masked out.  The restatement's parity against
pyworld is unpinned (it is not installed).  The last tests take a 24 kHz corpus from waveforms to an mcep dataset and back
to a waveform, which stops with the store's KeyError without D4C."""
import functools
import gc

import numpy as np
import pytest
import torch

from tests import d4c_cases as C
from tests import d4c_ref as D
from tests.harvest_cases import _harmonics

pytestmark = pytest.mark.gpu

NAMES = sorted(C.SPREADS)
SHAPE_KEYS = ("origin", "half_lt", "half_gb", "origin_c1", "origin_c2", "dc_limit", "bound_half", "bound_full")


@functools.lru_cache(maxsize=None)
def _cases():
    facts = C.edges_reached()  # on the host, before anything runs on the GPU
    assert all(facts.values()), facts
    assert sorted(c["name"] for c in C.cases()) == NAMES
    for name in NAMES:
        assert C.threshold_margin(name) >= C.MARGIN, name
    return {c["name"]: c for c in C.cases()}


@functools.lru_cache(maxsize=None)
def _analyzer(fs, shiftms):
    from crank_amd.world import WorldAnalyzer

    return WorldAnalyzer(fs, 1024, shiftms)


def _an(c):
    return _analyzer(c["fs"], c["shiftms"])


@pytest.mark.parametrize("name", NAMES)
def test_frame_integers_pass_flags_and_draw_offsets_equal_the_restatements(name):
    c = _cases()[name]
    got = _an(c).d4c_frame_shapes_batch(c["waves"], c["f0s"])
    for g, d in zip(got, C.reference(name)[2]):
        for key in SHAPE_KEYS:
            assert np.array_equal(g[key], d["shapes"][key]), (name, key)
        assert np.array_equal(g["passed"], d["passed"]), name
        assert np.array_equal(g["lt_offset"], d["shapes"]["lt_offset"]), name
        assert np.array_equal(g["gb_offset"], d["gb_offset"]), name


@pytest.mark.parametrize("name", NAMES)
def test_aperiodicity_and_coded_bands_within_the_cases_own_spread(name):
    c = _cases()[name]
    b_ap, b_cap = C.bounds(name)
    an = _an(c)
    aps = an.d4c_batch(c["waves"], c["f0s"])
    caps = an.codeap_batch(c["waves"], c["f0s"])
    w_aps, w_caps, det = C.reference(name)
    e_ap = e_cap = 0.0
    for ap, cap, w_ap, w_cap, d in zip(aps, caps, w_aps, w_caps, det):
        ap, cap = ap.cpu().numpy(), cap.cpu().numpy()
        assert ap.shape == w_ap.shape and cap.shape == w_cap.shape
        assert np.isfinite(ap).all() and (ap > 0).all() and (ap <= 1.0).all()  # 1.0: a band clamped to 0 dB, at its knot
        assert (ap[~d["passed"]] == 1.0 - 1e-12).all()  # unvoiced and below-threshold frames exactly
        e_ap = max(e_ap, float(np.abs(20.0 * np.log10(ap) - 20.0 * np.log10(w_ap)).max()))
        e_cap = max(e_cap, float(np.abs(cap - w_cap).max()))
    print(f"{name}: ap err {e_ap:.3e} dB (bound {b_ap:.3e}), cap err {e_cap:.3e} dB (bound {b_cap:.3e})")
    assert e_ap <= b_ap
    assert e_cap <= b_cap


def test_coded_bands_are_bitwise_the_coding_of_the_table_and_rows_do_not_depend_on_the_batch():
    c = _cases()["ragged"]
    an = _an(c)
    aps = an.d4c_batch(c["waves"], c["f0s"])
    caps = an.codeap_batch(c["waves"], c["f0s"])
    coded = an.code_aperiodicity_batch(aps)
    aps2, caps2 = an.d4c_batch(c["waves"], c["f0s"]), an.codeap_batch(c["waves"], c["f0s"])
    for i, (w, f) in enumerate(zip(c["waves"], c["f0s"])):
        assert torch.equal(caps[i], coded[i]), i
        assert torch.equal(aps[i], aps2[i]) and torch.equal(caps[i], caps2[i]), i
        assert torch.equal(an.d4c_batch([w], [f])[0], aps[i]), i
        assert torch.equal(an.codeap_batch([w], [f])[0], caps[i]), i
    rev = an.codeap_batch(c["waves"][::-1], c["f0s"][::-1])
    assert all(torch.equal(a, b) for a, b in zip(rev[::-1], caps))
    # the other rates' coding (1 and 3 bands), and low cut as in mcep_batch
    for name in ("fs16000_shift5", "fs24000_shift5"):
        c2 = _cases()[name]
        an2 = _an(c2)
        assert torch.equal(an2.codeap_batch(c2["waves"], c2["f0s"])[0],
                           an2.code_aperiodicity_batch(an2.d4c_batch(c2["waves"], c2["f0s"]))[0])
    cut = torch.cat(an.low_cut_batch(c["waves"][2:4], 70)).split([len(w) for w in c["waves"][2:4]])
    assert all(torch.equal(a, b) for a, b in zip(an.codeap_batch(c["waves"][2:4], c["f0s"][2:4], low_cut=70),
                                                 an.codeap_batch(list(cut), c["f0s"][2:4])))


def _raw(an, c):
    """Device buffers and a closure over the C entry itself (no host work: what a stream or a graph can carry)."""
    from crank_amd import _lib
    from crank_amd._ragged import offsets
    from crank_amd.world import K, n_bands

    lens, slens = [len(f) for f in c["f0s"]], [len(w) for w in c["waves"]]
    F, S = sum(lens), sum(slens)
    ws, draws = an.reserve_d4c(len(lens), F, max(lens))
    t = dict(x=torch.as_tensor(np.concatenate(c["waves"]), device="cuda"), f0=torch.as_tensor(np.concatenate(c["f0s"]), device="cuda"),
             foff=offsets(lens, an.device), soff=offsets(slens, an.device), ws=ws,
             ap=torch.zeros(F, K, dtype=torch.float64, device="cuda"),
             cap=torch.zeros(F, n_bands(c["fs"]), dtype=torch.float64, device="cuda"))
    h, lib = an.handle(), _lib.lib()

    def call(draws=draws, wsb=ws.numel(), handle=h):
        return lib.crk_wana_d4c(handle, t["x"].data_ptr(), t["f0"].data_ptr(), t["foff"].data_ptr(), t["soff"].data_ptr(),
                                len(lens), F, S, draws, 0.85, t["ap"].data_ptr(), t["cap"].data_ptr(), t["ws"].data_ptr(), wsb,
                                _lib.stream_ptr())

    return t, call, lens


def test_a_second_stream_and_a_captured_graph_give_the_same_bits_and_nothing_allocates():
    from crank_amd import _lib
    from crank_amd.net.trainer.basetrainer import hold_collector_for_capture

    c = _cases()["fs22050_shift5"]
    an = _an(c)
    want_ap, want_cap = an.d4c_batch(c["waves"], c["f0s"])[0], an.codeap_batch(c["waves"], c["f0s"])[0]
    t, call, _ = _raw(an, c)
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.crk_debug_alloc_count()
    assert call() == 0
    torch.cuda.synchronize()
    assert lib.crk_debug_alloc_count() == before
    assert torch.equal(t["ap"], want_ap) and torch.equal(t["cap"], want_cap)
    for k in ("ap", "cap"):
        t[k].zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call() == 0
    side.synchronize()
    assert torch.equal(t["ap"], want_ap) and torch.equal(t["cap"], want_cap)
    for k in ("ap", "cap"):
        t[k].zero_()
    torch.cuda.synchronize()
    gc_was_on = hold_collector_for_capture()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream(), capture_error_mode="thread_local"):
            rc = call()
    finally:
        if gc_was_on:
            gc.enable()
    assert rc == 0
    torch.cuda.synchronize()
    assert not t["ap"].any()  # the capture itself ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(t["ap"], want_ap) and torch.equal(t["cap"], want_cap)
    assert lib.crk_debug_alloc_count() == before
    del g


def test_a_draw_table_too_small_a_short_workspace_and_an_unsupported_rate_are_refused():
    from crank_amd import _lib

    c = _cases()["ends"]
    an = _an(c)
    t, call, lens = _raw(an, c)
    lib = _lib.lib()
    assert lib.crk_wana_d4c_draws_per_frame(an.handle()) == D.draws_per_frame(c["fs"])
    assert lib.crk_wana_d4c_workspace_bytes(1, sum(lens)) <= t["ws"].numel()
    fresh = lib.crk_wana_create(c["fs"], 1024, c["shiftms"], 0.0, 1)
    other = lib.crk_wana_create(44100, 1024, 5.0, 0.0, 1)
    assert fresh and other
    try:
        need = max(lens) * D.draws_per_frame(c["fs"])
        assert call(draws=need, handle=fresh) == 1  # CRK_ERR_ARG: no table yet
        assert lib.crk_wana_reserve(fresh, need - 1) == 0
        assert call(draws=need, handle=fresh) == 1
        assert lib.crk_wana_reserve(fresh, need) == 0
        assert call(draws=need, wsb=lib.crk_wana_d4c_workspace_bytes(1, sum(lens)) - 1, handle=fresh) == 1
        assert call(draws=need, handle=fresh) == 0
        assert lib.crk_wana_reserve(other, need) == 0
        assert call(draws=need, handle=other) == 3  # CRK_ERR_UNSUPPORTED
        assert lib.crk_wana_d4c_draws_per_frame(other) == -1
        torch.cuda.synchronize()
        assert torch.equal(t["ap"], an.d4c_batch(c["waves"], c["f0s"])[0])
    finally:
        lib.crk_wana_destroy(fresh)
        lib.crk_wana_destroy(other)


def test_silence_and_a_constant_signal_stay_finite_and_in_range():
    """The window holds only the 1e-12 noise (and the rounding of x w) once the mean is removed: nothing can be asked bin
    by bin, only that the table is an aperiodicity."""
    c = C.degenerate()
    an = _an(c)
    for ap, cap in zip(an.d4c_batch(c["waves"], c["f0s"]), an.codeap_batch(c["waves"], c["f0s"])):
        assert torch.isfinite(ap).all() and bool((ap > 0).all()) and bool((ap <= 1.0 - 1e-12).all())
        assert torch.isfinite(cap).all() and bool((cap <= 0).all())
        assert bool((ap[0] == 1.0 - 1e-12).all())


def test_refusals_before_any_launch():
    from crank_amd.world import WorldAnalyzer

    c = _cases()["ends"]
    an = _an(c)
    w, f = c["waves"][0], c["f0s"][0]
    for bad, msg in ((np.nan, "finite"), (np.inf, "finite"), (-1.0, "not negative"), (c["fs"] / 4.0 + 1.0, "fs / 4")):
        g = f.copy()
        g[3] = bad
        for fn in (an.d4c_batch, an.codeap_batch):
            with pytest.raises(ValueError, match=msg):
                fn([w], [g])
    with pytest.raises(ValueError, match="past the waveform's end"):
        an.d4c_batch([w[:100]], [f])
    for fs, size in ((44100, "4096"), (48000, "4096"), (8000, "1024")):
        with pytest.raises(ValueError, match=size):
            WorldAnalyzer(fs, 1024, 5.0).codeap_batch([w], [f])
    with pytest.raises(ValueError, match="no band"):
        WorldAnalyzer(8000, 1024, 5.0).code_aperiodicity_batch([torch.full((2, 513), 0.5)])


# ------------------------------------------------------------------------------------------------- end to end at 24 kHz
FS = 24000
FEATURE = dict(label="mcep", fs=FS, fftl=1024, win_length=1024, hop_size=120, window_types=["hann"], fmin=80, fmax=7600,
               mlfb_dim=80, n_iteration=100, shiftms=5, mcep_dim=34, mcep_alpha=0.466)
SPKR_CONF = {"SF1": {"minf0": 120, "maxf0": 400}, "TM1": {"minf0": 70, "maxf0": 300}}
UTTS = [("SF1", "E1", 0.30, 221.0), ("TM1", "E1", 0.50, 103.0), ("SF1", "E2", 0.43, 247.0), ("TM1", "E2", 0.36, 131.0)]


def _h5(spk, utt):
    return f"/feats/mcep/train/{spk}/{utt}.h5"


@functools.lru_cache(maxsize=None)
def corpus():
    from crank_amd.feature import Feature

    rng = np.random.default_rng(78)
    waves = [_harmonics(rng, np.linspace(f0, 1.1 * f0, int(sec * FS) + 3), FS) for _, _, sec, f0 in UTTS]
    flbls = [f"{s}/{u}" for s, u, _, _ in UTTS]
    store = Feature(FEATURE, "cuda").analyze_batch(waves, flbls, [SPKR_CONF[s] for s, *_ in UTTS])
    return waves, flbls, store


def test_the_store_files_cap_ccap_and_cap_uv_as_the_postprocessing_of_codeap_batch():
    from crank_amd.feature import Feature
    from crank_amd.world import WorldAnalyzer

    waves, flbls, store = corpus()
    store(flbls[0], ext="cap")  # without D4C the store's KeyError ends the test here
    from crank_amd.world import cap_postprocess_batch

    raws = [np.asarray(w, np.float32) for w in waves]
    an = WorldAnalyzer(FS, 1024, 5, "cuda")
    f0s, _ = an.analyze_batch(raws, [SPKR_CONF[s]["minf0"] for s, *_ in UTTS], [SPKR_CONF[s]["maxf0"] for s, *_ in UTTS], low_cut=70)
    caps = an.codeap_batch(raws, f0s, low_cut=70)
    post = cap_postprocess_batch(caps, "cuda")
    for lbl, cap0, (cap, ccap, cap_uv) in zip(flbls, caps, post):
        assert sorted(store.feats[lbl]) == sorted(["raw", "mlfb", "f0", "uv", "cf0", "lf0", "lcf0", "mcep", "npow", "cap",
                                                   "ccap", "cap_uv"])  # ap only with keep_ap
        T = store(lbl, ext="mcep").shape[0]
        for name, ref in (("cap", cap), ("ccap", ccap), ("cap_uv", cap_uv)):
            got = store(lbl, ext=name)
            assert got.dtype == torch.float32 and got.shape == (T, 3) and torch.equal(got, ref.to(torch.float32)), name
        # against the restatement of feature.py:98-107 on the same coded bands
        w_cap, w_ccap, w_uv = D.postprocess(cap0.cpu().numpy())
        assert np.array_equal(cap.cpu().numpy(), w_cap) and np.array_equal(cap_uv.cpu().numpy(), w_uv)
        err = float(np.abs(ccap.cpu().numpy() - w_ccap).max())
        print(f"{lbl}: ccap err {err:.3e} dB, cap range {float(cap.min()):.2f} .. {float(cap.max()):.2f} dB")
        assert err <= 4 * 2.0**-52 * float(np.abs(w_cap).max())  # one interpolation: a few roundings of the column's size
        assert bool((cap < -1.0).any())  # a harmonic signal is not reported as noise
    # ap on request, the table codeap_batch codes
    one = Feature(FEATURE, "cuda", keep_ap=True).analyze_batch(waves[:1], flbls[:1], [SPKR_CONF["SF1"]])
    ap = one(flbls[0], ext="ap")
    assert ap.dtype == torch.float32 and ap.shape == (store(flbls[0], ext="mcep").shape[0], 513)
    assert torch.equal(ap, an.d4c_batch(raws[:1], f0s[:1], low_cut=70)[0].to(torch.float32))


def test_an_mcep_dataset_builds_over_the_store_and_its_features_synthesise():
    from crank_amd.bin.extract_statistics import fit_scalers
    from crank_amd.net.trainer.dataset import BaseDataset
    from crank_amd.world import WorldSynthesizer, y_length

    waves, flbls, store = corpus()
    feats = {f"{s}_{u}": _h5(s, u) for s, u, _, _ in UTTS}
    fit_scp = {"feats": feats, "spkrs": ["SF1", "TM1"],
               "spk2utt": {sp: [f"{s}_{u}" for s, u, _, _ in UTTS if s == sp] for sp in ("SF1", "TM1")}}
    scaler = fit_scalers(store, fit_scp, {"feature": FEATURE})
    assert "mcep" in scaler
    scp = {"train": {"feats": feats, "spkrs": ["SF1", "TM1"]}}
    conf = {"batch_len": 60, "input_feat_type": "mcep", "output_feat_type": "mcep", "use_raw": False, "ignore_scaler": [],
            "use_mcep_0th": False, "spec_augment": False, "feature": FEATURE}

    def host_reader(h5f, ext="mlfb"):
        return store(h5f, ext=ext).cpu().numpy()

    on_device = BaseDataset(conf, scp, scaler, phase="train", reader=store)
    through_host = BaseDataset(conf, scp, scaler, phase="train", reader=host_reader)
    assert on_device.has_cap and on_device.lens == through_host.lens
    draws = [("TM1", 0), ("SF1", 13), ("TM1", 0), ("SF1", 0)]
    a, b = on_device.assemble([0, 1, 2, 3], draws=draws), through_host.assemble([0, 1, 2, 3], draws=draws)
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b) and "cap" in a
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert v.dtype == b[k].dtype and torch.equal(v, b[k]), k
        else:
            assert v == b[k], k
    syn = WorldSynthesizer(FS, 1024, 5.0, FEATURE["mcep_alpha"])
    for lbl in flbls:
        f0, mcep, cap = (store(lbl, ext=k) for k in ("f0", "mcep", "cap"))
        y = syn.synthesis(f0, mcep, cap)
        assert y.shape == (y_length(len(f0), FS, 5.0),) and torch.isfinite(y).all() and float(y.abs().max()) > 0
