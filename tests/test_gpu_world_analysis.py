"""crank_amd.world.WorldAnalyzer (csrc/world_analysis_kernels.hip, all float64) against the CPU restatement
tests/world_analysis_ref.py on the cases of tests/world_analysis_cases.py.  The bounds are 10 x the case's own spread of
the restatement (two FFTs) plus 1e-12, derived on the CPU (test_world_analysis_cpu.py); no frame and no bin is masked
out.  The restatement's parity against pyworld / pysptk / sprocket is unpinned (none of them is installed)."""
import functools

import numpy as np
import pytest
import torch

from tests import world_analysis_cases as C
from tests import world_analysis_ref as A

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases():
    cs = C.cases()
    facts = C.edges_reached(cs)  # on the host, before anything runs on the GPU
    assert all(facts.values()), facts
    return {c["name"]: c for c in cs}


@functools.lru_cache(maxsize=None)
def _reference(name):
    return C.reference(_cases()[name])


def _analyzer(c):
    from crank_amd.world import WorldAnalyzer

    return WorldAnalyzer(c["fs"], 1024, c["shiftms"])


NAMES = sorted(C.SPREADS)


def test_low_cut_matches_the_restatement_at_every_tile_edge():
    from crank_amd import _lib
    from crank_amd.world import WorldAnalyzer

    assert _lib.lib().crk_wana_lowcut_tile() == C.LOWCUT_TILE
    rng = np.random.default_rng(11)
    for fs in (22050, 16000, 48000):
        waves = [rng.standard_normal(n) * 0.3 for n in C.lowcut_lengths()]
        got = WorldAnalyzer(fs, 1024, 5.0).low_cut_batch(waves, 70)
        for w, g in zip(waves, got):
            want = A.low_cut_filter(w.astype(np.float32), fs, 70)
            g = g.cpu().numpy()
            assert g.dtype == np.float64 and g.shape == want.shape
            err = np.linalg.norm(g - want) / np.linalg.norm(want)
            print(f"low cut fs {fs} n {len(w)}: rel l2 {err:.3e}")
            assert err <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_frame_shapes_equal_the_restatements_integers(name):
    c = _cases()[name]
    got = _analyzer(c).frame_shapes_batch(c["f0s"])
    for f0, g in zip(c["f0s"], got):
        want = A.frame_shapes(f0, c["fs"], c["shiftms"])
        for key in ("origin", "half", "dc_limit", "boundary", "offset"):
            assert np.array_equal(g[key], want[key]), (name, key)


@pytest.mark.parametrize("name", NAMES)
def test_envelope_and_mel_cepstrum_within_the_cases_own_spread(name):
    c = _cases()[name]
    b_sp, b_mc = C.bounds(name)
    an = _analyzer(c)
    sps = an.cheaptrick_batch(c["waves"], c["f0s"])
    mcs, sps2 = an.mcep_batch(c["waves"], c["f0s"], c["dim"], c["alpha"], low_cut=None, return_sp=True)
    w_sps, w_mcs = _reference(name)
    e_sp = e_mc = 0.0
    for sp, sp2, mc, w_sp, w_mc in zip(sps, sps2, mcs, w_sps, w_mcs):
        sp, mc = sp.cpu().numpy(), mc.cpu().numpy()
        assert sp.shape == w_sp.shape and mc.shape == w_mc.shape
        assert np.isfinite(sp).all() and (sp > 0).all() and np.isfinite(mc).all()
        assert np.array_equal(sp, sp2.cpu().numpy())  # the envelope does not depend on the entry that made it
        e_sp = max(e_sp, float(np.abs(np.log(sp) - np.log(w_sp)).max()))
        e_mc = max(e_mc, float(np.abs(mc - w_mc).max()))
    print(f"{name}: log sp err {e_sp:.3e} (bound {b_sp:.3e}), mcep err {e_mc:.3e} (bound {b_mc:.3e})")
    assert e_sp <= b_sp
    assert e_mc <= b_mc


@pytest.mark.parametrize("name", ["vowel", "silence", "mixed", "ragged", "voicing"])
def test_npow_matches_the_restatement(name):
    c = _cases()[name]
    got = _analyzer(c).npow_batch(c["waves"], c["f0s"])
    for g, w_sp in zip(got, _reference(name)[0]):
        err = float(np.abs(g.cpu().numpy() - A.spc2npow(w_sp)).max())
        print(f"{name}: npow err {err:.3e} dB")
        assert err <= 1e-9


def test_full_chain_with_low_cut_matches_analyze_mcep():
    c = _cases()["vowel"]
    _, b_mc = C.bounds("vowel")
    got = _analyzer(c).analyze_mcep(c["waves"][0], c["f0s"][0], 34, 0.455, low_cut=70).cpu().numpy()
    want = A.analyze_mcep(c["waves"][0], c["f0s"][0], c["fs"], 1024, c["shiftms"], 34, 0.455)
    err = float(np.abs(got - want).max())
    print(f"analyze_mcep err {err:.3e} (bound {b_mc:.3e})")
    assert err <= b_mc


def test_constant_signal_stays_positive_and_finite():
    """A 1-sample utterance and a constant one: every window sees a constant, which the mean removal cancels; what is
    left is the randn noise plus the rounding of the products, so the envelope is compared for its order of magnitude
    (the restatement's, within a factor of 2 per bin: both are the 1e-24 noise floor smoothed) and not bin by bin."""
    from crank_amd.world import WorldAnalyzer

    an = WorldAnalyzer(22050, 1024, 5.0)
    waves, f0s = [np.array([0.25]), np.full(3000, -0.7)], [np.array([100.0]), np.array([0.0, 150.0, 300.0, 0.0])]
    sps = an.cheaptrick_batch(waves, f0s)
    mcs = an.mcep_batch(waves, f0s, 34, 0.455)
    for w, f, sp, mc in zip(waves, f0s, sps, mcs):
        sp = sp.cpu().numpy()
        assert np.isfinite(sp).all() and (sp > 0).all() and torch.isfinite(mc).all()
        ratio = sp / A.cheaptrick(w, f, 22050, 5.0)
        print(f"constant signal of {len(w)} samples: sp / restatement in [{ratio.min():.6f}, {ratio.max():.6f}]")
        assert 0.5 < ratio.min() and ratio.max() < 2.0


def test_ragged_batch_and_repeated_call_are_bit_identical_to_single_calls():
    c = _cases()["ragged"]
    an = _analyzer(c)
    mcs, sps = an.mcep_batch(c["waves"], c["f0s"], 34, 0.455, low_cut=70, return_sp=True)
    mcs2, sps2 = an.mcep_batch(c["waves"], c["f0s"], 34, 0.455, low_cut=70, return_sp=True)
    npw = an.npow_batch(c["waves"], c["f0s"])
    for i, (w, f) in enumerate(zip(c["waves"], c["f0s"])):
        assert torch.equal(mcs[i], mcs2[i]) and torch.equal(sps[i], sps2[i])
        one_mc, one_sp = an.mcep_batch([w], [f], 34, 0.455, low_cut=70, return_sp=True)
        assert torch.equal(one_mc[0], mcs[i]) and torch.equal(one_sp[0], sps[i])
        assert torch.equal(an.npow_batch([w], [f])[0], npw[i])
    # and in another order
    rev = an.mcep_batch(c["waves"][::-1], c["f0s"][::-1], 34, 0.455, low_cut=70)
    assert all(torch.equal(a, b) for a, b in zip(rev[::-1], mcs))


def test_device_inputs_and_bad_f0_values():
    c = _cases()["vowel"]
    an = _analyzer(c)
    w = torch.as_tensor(c["waves"][0], device="cuda")
    f = torch.as_tensor(c["f0s"][0], device="cuda")
    assert torch.equal(an.cheaptrick_batch([w], [f])[0], an.cheaptrick_batch(c["waves"], c["f0s"])[0])
    for bad, msg in ((np.nan, "finite"), (-1.0, "not negative"), (c["fs"] / 4.0 + 1.0, "fs / 4")):
        g = f.clone()
        g[3] = bad
        with pytest.raises(ValueError, match=msg):
            an.cheaptrick_batch([w], [g])


def test_mcd_from_waveforms_matches_restatement_analysis_and_the_oracle_dtw():
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw_from_waveforms
    from oracle import mcd as O

    pairs = C.mcd_pairs()
    assert len(pairs) == 6 and len({len(p[1]) for p in pairs}) > 1
    assert all((p[1] > 0).sum() >= 20 and (p[3] > 0).sum() >= 20 for p in pairs)
    conf = {"feature": {"fs": 22050, "fftl": 1024, "shiftms": 5.0, "mcep_dim": 34, "mcep_alpha": 0.455}}
    waves, f0s, gmcs, gf0s = (list(x) for x in zip(*pairs))
    vals, paths = mcd_fastdtw_from_waveforms(waves, f0s, gmcs, gf0s, conf, return_paths=True)
    assert vals == mcd_fastdtw_from_waveforms([torch.as_tensor(w, device="cuda") for w in waves], f0s, gmcs, gf0s, conf)
    for i, (y, f0, gmc, gf0) in enumerate(pairs):
        cv = A.analyze_mcep(y, f0, 22050, 1024, 5.0, 34, 0.455)
        want, want_path = O.mcd(cv, f0, gmc, gf0, radius=1)
        assert np.array_equal(np.asarray(paths[i]), np.asarray(want_path).reshape(-1, 2)), i
        print(f"pair {i}: MCD {vals[i]:.6f} dB, oracle {want:.6f} dB")
        assert abs(vals[i] - want) <= 1e-9 * abs(want)


def test_compute_entries_never_allocate_and_refuse_an_unreserved_table():
    from crank_amd import _lib
    from crank_amd._lib import stream_ptr

    c = _cases()["ragged"]
    an = _analyzer(c)
    lib = _lib.lib()
    an.mcep_batch(c["waves"], c["f0s"], 34, 0.455, low_cut=70)  # reserves and warms up
    an.npow_batch(c["waves"], c["f0s"])
    an.frame_shapes_batch(c["f0s"])
    torch.cuda.synchronize()
    before = lib.crk_debug_alloc_count()
    an.mcep_batch(c["waves"], c["f0s"], 34, 0.455, low_cut=70)
    an.cheaptrick_batch(c["waves"], c["f0s"])
    an.npow_batch(c["waves"], c["f0s"])
    an.frame_shapes_batch(c["f0s"])
    torch.cuda.synchronize()
    assert lib.crk_debug_alloc_count() == before
    # a fresh handle has no randn table; one reserved for 10 draws refuses a call that states 5000
    h = lib.crk_wana_create(22050, 1024, 5.0, 0.455, 35)
    assert h
    try:
        x = torch.zeros(1000, dtype=torch.float64, device="cuda")
        f0 = torch.full((3,), 100.0, dtype=torch.float64, device="cuda")
        foff = torch.tensor([0, 3], dtype=torch.int64, device="cuda")
        soff = torch.tensor([0, 1000], dtype=torch.int64, device="cuda")
        sp = torch.empty(3, 513, dtype=torch.float64, device="cuda")
        mc = torch.empty(3, 35, dtype=torch.float64, device="cuda")
        nbytes = lib.crk_wana_workspace_bytes(1, 3, 1000)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def cheaptrick(draws, wsb=nbytes):
            return lib.crk_wana_cheaptrick(h, x.data_ptr(), f0.data_ptr(), foff.data_ptr(), soff.data_ptr(), 1, 3, 1000, draws,
                                           sp.data_ptr(), ws.data_ptr(), wsb, stream_ptr())

        assert cheaptrick(5000) == 1  # CRK_ERR_ARG
        assert lib.crk_wana_reserve(h, 10) == 0
        assert cheaptrick(5000) == 1
        assert lib.crk_wana_mcep(h, x.data_ptr(), f0.data_ptr(), foff.data_ptr(), soff.data_ptr(), 1, 3, 1000, 5000, 35,
                                 mc.data_ptr(), None, ws.data_ptr(), nbytes, stream_ptr()) == 1
        assert lib.crk_wana_reserve(h, 5000) == 0
        assert cheaptrick(5000, nbytes - 1) == 1  # a workspace too small
        assert cheaptrick(5000) == 0
        assert lib.crk_wana_mcep(h, x.data_ptr(), f0.data_ptr(), foff.data_ptr(), soff.data_ptr(), 1, 3, 1000, 5000, 25,
                                 mc.data_ptr(), None, ws.data_ptr(), nbytes, stream_ptr()) == 3  # another order: unsupported
        torch.cuda.synchronize()
        assert torch.isfinite(sp).all()
    finally:
        lib.crk_wana_destroy(h)
    assert not lib.crk_wana_create(22050, 2048, 5.0, 0.455, 35)
    assert not lib.crk_wana_create(22050, 1024, 5.0, 0.455, 129)


def test_eval_output_helper_feeds_vocoder_waveforms_to_the_analysis():
    c = _cases()["ragged"]
    an = _analyzer(c)
    waves = [torch.as_tensor(w, device="cuda") for w in c["waves"][2:]]
    outputs = [{"f0": torch.as_tensor(f, device="cuda").reshape(-1, 1)} for f in c["f0s"][2:]]
    got = an.mcep_of_eval_outputs(waves, outputs, 34, 0.455)
    want = an.mcep_batch(c["waves"][2:], c["f0s"][2:], 34, 0.455, low_cut=70)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    both = an.mcep_of_eval_outputs({"a": waves, "b": waves[:1]}, {"a": outputs, "b": outputs[:1]}, 34, 0.455)
    assert torch.equal(both["b"][0], want[0]) and len(both["a"]) == len(want)
