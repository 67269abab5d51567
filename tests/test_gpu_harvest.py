"""Harvest F0 estimation on the device (crank_amd.world.HarvestF0, crk_f0_*) against the float64 restatement
tests/harvest_ref.py, stage by stage and end to end, on the cases of tests/harvest_cases.py.

The bounds are 10 x the spread between the restatement's own two evaluation orders (harvest_cases.RECORDED, recomputed by
tests/test_harvest_cpu.py) plus the floors the stages were given: 1e-15 of the peak for the decimated signal, 1e-12
relative for raw and refined F0, 1e-9 relative for scores.  The contour stage, fed the restatement's tables, is held to
identical voicing and 1e-12; the whole chain to identical voicing and 1e-6.  Parity with pyworld is unpinned.
"""
import numpy as np
import pytest
import torch

from tests import harvest_cases as C
from tests import harvest_ref as H

pytestmark = pytest.mark.gpu

NAMES = list(C.cases())
_HANDLES = {}


def _hf(case):
    from crank_amd.world import HarvestF0

    key = (case["fs"], case["shiftms"])
    if key not in _HANDLES:
        _HANDLES[key] = HarvestF0(case["fs"], case["shiftms"], "cuda")
    return _HANDLES[key]


def _args(case):
    return ([w["x"] for w in case["utts"]], [w["minf0"] for w in case["utts"]], [w["maxf0"] for w in case["utts"]])


def _np(t):
    return t.cpu().numpy()


def _stages(name):
    """The restatement's stages per utterance: computed once (harvest_cases caches them read-only), copied for upload."""
    return [{k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in C.stages(name, u).items()}
            for u in range(len(C.cases()[name]["utts"]))]


@pytest.mark.parametrize("name", NAMES)
def test_decimation(name):
    case = C.cases()[name]
    got = _hf(case).decimate_batch(*_args(case))
    for g, st in zip(got, _stages(name)):
        g, ref = _np(g), st["yd"]
        assert g.shape == ref.shape
        peak = np.max(np.abs(ref))
        err, bound = np.max(np.abs(g - ref)), (10.0 * C.RECORDED[name]["s_dec"] + 1e-15) * peak
        print(f"{name}: r {st['cfg']['r']} decimated worst {err:.3e} bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("name", NAMES)
def test_raw_candidates(name):
    case = C.cases()[name]
    sts = _stages(name)
    got = _hf(case).raw_candidates_batch(*_args(case), decimated=[st["yd"] for st in sts])
    for g, st in zip(got, sts):
        g, ref, avg, cfg = _np(g), st["raw"], st["raw_average"], st["cfg"]
        assert g.shape == ref.shape
        both = (g != 0) & (ref != 0)
        err = np.max(np.abs(g[both] - ref[both]) / ref[both]) if both.any() else 0.0
        bound = 10.0 * C.RECORDED[name]["s_raw"] + 1e-12
        flips = np.argwhere((g != 0) != (ref != 0))
        print(f"{name}: raw worst {err:.3e} bound {bound:.3e} filled {int(both.sum())} flips {len(flips)} of {ref.size}")
        assert err <= bound
        for c, i in flips:  # only where the restatement's own average sits on one of its limits
            lim = np.array([0.9 * cfg["bf"][c], 1.1 * cfg["bf"][c], cfg["floor"], cfg["ceil"]])
            assert np.min(np.abs(avg[c, i] - lim) / lim) <= 1e-9, (c, i, avg[c, i], g[c, i])
        assert len(flips) <= 1e-3 * ref.size


def test_run_detection_and_overlap():
    """Runs of exactly 9 and 10 channels, runs touching the forced-empty first and last channel, 16 runs in one frame and
    the overlap at both ends of the utterance: equal to the restatement bit for bit (the mean is one ordered sum)."""
    from crank_amd.world import HarvestF0

    r = C.RAW_TABLE
    raw = C.raw_table()
    hf = HarvestF0(r["fs"], 5, "cuda")
    got = _np(hf.candidates_batch([np.zeros(r["samples"])], [r["minf0"]], [r["maxf0"]], [raw])[0])
    assert np.array_equal(got, H.overlap(H.official_candidates(raw)))
    for name in ("const_16k", "ragged_16k"):
        case = C.cases()[name]
        sts = _stages(name)
        got = _hf(case).candidates_batch(*_args(case), [st["raw"] for st in sts])
        for g, st in zip(got, sts):
            assert np.array_equal(_np(g), st["cands"])


@pytest.mark.parametrize("name", NAMES)
def test_refinement(name):
    case = C.cases()[name]
    sts = _stages(name)
    got = _hf(case).refine_batch(*_args(case), [st["cands"] for st in sts])
    for (gr, gs), st in zip(got, sts):
        gr, gs = _np(gr), _np(gs)
        live = st["refined"] != 0
        assert np.array_equal(gr != 0, live) and np.array_equal(gs != 0, live)
        if not live.any():
            continue
        e_ref = np.max(np.abs(gr[live] - st["refined"][live]) / st["refined"][live])
        e_sc = np.max(np.abs(gs[live] - st["scores"][live]) / st["scores"][live])
        b_ref, b_sc = 10.0 * C.RECORDED[name]["s_ref"] + 1e-12, 10.0 * C.RECORDED[name]["s_score"] + 1e-9
        print(f"{name}: refined worst {e_ref:.3e} bound {b_ref:.3e}; score worst {e_sc:.3e} bound {b_sc:.3e}; "
              f"live {int(live.sum())}")
        assert e_ref <= b_ref and e_sc <= b_sc


def _same_contour(got, ref, what):
    assert got.shape == ref.shape
    assert np.array_equal(got != 0, ref != 0), (what, np.nonzero((got != 0) != (ref != 0))[0])
    v = ref != 0
    err = np.max(np.abs(got[v] - ref[v]) / ref[v]) if v.any() else 0.0
    print(f"{what}: contour worst {err:.3e}, {int(v.sum())} voiced of {len(ref)}")
    return err


@pytest.mark.parametrize("name", NAMES)
def test_contour(name):
    case = C.cases()[name]
    sts = _stages(name)
    got = _hf(case).contour_batch(*_args(case), [st["refined"] for st in sts], [st["scores"] for st in sts])
    for g, st in zip(got, sts):
        assert _same_contour(_np(g), st["f1"], name) <= 1e-12


def test_contour_structure():
    """The hand-built tables: an 8-frame gap bridged and a 9-frame gap left open, a 5-frame run dropped and a 6-frame run
    kept and grown, two runs merged by score, a lone candidate removed."""
    from crank_amd.world import HarvestF0

    assert C.edges_reached()
    c, s, e = C.contour_tables()
    n = (e["T"] - 1) * 8  # int(1000 n / 8000) + 1 = T frames
    hf = HarvestF0(8000, 5, "cuda")
    got = _np(hf.contour_batch([np.zeros(n)], [70], [400], [c], [s])[0])
    assert _same_contour(got, H.contour(c, s), "structure") <= 1e-12
    # in a ragged batch, behind an utterance of another length
    case = C.cases()["gap_8k"]
    st = _stages("gap_8k")[0]
    got = hf.contour_batch([case["utts"][0]["x"], np.zeros(n)], [70, 70], [400, 400], [st["refined"], c], [st["scores"], s])
    assert _same_contour(_np(got[0]), st["f1"], "batch row 0") <= 1e-12
    assert _same_contour(_np(got[1]), H.contour(c, s), "batch row 1") <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end(name):
    case = C.cases()[name]
    hf = _hf(case)
    got = hf.harvest_batch(*_args(case))
    for g, st in zip(got, _stages(name)):
        assert g.dtype == torch.float64
        assert _same_contour(_np(g), st["f0"], name) <= 1e-6
    again = hf.harvest_batch(*_args(case))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    if len(case["utts"]) > 1:  # a ragged batch equals its rows run alone, bit for bit
        for u, w in enumerate(case["utts"]):
            assert torch.equal(hf.harvest(w["x"], w["minf0"], w["maxf0"]), got[u])


def test_silence_is_unvoiced():
    case = C.cases()["gap_8k"]
    f0 = _hf(case).harvest(np.zeros(4000), 70, 400)
    assert f0.shape == (101,) and not bool(f0.any())


def test_continuous_f0_against_the_reference_fixture():
    import os

    from crank_amd.world import continuous_f0_batch

    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "continuous_f0.npz"))
    n = len([k for k in d.files if k.startswith("in_")])
    outs = continuous_f0_batch([d[f"in_{k}"] for k in range(n)], return_filled=True)
    for k, (uv, cf0, lf0, lcf0, filled) in enumerate(outs):
        assert uv.dtype == torch.float32 and np.array_equal(_np(uv), d[f"uv_{k}"])
        assert np.array_equal(_np(filled), d[f"f0_{k}"])
        for got, key in ((cf0, "cf0"), (lf0, "lf0"), (lcf0, "lcf0")):
            ref = d[f"{key}_{k}"]
            assert np.all(np.abs(_np(got) - ref) <= 4 * np.spacing(np.abs(ref))), (k, key)
    with pytest.raises(ValueError):
        continuous_f0_batch([d["in_0"], np.zeros(12)])


def test_mcd_from_waveforms_reestimates_f0():
    """cv_f0s=None re-estimates the contour as the reference does: the same MCD as the call given analyze_batch's F0."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw_from_waveforms
    from crank_amd.world import WorldAnalyzer

    case = C.cases()["vowel_22k"]
    conf = dict(feature=dict(fs=22050, fftl=1024, shiftms=5, mcep_dim=24, mcep_alpha=0.455))
    y = case["utts"][0]["x"]
    ana = WorldAnalyzer(22050, 1024, 5, "cuda")
    f0s, sps = ana.analyze_batch([y], [70], [400])
    assert int((f0s[0] > 0).sum()) > 40 and sps[0].shape == (f0s[0].numel(), 513)
    rng = np.random.default_rng(3)
    gt = [rng.standard_normal((60, 25)) * 0.1]
    gtf = [np.full(60, 150.0)]
    a = mcd_fastdtw_from_waveforms([y], None, gt, gtf, conf, f0_ranges=[(70, 400)], analyzer=ana)
    b = mcd_fastdtw_from_waveforms([y], f0s, gt, gtf, conf, analyzer=ana)
    assert a == b and np.isfinite(a[0])
    with pytest.raises(ValueError):
        mcd_fastdtw_from_waveforms([y], None, gt, gtf, conf, analyzer=ana)


def test_envelope_and_reservation():
    from crank_amd import _lib
    from crank_amd.world import HarvestF0, WorldAnalyzer

    for fs, shift in ((7999, 5), (48001, 5), (16000, 5.5), (16000, 0)):
        with pytest.raises(ValueError):
            HarvestF0(fs, shift, "cuda")
    hf = HarvestF0(16000, 5, "cuda")
    x = np.zeros(4000)
    for lo, hi in ((39.9, 400), (70, 800.5), (400, 70), (float("nan"), 400)):
        with pytest.raises(ValueError):
            hf.harvest(x, lo, hi)
    with pytest.raises(ValueError):
        hf.harvest(np.zeros(63), 70, 400)
    with pytest.raises(ValueError):
        WorldAnalyzer(16000, 1024, 5.5, "cuda").analyze_batch([x], [70], [400])
    # an undersized workspace or event reservation is refused, not run
    L = hf._batch([x], [70], [400])
    f0 = torch.empty(L["O"], dtype=torch.float64, device="cuda")
    status = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = hf._ws

    def call(events, ws_bytes):
        return _lib.lib().crk_f0_harvest(hf._h, L["x"].data_ptr(), L["utt"].data_ptr(), L["range"].data_ptr(),
                                         L["chan_bf"].data_ptr(), L["chan"].data_ptr(), 1, L["S"], L["C"], L["F"], events,
                                         L["O"], f0.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                                         _lib.stream_ptr())

    need = _lib.lib().crk_f0_workspace_bytes(1, L["S"], L["F"], L["C"])
    assert call(L["E"], need - 1) == 1 and call(hf._events + 1, need) == 1 and call(L["E"], need) == 0
    torch.cuda.synchronize()
