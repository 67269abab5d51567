"""The D4C restatement (tests/d4c_ref.py) on the CPU: the spreads the GPU bounds are made of, its exact properties, its
integers by hand, a synthesis round trip, the recipe's post-processing and every refusal that needs no GPU."""
import numpy as np
import pytest

from tests import d4c_cases as C
from tests import d4c_ref as D
from tests import world_synth_ref as R

NAMES = sorted(C.SPREADS)

# mean over the interior voiced frames of |coded band - level| at 22050 Hz, worst band, as measured when this file was
# written: D4C on 40 synthesised frames recovers a level to a few dB
ROUND_TRIP = {-5.0: 5.390, -15.0: 4.395, -25.0: 2.703}


def test_cases_reach_their_edges_and_keep_away_from_the_threshold():
    facts = C.edges_reached()
    assert all(facts.values()), facts
    assert sorted(c["name"] for c in C.cases()) == NAMES
    for name in NAMES:
        m = C.threshold_margin(name)
        print(f"{name}: least |aperiodicity0 - 0.85| {m:.3e}")
        assert m >= C.MARGIN, name


@pytest.mark.parametrize("name", NAMES)
def test_recorded_spreads_are_reproduced(name):
    got = C.spread(name)
    for g, rec, what in zip(got, C.SPREADS[name], ("ap", "cap")):
        print(f"{name}: {what} spread {g:.3e} dB (recorded {rec:.3e})")
        assert g <= C.LIMIT
        assert g <= 2.0 * rec + 1e-15 and rec <= 2.0 * g + 1e-15


@pytest.mark.parametrize("name", NAMES)
def test_frames_outside_the_general_pass_are_exactly_one_minus_the_safeguard(name):
    aps, caps, det = C.reference(name)
    for ap, cap, d in zip(aps, caps, det):
        assert (ap[~d["passed"]] == 1.0 - 1e-12).all()
        assert (ap[d["passed"]][:, 0] == 1e-3).all() and (ap <= 1.0).all() and (ap > 0).all()  # a band clamped to 0 dB is 1.0 at its knot
        assert (cap <= 0.0).all()


def test_coding_inverts_decoding_where_the_knots_sit_on_bins():
    """At 16 and 24 kHz every 3 kHz knot is a bin of the 1024-point axis, so code(decode(cap)) is cap up to the rounding
    of 10^(x / 20) and 20 log10: 1e-12.  An unvoiced row decodes to 1 - 1e-12 on every bin and so codes to
    20 log10(1 - 1e-12) = -8.7e-12 dB, not to the 0 it was given: it is compared with that value, to the same 1e-12.
    (At 22050 Hz a knot lies between two bins on either side of a kink of the decoded curve, and the coded value is off by
    the kink's share: not a rounding matter, not asserted.)"""
    rng = np.random.default_rng(99)
    for fs in (16000, 24000):
        B = R.n_bands(fs)
        cap = -rng.uniform(1.0, 55.0, (50, B))
        cap[::7] = 0.0
        back = D.code_aperiodicity(R.decode_aperiodicity(cap, fs, 1024), fs)
        voiced = cap.sum(1) / B <= -0.5
        assert voiced.sum() == 42
        err = float(np.abs(back[voiced] - cap[voiced]).max())
        err_uv = float(np.abs(back[~voiced] - 20.0 * np.log10(1.0 - 1e-12)).max())
        print(f"fs {fs}: voiced rows {err:.3e} dB, unvoiced rows {err_uv:.3e} dB from 20 log10(1 - 1e-12)")
        assert err <= 1e-12 and err_uv <= 1e-12
    with pytest.raises(ValueError, match="no band"):
        D.code_aperiodicity(np.full((2, 513), 0.5), 8000)


@pytest.mark.parametrize("level", sorted(ROUND_TRIP))
def test_round_trip_through_the_synthesis_restatement(level):
    """A guard against later edits, not a quality claim: 1.5 x the recorded deviation."""
    rng = np.random.default_rng(515)
    y, f0 = C.vowel(rng, 40, 22050, 5.0, level)
    ap, d = D.d4c(y, f0, 22050, 5.0, detail=True)
    cap = D.code_aperiodicity(ap, 22050)
    sel = np.zeros(40, bool)
    sel[8:32] = True
    sel &= f0 != 0
    assert d["passed"][sel].all()
    dev = float(np.abs(cap[sel].mean(0) - level).max())
    print(f"level {level} dB: bands come back at {np.round(cap[sel].mean(0), 2)}, deviation {dev:.3f} dB")
    assert dev <= 1.5 * ROUND_TRIP[level]


def test_frame_integers_and_draw_counts_by_hand():
    # fs 16000, 5 ms: 1.5 fs / 40 = 600, 2 fs / 47 = 680.85, 1.5 fs / 47 = 510.6, 1.5 fs / 100 = 240, 2 fs / 100 = 320
    f0 = np.array([40.0, 47.0, 0.0, 100.0, np.nextafter(40.0, 0.0), 30.0])
    sh = D.frame_shapes(f0, 16000, 5.0)
    assert sh["origin"].tolist() == [0, 80, 160, 240, 320, 400]
    assert sh["half_lt"].tolist() == [600, 511, 0, 240, 600, 600]
    assert sh["half_gb"].tolist() == [681, 681, 0, 320, 681, 681]
    # t -+ 1 / (4 * 47) = -+ 85.106 samples, -+ 40 samples at 100 Hz; the 0.001 breaks the tie upwards
    assert sh["origin_c1"].tolist() == [-85, -5, 0, 200, 235, 315]
    assert sh["origin_c2"].tolist() == [85, 165, 0, 280, 405, 485]
    assert sh["dc_limit"].tolist() == [8, 8, 0, 14, 8, 8]  # 2 + int(47 * 2048 / 16000 = 6.016), 2 + int(12.8)
    assert sh["bound_half"].tolist() == [4, 4, 0, 7, 4, 4] and sh["bound_full"].tolist() == [7, 7, 0, 13, 7, 7]
    assert sh["lt_offset"].tolist() == [0, 1201, 2224, 2224, 2705, 3906] and sh["lt_draws"] == 5107
    off, total = D.general_offsets(sh, np.array([True, True, False, True, False, True]))
    assert off.tolist() == [5107, 9196, 13285, 13285, 15208, 15208] and total == 15208 + 4089
    assert D.draws_per_frame(16000) == 1201 + 4089 and D.draws_per_frame(24000) == 1801 + 3 * 2043
    # one ulp either side of a rounding point of each half window
    for c, key, h in ((1.5, "half_lt", 100), (2.0, "half_gb", 300)):
        f = c * 22050 / (h + 0.5)
        got = D.frame_shapes(np.array([np.nextafter(f, 1e9), np.nextafter(f, 0.0)]), 22050, 5.0)[key].tolist()
        assert got == [h, h + 1]
    assert D.fft_sizes(13640) == (2048, 2048) and D.fft_sizes(24052) == (2048, 2048)
    assert D.fft_sizes(13639)[0] == 1024 and D.fft_sizes(24053)[1] == 4096
    from crank_amd import world

    for fs in (13640, 16000, 22050, 24000, 24052):
        assert world.d4c_draws_per_frame(fs) == D.draws_per_frame(fs) and world.d4c_fft_sizes(fs) == D.fft_sizes(fs)
    assert (world.D4C_FS_MIN, world.D4C_FS_MAX, world.D4C_FFT) == (D.FS_MIN, D.FS_MAX, D.FFT)


def test_postprocessing_is_the_recipes():
    """feature.py:98-107 through tests/harvest_ref.continuous_f0, which tests/golden/continuous_f0.npz pins to the
    reference's own convert_continuos_f0."""
    u = 20.0 * np.log10(1.0 - 1e-12)  # what an unvoiced frame codes to
    cap = np.array([[u, u], [-20.0, -12.0], [u, u], [u, 0.0], [-10.0, -8.0], [u, u]])
    out, ccap, uv = D.postprocess(cap)
    assert np.array_equal(cap[:, 0], [u, -20.0, u, u, -10.0, u])  # the input is not touched
    # column 0: its maximum is the unvoiced value, which is zeroed; the ends are filled in place
    assert out[:, 0].tolist() == [-20.0, -20.0, 0.0, 0.0, -10.0, -10.0] and uv[:, 0].tolist() == [0, 1, 0, 0, 1, 0]
    assert np.allclose(ccap[:, 0], [-20.0, -20.0, -20.0 + 10.0 / 3, -20.0 + 20.0 / 3, -10.0, -10.0], rtol=0, atol=1e-14)
    # column 1: a voiced frame clamped to 0 dB is the maximum, so the unvoiced frames are NOT zeroed and count as voiced
    assert out[:, 1].tolist() == [u, -12.0, u, 0.0, -8.0, u] and uv[:, 1].tolist() == [1, 1, 1, 0, 1, 1]
    assert np.allclose(ccap[:, 1], [u, -12.0, u, (u - 8.0) / 2, -8.0, u], rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="no voiced frame"):
        D.postprocess(np.full((4, 1), u))


def test_refusals_that_need_no_gpu():
    from crank_amd import world

    for fs, size in ((44100, 4096), (48000, 4096), (8000, 1024), (13639, 1024), (24053, 4096)):
        with pytest.raises(ValueError, match=f"{size}-point"):
            world.check_d4c_fs(fs)
        with pytest.raises(ValueError, match=f"{size}-point"):
            D.check_fs(fs)
        an = world.WorldAnalyzer(fs, 1024, 5.0, "cpu")
        for fn in (an.d4c_batch, an.codeap_batch):
            with pytest.raises(ValueError, match=f"{size}-point"):
                fn([np.zeros(100)], [np.zeros(2)])
        with pytest.raises(ValueError, match=f"{size}-point"):
            an.analyze_batch([np.zeros(100)], [70.0], [300.0], return_ap=True)
    for fs in (13640, 16000, 24052):
        world.check_d4c_fs(fs)
        D.check_fs(fs)
    with pytest.raises(ValueError, match="no band"):
        world.WorldAnalyzer(8000, 1024, 5.0, "cpu").code_aperiodicity_batch([np.full((2, 513), 0.5)])
    an = world.WorldAnalyzer(22050, 1024, 5.0, "cpu")
    with pytest.raises(ValueError, match="same non-zero length"):
        an.d4c_batch([np.zeros(100)], [])
    with pytest.raises(ValueError, match="past the waveform's end"):
        an.codeap_batch([np.zeros(100)], [np.full(9, 100.0)])
    with pytest.raises(ValueError, match="threshold"):
        an.d4c_batch([np.zeros(100)], [np.zeros(1)], threshold=float("nan"))
    with pytest.raises(ValueError):
        D.d4c(np.zeros(100), np.zeros(2), 48000, 5.0)
