"""Properties of the CPU restatement tests/world_synth_ref.py (the oracle of the WORLD synthesis kernels), so that the
oracle is not trusted blindly, and the refusals of crank_amd.world that need no device.  Parity with pyworld / pysptk
/ sprocket is unpinned (none of them is installed)."""
import math

import numpy as np
import pytest

from tests import world_synth_ref as R
from tests.world_inputs import utterance


def _mc(rng, T, m1, scale=0.5):
    mc = rng.standard_normal((T, m1)) * scale * 0.6 ** np.arange(m1)
    mc[:, 0] -= 2.0
    return mc


def test_freqt_identity_at_alpha_zero_and_inverse():
    rng = np.random.default_rng(0)
    c = _mc(rng, 3, 25)
    assert np.array_equal(R.freqt(c, 24, 0.0), c)
    back = R.freqt(R.freqt(c, 400, 0.42), 24, -0.42)
    assert np.abs(back - c).max() <= 1e-10


def test_mc2sp_at_alpha_zero_is_exp_of_twice_the_dft():
    rng = np.random.default_rng(1)
    c = _mc(rng, 2, 30)
    N = 1024
    sp = R.mc2sp(c, 0.0, N)
    k = np.arange(N // 2 + 1)
    for t in range(2):
        dft = sum(c[t, n] * np.cos(2 * np.pi * k * n / N) for n in range(30))
        assert np.allclose(sp[t], np.exp(2 * dft), rtol=1e-12, atol=0)


def test_mc2e_is_the_energy_of_the_exponentiated_cepstrum():
    rng = np.random.default_rng(2)
    mc = _mc(rng, 3, 35, 0.3)
    e = R.mc2e(mc, 0.455)
    L = 1 << 16
    c = R.freqt(mc, 4096, -0.455)
    for t in range(3):
        full = np.zeros(L)
        full[:4097] = c[t]
        h = np.fft.irfft(np.exp(np.fft.rfft(full)), L)  # the minimum-phase impulse response, alias-free at this length
        assert abs(e[t] / (h[:R.IRLEN] ** 2).sum() - 1) < 1e-9


def test_power_modification_matches_energies():
    rng = np.random.default_rng(3)
    mc, rm = _mc(rng, 4, 35, 0.3), _mc(rng, 4, 35, 0.3)
    mod = R.mod_power(mc, rm, 0.455)
    assert np.array_equal(mod[:, 1:], mc[:, 1:])
    assert np.abs(R.mc2e(mod, 0.455) / R.mc2e(rm, 0.455) - 1).max() < 1e-12


def test_decoded_aperiodicity_knots_and_unvoiced_frames():
    assert [R.n_bands(fs) for fs in (16000, 22050, 24000)] == [1, 2, 3]
    fs, N = 24000, 1024
    cap = np.array([[-20.0, -12.0, -5.0], [0.0, 0.0, 0.0]])
    ap = R.decode_aperiodicity(cap, fs, N)
    assert np.all(ap[1] == 1.0 - 1e-12)
    fk = fs / N * np.arange(N // 2 + 1)
    assert ap[0, 0] == pytest.approx(10 ** (-60 / 20), rel=1e-12)
    assert ap[0, -1] == pytest.approx(10 ** (-1e-12 / 20), rel=1e-12)
    for b, v in enumerate(cap[0], 1):  # bins on either side of the knot interpolate towards 10^(v/20)
        i = int(np.searchsorted(fk, 3000.0 * b))
        lo, hi = np.log10(ap[0, i - 1]) * 20, np.log10(ap[0, i]) * 20
        w = (3000.0 * b - fk[i - 1]) / (fk[i] - fk[i - 1])
        assert lo + w * (hi - lo) == pytest.approx(v, abs=1e-9)


@pytest.mark.parametrize("F", [100.0, 173.0, 240.0])
def test_constant_f0_pulse_spacing_and_shifts(F):
    fs = 22050
    pos, shift, vuv, ylen = R.time_base(np.full(60, F), fs, 1024, 10.0)
    d = np.diff(pos)
    assert np.all(np.abs(d - fs / F) <= 1.0)
    assert np.all(vuv == 1.0)
    assert np.all((shift >= 0) & (shift < 1.0 / fs))
    pos, shift, vuv, _ = R.time_base(np.zeros(60), fs, 1024, 10.0)
    assert np.all(np.abs(np.diff(pos) - fs / 500.0) <= 1.0) and np.all(vuv == 0.0)
    assert np.all((shift >= 0) & (shift < 1.0 / fs))


def test_periodic_spectrum_magnitude():
    rng = np.random.default_rng(4)
    K = 513
    env = np.exp(np.cumsum(rng.standard_normal(K)) * 0.05) * 0.1
    ratio = np.clip(rng.random(K), 0.001, 0.9) ** 2
    X = R.periodic_spectrum(env, ratio)
    assert np.allclose(np.abs(X), np.sqrt(env * (1 - ratio) + 1e-12), rtol=1e-9, atol=0)


def test_randn_stream():
    a, b = R.randn_table(20000), R.randn_table(20000)
    assert np.array_equal(a, b)
    assert a.min() >= -6 and a.max() <= 6
    assert abs(a.mean()) < 0.03 and abs(a.var() - 1) < 0.05


def test_constant_f0_synthesis_autocorrelation_peaks_at_the_period():
    fs, F, T = 22050, 147.0, 40
    rng = np.random.default_rng(5)
    mc = np.tile(_mc(rng, 1, 35, 0.3), (T, 1))
    cap = np.full((T, 2), -30.0)
    y = R.synthesis(np.full(T, F), mc, cap, fs=fs, shiftms=10.0, alpha=0.455)
    y = y[2048:-2048]
    ac = np.correlate(y, y, "full")[len(y) - 1:]
    lag = int(np.argmax(ac[60:400])) + 60
    assert abs(lag - fs / F) <= 1.0


def test_restatement_refusals():
    rng = np.random.default_rng(6)
    f0, mc, cap, _ = utterance(rng, 20, 35, 2)
    with pytest.raises(ValueError):
        R.synthesis(f0, mc, cap, fftl=2048)
    with pytest.raises(ValueError):
        R.synthesis(f0, mc, cap[:, :1])
    with pytest.raises(ValueError):
        R.synthesis(f0[:1], mc[:1], cap[:1])
    with pytest.raises(ValueError):
        R.synthesis(f0, mc, cap, rmcep=mc[:, :10])


def test_module_refusals_before_the_device():
    from crank_amd.world import WorldSynthesizer, n_bands, y_length

    assert [n_bands(fs) for fs in (16000, 22050, 24000)] == [1, 2, 3]
    assert y_length(500, 22050, 10) == 110250 and y_length(400, 22050, 5.80499) == int(400 * 5.80499 * 22050 / 1000)
    with pytest.raises(ValueError):
        WorldSynthesizer(22050, 512, 10.0, 0.455, device="cpu")
    syn = WorldSynthesizer(22050, 1024, 10.0, 0.455, device="cpu")
    rng = np.random.default_rng(7)
    f0, mc, cap, rm = utterance(rng, 20, 35, 2)
    for args in ((f0, mc, cap[:, :1], None), (f0[:1], mc[:1], cap[:1], None), (f0, mc, cap, rm[:, :5]),
                 (f0[:5], mc, cap, None)):
        with pytest.raises(ValueError):
            syn.synthesis(*args)


def test_world2wav_clips():
    rng = np.random.default_rng(8)
    f0, mc, cap, _ = utterance(rng, 30, 35, 2)
    mc[:, 0] += 3.0
    y = R.world2wav(f0, mc, cap, fs=22050, shiftms=10, alpha=0.455)
    assert y.shape == (R.y_length(30, 22050, 10),) and np.abs(y).max() <= 1.0
    assert math.isclose(np.abs(y).max(), 1.0)


def test_module_refusals_at_the_limits():
    """The limits of crank_amd.world, refused before the device: order + 1 outside 1..128, a sampling rate without
    an aperiodicity band (below 12 kHz), and a batch of mixed orders.  The accepted side of each limit reaches the
    device check (RuntimeError on a CPU synthesizer) instead."""
    from crank_amd.world import MAX_ORDER1, WorldSynthesizer, n_bands

    assert MAX_ORDER1 == 128
    assert [n_bands(fs) for fs in (11025, 11999, 12000, 44100, 48000)] == [0, 0, 1, 5, 5]
    for fs in (8000, 11025, 11999):
        with pytest.raises(ValueError):
            WorldSynthesizer(fs, 1024, 10.0, 0.455, device="cpu")
    assert WorldSynthesizer(12000, 1024, 10.0, 0.455, device="cpu").bands == 1
    syn = WorldSynthesizer(22050, 1024, 10.0, 0.455, device="cpu")
    rng = np.random.default_rng(9)
    f0, _, cap, _ = utterance(rng, 6, 1, 2)
    for order1 in (0, MAX_ORDER1 + 1):
        with pytest.raises(ValueError, match="mcep must be"):
            syn.synthesis(f0, np.zeros((6, order1)), cap)
    for order1 in (1, MAX_ORDER1):
        with pytest.raises(RuntimeError, match="device must be the GPU"):
            syn.synthesis(f0, np.zeros((6, order1)), cap)
    with pytest.raises(ValueError, match="same order"):
        syn.synthesis_batch([f0, f0], [np.zeros((6, 35)), np.zeros((6, 36))], [cap, cap])
    with pytest.raises(RuntimeError, match="device must be the GPU"):
        syn.synthesis_batch([f0, f0], [np.zeros((6, 36)), np.zeros((6, 36))], [cap, cap])
