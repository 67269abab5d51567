"""Inputs of the WORLD analysis tests and the tolerance of the GPU tests, derived from the restatement alone.

Every case is a ragged batch (name, fs, shiftms, waves, f0s, dim, alpha) built from a fixed seed.  ``spread(case)``
evaluates tests/world_analysis_ref.py twice on the case, once with numpy.fft and once with the plain radix-2 FFT of
the restatement file: two correct evaluations that differ only in rounding.  ``s_sp = max |log sp_a - log sp_b|`` and
``s_mc = max |mc_a - mc_b|`` over every bin of every frame.  The kernels get ``10 * s + 1e-12`` (one more FFT ordering and
another libm: a factor, not a new measurement; the cumulative sum of the smoothing runs in the restatement's order).  SPREADS holds the values of

    python -m tests.world_analysis_cases

and tests/test_world_analysis_cpu.py recomputes them and fails if one moved by more than 2x or exceeds 1e-8 (the sign
of an ill-conditioned input, which is fixed at the input, not by a wider bound).
"""
import math

import numpy as np

from tests import world_analysis_ref as A
from tests import world_synth_ref as R

FLOOR = 1e-12
FACTOR = 10.0
LOWCUT_TILE = 256  # crk_wana_lowcut_tile(); the GPU test asserts it

# name -> (s_sp, s_mc)
SPREADS = {
    "vowel": (6.040e-14, 8.882e-16),
    "silence": (1.421e-14, 4.788e-16),
    "mixed": (3.766e-13, 1.424e-14),
    "ragged": (2.888e-12, 3.084e-14),
    "high_f0": (1.643e-13, 5.135e-15),
    "ends": (4.114e-12, 7.952e-15),
    "voicing": (5.480e-13, 4.295e-15),
    "fs16000_shift5": (7.097e-13, 1.809e-14),
    "fs16000_shift10": (9.139e-13, 9.270e-15),
    "fs16000_shift5.33333": (1.945e-13, 5.246e-15),
    "fs24000_shift5": (7.292e-13, 8.937e-15),
    "fs24000_shift10": (2.084e-12, 1.481e-14),
    "fs24000_shift5.33333": (7.629e-13, 1.082e-14),
    "fs44100_shift5": (4.207e-12, 2.408e-14),
    "fs44100_shift10": (1.036e-12, 5.856e-15),
    "fs44100_shift5.33333": (5.596e-13, 4.663e-15),
    "fs48000_shift5": (3.846e-13, 8.465e-15),
    "fs48000_shift10": (3.046e-13, 1.052e-14),
    "fs48000_shift5.33333": (3.935e-13, 4.878e-15),
    "order1_1_alpha0.455": (2.212e-13, 1.110e-15),
    "order1_25_alpha0.41": (2.212e-13, 3.428e-15),
    "order1_35_alpha0": (2.212e-13, 7.980e-15),
    "order1_60_alpha0.544": (2.212e-13, 2.495e-15),
    "order1_128_alpha0.455": (2.212e-13, 3.136e-15),
}


def _harmonic(rng, n, fs, f):
    t = np.arange(n) / fs
    y = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * f * h * t + rng.uniform(0, 6.28)) for h in range(1, 9))
    # The noise floor keeps every bin within about 1e3 of the frame's peak.  The linear smoothing reads a bin as the
    # difference of two values of a cumulative sum, so one last-bit flip of that sum moves a bin 1e5 below the peak by
    # 1e-11 in log sp.  Such flips are rare (a few frames in a hundred) and any change of FFT rounding can cause one:
    # with a floor of 1e-2 the twelve fs / shift cases had two-FFT spreads of either 1e-14 or 1e-11 .. 4e-11, depending
    # on whether the one pair of evaluations happened to hit one, so a single pair understated the conditioning of half
    # of them (and the kernels, hitting a flip in 3 other frames, were 6e-12 and 7e-11 off in two cases with a spread
    # of 1e-14).  The input is fixed, not the bound.
    return y + 0.1 * rng.standard_normal(n)


def _samples(T, fs, shiftms):
    return int(T * shiftms * fs / 1000)


def vowel(rng, T, fs, shiftms, order=34, alpha=0.455):
    """A synthesised utterance: random-walk mel-cepstrum, F0 contour with unvoiced stretches."""
    mc = np.zeros((T, order + 1))
    mc[:, 0] = -3.0
    mc[0, 1:] = rng.standard_normal(order) * 0.5 / np.arange(1, order + 1)
    for t in range(1, T):
        mc[t, 1:] = 0.95 * mc[t - 1, 1:] + 0.05 * rng.standard_normal(order) * 0.5 / np.arange(1, order + 1)
        mc[t, 0] = -3.0 + 0.5 * math.sin(t / 9.0)
    f0 = 170.0 + 60.0 * np.sin(np.arange(T) / 11.0) + rng.uniform(-3, 3, T)
    for s in range(0, T, 40):
        f0[s:s + int(rng.integers(2, 8))] = 0.0
    cap = np.full((T, R.n_bands(fs)), -25.0)
    cap[f0 == 0.0] = 0.0
    y = R.synthesis(f0, mc, cap, None, fs, 1024, shiftms, alpha)
    return y, f0, mc


def floor_f0s(fs):
    """F0 exactly at, one ulp above and below CheapTrick's floor, and F0 whose half window 1.5 fs / F0 sits at, one ulp
    above and below a rounding point (x.5)."""
    fl = A.f0_floor(fs)
    out = [fl, np.nextafter(fl, 1e9), np.nextafter(fl, 0.0)]
    for h in (40.5, 100.5, 250.5):
        f = 1.5 * fs / h
        out += [f, np.nextafter(f, 1e9), np.nextafter(f, 0.0)]
    for k in (7, 23):  # DC limit and smoothing boundary at an integer
        f = k * fs / 1024.0
        out += [f, np.nextafter(f, 1e9), np.nextafter(f, 0.0), 1.5 * f, np.nextafter(1.5 * f, 0.0)]
    return np.array(out)


def cases():
    out = []

    def add(name, fs, shiftms, waves, f0s, dim=34, alpha=0.455):
        out.append(dict(name=name, fs=fs, shiftms=shiftms, waves=[np.asarray(w, np.float64) for w in waves],
                        f0s=[np.asarray(f, np.float64) for f in f0s], dim=dim, alpha=alpha))

    rng = np.random.default_rng(20240)
    y, f0, _ = vowel(rng, 120, 22050, 5.0)
    add("vowel", 22050, 5.0, [y], [f0])
    # the padding of a vocoded batch: digital silence, F0 mixed
    f0 = rng.uniform(60, 400, 60)
    f0[::3] = 0.0
    add("silence", 22050, 5.0, [np.zeros(_samples(60, 22050, 5.0))], [f0])
    # white noise, silence and a full-scale square wave in one utterance, F0 60 - 900 Hz
    T = 150
    n = _samples(T, 22050, 5.0)
    y = np.zeros(n)
    y[:n // 3] = rng.standard_normal(n // 3) * 0.3
    y[2 * n // 3:] = np.where((np.arange(n - 2 * n // 3) // 55) % 2 == 0, 1.0, -1.0)
    add("mixed", 22050, 5.0, [y], [rng.uniform(60, 900, T)])
    # ragged batch
    lens = [1, 2, 37, 500, 501]
    waves, f0s = [], []
    for T in lens:
        n = max(1, _samples(T, 22050, 5.0))
        waves.append(_harmonic(rng, n, 22050, 140.0))
        f = np.full(T, 140.0) + rng.uniform(-20, 20, T)
        f[rng.uniform(size=T) < 0.2] = 0.0
        f0s.append(f)
    add("ragged", 22050, 5.0, waves, f0s)
    # F0 800 - 1000 Hz: a window of about 70 samples, the DC-correction limit near bin 40
    T = 40
    add("high_f0", 22050, 5.0, [_harmonic(rng, _samples(T, 22050, 5.0), 22050, 900.0)], [rng.uniform(800, 1000, T)])
    # frame centres within half a window of both ends of a short signal (clamped indices), a 1-sample utterance.  Its one
    # sample is zero: a constant signal cancels in the removal of the window-weighted mean and leaves the rounding of
    # the products x w, which depends on the last bit of cos and so differs between any two implementations; the
    # two-FFT spread cannot see that.  A non-zero constant is checked for a positive, finite result only
    # (test_constant_signal_stays_positive_and_finite).
    add("ends", 22050, 5.0, [_harmonic(rng, 700, 22050, 80.0), np.array([0.0])], [np.full(7, 70.0), np.array([100.0])])
    # all unvoiced; voicing flipping every frame
    T = 30
    w = _harmonic(rng, _samples(T, 22050, 5.0), 22050, 200.0)
    flip = np.where(np.arange(T) % 2 == 0, 200.0, 0.0)
    add("voicing", 22050, 5.0, [w, w], [np.zeros(T), flip])
    # other rates and shifts, with F0 at the floor and at the rounding points of the frame's integers
    for fs in (16000, 24000, 44100, 48000):
        for shiftms in (5.0, 10.0, 5.333333):
            f0 = np.concatenate([floor_f0s(fs), rng.uniform(70, 600, 5)])
            T = len(f0)
            add(f"fs{fs}_shift{shiftms:g}", fs, shiftms, [_harmonic(rng, _samples(T, fs, shiftms), fs, 180.0)], [f0])
    # orders and alpha 0
    T = 20
    w = _harmonic(rng, _samples(T, 22050, 5.0), 22050, 220.0)
    f0 = np.full(T, 220.0)
    f0[5:8] = 0.0
    for order1, alpha in ((1, 0.455), (25, 0.41), (35, 0.0), (60, 0.544), (128, 0.455)):
        add(f"order1_{order1}_alpha{alpha:g}", 22050, 5.0, [w], [f0], order1 - 1, alpha)
    return out


def edges_reached(cs):
    """Host-side facts the GPU tests assert before they run: every edge the cases are meant to reach is reached."""
    by = {c["name"]: c for c in cs}
    facts = {}
    c = by["fs16000_shift5"]
    fl = A.f0_floor(16000)
    sh = A.frame_shapes(c["f0s"][0], 16000, 5.0)
    facts["floor"] = (c["f0s"][0][0] == fl and sh["f0"][0] == 500.0 and sh["f0"][1] == np.nextafter(fl, 1e9)
                      and sh["f0"][2] == 500.0)
    facts["half_flips"] = len(set(sh["half"][3:6].tolist())) == 2
    sh = A.frame_shapes(by["high_f0"]["f0s"][0], 22050, 5.0)
    facts["high_f0"] = bool((sh["half"] <= 42).all() and (sh["dc_limit"] >= 39).all() and (sh["dc_limit"] <= 48).all())
    c = by["ends"]
    sh = A.frame_shapes(c["f0s"][0], 22050, 5.0)
    n = len(c["waves"][0])
    facts["ends"] = bool((sh["origin"] - sh["half"] < 0).any() and (sh["origin"] + sh["half"] > n - 1).any())
    facts["one_sample"] = len(c["waves"][1]) == 1
    facts["unvoiced"] = bool((by["voicing"]["f0s"][0] == 0).all())
    facts["flip"] = bool((np.diff((by["voicing"]["f0s"][1] > 0).astype(int)) != 0).all())
    facts["silence"] = bool((by["silence"]["waves"][0] == 0).all())
    facts["ragged"] = [len(f) for f in by["ragged"]["f0s"]] == [1, 2, 37, 500, 501]
    return facts


def reference(case, fft=None):
    """(sps, mcs): the restatement's envelopes and mel-cepstra (no low cut) of a case."""
    sps = [A.cheaptrick(w, f, case["fs"], case["shiftms"], fft=fft) for w, f in zip(case["waves"], case["f0s"])]
    mcs = [A.sp2mc(sp, case["dim"], case["alpha"], fft=fft) for sp in sps]
    return sps, mcs


def spread(case, ref=None):
    a_sp, a_mc = ref if ref is not None else reference(case)
    b_sp, b_mc = reference(case, fft=A.fft_radix2)
    s_sp = max(float(np.abs(np.log(a) - np.log(b)).max()) for a, b in zip(a_sp, b_sp))
    s_mc = max(float(np.abs(a - b).max()) for a, b in zip(a_mc, b_mc))
    return s_sp, s_mc


def bounds(name):
    s_sp, s_mc = SPREADS[name]
    return FACTOR * s_sp + FLOOR, FACTOR * s_mc + FLOOR


def lowcut_lengths():
    """Waveform lengths exactly, one below and one past a multiple of the low-cut kernel's tile, and shorter than the
    filter."""
    return [LOWCUT_TILE * 3, LOWCUT_TILE * 3 - 1, LOWCUT_TILE * 3 + 1, 1, 100, 255, 1000]


def mcd_pairs(n=6, fs=22050, shiftms=5.0, order=34, alpha=0.455):
    """Ragged (converted waveform, converted F0, ground-truth mcep, ground-truth F0) tuples for the MCD test."""
    rng = np.random.default_rng(777)
    out = []
    for i in range(n):
        T = int(rng.integers(50, 110))
        y, f0, mc = vowel(rng, T, fs, shiftms, order, alpha)
        Tg = int(rng.integers(50, 110))
        _, gf0, gmc = vowel_features(rng, Tg, order)
        out.append((np.clip(y, -1.0, 1.0), f0, gmc, gf0))
    return out


def vowel_features(rng, T, order):
    mc = np.zeros((T, order + 1))
    mc[:, 0] = -3.0 + 0.3 * rng.standard_normal(T)
    mc[:, 1:] = np.cumsum(rng.standard_normal((T, order)) * 0.03, 0) + rng.standard_normal(order) * 0.5 / np.arange(1, order + 1)
    f0 = 150.0 + 30.0 * np.sin(np.arange(T) / 7.0)
    f0[rng.uniform(size=T) < 0.15] = 0.0
    return None, f0, mc


if __name__ == "__main__":
    print("SPREADS = {")
    for c in cases():
        s_sp, s_mc = spread(c)
        print(f'    "{c["name"]}": ({s_sp:.3e}, {s_mc:.3e}),')
    print("}")
