"""Inputs of the D4C tests and the tolerance of the GPU tests, derived from the restatement alone.

Every case is a ragged batch (name, fs, shiftms, waves, f0s) built from a fixed seed.  ``spread(case)`` evaluates
tests/d4c_ref.py twice on the case, once with numpy.fft and once with the plain radix-2 FFT of
tests/world_analysis_ref.py: two correct evaluations that differ only in rounding.  ``s_ap = max |20 log10 ap_a -
20 log10 ap_b|`` and ``s_cap = max |cap_a - cap_b|`` in dB over every bin of every frame.  The kernels get
``10 * s + 1e-12`` (one more FFT ordering and another libm; a factor, not a new measurement).
SPREADS holds the values of

    python -m tests.d4c_cases

and tests/test_d4c_cpu.py recomputes them and fails if one moved by more than 2x or exceeds 1e-8 dB (the sign of an
ill-conditioned input, which is fixed at the input, not by a wider bound).  Digital silence and constant signals are such
a class (the window holds only the 1e-12 noise after the mean removal): ``degenerate()`` is checked for range and
finiteness only.

A frame whose Love-Train value is within rounding of the threshold flips whether it draws noise and so moves the noise
of every later frame: ``threshold_margin(case)`` is asserted to be at least MARGIN under both FFTs.  It is a condition
on the inputs, not a tolerance.
"""
import functools
import math

import numpy as np

from tests import d4c_ref as D
from tests import world_analysis_ref as A
from tests import world_synth_ref as R

FLOOR = 1e-12
FACTOR = 10.0
LIMIT = 1e-8
MARGIN = 1e-6

# name -> (s_ap, s_cap) in dB
SPREADS = {
    "ragged": (1.244e-12, 1.243e-12),
    "fs16000_shift5": (3.730e-14, 3.464e-14),
    "fs16000_shift10": (6.484e-14, 6.106e-14),
    "fs16000_shift5.33333": (1.994e-13, 1.990e-13),
    "fs22050_shift5": (5.773e-14, 5.729e-14),
    "fs22050_shift10": (5.862e-14, 5.862e-14),
    "fs22050_shift5.33333": (3.273e-13, 3.244e-13),
    "fs24000_shift5": (9.064e-13, 9.064e-13),
    "fs24000_shift10": (1.712e-13, 1.712e-13),
    "fs24000_shift5.33333": (7.061e-14, 7.017e-14),
    "ends": (5.107e-14, 5.018e-14),
    "voicing": (6.306e-14, 6.217e-14),
    "noise": (0.000e+00, 0.000e+00),
    "vowel": (8.385e-12, 8.376e-12),
    "high_f0": (3.482e-13, 3.482e-13),
}


def _harmonic(rng, n, fs, f, noise=0.02):
    t = np.arange(n) / fs
    y = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * f * h * t + rng.uniform(0, 6.28)) for h in range(1, 9))
    return y + noise * rng.standard_normal(n)


def _samples(T, fs, shiftms):
    return int(T * shiftms * fs / 1000)


def edge_f0s(fs):
    """F0 exactly at, one ulp below and above the two floors (40 Hz Love Train, 47 Hz general body), and F0 whose half
    windows 1.5 fs / F0 and 2 fs / F0 sit at, one ulp above and below a rounding point (x.5)."""
    out = []
    for fl in (D.LOWEST_F0, D.FLOOR_F0):
        out += [fl, np.nextafter(fl, 0.0), np.nextafter(fl, 1e9)]
    for c, h in ((1.5, 100.5), (1.5, 250.5), (2.0, 120.5), (2.0, 300.5)):
        f = c * fs / h
        out += [f, np.nextafter(f, 1e9), np.nextafter(f, 0.0)]
    return np.array(out)


def vowel(rng, T, fs, shiftms, level=-25.0):
    """A synthesised utterance (tests/world_synth_ref.synthesis) at a constant coded aperiodicity."""
    order, alpha = 24, 0.455
    mc = np.zeros((T, order + 1))
    mc[:, 0] = -3.0 + 0.5 * np.sin(np.arange(T) / 9.0)
    mc[:, 1:] = rng.standard_normal(order) * 0.5 / np.arange(1, order + 1)
    mc[:, 1] = 2.0  # the tilt of speech: most of the power below 4 kHz, which is what the Love Train asks of a voiced frame
    f0 = 170.0 + 40.0 * np.sin(np.arange(T) / 11.0)
    f0[T // 2:T // 2 + 4] = 0.0
    cap = np.full((T, R.n_bands(fs)), level)
    cap[f0 == 0.0] = 0.0
    return R.synthesis(f0, mc, cap, None, fs, 1024, shiftms, alpha), f0


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, fs, shiftms, waves, f0s):
        out.append(dict(name=name, fs=fs, shiftms=shiftms, waves=[np.asarray(w, np.float64) for w in waves],
                        f0s=[np.asarray(f, np.float64) for f in f0s]))

    rng = np.random.default_rng(4047)
    # ragged batch: 1, 2, 37 and 120 frames, and a 1-sample waveform (its one sample zero: see degenerate())
    waves, f0s = [], []
    for T in (1, 2, 37, 120):
        waves.append(_harmonic(rng, max(1, _samples(T, 22050, 5.0)), 22050, 140.0))
        f = np.full(T, 140.0) + rng.uniform(-10, 10, T)
        f[rng.uniform(size=T) < 0.15] = 0.0
        f0s.append(f)
    waves.append(np.array([0.0]))
    f0s.append(np.array([0.0]))
    add("ragged", 22050, 5.0, waves, f0s)
    # the three rates (1 / 2 / 3 bands) and shifts, F0 at the floors and the rounding points of both half windows
    for fs in (16000, 22050, 24000):
        for shiftms in (5.0, 10.0, 5.333333):
            f0 = np.concatenate([edge_f0s(fs), rng.uniform(70, 300, 3)])
            T = len(f0)
            add(f"fs{fs}_shift{shiftms:g}", fs, shiftms, [_harmonic(rng, _samples(T, fs, shiftms), fs, 90.0)], [f0])
    # frame centres within half a window of both ends of a short signal; the first centroid sits before sample 0
    add("ends", 22050, 5.0, [_harmonic(rng, 900, 22050, 80.0)], [np.full(9, 75.0)])
    # all unvoiced; voicing flipping every frame
    T = 16
    w = _harmonic(rng, _samples(T, 22050, 5.0), 22050, 200.0)
    add("voicing", 22050, 5.0, [w, w], [np.zeros(T), np.where(np.arange(T) % 2 == 0, 200.0, 0.0)])
    # white noise with a voiced F0: the Love Train keeps it out of the general pass
    T = 12
    add("noise", 24000, 5.0, [0.3 * rng.standard_normal(_samples(T, 24000, 5.0))], [rng.uniform(90, 300, T)])
    # a synthesised vowel at -25 dB
    y, f0 = vowel(rng, 40, 22050, 5.0)
    add("vowel", 22050, 5.0, [y], [f0])
    # F0 so high that (f0 - 100) / 50 lifts a band to the 0 dB clamp (the analysis F0 is the second harmonic's)
    T = 10
    add("high_f0", 24000, 5.0, [_harmonic(rng, _samples(T, 24000, 5.0), 24000, 350.0, noise=0.1)], [rng.uniform(650, 750, T)])
    return out


def degenerate():
    """Digital silence and a constant signal with voiced F0: finite and in (0, 1 - 1e-12] is all that can be asked."""
    f0 = np.array([0.0, 60.0, 150.0, 150.0, 400.0, 0.0, 220.0, 220.0])
    n = _samples(len(f0), 22050, 5.0)
    return dict(name="degenerate", fs=22050, shiftms=5.0, waves=[np.zeros(n), np.full(n, 0.25)], f0s=[f0, f0])


@functools.lru_cache(maxsize=None)
def reference(name, radix2=False):
    """(aps, caps, details) of the restatement on a case; computed once and shared (treat as read-only)."""
    case = {c["name"]: c for c in cases()}[name]
    fft = A.fft_radix2 if radix2 else None
    aps, caps, det = [], [], []
    for w, f in zip(case["waves"], case["f0s"]):
        ap, d = D.d4c(w, f, case["fs"], case["shiftms"], fft=fft, detail=True)
        aps.append(ap)
        caps.append(D.code_aperiodicity(ap, case["fs"]))
        det.append(d)
    return aps, caps, det


def spread(name):
    a_ap, a_cap, _ = reference(name)
    b_ap, b_cap, _ = reference(name, True)
    s_ap = max(float(np.abs(20.0 * np.log10(a) - 20.0 * np.log10(b)).max()) for a, b in zip(a_ap, b_ap))
    s_cap = max(float(np.abs(a - b).max()) for a, b in zip(a_cap, b_cap))
    return s_ap, s_cap


def threshold_margin(name, threshold=D.THRESHOLD):
    """The least |aperiodicity0 - threshold| over the voiced frames of a case, under both FFTs."""
    case = {c["name"]: c for c in cases()}[name]
    m = math.inf
    for radix2 in (False, True):
        for f0, d in zip(case["f0s"], reference(name, radix2)[2]):
            if (f0 != 0).any():
                m = min(m, float(np.abs(d["ap0"][f0 != 0] - threshold).min()))
    return m


def bounds(name):
    s_ap, s_cap = SPREADS[name]
    return FACTOR * s_ap + FLOOR, FACTOR * s_cap + FLOOR


def edges_reached():
    """Host-side facts the tests assert before they rely on the cases: every edge they are meant to reach is reached."""
    by = {c["name"]: c for c in cases()}
    facts = {}
    c = by["ragged"]
    facts["ragged"] = [len(f) for f in c["f0s"]] == [1, 2, 37, 120, 1] and len(c["waves"][4]) == 1
    facts["bands"] = [R.n_bands(fs) for fs in (16000, 22050, 24000)] == [1, 2, 3]
    half = int(D.INTERVAL * D.FFT / 24000)
    facts["top_slice"] = int(D.INTERVAL * 3 * D.FFT / 24000) + half == D.FFT // 2
    for fs in (16000, 22050, 24000):
        sh = D.frame_shapes(by[f"fs{fs}_shift5"]["f0s"][0], fs, 5.0)
        f0 = by[f"fs{fs}_shift5"]["f0s"][0]
        facts[f"floors_{fs}"] = bool(f0[0] == 40.0 and f0[1] < 40.0 < f0[2] and f0[3] == 47.0 and f0[4] < 47.0 < f0[5]
                                     and sh["half_lt"][0] == sh["half_lt"][1] and sh["half_gb"][3] == sh["half_gb"][4])
        facts[f"half_flips_{fs}"] = all(len(set(sh[k][i:i + 3].tolist())) == 2
                                        for k, i in (("half_lt", 6), ("half_lt", 9), ("half_gb", 12), ("half_gb", 15)))
    facts["shifts"] = all(f"fs{fs}_shift{s}" in by for fs in (16000, 22050, 24000) for s in ("5", "10", "5.33333"))
    c = by["ends"]
    sh = D.frame_shapes(c["f0s"][0], 22050, 5.0)
    n = len(c["waves"][0])
    facts["ends"] = bool((sh["origin"] - sh["half_gb"] < 0).any() and (sh["origin"] + sh["half_gb"] > n - 1).any())
    facts["centroid_before_0"] = bool(sh["origin_c1"][0] < 0)
    facts["unvoiced"] = bool((by["voicing"]["f0s"][0] == 0).all())
    facts["flip"] = bool((np.diff((by["voicing"]["f0s"][1] > 0).astype(int)) != 0).all())
    passed = np.concatenate([d["passed"] for n_ in by for d in reference(n_)[2]])
    voiced = np.concatenate([f != 0 for c_ in cases() for f in c_["f0s"]])
    facts["threshold_both"] = bool(passed.any() and (voiced & ~passed).any())
    facts["noise_fails"] = not any(d["passed"].any() for d in reference("noise")[2])
    facts["vowel_passes"] = bool(reference("vowel")[2][0]["passed"].sum() >= 30)
    co = reference("high_f0")[2][0]
    facts["clamped"] = bool(((co["coarse"] == 0.0) & co["passed"][:, None]).any())
    return facts


if __name__ == "__main__":
    import time

    print("SPREADS = {")
    for c in cases():
        t = time.time()
        s_ap, s_cap = spread(c["name"])
        print(f'    "{c["name"]}": ({s_ap:.3e}, {s_cap:.3e}),  # margin {threshold_margin(c["name"]):.2e}, '
              f'{time.time() - t:.1f} s')
    print("}")
    print({k: v for k, v in edges_reached().items() if not v} or "every edge reached")
