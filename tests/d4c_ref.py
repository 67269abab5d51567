"""Test-side CPU restatement of WORLD's D4C aperiodicity and CodeAperiodicity (float64, numpy): what sprocket's
``FeatureExtractor.analyze`` (pyworld ``d4c(x, f0, time_axis, fs, fft_size=fftl)``, threshold 0.85) and ``.codeap()``
(pyworld ``code_aperiodicity``) compute, plus the recipe's post-processing of the coded bands (feature.py:98-107).  It is
the oracle of ``WorldAnalyzer.d4c_batch`` / ``codeap_batch`` (csrc/d4c_kernels.hip).

Parity with pyworld is UNPINNED: it is not installed.  The steps are restated from the published algorithm (WORLD d4c.cpp,
common.cpp, codec.cpp).  Restated without a source to check against, all shared with the kernels:
  * the randn stream restarts once per D4C call (utterance); a voiced frame of the Love-Train pass draws 2 * half + 1
    values, a frame of the general pass three times 2 * half4 + 1 (centroid before, centroid after, power window), and
    every Love-Train frame draws before any general frame;
  * half = matlab_round(1.5 fs / max(f0, 40)), half4 = matlab_round(2 fs / max(f0, 47)); the window position of sample j
    is 2 j / ratio / fs, the Blackman window 0.42 + 0.5 cos(pi p f0) + 0.08 cos(2 pi p f0), the Hanning window
    0.5 cos(pi p f0) + 0.5, neither normalised; the noise is randn * 1e-12 and the window-weighted mean is removed;
  * a centroid is Re X Re Y + Im X Im Y with X the transform of the unit-energy windowed waveform and Y that of
    (n + 1) x[n] (the numerator of the group delay; the outline in the project's issue writes the cross terms, which is
    the imaginary part of conj(X) Y and not a delay);
  * the centroids sit at t -+ 0.25 / f0, their origin matlab_round(pos fs + 0.001) with matlab_round rounding half away
    from zero also below zero;
  * DC correction and linear smoothing are those of tests/world_analysis_ref.py at 2048 points;
  * the Nuttall window is 0.355768 - 0.487396 cos(2 pi u) + 0.144232 cos(4 pi u) - 0.012604 cos(6 pi u), u = i / (len - 1);
  * the Love-Train power is zero up to and including bin ceil(100 fft / fs) and summed from there;
  * coding interpolates 20 log10(ap) on k fs / fftl with WORLD's interp1 (tests/world_analysis_ref.interp1).
Every FFT goes through the ``fft`` hook of tests/world_analysis_ref.py.

Upstream notice: the algorithm restated here is that of WORLD (Copyright (c) 2010 M. Morise, modified BSD licence); the
post-processing is that of crank (Copyright (c) 2020 K. Kobayashi, MIT License).  No upstream source text is in this
file; the notices quoted in tests/world_analysis_ref.py apply to the design it follows.
"""
import math

import numpy as np

from tests import world_analysis_ref as A
from tests.world_synth_ref import SAFE, n_bands, noise

FFTL = 1024
FFT = 2048  # both internal transforms at the supported rates
FS_MIN, FS_MAX = 13640, 24052
LOWEST_F0 = 40.0  # Love Train
FLOOR_F0 = 47.0  # kFloorF0D4C
INTERVAL = 3000.0
THRESHOLD = 0.85
BLACKMAN, HANNING = 0, 1


def fft_sizes(fs):
    """(Love-Train fft, D4C fft) of WORLD at fs."""
    lt = 2 ** (1 + int(math.log2(3.0 * fs / LOWEST_F0 + 1)))
    d4 = 2 ** (1 + int(math.log2(4.0 * fs / FLOOR_F0 + 1)))
    return lt, d4


def check_fs(fs):
    lt, d4 = fft_sizes(fs)
    if lt != FFT or d4 != FFT:
        raise ValueError(f"fs {fs}: D4C would need a {lt}-point Love-Train transform and a {d4}-point one; only {FFT} "
                         f"for both is supported ({FS_MIN} <= fs <= {FS_MAX})")


def matlab_round(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def frame_shapes(f0, fs, shiftms):
    """Per frame, in plain IEEE float64, the integers D4C forms before it knows any spectrum: Love-Train origin and half
    window, the general body's half window, the two centroid origins, the DC-correction limit and the two smoothing
    boundaries (width f0 / 2 and f0) at max(f0, 47); and the Love-Train draw offsets (voiced frames only)."""
    f0 = np.asarray(f0, np.float64).reshape(-1)
    T = len(f0)
    names = ("origin", "half_lt", "half_gb", "origin_c1", "origin_c2", "dc_limit", "bound_half", "bound_full")
    out = {k: np.zeros(T, np.int64) for k in names}
    off = np.zeros(T, np.int64)
    acc = 0
    for i in range(T):
        t = i * float(shiftms) / 1000.0
        out["origin"][i] = matlab_round(t * fs + 0.001)
        off[i] = acc
        if f0[i] == 0.0:
            continue
        lt = max(float(f0[i]), LOWEST_F0)
        gb = max(float(f0[i]), FLOOR_F0)
        out["half_lt"][i] = matlab_round(3.0 * fs / lt / 2.0)
        out["half_gb"][i] = matlab_round(4.0 * fs / gb / 2.0)
        out["origin_c1"][i] = matlab_round((t - 0.25 / gb) * fs + 0.001)
        out["origin_c2"][i] = matlab_round((t + 0.25 / gb) * fs + 0.001)
        out["dc_limit"][i] = 2 + int(gb * FFT / fs)
        out["bound_half"][i] = int(gb / 2.0 * FFT / fs) + 1
        out["bound_full"][i] = int(gb * FFT / fs) + 1
        acc += 2 * int(out["half_lt"][i]) + 1
    out["lt_offset"] = off
    out["lt_draws"] = acc
    return out


def general_offsets(shapes, passed):
    """Draw offsets of the general pass: after every Love-Train draw, 3 windows per passing frame."""
    T = len(passed)
    off = np.zeros(T, np.int64)
    acc = int(shapes["lt_draws"])
    for i in range(T):
        off[i] = acc
        if passed[i]:
            acc += 3 * (2 * int(shapes["half_gb"][i]) + 1)
    return off, acc


def draws_per_frame(fs):
    """The most randn values one frame can draw: the Love-Train window at 40 Hz and the general pass's three at 47 Hz."""
    return (2 * matlab_round(1.5 * fs / LOWEST_F0) + 1) + 3 * (2 * matlab_round(2.0 * fs / FLOOR_F0) + 1)


def windowed(x, fs, cur, origin, half, kind, ratio, draws):
    base = np.arange(-half, half + 1)
    safe = np.clip(origin + base, 0, len(x) - 1)
    pos = (2.0 * base / ratio) / fs
    if kind == HANNING:
        w = 0.5 * np.cos(np.pi * pos * cur) + 0.5
    else:
        w = 0.42 + 0.5 * np.cos(np.pi * pos * cur) + 0.08 * np.cos(np.pi * pos * cur * 2)
    wav = x[safe] * w + draws * SAFE
    return wav - w * (wav.sum() / w.sum())


def _pad(v, n=FFT):
    buf = np.zeros(n)
    buf[:len(v)] = v
    return buf


def dc_correction(p, cur, fs, n=FFT):
    lim = 2 + int(cur * n / fs)
    i = np.arange(lim - 1)
    out = p.copy()
    out[:lim - 1] = p[:lim - 1] + A.interp_equal(cur, -(fs / n), p[:lim + 1], i * fs / n)
    return out


def smoothing(p, width, fs, n=FFT):
    return A.linear_smoothing(p, width, int(width * n / fs) + 1, fs, n)


def love_train(x, fs, cur, origin, half, draws, fft=None):
    wav = windowed(x, fs, cur, origin, half, BLACKMAN, 3.0, draws)
    X = A._rfft(_pad(wav), fft)
    p = X.real * X.real + X.imag * X.imag
    b0, b1, b2 = (int(math.ceil(f * FFT / fs)) for f in (100.0, 4000.0, 7900.0))
    p[:b0 + 1] = 0.0
    c = np.cumsum(p[:b2 + 1])
    return c[b1] / c[b2]


def centroid(x, fs, cur, origin, half, draws, fft=None):
    wav = windowed(x, fs, cur, origin, half, BLACKMAN, 4.0, draws)
    wav = wav / math.sqrt((wav * wav).sum())
    X = A._rfft(_pad(wav), fft)
    Y = A._rfft(_pad(wav * (np.arange(len(wav)) + 1.0)), fft)
    return Y.real * X.real + X.imag * Y.imag


def nuttall(n):
    u = np.arange(n) / (n - 1.0)
    return (0.355768 - 0.487396 * np.cos(2.0 * np.pi * u) + 0.144232 * np.cos(4.0 * np.pi * u)
            - 0.012604 * np.cos(6.0 * np.pi * u))


def coarse_aperiodicity(gd, fs, bands, fft=None):
    half = int(INTERVAL * FFT / fs)
    wlen = 2 * half + 1
    win = nuttall(wlen)
    boundary = matlab_round(FFT * 8.0 / wlen)
    out = np.empty(bands)
    for b in range(bands):
        center = int(INTERVAL * (b + 1) * FFT / fs)
        X = A._rfft(_pad(gd[center - half:center + half + 1] * win), fft)
        s = np.cumsum(np.sort(X.real * X.real + X.imag * X.imag))
        out[b] = 10.0 * math.log10(s[FFT // 2 - boundary - 1] / s[FFT // 2])
    return out


def general_body(x, fs, cur, sh, i, draws, bands, fft=None):
    half = int(sh["half_gb"][i])
    n = 2 * half + 1
    c1 = centroid(x, fs, cur, int(sh["origin_c1"][i]), half, draws[:n], fft)
    c2 = centroid(x, fs, cur, int(sh["origin_c2"][i]), half, draws[n:2 * n], fft)
    cen = dc_correction(c1 + c2, cur, fs)
    wav = windowed(x, fs, cur, int(sh["origin"][i]), half, HANNING, 4.0, draws[2 * n:3 * n])
    X = A._rfft(_pad(wav), fft)
    p = smoothing(dc_correction(X.real * X.real + X.imag * X.imag, cur, fs), cur, fs)
    gd = smoothing(cen / p, cur / 2.0, fs)
    gd = gd - smoothing(gd, cur, fs)
    coarse = coarse_aperiodicity(gd, fs, bands, fft)
    return np.minimum(0.0, coarse + (cur - 100.0) / 50.0)


def coarse_axis(fs, bands):
    return np.array([INTERVAL * b for b in range(bands + 1)] + [fs / 2.0])


def frequency_axis(fs, fftl=FFTL):
    return np.array([float(k) * fs / fftl for k in range(fftl // 2 + 1)])


def d4c(x, f0, fs, shiftms, fftl=FFTL, threshold=THRESHOLD, fft=None, detail=False):
    """pyworld d4c(x, f0, i * shiftms / 1000, fs, threshold, fft_size=fftl): (T, fftl / 2 + 1).  With ``detail`` also a
    dict of the Love-Train values, the pass flags, the coarse bands and both draw-offset tables."""
    if fftl != FFTL:
        raise ValueError(f"fftl {fftl}: only {FFTL} is supported")
    check_fs(fs)
    x = np.asarray(x, np.float64).reshape(-1)
    f0 = np.asarray(f0, np.float64).reshape(-1)
    if len(x) < 1:
        raise ValueError("an empty waveform")
    T, K, bands = len(f0), fftl // 2 + 1, n_bands(fs)
    sh = frame_shapes(f0, fs, shiftms)
    nz = noise(int(sh["lt_draws"]))
    ap0 = np.zeros(T)
    for i in range(T):
        if f0[i] == 0.0:
            continue
        half, off = int(sh["half_lt"][i]), int(sh["lt_offset"][i])
        ap0[i] = love_train(x, fs, max(float(f0[i]), LOWEST_F0), int(sh["origin"][i]), half, nz[off:off + 2 * half + 1], fft)
    passed = (f0 != 0.0) & (ap0 > threshold)
    goff, total = general_offsets(sh, passed)
    nz = noise(int(total))
    ap = np.full((T, K), 1.0 - SAFE)
    coarse = np.zeros((T, bands))
    for i in range(T):
        if not passed[i]:
            continue
        cur = max(float(f0[i]), FLOOR_F0)
        n3 = 3 * (2 * int(sh["half_gb"][i]) + 1)
        coarse[i] = general_body(x, fs, cur, sh, i, nz[goff[i]:goff[i] + n3], bands, fft)
        vals = np.concatenate([[-60.0], coarse[i], [-SAFE]])
        ap[i] = 10.0 ** (A.interp1(coarse_axis(fs, bands), vals, frequency_axis(fs, fftl)) / 20.0)
    if detail:
        return ap, dict(ap0=ap0, passed=passed, coarse=coarse, shapes=sh, gb_offset=goff, draws=total)
    return ap


def code_aperiodicity(ap, fs, fftl=FFTL):
    """pyworld code_aperiodicity: (T, fftl / 2 + 1) -> (T, bands) in dB."""
    ap = np.asarray(ap, np.float64)
    bands = n_bands(fs)
    if bands < 1:
        raise ValueError(f"fs {fs}: WORLD's coded aperiodicity has no band below fs / 2 - 3 kHz")
    axis = frequency_axis(fs, fftl)
    knots = INTERVAL * (np.arange(bands) + 1.0)
    return np.stack([A.interp1(axis, 20.0 * np.log10(row), knots) for row in ap]) if len(ap) else np.zeros((0, bands))


def codeap(x, f0, fs, shiftms, fftl=FFTL, threshold=THRESHOLD, fft=None):
    return code_aperiodicity(d4c(x, f0, fs, shiftms, fftl, threshold, fft), fs, fftl)


def postprocess(cap):
    """feature.py:98-107 on a copy of cap: (cap as saved, ccap, cap_uv).  ``convert_continuos_f0`` is
    tests/harvest_ref.continuous_f0, which a golden fixture pins to the reference's own function; the saved cap is the
    column with the ends that function fills in place."""
    from tests.harvest_ref import continuous_f0

    cap = np.array(cap, np.float64)
    ccap, uv = np.zeros(cap.shape), np.zeros(cap.shape)
    for d in range(cap.shape[-1]):
        cap[np.where(cap[:, d] == max(cap[:, d])), d] = 0.0
        with np.errstate(invalid="ignore"):  # the function also takes logarithms, which only F0 has
            uv[:, d], ccap[:, d], _, _, cap[:, d] = continuous_f0(cap[:, d])
    return cap, ccap, uv
