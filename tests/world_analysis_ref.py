"""Test-side CPU restatement of the spectral half of WORLD analysis (float64, numpy): what the reference's
``crank/bin/evaluate_mcd.py`` runs on a converted waveform - ``low_cut_filter``, then sprocket's
``FeatureExtractor.analyze`` / ``.mcep`` / ``.npow`` (pyworld ``cheaptrick``, pysptk ``sp2mc``, sprocket ``spc2npow``) -
with the F0 contour GIVEN by the caller instead of estimated by Harvest.  It is the oracle of crank_amd/world.py's
``WorldAnalyzer`` (csrc/world_analysis_kernels.hip).

``low_cut_filter`` is pinned: scipy is installed and the tests compare it with ``scipy.signal.lfilter``.  Parity of
CheapTrick / sp2mc / spc2npow against pyworld / pysptk / sprocket is UNPINNED: none of them is installed.  The steps are
restated from the published algorithms (WORLD cheaptrick.cpp / common.cpp / matlabfunctions.cpp, pysptk sp2mc, sprocket
spc2npow).  Details restated without a source to check them against, all shared with the kernels:
  * reseeding: the randn stream restarts once per utterance (CheapTrick of recent WORLD versions calls randn_reseed at
    its start; older ones never reseed) and is consumed in frame order, 2 * half + 1 window draws, then fftl / 2 + 1;
  * the window noise is randn * 1e-12 (the figure the project's issue states; WORLD's safeguard constant);
  * the half window is matlab_round(1.5 fs / f0) = int(x + 0.5), the frame origin matlab_round(t fs + 0.001);
  * the DC correction and the linear smoothing interpolate on EQUALLY SPACED knots by index arithmetic
    (base = int((xi - x0) / dx), WORLD's interp1Q), not by a knot search: at a knot the interpolant is continuous, so
    a base that flips by one ulp of xi changes nothing beyond rounding.  The slope past the last knot is zero;
  * ``interp1`` below (knot search, WORLD's histc edge rule: the last knot at or below xi, at most the one before
    last) is the vectorised form of world_synth_ref.interp1 and is what the tests check against it;
  * sp2mc passes all fftl coefficients of irfft(log sp) to freqt, as pysptk does; the mirrored half contributes
    alpha ** (fftl / 2) and less;
  * F0 at or below 3 fs / (fftl - 3) - unvoiced frames included - is analysed at 500 Hz.
Every FFT goes through one hook (``fft``: complex (N,) -> complex (N,)), so that the tests can evaluate the restatement
with two different, equally correct transforms and take the spread as the measure of its own rounding.

Upstream notice: the algorithms restated here are those of WORLD (Copyright (c) 2010 M. Morise, modified BSD licence),
SPTK (Copyright (c) 1984-2007 Tokyo Institute of Technology, 1996-2017 Nagoya Institute of Technology, modified BSD
licence), pysptk (Copyright (c) 2015 Ryuichi Yamamoto, MIT License) and sprocket (Copyright (c) 2017 Kazuhiro
Kobayashi, MIT License).  No upstream source text is in this file; the notices of those licences apply to the design
it follows: "Redistribution and use in source and binary forms, with or without modification, are permitted provided
that ... THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS IS" AND ANY EXPRESS OR IMPLIED
WARRANTIES ... ARE DISCLAIMED" and "Permission is hereby granted, free of charge, to any person obtaining a copy of this
software ... THE SOFTWARE IS PROVIDED "AS IS", WITHOUT WARRANTY OF ANY KIND".
"""
import math

import numpy as np

from tests.world_synth_ref import DEFAULT_F0, FFTL, freqt, mc2sp, noise, randn_table  # noqa: F401

EPS = 2.220446049250313e-16  # WORLD's kEps
NOISE_SCALE = 1e-12
Q1 = -0.15
LOWCUT_TAPS = 255


# ---- the reference's low_cut_filter
def low_cut_taps(fs, cutoff=70):
    from scipy.signal import firwin

    return firwin(LOWCUT_TAPS, cutoff / (fs // 2), pass_zero=False)


def low_cut_filter(x, fs, cutoff=70):
    """crank.utils.low_cut_filter: a causal 255-tap FIR high-pass with zero history (float64 out)."""
    x = np.asarray(x)
    return np.convolve(x.astype(np.float64), low_cut_taps(fs, cutoff))[:len(x)]


# ---- WORLD
def interp1(x, y, xi):
    """world_synth_ref.interp1, vectorised: j = the last knot with x[j] <= xi, within [0, len(x) - 2]."""
    x, y, xi = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(xi, np.float64)
    j = np.clip(np.searchsorted(x, xi, side="right") - 1, 0, len(x) - 2)
    s = (xi - x[j]) / (x[j + 1] - x[j])
    return y[j] + s * (y[j + 1] - y[j])


def interp_equal(x0, dx, y, xi):
    """Linear interpolation on the knots x0 + i dx by index arithmetic; zero slope from the last knot on."""
    fr = (xi - x0) / dx
    base = fr.astype(np.int64)
    fr = fr - base
    yp = np.concatenate([y, y[-1:]])
    return yp[base] + (yp[base + 1] - yp[base]) * fr


def matlab_round(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def f0_floor(fs, fftl=FFTL):
    return 3.0 * fs / (fftl - 3.0)


def frame_shapes(f0, fs, shiftms, fftl=FFTL):
    """Per frame, in plain IEEE float64: the F0 used, the frame origin (sample), the half window, the DC-correction
    limit, the smoothing boundary and where the frame's randn draws start in the utterance's stream."""
    f0 = np.asarray(f0, np.float64).reshape(-1)
    T = len(f0)
    floor = f0_floor(fs, fftl)
    used = np.empty(T)
    origin, half, dc, bound, off = (np.empty(T, np.int64) for _ in range(5))
    acc = 0
    for i in range(T):
        cur = DEFAULT_F0 if f0[i] <= floor else float(f0[i])
        t = i * float(shiftms) / 1000.0
        used[i] = cur
        origin[i] = matlab_round(t * fs + 0.001)
        half[i] = matlab_round(1.5 * fs / cur)
        dc[i] = 2 + int(cur * fftl / fs)
        width = cur * 2.0 / 3.0
        bound[i] = int(width * fftl / fs) + 1
        off[i] = acc
        acc += 2 * int(half[i]) + 1 + fftl // 2 + 1
    return dict(f0=used, origin=origin, half=half, dc_limit=dc, boundary=bound, offset=off, draws=acc)


def n_draws(f0, fs, shiftms, fftl=FFTL):
    return int(frame_shapes(f0, fs, shiftms, fftl)["draws"])


def _rfft(x, fft):
    if fft is None:
        return np.fft.rfft(x)
    return fft(x.astype(np.complex128))[:len(x) // 2 + 1]


def _even_fft(v, fft):
    """The (real, even) transform of the even extension of v (fftl / 2 + 1 values): fftl / 2 + 1 real values."""
    n = 2 * (len(v) - 1)
    if fft is None:
        return np.fft.irfft(v, n)[:len(v)] * n
    return fft(np.concatenate([v, v[-2:0:-1]]).astype(np.complex128)).real[:len(v)]


def window(half, cur, fs):
    """The F0-adaptive Hanning-type window of 2 * half + 1 samples, unit energy."""
    base = np.arange(-half, half + 1)
    pos = base / 1.5 / fs
    w = 0.5 * np.cos(np.pi * pos * cur) + 0.5
    return w / math.sqrt((w * w).sum())


def frame_power(x, cur, origin, half, dc_limit, fs, fftl, draws, fft=None):
    """Windowed waveform -> power spectrum with DC correction (fftl / 2 + 1 values)."""
    base = np.arange(-half, half + 1)
    safe = np.clip(origin + base, 0, len(x) - 1)
    w = window(half, cur, fs)
    wav = x[safe] * w + draws * NOISE_SCALE
    wav = wav - w * (wav.sum() / w.sum())
    buf = np.zeros(fftl)
    buf[:2 * half + 1] = wav
    X = _rfft(buf, fft)
    p = X.real * X.real + X.imag * X.imag
    # the replica mirrored at F0, added below it
    i = np.arange(dc_limit - 1)
    rep = interp_equal(cur, -(fs / fftl), p[:dc_limit + 1], i * fs / fftl)
    p[:dc_limit - 1] = p[:dc_limit - 1] + rep
    return p


def linear_smoothing(p, width, boundary, fs, fftl):
    K = fftl // 2 + 1
    b = boundary
    mir = np.concatenate([p[b:0:-1], p[:K - 1], p[K - 1 - np.arange(b + 1)]])
    seg = np.cumsum(mir * fs / fftl)
    axis = np.arange(K) / fftl * fs - width / 2.0
    x0 = -(b - 0.5) * fs / fftl
    dx = fs / fftl
    low = interp_equal(x0, dx, seg, axis)
    high = interp_equal(x0, dx, seg, axis + width)
    return (high - low) / width


def lifters(cur, fs, fftl, q1=Q1):
    K = fftl // 2 + 1
    q = np.arange(K) / fs
    sm, cp = np.ones(K), np.ones(K)
    sm[1:] = np.sin(np.pi * cur * q[1:]) / (np.pi * cur * q[1:])
    cp[1:] = (1.0 - 2.0 * q1) + 2.0 * q1 * np.cos(2.0 * np.pi * q[1:] * cur)
    return sm, cp


def cheaptrick(x, f0, fs, shiftms, fftl=FFTL, q1=Q1, fft=None):
    """pyworld cheaptrick(x, f0, temporal_positions = i * shiftms / 1000, fs, q1, fft_size = fftl): (T, fftl / 2 + 1)."""
    if fftl != FFTL:
        raise ValueError(f"fftl {fftl}: only {FFTL} is supported")
    x = np.asarray(x, np.float64).reshape(-1)
    if len(x) < 1:
        raise ValueError("an empty waveform")
    sh = frame_shapes(f0, fs, shiftms, fftl)
    T = len(sh["f0"])
    K = fftl // 2 + 1
    nz = noise(int(sh["draws"]))
    sp = np.empty((T, K))
    for i in range(T):
        cur, half, off = float(sh["f0"][i]), int(sh["half"][i]), int(sh["offset"][i])
        n = 2 * half + 1
        p = frame_power(x, cur, int(sh["origin"][i]), half, int(sh["dc_limit"][i]), fs, fftl, nz[off:off + n], fft)
        p = linear_smoothing(p, cur * 2.0 / 3.0, int(sh["boundary"][i]), fs, fftl)
        p = p + np.abs(nz[off + n:off + n + K]) * EPS
        c = _even_fft(np.log(p), fft)
        sm, cp = lifters(cur, fs, fftl, q1)
        sp[i] = np.exp(_even_fft(c * sm * cp / fftl, fft))
    return sp


# ---- pysptk / sprocket
def sp2mc(sp, order, alpha, fft=None):
    """pysptk sp2mc: c = irfft(log sp); c[0] /= 2; freqt(c, order, alpha)."""
    sp = np.asarray(sp, np.float64)
    lg = np.log(sp)
    n = 2 * (sp.shape[-1] - 1)
    if fft is None:
        c = np.fft.irfft(lg, n)
    else:
        flat = lg.reshape(-1, lg.shape[-1])
        c = np.stack([fft(np.concatenate([v, v[-2:0:-1]]).astype(np.complex128)).real / n for v in flat])
        c = c.reshape(lg.shape[:-1] + (n,))
    c = np.array(c)
    c[..., 0] /= 2.0
    return freqt(c, order, alpha)


def spc2npow(sp):
    """sprocket spc2npow: per-frame power (sp[0] + sp[-1] + 2 sum(sp[1:-1])) / fftl, in dB over the utterance's mean."""
    sp = np.asarray(sp, np.float64)
    fftl = 2 * (sp.shape[1] - 1)
    p = (sp[:, 0] + sp[:, -1] + 2.0 * sp[:, 1:-1].sum(1)) / fftl
    return 10.0 * np.log10(p / p.mean())


def analyze_mcep(x, f0, fs=22050, fftl=FFTL, shiftms=5.0, dim=34, alpha=0.455, cutoff=70, fft=None):
    """evaluate_mcd.py's get_world_features with the F0 given: float32 cast, low cut, CheapTrick, sp2mc."""
    x = low_cut_filter(np.array(x, dtype=np.float32), fs, cutoff)
    return sp2mc(cheaptrick(x, f0, fs, shiftms, fftl, fft=fft), dim, alpha, fft=fft)


def fft_radix2(z):
    """A plain iterative radix-2 decimation-in-time FFT (float64): the second, equally correct transform."""
    z = np.asarray(z, np.complex128)
    n = len(z)
    bits = n.bit_length() - 1
    if 1 << bits != n:
        raise ValueError("length must be a power of two")
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    a = z[rev].copy()
    half = 1
    while half < n:
        tw = np.exp(-2j * np.pi * np.arange(half) / (2 * half))
        a = a.reshape(-1, 2 * half)
        t = a[:, half:] * tw
        a = np.concatenate([a[:, :half] + t, a[:, :half] - t], axis=1).reshape(-1)
        half *= 2
    return a
