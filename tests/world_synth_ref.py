"""Test-side CPU restatement of WORLD waveform synthesis for mel-cepstral models (float64, numpy): what the reference's
``crank.utils.world2wav`` runs through sprocket's ``Synthesizer.synthesis`` - power modification (sprocket
``mod_power`` with pysptk ``mc2e``), pysptk ``mc2sp``, pyworld ``decode_aperiodicity`` and pyworld ``synthesize``.
It is the oracle of crank_amd/world.py (csrc/world_kernels.hip).

Parity of this restatement against pyworld / pysptk / sprocket is UNPINNED: none of them is installed.  The steps are
restated from the published algorithms (WORLD synthesis.cpp / codec.cpp / matlabfunctions.cpp, SPTK freqt / c2ir,
pysptk mc2sp / mc2e, sprocket mod_power).  Three choices are this project's and are shared with the kernels:
  * the cepstra of the minimum-phase recipe are taken as the real part of the FFT of the (real, even) log spectrum;
  * cos of the fractional delay is one fixed polynomial (cos_poly), since WORLD's sin = sqrt(1 - cos^2) magnifies a
    last-bit difference between two cosine implementations at small angles;
  * a pulse whose interval exceeds fftl (voiced F0 below about 2 fs / fftl) draws noise_size values from the stream as
    always but uses only the first fftl of them (their own mean removed); the periodic part keeps sqrt(noise_size).
    WORLD itself writes past its fftl-sized buffer in that case.
The lowest F0 of the time base is ``fs // fftl + 1`` (WORLD divides the integers).

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

IRLEN = 1024  # sprocket mod_power's impulse response length
SAFE = 1e-12  # WORLD's kMySafeGuardMinimum
DEFAULT_F0 = 500.0  # WORLD's kDefaultF0: the pulse rate of unvoiced samples
FFTL = 1024  # the only fftl supported


def n_bands(fs):
    """WORLD GetNumberOfAperiodicities: bands of 3 kHz below min(15 kHz, fs/2 - 3 kHz)."""
    return int(min(15000.0, fs / 2.0 - 3000.0) / 3000.0)


def check_args(fs, fftl, T, bands):
    if fftl != FFTL:
        raise ValueError(f"fftl {fftl}: only {FFTL} is supported")
    if T < 2:
        raise ValueError(f"{T} frames: WORLD synthesis needs at least 2")
    if bands != n_bands(fs):
        raise ValueError(f"coded aperiodicity of {bands} bands; fs {fs} has {n_bands(fs)}")


# ---- SPTK / pysptk
def freqt(c, order, alpha):
    """SPTK freqt, vectorised over leading axes: c (..., m1 + 1) -> (..., order + 1)."""
    c = np.asarray(c, np.float64)
    g = np.zeros(c.shape[:-1] + (order + 1,))
    b = 1.0 - alpha * alpha
    for i in range(c.shape[-1] - 1, -1, -1):
        d = g.copy()
        g[..., 0] = c[..., i] + alpha * d[..., 0]
        if order >= 1:
            g[..., 1] = b * d[..., 0] + alpha * d[..., 1]
        for m in range(2, order + 1):
            g[..., m] = d[..., m - 1] + alpha * (d[..., m] - g[..., m - 1])
    return g


def c2ir(c, irlen):
    """SPTK c2ir: h[0] = exp(c0), h[n] = sum_{k=1..n} k c_k h[n-k] / n (c has at least irlen coefficients)."""
    c = np.asarray(c, np.float64)
    kc = c[..., :irlen] * np.arange(irlen)
    h = np.zeros(c.shape[:-1] + (irlen,))
    h[..., 0] = np.exp(c[..., 0])
    for n in range(1, irlen):
        h[..., n] = (kc[..., 1:n + 1] * h[..., n - 1::-1][..., :n]).sum(-1) / n
    return h


def mc2e(mc, alpha, irlen=IRLEN):
    """pysptk mc2e: the energy of the impulse response of the mel-cepstrum."""
    h = c2ir(freqt(mc, irlen, -alpha), irlen)
    return (h * h).sum(-1)


def mod_power(mcep, rmcep, alpha, irlen=IRLEN):
    """sprocket mod_power: the 0th coefficient shifted so that every frame has the energy of rmcep's frame."""
    mcep = np.array(mcep, np.float64)
    rmcep = np.asarray(rmcep, np.float64)
    if rmcep.shape != mcep.shape:
        raise ValueError(f"rmcep {rmcep.shape} and mcep {mcep.shape} differ")
    mcep[:, 0] += np.log(mc2e(rmcep, alpha, irlen) / mc2e(mcep, alpha, irlen)) / 2
    return mcep


def mc2sp(mc, alpha, fftl):
    """pysptk mc2sp: exp(Re rfft(symmetric cepstrum)), the cepstrum being freqt(mc, fftl / 2, -alpha)."""
    c = freqt(mc, fftl // 2, -alpha)
    symc = np.zeros(c.shape[:-1] + (fftl,))
    symc[..., 0] = 2 * c[..., 0]
    symc[..., 1:fftl // 2 + 1] = c[..., 1:]
    symc[..., fftl // 2 + 1:] = c[..., 1:fftl // 2][..., ::-1]
    return np.exp(np.fft.rfft(symc).real)


# ---- WORLD
def interp1(x, y, xi):
    """WORLD interp1 (histc + linear): j = the last knot with x[j] <= xi, at most len(x) - 2."""
    out = np.empty(len(xi))
    for i, v in enumerate(xi):
        j = 0
        while j + 1 < len(x) - 1 and x[j + 1] <= v:
            j += 1
        s = (v - x[j]) / (x[j + 1] - x[j])
        out[i] = y[j] + s * (y[j + 1] - y[j])
    return out


def decode_aperiodicity(cap, fs, fftl):
    """WORLD DecodeAperiodicity: (T, B) coded band aperiodicity in dB -> (T, fftl / 2 + 1)."""
    cap = np.asarray(cap, np.float64)
    T, B = cap.shape
    check_args(fs, fftl, max(T, 2), B)
    K = fftl // 2 + 1
    ap = np.full((T, K), 1.0 - SAFE)
    faxis = np.array([float(fs) / fftl * k for k in range(K)])
    knots = np.array([3000.0 * b for b in range(B + 1)] + [fs / 2.0])
    for t in range(T):
        if cap[t].sum() / B > -0.5:
            continue  # unvoiced
        vals = np.concatenate([[-60.0], cap[t], [-SAFE]])
        ap[t] = 10.0 ** (interp1(knots, vals, faxis) / 20.0)
    return ap


def randn_table(n):
    """WORLD randn after randn_reseed: n values, each the sum of 12 xorshift128 draws >> 4, / 2^28, - 6."""
    x, y, z, w = 123456789, 362436069, 521288629, 88675123
    M = 0xFFFFFFFF
    out = np.empty(n)
    for i in range(n):
        acc = 0
        for _ in range(12):
            t = (x ^ (x << 11)) & M
            x, y, z = y, z, w
            w = (w ^ (w >> 19)) ^ (t ^ (t >> 8))
            acc += w >> 4
        out[i] = acc / 268435456.0 - 6.0
    return out


_NOISE = np.zeros(0)


def noise(n):
    global _NOISE
    if len(_NOISE) < n:
        _NOISE = randn_table(max(n, 2 * len(_NOISE)))
    return _NOISE[:n]


def y_length(T, fs, shiftms):
    """pyworld synthesize's output length."""
    return int(T * shiftms * fs / 1000)


def time_base(f0, fs, fftl, shiftms):
    """WORLD GetTimeBase: (pulse samples, fractional shifts in seconds, interpolated vuv per sample, y_length)."""
    f0 = np.asarray(f0, np.float64).reshape(-1)
    T = len(f0)
    ylen = y_length(T, fs, shiftms)
    fp = shiftms / 1000.0
    lowest = fs // fftl + 1.0
    cf0 = [0.0 if v < lowest else float(v) for v in f0]
    cvuv = [0.0 if v == 0.0 else 1.0 for v in cf0]
    cf0.append(cf0[T - 1] * 2 - cf0[T - 2])
    cvuv.append(cvuv[T - 1] * 2 - cvuv[T - 2])
    tx = [t * fp for t in range(T + 1)]
    two_pi = 2.0 * math.pi
    vuv = np.zeros(ylen)
    wrap = np.zeros(ylen)
    total = 0.0
    j = 0
    for i in range(ylen):
        xi = i / fs
        while j + 1 < T and tx[j + 1] <= xi:
            j += 1
        s = (xi - tx[j]) / (tx[j + 1] - tx[j])
        v = 1.0 if cvuv[j] + s * (cvuv[j + 1] - cvuv[j]) > 0.5 else 0.0
        f = cf0[j] + s * (cf0[j + 1] - cf0[j]) if v != 0.0 else DEFAULT_F0
        total = total + two_pi * f / fs  # in sample order: the pulse positions depend on every rounding
        vuv[i] = v
        wrap[i] = math.fmod(total, two_pi)
    pos, shift = [], []
    for i in range(ylen - 1):
        if abs(wrap[i + 1] - wrap[i]) > math.pi:
            y1, y2 = wrap[i] - two_pi, wrap[i + 1]
            pos.append(i)
            shift.append(-y1 / (y2 - y1) / fs)
    return np.array(pos, np.int64), np.array(shift), vuv, ylen


def minimum_phase(log_amp):
    """The minimum-phase spectrum (K complex) of a log amplitude (K real): real cepstrum, fold, FFT, exp."""
    K = len(log_amp)
    N = 2 * (K - 1)
    sym = np.concatenate([log_amp, log_amp[1:K - 1][::-1]])
    c = np.fft.fft(sym).real
    c[1:N // 2] *= 2.0
    c[N // 2 + 1:] = 0.0
    return np.exp(np.fft.fft(c)[:K] / N)


COS_TAYLOR = [(-1) ** n / math.factorial(2 * n) for n in range(16)]


def cos_poly(x):
    """cos(x), x in [0, pi], as the 16-term Taylor polynomial in x^2 (Horner, every operation rounded on its own): the
    kernels evaluate the same operations, because sqrt(1 - cos^2) below magnifies a last-bit difference of cos."""
    x2 = x * x
    r = np.full_like(x2, COS_TAYLOR[15])
    for n in range(14, -1, -1):
        r = r * x2 + COS_TAYLOR[n]
    return r


def dc_remover(N):
    w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 1.0) / (1.0 + N)) for i in range(N // 2)])
    w = w / (2.0 * w.sum())
    return np.concatenate([w, w[::-1]])


def periodic_spectrum(env, ratio):
    """The periodic part's spectrum before the time shift: minimum phase of log(sp (1 - ratio) + 1e-12) / 2."""
    return minimum_phase(np.log(env * (1.0 - ratio) + SAFE) / 2.0)


def pulse_response(env, ratio, vuv, ns, shift, fs, noise_seg):
    """One pulse's response (N samples) of WORLD GetOneFrameSegment."""
    K = len(env)
    N = 2 * (K - 1)
    if vuv <= 0.5 or ratio[0] > 0.999:
        per = np.zeros(N)
    else:
        X = periodic_spectrum(env, ratio)
        coef = 2.0 * math.pi * shift * fs / N
        cs = cos_poly(coef * np.arange(K))
        sn = np.sqrt(np.maximum(1.0 - cs * cs, 0.0))  # the polynomial may round past -1 near pi
        X = X * (cs - 1j * sn)
        per = np.fft.fftshift(np.fft.irfft(X, N) * N)
        dc = per[N // 2:].sum()
        w = dc_remover(N)
        per[:N // 2] = -dc * w[:N // 2]
        per[N // 2:] -= dc * w[N // 2:]
    la = np.log(env * ratio + SAFE) / 2.0 if vuv != 0.0 else np.log(env + SAFE) / 2.0
    nz = np.zeros(N)
    m = min(ns, N)
    if m > 0:
        nz[:m] = noise_seg[:m] - noise_seg[:m].mean()
    ape = np.fft.fftshift(np.fft.irfft(minimum_phase(la) * np.fft.rfft(nz), N) * N)
    return (per * math.sqrt(ns) + ape) / N


def frame_tables(mcep, codeap, rmcep, fs, fftl, alpha):
    """(sp, ap): the per-frame power spectrum and aperiodicity synthesis reads."""
    mcep = np.asarray(mcep, np.float64)
    if rmcep is not None:
        mcep = mod_power(mcep, rmcep, alpha)
    return mc2sp(mcep, alpha, fftl), decode_aperiodicity(codeap, fs, fftl)


def pulses(f0, fs, fftl, shiftms):
    """(pulse samples, noise sizes, shifts, vuv at each pulse, y_length)."""
    pos, shift, vuv, ylen = time_base(f0, fs, fftl, shiftms)
    ns = np.zeros(len(pos), np.int64)
    ns[:-1] = pos[1:] - pos[:-1]
    return pos, ns, shift, vuv[pos], ylen


def synthesize(f0, sp, ap, fs, shiftms, fftl=FFTL):
    """pyworld synthesize(f0, sp, ap, fs, frame_period=shiftms): the waveform of y_length(T) samples (not clipped)."""
    sp, ap = np.asarray(sp, np.float64), np.asarray(ap, np.float64)
    T = sp.shape[0]
    N = fftl
    pos, ns, shift, pvuv, ylen = pulses(f0, fs, fftl, shiftms)
    y = np.zeros(ylen)
    if len(pos) == 0:
        return y
    fp = shiftms / 1000.0
    tab = noise(int(pos[-1] - pos[0]) + 1)
    asafe = np.clip(ap, 0.001, 0.999999999999)
    for p in range(len(pos)):
        q = pos[p] / fs / fp
        lo, hi = min(T - 1, int(math.floor(q))), min(T - 1, int(math.ceil(q)))
        if lo == hi:
            env, ratio = np.abs(sp[lo]), asafe[lo] ** 2
        else:
            a = q - lo
            env = (1.0 - a) * np.abs(sp[lo]) + a * np.abs(sp[hi])
            ratio = ((1.0 - a) * asafe[lo] + a * asafe[hi]) ** 2
        st = int(pos[p] - pos[0])
        seg = noise(st + min(int(ns[p]), N))[st:]
        r = pulse_response(env, ratio, pvuv[p], int(ns[p]), shift[p], fs, seg)
        off = int(pos[p]) - N // 2 + 1
        a0, a1 = max(0, -off), min(N, ylen - off)
        y[a0 + off:a1 + off] += r[a0:a1]  # overlap-add, pulse after pulse
    return y


def synthesis(f0, mcep, codeap, rmcep=None, fs=22050, fftl=FFTL, shiftms=5.0, alpha=0.42):
    """sprocket Synthesizer(fs, fftl, shiftms).synthesis(f0, mcep, codeap, rmcep, alpha)."""
    mcep = np.asarray(mcep, np.float64)
    check_args(fs, fftl, mcep.shape[0], np.asarray(codeap).shape[1])
    if np.asarray(f0).reshape(-1).shape[0] != mcep.shape[0] or np.asarray(codeap).shape[0] != mcep.shape[0]:
        raise ValueError("f0, mcep and codeap must have the same number of frames")
    sp, ap = frame_tables(mcep, codeap, rmcep, fs, fftl, alpha)
    return synthesize(f0, sp, ap, fs, shiftms, fftl)


def world2wav(f0, mcep, codeap, rmcep=None, fs=22050, fftl=FFTL, shiftms=10, alpha=0.455):
    """crank.utils.world2wav without the file: the synthesis clipped to [-1, 1]."""
    return np.clip(synthesis(f0, mcep, codeap, rmcep, fs, fftl, shiftms, alpha), -1.0, 1.0)
