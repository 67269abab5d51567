"""Harvest F0 estimation restated in float64 numpy / scipy: the definition the crk_f0_* kernels are tested against.

It restates the published algorithm (M. Morise, "Harvest: a high-performance fundamental frequency estimator from speech
signals", Interspeech 2017) and what WORLD's implementation is known to do.  pyworld, sprocket and the WORLD sources are
not available to this project, so parity with ``pyworld.harvest`` is UNPINNED; DESIGN.md section 6e lists every constant
and edge rule that was chosen rather than known.  What is pinned: the kernels against this file stage by stage, and this
file against signals whose F0 is known (tests/test_harvest_cpu.py).

Every stage exists in two evaluation orders that differ only in rounding (direct / FFT band-pass, direct bins / numpy.fft
refinement spectra, float64 / numpy.longdouble decimation recurrence); their spread sizes the GPU tests' bounds.
"""
import math

import numpy as np

CH_PER_OCT = 40
NC = 16  # official candidates kept per frame (a frame of <= 192 channels holds at most 17 runs of 10; 16 are kept)
NS = 7 * NC  # slots per frame after the overlap
SHIFTS = (0, -1, -2, -3, 1, 2, 3)  # slot block b holds the candidates of frame i + SHIFTS[b]
NUTTALL = (0.355768, 0.487396, 0.144232, 0.012604)
SMOOTH_B = 0.0078202080334971724
SMOOTH_A = (-1.7347257688092754, 0.76600660094326412)
SMOOTH_PAD = 300
PAD = 9  # odd reflection of the decimation filter


def setup(fs, n, minf0, maxf0):
    floor, ceil = 0.9 * minf0, 1.1 * maxf0
    n_ch = 1 + int(np.log2(ceil / floor) * CH_PER_OCT)
    bf = floor * 2.0 ** ((np.arange(n_ch) + 1.0) / CH_PER_OCT)
    r = int(min(12, max(1, math.floor(fs / 8000.0 + 0.5))))
    fs_d = fs / r
    h = np.floor(2.0 * fs_d / bf + 0.5).astype(np.int64)
    return dict(fs=fs, n=n, floor=floor, ceil=ceil, n_ch=n_ch, bf=bf, r=r, fs_d=fs_d, h=h,
                frames=int(1000.0 * n / fs) + 1, nd=-(-n // r))


def cheby_coefficients(r):
    from scipy.signal import cheby1

    b, a = cheby1(3, 0.05, 0.8 / r)
    return np.asarray(b, np.float64), np.asarray(a, np.float64)


def _iir3(b, a, x, dtype):
    """y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] + b3 x[i-3] - a1 y[i-1] - a2 y[i-2] - a3 y[i-3], zero state, summed left to
    right."""
    b = [dtype(v) for v in b]
    a = [dtype(v) for v in a]
    y = np.zeros(len(x), dtype)
    x1 = x2 = x3 = y1 = y2 = y3 = dtype(0)
    for i in range(len(x)):
        x0 = x[i]
        v = b[0] * x0 + b[1] * x1 + b[2] * x2 + b[3] * x3 - a[1] * y1 - a[2] * y2 - a[3] * y3
        y[i] = v
        x3, x2, x1 = x2, x1, x0
        y3, y2, y1 = y2, y1, v
    return y


def decimate(x, r, dtype=np.float64):
    """Zero-phase order-3 Chebyshev-I low-pass (forward and backward, zero state, odd reflection of 9 samples), every r-th
    sample, mean removed.  r = 1 only removes the mean."""
    x = np.asarray(x, np.float64).astype(dtype)
    if r > 1:
        b, a = cheby_coefficients(r)
        n = len(x)
        p = np.concatenate([2 * x[0] - x[PAD:0:-1], x, 2 * x[-1] - x[-2:-PAD - 2:-1]])
        y = _iir3(b, a, _iir3(b, a, p, dtype)[::-1], dtype)[::-1]
        x = y[PAD:PAD + n][::r]
    return (x - x.sum() / dtype(len(x))).astype(np.float64)


def bandpass_taps(h, bf, fs_d):
    k = np.arange(-h, h + 1)
    p = (k + h) / (2.0 * h)
    w = (NUTTALL[0] - NUTTALL[1] * np.cos(2 * np.pi * p) + NUTTALL[2] * np.cos(4 * np.pi * p)
         - NUTTALL[3] * np.cos(6 * np.pi * p))
    return w * np.cos(2 * np.pi * bf * k / fs_d)


def bandpass(y, h, bf, fs_d, fft=False):
    taps = bandpass_taps(int(h), bf, fs_d)
    if not fft:
        return np.convolve(y, taps)[h:h + len(y)]
    n = 1 << int(np.ceil(np.log2(len(y) + len(taps))))
    return np.fft.irfft(np.fft.rfft(y, n) * np.fft.rfft(taps, n), n)[h:h + len(y)]


GATE = 1e-10  # a filtered value within GATE * peak |input| * h of zero is rounding residue and taken as exactly zero


def crossings(s):
    """(negative-going, positive-going) sub-sample zero crossings of s, 0-based."""
    a, b = s[:-1], s[1:]
    out = []
    for m in ((a > 0) & (b <= 0), (a < 0) & (b >= 0)):
        i = np.nonzero(m)[0]
        out.append(i + a[i] / (a[i] - b[i]))
    return out


def event_streams(s, gate):
    """The four event streams of a filtered signal: crossings of s and of its first difference, both with the values
    within `gate` of zero flushed to zero first."""
    s = np.where(np.abs(s) <= gate, 0.0, s)
    d = s[1:] - s[:-1]
    return crossings(s) + crossings(np.where(np.abs(d) <= gate, 0.0, d))


def interp_stream(e, fs_d, t):
    """WORLD interp1 of the stream's (location, frequency) knots at the frame times t."""
    x = (e[:-1] + e[1:]) / 2.0 / fs_d
    y = fs_d / (e[1:] - e[:-1])
    j = np.clip(np.searchsorted(x, t, side="right") - 1, 0, len(x) - 2)
    s = (t - x[j]) / (x[j + 1] - x[j])
    return y[j] + s * (y[j + 1] - y[j])


def raw_candidates(yd, cfg, fft=False, return_average=False):
    """(channels, frames) table of raw candidates; 0 marks an empty cell."""
    T = cfg["frames"]
    t = np.arange(T) / 1000.0
    raw = np.zeros((cfg["n_ch"], T))
    avg = np.zeros((cfg["n_ch"], T))
    peak = float(np.max(np.abs(yd)))
    for c in range(cfg["n_ch"]):
        bf = cfg["bf"][c]
        ev = event_streams(bandpass(yd, int(cfg["h"][c]), bf, cfg["fs_d"], fft), GATE * peak * int(cfg["h"][c]))
        if min(len(e) for e in ev) < 3:
            continue
        v = [interp_stream(e, cfg["fs_d"], t) for e in ev]
        a = (((v[0] + v[1]) + v[2]) + v[3]) / 4.0
        avg[c] = a
        keep = (a >= 0.9 * bf) & (a <= 1.1 * bf) & (a >= cfg["floor"]) & (a <= cfg["ceil"])
        raw[c] = np.where(keep, a, 0.0)
    return (raw, avg) if return_average else raw


def official_candidates(raw):
    """(frames, NC): the mean of every run of at least 10 non-empty channels, first and last channel forced empty."""
    n_ch, T = raw.shape
    out = np.zeros((T, NC))
    for i in range(T):
        k, c = 0, 1
        while c < n_ch - 1:
            if raw[c, i] == 0.0:
                c += 1
                continue
            e, acc = c, 0.0
            while e < n_ch - 1 and raw[e, i] != 0.0:
                acc += raw[e, i]
                e += 1
            if e - c >= 10 and k < NC:
                out[i, k] = acc / (e - c)
                k += 1
            c = e
    return out


def overlap(off):
    T = off.shape[0]
    out = np.zeros((T, NS))
    for b, sh in enumerate(SHIFTS):
        lo, hi = max(0, -sh), min(T, T - sh)
        out[lo:hi, b * NC:(b + 1) * NC] = off[lo + sh:hi + sh]
    return out


def refine_one(x, fs, f, t, floor, ceil, fft=False):
    """(refined F0, score) of candidate f at time t; (0, 0) when rejected."""
    half = int(1.5 * fs / f + 1.0)
    n = 2 * half + 1
    N = 1 << (2 + int(math.floor(math.log2(n))))
    k = np.arange(n)
    idx = np.floor((t + (k - half) / float(fs)) * fs + 0.001 + 0.5).astype(np.int64)
    tt = idx / float(fs) - t
    T = n / float(fs)
    w = 0.42 + 0.5 * np.cos(2 * np.pi * tt / T) + 0.08 * np.cos(4 * np.pi * tt / T)
    d = np.empty(n)
    d[0] = -w[1] / 2.0
    d[1:-1] = -(w[2:] - w[:-2]) / 2.0
    d[-1] = w[-2] / 2.0
    xs = x[np.clip(idx, 0, len(x) - 1)]
    nh = min(int(fs / 2.0 / f), 6)
    m = np.arange(1, nh + 1)
    km = np.floor(f * N / fs * m + 0.5).astype(np.int64)
    if fft:
        M = np.fft.fft(xs * w, N)[km % N]
        D = np.fft.fft(xs * d, N)[km % N]
    else:
        ph = 2 * np.pi * ((km[:, None] * k[None, :]) % N) / N
        tw = np.cos(ph) - 1j * np.sin(ph)
        M, D = tw @ (xs * w), tw @ (xs * d)
    with np.errstate(all="ignore"):
        power = M.real ** 2 + M.imag ** 2
        inst = km * float(fs) / N + (M.real * D.imag - M.imag * D.real) / power * fs / (2 * np.pi)
        amp = np.sqrt(power)
        ref = np.sum(amp * inst) / np.sum(amp * m)
        score = 1.0 / (1e-12 + np.sum(np.abs(inst / m - f)) / nh / f)
    if ref >= floor and ref <= ceil and score >= 2.5:
        return ref, score
    return 0.0, 0.0


def refine(x, fs, cands, floor, ceil, fft=False):
    x = np.asarray(x, np.float64)
    ref, sc = np.zeros_like(cands), np.zeros_like(cands)
    for i, j in zip(*np.nonzero(cands)):
        ref[i, j], sc[i, j] = refine_one(x, fs, cands[i, j], i / 1000.0, floor, ceil, fft)
    return ref, sc


def remove_unreliable(cands, scores):
    c, s = cands.copy(), scores.copy()
    T = len(cands)
    for i in range(1, T - 1):
        for j in np.nonzero(cands[i])[0]:
            f = cands[i, j]
            e = min(np.min(np.abs(f - cands[i - 1]) / f), np.min(np.abs(f - cands[i + 1]) / f))
            if e > 0.05:
                c[i, j] = s[i, j] = 0.0
    return c, s


def _boundaries(f):
    v = f != 0
    v[0] = v[-1] = False
    d = np.diff(v.astype(np.int8))
    return list(zip(np.nonzero(d == 1)[0] + 1, np.nonzero(d == -1)[0]))  # inclusive (start, end)


def _select(prev, row, allowed):
    best, err = 0.0, allowed
    for c in row:
        e = abs(prev - c) / prev
        if e > err:
            continue
        best, err = c, e
    return best


def _search_score(f, row, srow):
    m = row == f
    return max(0.0, srow[m].max()) if m.any() else 0.0


def _smooth(seg):
    def run(v):
        y = np.zeros(len(v))
        x1 = x2 = y1 = y2 = 0.0
        for i, x0 in enumerate(v):
            o = SMOOTH_B * x0 + 2.0 * SMOOTH_B * x1 + SMOOTH_B * x2 - SMOOTH_A[0] * y1 - SMOOTH_A[1] * y2
            y[i] = o
            x2, x1, y2, y1 = x1, x0, y1, o
        return y

    p = np.concatenate([np.full(SMOOTH_PAD, seg[0]), seg, np.full(SMOOTH_PAD, seg[-1])])
    return run(run(p)[::-1])[::-1][SMOOTH_PAD:SMOOTH_PAD + len(seg)]


def contour(cands, scores, return_steps=False):
    """Steps 7 - 9: the 1 ms contour from the refined candidate and score tables."""
    T = len(cands)
    c, s = remove_unreliable(cands, scores)
    best = np.argmax(s, axis=1)
    base = np.where(s.max(axis=1) > 0, c[np.arange(T), best], 0.0)
    step1 = np.zeros(T)
    with np.errstate(all="ignore"):
        for i in range(2, T):
            if base[i] == 0:
                continue
            ref = base[i - 1] * 2 - base[i - 2]
            jump = abs((base[i] - ref) / ref) > 0.008 and abs((base[i] - base[i - 1]) / base[i - 1]) > 0.008
            step1[i] = 0.0 if jump else base[i]
    step2 = step1.copy()
    for a, b in _boundaries(step1):
        if b - a + 1 < 6:
            step2[a:b + 1] = 0.0
    merged = np.zeros(T)
    cs = ce = -1
    for a, b in _boundaries(step2):
        ext = np.zeros(T)
        ext[a:b + 1] = step2[a:b + 1]
        na, nb, prev = a, b, step2[b]
        for i in range(b + 1, min(T - 2, b + 100) + 1):
            v = _select(prev, c[i], 0.18)
            if v == 0:
                break
            ext[i], prev, nb = v, v, i
        prev = step2[a]
        for i in range(a - 1, max(1, a - 100) - 1, -1):
            v = _select(prev, c[i], 0.18)
            if v == 0:
                break
            ext[i], prev, na = v, v, i
        if not (nb - na + 1) > 2200.0 / (ext[na:nb + 1].sum() / (nb - na + 1)):
            continue
        if ce < 0 or na > ce:
            merged[na:nb + 1] = ext[na:nb + 1]
            cs, ce = na, nb
        elif cs <= na and ce >= nb:
            pass
        else:
            s1 = sum(_search_score(merged[i], c[i], s[i]) for i in range(na, ce + 1))
            s2 = sum(_search_score(ext[i], c[i], s[i]) for i in range(na, ce + 1))
            if s1 > s2:
                merged[ce + 1:nb + 1] = ext[ce + 1:nb + 1]
            else:
                merged[na:nb + 1] = ext[na:nb + 1]
            ce = nb
    step4 = merged.copy()
    runs = _boundaries(merged)
    for (_, e0), (s1, _) in zip(runs, runs[1:]):
        if s1 - e0 - 1 < 9:
            for j in range(e0 + 1, s1):
                step4[j] = merged[e0] + (merged[s1] - merged[e0]) * (j - e0) / (s1 - e0)
    out = np.zeros(T)
    for a, b in _boundaries(step4):
        out[a:b + 1] = _smooth(step4[a:b + 1])
    if return_steps:
        return out, dict(base=base, step1=step1, step2=step2, merged=merged, step4=step4)
    return out


def subsample(f1, n, fs, shiftms):
    T = int(1000.0 * n / fs / shiftms) + 1
    return f1[np.minimum(np.arange(T) * int(round(shiftms)), len(f1) - 1)]


def harvest(x, fs, minf0, maxf0, shiftms=5, variant=False, return_stages=False):
    """F0 contour at shiftms.  variant=True takes the other evaluation order at every stage."""
    x = np.asarray(x, np.float64)
    cfg = setup(fs, len(x), minf0, maxf0)
    yd = decimate(x, cfg["r"], np.longdouble if variant else np.float64)
    raw, avg = raw_candidates(yd, cfg, fft=variant, return_average=True)
    cands = overlap(official_candidates(raw))
    ref, sc = refine(x, fs, cands, cfg["floor"], cfg["ceil"], fft=variant)
    f1 = contour(ref, sc)
    f0 = subsample(f1, len(x), fs, shiftms)
    if return_stages:
        return f0, dict(cfg=cfg, yd=yd, raw=raw, raw_average=avg, cands=cands, refined=ref, scores=sc, f1=f1)
    return f0


def continuous_f0(f0):
    """The reference's convert_continuos_f0 and feature.py:86-88: (uv float32, cf0, lf0, lcf0) and the contour with its
    ends overwritten, which is what lf0 is taken from."""
    f0 = np.array(f0, np.float64)
    uv = np.float32(f0 != 0)
    nz = f0[f0 != 0]
    if len(nz) == 0:
        raise ValueError("no voiced frame")
    si = np.where(f0 == nz[0])[0][0]
    ei = np.where(f0 == nz[-1])[0][-1]
    f0[:si] = nz[0]
    f0[ei:] = nz[-1]
    k = np.where(f0 != 0)[0]
    cf0 = np.empty(len(f0))
    for i in range(len(f0)):  # scipy interp1d, which for 1-D linear data is numpy.interp: a knot returns its own value
        if f0[i] != 0:
            cf0[i] = f0[i]
            continue
        j = np.searchsorted(k, i)
        lo, hi = k[j - 1], k[j]
        cf0[i] = (f0[hi] - f0[lo]) / (hi - lo) * (i - lo) + f0[lo]
    return uv, cf0, np.log(f0 + 1e-10), np.log(cf0), f0
