"""Seeded WORLD synthesis inputs shared by the tests and tools/bench_world.py: smooth decaying mel-cepstra, F0 contours
of 90-260 Hz with unvoiced runs, and coded aperiodicity (0 dB on unvoiced frames, as WORLD codes them)."""
import numpy as np


def _smooth(rng, T, scale):
    """A random walk low-passed over ~8 frames."""
    w = np.cumsum(rng.standard_normal(T)) * scale
    L = min(8, T)
    return np.convolve(w, np.ones(L) / L, mode="same")


def _cepstra(rng, T, order1):
    """(mcep, rmcep), each [T][order1]."""
    k = np.arange(order1)
    mcep = np.stack([_smooth(rng, T, 0.05) for _ in k], 1) * 0.6 ** k + rng.standard_normal(order1) * 0.5 * 0.6 ** k
    mcep[:, 0] += -2.0
    rmcep = mcep + np.stack([_smooth(rng, T, 0.02) for _ in k], 1) * 0.5 ** k
    return mcep, rmcep


def _codeap(rng, voiced, bands):
    return np.where(voiced[:, None], -25.0 + 8.0 * rng.random((len(voiced), bands)) + np.arange(bands) * 4.0, 0.0)


def utterance(rng, T, order1, bands):
    """(f0 [T], mcep [T][order1], codeap [T][bands], rmcep [T][order1]) of one utterance."""
    t = np.arange(T)
    mcep, rmcep = _cepstra(rng, T, order1)
    base = rng.uniform(110, 200)
    f0 = np.clip(base + 40 * np.sin(2 * np.pi * t / rng.uniform(40, 120) + rng.uniform(0, 6)) + _smooth(rng, T, 0.5),
                 90, 260)
    voiced = np.ones(T, bool)
    start = int(rng.integers(0, 25))
    while start < T:  # unvoiced runs of 5-20 frames every 30-90 frames
        voiced[start:start + int(rng.integers(5, 21))] = False
        start += int(rng.integers(30, 91))
    if T <= 3:
        voiced[:] = True
        voiced[-1] = T == 2
    f0 = np.where(voiced, f0, 0.0)
    return f0, mcep, _codeap(rng, voiced, bands), rmcep


def with_f0(rng, f0, order1, bands):
    """The same 4-tuple for a given F0 contour: seeded cepstra, coded aperiodicity voiced wherever f0 > 0."""
    f0 = np.asarray(f0, np.float64).reshape(-1)
    mcep, rmcep = _cepstra(rng, len(f0), order1)
    return f0, mcep, _codeap(rng, f0 > 0, bands), rmcep


def contour(rng, T, lo, hi):
    """A voiced F0 contour of T frames wandering smoothly inside [lo, hi]."""
    t = np.arange(T)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    return np.clip(mid + 0.8 * half * np.sin(2 * np.pi * t / rng.uniform(6, 30) + rng.uniform(0, 6)), lo, hi)
