"""Seeded WORLD synthesis inputs shared by the tests and tools/bench_world.py: smooth decaying mel-cepstra, F0 contours
of 90-260 Hz with unvoiced runs, and coded aperiodicity (0 dB on unvoiced frames, as WORLD codes them)."""
import numpy as np


def utterance(rng, T, order1, bands):
    """(f0 [T], mcep [T][order1], codeap [T][bands], rmcep [T][order1]) of one utterance."""
    t = np.arange(T)
    k = np.arange(order1)

    def smooth(scale):  # a random walk low-passed over ~8 frames
        w = np.cumsum(rng.standard_normal(T)) * scale
        L = min(8, T)
        return np.convolve(w, np.ones(L) / L, mode="same")

    mcep = np.stack([smooth(0.05) for _ in k], 1) * 0.6 ** k + rng.standard_normal(order1) * 0.5 * 0.6 ** k
    mcep[:, 0] += -2.0
    rmcep = mcep + np.stack([smooth(0.02) for _ in k], 1) * 0.5 ** k
    base = rng.uniform(110, 200)
    f0 = np.clip(base + 40 * np.sin(2 * np.pi * t / rng.uniform(40, 120) + rng.uniform(0, 6)) + smooth(0.5), 90, 260)
    voiced = np.ones(T, bool)
    start = int(rng.integers(0, 25))
    while start < T:  # unvoiced runs of 5-20 frames every 30-90 frames
        voiced[start:start + int(rng.integers(5, 21))] = False
        start += int(rng.integers(30, 91))
    if T <= 3:
        voiced[:] = True
        voiced[-1] = T == 2
    f0 = np.where(voiced, f0, 0.0)
    cap = np.where(voiced[:, None], -25.0 + 8.0 * rng.random((T, bands)) + np.arange(bands) * 4.0, 0.0)
    return f0, mcep, cap, rmcep
