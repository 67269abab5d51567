"""F0 contours shared by the streaming WORLD synthesis tests (tests/test_wsyn_stream_cpu.py, tests/
test_gpu_wsyn_stream.py) at fs 16000, shiftms 5: each holds voiced and unvoiced runs of at least 3 frames entered and left
from both sides, one row below the time base's floor fs // 1024 + 1 = 16 Hz (treated as 0), 17 Hz rows next to zeros
(the longest pulse intervals the rate allows), one row at 800 Hz; one ends 300 then 100 Hz (the extrapolated knot is
negative), one is unvoiced throughout."""
import numpy as np

FS, SHIFTMS, ALPHA = 16000, 5.0, 0.41


def contour(T, seed):
    """T frames (T >= 20): unvoiced, voiced, a 12 Hz row, unvoiced, a run of 17 Hz, unvoiced, 800 Hz, voiced to the end."""
    rng = np.random.default_rng(seed)
    f0 = 120.0 + 60.0 * np.sin(np.arange(T) / 3.0 + rng.uniform(0, 6)) + rng.uniform(0, 20, T)
    f0[:3] = 0.0
    f0[6] = 12.0
    f0[9:12] = 0.0
    run = min(26, T - 19)
    f0[12:12 + run] = 17.0
    f0[12 + run:15 + run] = 0.0
    f0[16 + run] = 800.0
    return f0


def streams():
    """The four contours of the GPU tests: 60, 41, 33 and 2 frames."""
    a = contour(60, 0)
    b = contour(41, 1)
    b[-2:] = (300.0, 100.0)  # the extrapolated knot is -100 Hz
    b[-6:-3] = 0.0           # an unvoiced run left into voiced rows before the end
    c = np.zeros(33)         # unvoiced throughout
    d = np.array([180.0, 0.0])
    return [a, b, c, d]


def short(T, seed):
    """T in 2 .. 12 frames for the CPU walk of every cut: the same edges packed tightly."""
    base = np.array([0.0, 150.0, 12.0, 17.0, 0.0, 0.0, 800.0, 210.0, 0.0, 190.0, 300.0, 100.0])
    rng = np.random.default_rng(seed)
    f0 = base[-T:].copy() if T % 2 else base[:T].copy()
    if T == 7:
        f0[:] = 0.0  # unvoiced throughout
    return np.where((f0 > 20) & (f0 < 700), f0 + rng.uniform(0, 5, T), f0)
