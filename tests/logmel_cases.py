"""Inputs of the log-mel front-end tests (crank_amd/csrc/mlfb_kernels.hip), their float64 reference and the tolerance
of the GPU tests.  Host only: numpy and the fp32 oracle (oracle/modules.py: ``torch.stft`` in float32); nothing here
imports crank_amd.

A case is a dict: framing (fs, n_fft, hop, win, window, center), a mel basis (Slaney ``mel = (n_mels, fmin, fmax)``, or
``basis = <name>`` of a synthetic (n_bins, n_mels) matrix that goes through ``ops.logmel``), a seeded signal
``sig = (kind, B, n_samples)``, an optional scaler (mean / var of tests/golden/stft_layer.npz), the kernel that runs it
("wave": n_fft 1024; "radix2": every other size; "radix2_env": n_fft 1024 in a child process under CRK_LOGMEL_WAVE=0)
and the metrics that apply:

* ``lin``: max |10^got - 10^ref| / (largest mel energy of that frame), after the clamp and before the scaler (undone in
  float64) - every case, over its non-silent frames;
* ``log``: max |got - ref| of the values as returned - the broad, impulse and scaler cases (every cell of theirs is
  within 1e3 of its frame's largest: the condition under which a log10 bound can be tight without a mask).

A frame whose windowed samples are all zero is left out of both and compared bit for bit with ``silent_value(case)``.

``reference(case)`` is float64 throughout.  ``oracle_error(case)`` is the two metrics of OracleLogMel (float32) against
it: the reference's own error.  The kernels get ``FACTOR * oracle_error + FLOOR`` per case and metric (a second and a
third ordering of the same float32 arithmetic: a factor, not a new measurement; the floor is a few float32 ulps for the
cases where the oracle happens to be exact).  ERRORS holds the values of

    python -m tests.logmel_cases

and tests/test_logmel_cpu.py recomputes them and fails if one is further than the same factor and floor from what the
machine it runs on measures (the oracle's own rounding differs between CPUs by up to 4x).
"""
import os

import numpy as np
import torch

from oracle.modules import OracleLogMel, slaney_mel_basis

EPS = 1e-10
FLOOR = 2.0 ** -21
FACTOR = 10.0
# restated from mlfb_kernels.hip (LM_RUN, LM_WTAB and the launcher's pairs-per-wave formula): edges_reached() uses them to
# say which cases cross which threshold, nothing else does
LM_RUN = 64
LM_WTAB = 2048
LM_WAVES_PER_ROUND = 4 * 512  # ppw = ceil(ceil(T / 2) * B / 2048), capped at 32
LM_PPW_CAP = 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_layer.npz")

# name -> (lin, log); None where the metric does not apply
ERRORS = {
    "fs22050_hop128": (2.354e-07, 5.207e-07),
    "fs24000_hop128": (2.158e-07, 7.376e-07),
    "fs22050_hop221": (2.536e-07, 5.884e-07),
    "fs24000_hop240": (2.736e-07, 2.198e-06),
    "win800_hamming": (1.689e-07, 6.914e-07),
    "win1023": (1.693e-07, 1.342e-06),
    "win2": (5.789e-07, 2.716e-07),
    "blackman": (2.324e-07, 1.305e-06),
    "hop1": (2.111e-07, 6.745e-07),
    "hop1024": (2.007e-07, 3.969e-07),
    "hop1500": (1.744e-07, 2.982e-07),
    "r256": (3.703e-07, 4.367e-07),
    "r512_win400": (2.984e-07, 1.553e-06),
    "r2048": (1.681e-07, 3.124e-07),
    "r2048_hop300_win1200": (1.795e-07, 3.163e-07),
    "r1024_env": (2.354e-07, 5.207e-07),
    "r1024_env_win800": (1.689e-07, 6.914e-07),
    "r1024_env_centred": (2.722e-07, 2.011e-06),
    "r1024_env_mel20": (2.713e-07, 2.644e-07),
    "mel20_0_11025": (3.574e-07, 2.494e-07),
    "mel256": (2.316e-07, 3.142e-06),
    "mel1": (1.814e-07, 7.878e-08),
    "fs48000_mel80_full": (2.204e-07, 3.940e-07),
    "basis_fill40": (3.095e-07, 2.697e-07),
    "r1024_env_basis_fill40": (3.637e-07, 2.068e-07),
    "basis_fill_exact": (2.647e-07, 2.245e-07),
    "r1024_env_basis_fill_exact": (2.792e-07, 1.784e-07),
    "basis_run64_65": (3.918e-07, 1.816e-07),
    "r1024_env_basis_run64_65": (4.190e-07, 1.820e-07),
    "basis_empty": (2.550e-07, 1.633e-07),
    "r1024_env_basis_empty": (2.459e-07, 1.390e-07),
    "basis_ends": (2.994e-07, None),
    "r1024_env_basis_ends": (2.768e-07, None),
    "r512_basis_ends": (2.302e-07, None),
    "T1": (9.839e-08, 4.644e-07),
    "T2": (9.115e-08, 2.804e-07),
    "T3": (1.755e-07, 1.849e-07),
    "T37_B3": (2.194e-07, 1.425e-06),
    "r512_T37_B3": (2.628e-07, 1.320e-06),
    "B64_bench": (3.030e-07, 1.283e-06),
    "B270_ppw_cap": (2.904e-07, 1.410e-06),
    "B5_T129_hop1024": (2.405e-07, 1.363e-06),
    "centred_513": (1.534e-07, 3.107e-07),
    "centred_600": (1.377e-07, 6.792e-07),
    "centred_1500": (1.604e-07, 3.572e-07),
    "centred_9999": (2.307e-07, 4.314e-07),
    "centred_B4": (2.135e-07, 1.945e-06),
    "centred_60s_24k": (3.382e-07, 2.140e-06),
    "r512_centred_B3": (2.288e-07, 5.049e-06),
    "scaler_broad": (4.200e-07, 3.626e-07),
    "scaler_silence": (None, None),
    "scaler_centred": (5.616e-07, 3.888e-07),
    "tones": (8.041e-06, None),
    "tones_basis_ends": (3.060e-07, None),
    "r512_tones": (2.343e-06, None),
    "impulses": (3.333e-07, 2.687e-07),
    "impulses_hop221": (3.123e-07, 2.367e-07),
    "r512_impulses": (3.208e-07, 6.474e-07),
    "sweep_hamming": (9.130e-07, 4.268e-07),
    "sweep_win800": (1.172e-06, 5.116e-07),
    "r512_sweep_hamming": (7.144e-07, 3.721e-07),
    "silence": (None, None),
    "r512_silence": (None, None),
    "broad_1e4": (4.122e-07, 8.169e-07),
    "broad_clamp": (1.138e-06, 5.349e-07),
    "r512_broad_clamp": (1.161e-06, 5.500e-07),
    "fixture": (2.167e-06, None),
    "fixture_scaler": (2.151e-06, None),
    "fixture_centred_22050": (2.167e-06, None),
    "fixture_centred_9999": (2.167e-06, None),
    "fixture_centred_1500": (2.519e-06, None),
    "fixture_centred_513": (8.241e-07, None),
}


# ---------------------------------------------------------------------------------------------------------- signals
def _broad_base(rng, n, fs):
    """Harmonics 1 .. 29 of a fundamental gliding over 60 - 180 Hz under a slow amplitude envelope, plus white noise at
    0.03: every mel channel of every frame stays within 1e3 of the frame's largest (test_logmel_cpu.py asserts it)."""
    t = np.arange(n) / fs
    f0 = 120.0 + 60.0 * np.sin(2 * np.pi * 0.9 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / fs
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + rng.uniform(0, 6.28))
    y = np.zeros(n)
    for h in range(1, 30):
        y += rng.uniform(0.02, 0.08) * np.sin(h * ph + rng.uniform(0, 6.28))
    return env * y + 0.03 * rng.standard_normal(n)


def _rows(base, B, n, step=997):
    """B overlapping slices of one long signal (row i starts at i * step): a batch whose rows all differ."""
    return np.stack([base[i * step:i * step + n] for i in range(B)])


def _tone(n, n_fft, k, amp=0.5):
    return amp * np.cos(2 * np.pi * k * np.arange(n) / n_fft + 0.3 * (k % 7))


def signal(case, rows=None):
    """float32 (B, n_samples) - or the given rows of it."""
    kind, B, n = case["sig"]
    rng = np.random.default_rng(case["seed"])
    fs = case["fs"]
    if kind in ("broad", "broad_1e4", "broad_clamp"):
        x = _rows(_broad_base(rng, n + (B - 1) * 997, fs), B, n)
        if kind == "broad_1e4":
            x = x * 1e4
        if kind == "broad_clamp":  # mel energies around eps = 1e-10: part of them below the clamp
            x = x * 1.5e-9
    elif kind == "fixture":  # the recorded waveform of tests/golden/stft_layer.npz, cut to n samples
        x = np.load(GOLDEN)["wav"][None, :n]
        assert x.shape == (B, n)
    elif kind == "silence":
        x = np.zeros((B, n))
    elif kind == "tones":  # one row per tone: exactly on bins 1, 37, n_fft/2 - 1, n_fft/2 (Nyquist) and a constant (bin 0)
        nf = case["n_fft"]
        ks = [1, 37, nf // 2 - 1, nf // 2, 0][:B] if B == 5 else [1, nf // 2 - 1, nf // 2, 0]
        assert B == len(ks)
        x = np.stack([_tone(n, nf, k) for k in ks])
    elif kind == "impulses":  # trains with gaps of 40 .. 150 samples: several impulses in every window, no empty frame
        x = np.zeros((B, n))
        for b in range(B):
            pos = np.cumsum(rng.integers(40, 151, size=n // 40))
            pos = pos[pos < n]
            x[b, pos] = rng.uniform(0.3, 1.0, len(pos)) * rng.choice([-1.0, 1.0], len(pos))
    elif kind == "sweep":  # row i: one unit impulse at sample i of its single frame
        assert B == n == case["n_fft"]
        x = np.eye(n)
    else:
        raise ValueError(kind)
    x = x.astype(np.float32)
    return x if rows is None else x[list(rows)]


# ------------------------------------------------------------------------------------------------------------ bases
def synthetic_basis(name, n_bins=513):
    """(n_bins, n_mels) float32 matrices no Slaney basis gives."""
    rng = np.random.default_rng(abs(hash_name(name)))

    def runs(spans):
        fb = np.zeros((n_bins, len(spans)), np.float32)
        for m, (lo, hi) in enumerate(spans):
            fb[lo:hi, m] = rng.uniform(0.05, 1.0, hi - lo).astype(np.float32) / max(hi - lo, 1)
        return fb

    if name == "fill40":  # 64 x 40 = 2560 weights: filters 0 .. 50 fill 2040 of the 2048 table words, 51 .. 63 do not fit
        return runs([((7 * m) % (n_bins - 40), (7 * m) % (n_bins - 40) + 40) for m in range(64)])
    if name == "fill_exact":  # ... then an 8-bin run that ends exactly on word 2048, and one more that does not fit
        return runs([((7 * m) % (n_bins - 40), (7 * m) % (n_bins - 40) + 40) for m in range(64)] + [(100, 108), (300, 308)])
    if name == "run64_65":  # runs of exactly LM_RUN and LM_RUN + 1 bins, alternating, at both ends of the spectrum
        return runs([(0, 64), (0, 65), (200, 264), (200, 265), (449, 513), (448, 513), (31, 95), (30, 95)])
    if name == "empty":  # an all-zero filter between two live ones
        fb = runs([(10, 40), (50, 60), (200, 260)])
        fb[:, 1] = 0.0
        return fb
    if name == "ends":  # filters that touch bin 0 and bin n_bins - 1, single-bin filters on both
        return runs([(0, 10), (0, 1), (n_bins // 2 - 10, n_bins // 2 + 10), (n_bins - 10, n_bins), (n_bins - 1, n_bins)])
    raise ValueError(name)


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def basis_of(case):
    """The case's float32 basis, (n_bins, n_mels)."""
    if "basis" in case:
        return synthetic_basis(case["basis"], case["n_fft"] // 2 + 1)
    n_mels, fmin, fmax = case["mel"]
    return np.ascontiguousarray(slaney_mel_basis(case["fs"], case["n_fft"], n_mels, fmin, fmax).T)


def filter_runs(fb):
    """[lo, hi) of every filter's nonzero bins, (n_bins, 0) for an all-zero filter - what both kernels compute."""
    out = []
    for m in range(fb.shape[1]):
        nz = np.nonzero(fb[:, m])[0]
        out.append((int(nz[0]), int(nz[-1]) + 1) if len(nz) else (fb.shape[0], 0))
    return out


class Scaler:
    """mean_ / var_ of the committed fixture (80 mels)."""

    def __init__(self):
        fx = np.load(GOLDEN)
        self.mean_, self.var_ = fx["scaler_mean"], fx["scaler_var"]

    def mean_std32(self):
        """The float32 mean and std the layers hold, spelled as they spell it (torch's float32 sqrt on the host: on some
        CPUs its vectorised path is an ulp off numpy's for one value in eight, and the kernel divides by what it is given)."""
        return torch.from_numpy(self.mean_).float().numpy(), torch.from_numpy(self.var_).float().sqrt().numpy()


# ------------------------------------------------------------------------------------------------------------ cases
RECIPE_MEL = (80, 80, 7600)


def cases():
    out = []

    def add(name, sig, fs=22050, n_fft=1024, hop=128, win=None, window="hann", center=False, mel=RECIPE_MEL, basis=None,
            scaler=False, kernel=None, metrics=("lin", "log"), host_rows=None, seed=None):
        c = dict(name=name, sig=sig, fs=fs, n_fft=n_fft, hop=hop, win=n_fft if win is None else win, window=window,
                 center=center, scaler=scaler, metrics=tuple(metrics), host_rows=host_rows,
                 kernel=kernel or ("wave" if n_fft == 1024 else "radix2"), seed=1000 + len(out) if seed is None else seed)
        if basis is not None:
            c["basis"] = basis
        else:
            c["mel"] = mel
        out.append(c)

    def nc(T, hop, n_fft=1024):  # samples of exactly T uncentred frames
        return n_fft + (T - 1) * hop

    # recipes of the reference, wave kernel
    add("fs22050_hop128", ("broad", 2, nc(60, 128)))
    add("fs24000_hop128", ("broad", 2, nc(60, 128)), fs=24000)
    add("fs22050_hop221", ("broad", 2, nc(60, 221) + 100), hop=221)
    add("fs24000_hop240", ("broad", 2, nc(60, 240) + 239), fs=24000, hop=240)
    # window
    add("win800_hamming", ("broad", 2, nc(40, 128)), win=800, window="hamming")
    add("win1023", ("broad", 2, nc(40, 128)), win=1023)
    add("win2", ("broad", 2, nc(40, 128)), win=2)
    add("blackman", ("broad", 2, nc(40, 128)), window="blackman")
    # hop
    add("hop1", ("broad", 1, nc(201, 1)), hop=1)
    add("hop1024", ("broad", 2, nc(7, 1024)), hop=1024)
    add("hop1500", ("broad", 2, nc(6, 1500)), hop=1500)
    # radix-2 kernel
    add("r256", ("broad", 2, nc(80, 64, 256)), fs=16000, n_fft=256, hop=64, mel=(40, 80, 7600))
    add("r512_win400", ("broad", 3, nc(61, 128, 512)), n_fft=512, hop=128, win=400)
    add("r2048", ("broad", 2, nc(30, 256, 2048)), n_fft=2048, hop=256)
    add("r2048_hop300_win1200", ("broad", 2, nc(31, 300, 2048) + 7), n_fft=2048, hop=300, win=1200)
    add("r1024_env", ("broad", 2, nc(60, 128)), kernel="radix2_env", seed=1000)  # (fs22050_hop128's signal)
    add("r1024_env_win800", ("broad", 2, nc(40, 128)), win=800, window="hamming", kernel="radix2_env", seed=1004)
    add("r1024_env_centred", ("broad", 4, 9999), center=True, kernel="radix2_env")
    add("r1024_env_mel20", ("broad", 2, nc(40, 128)), mel=(20, 0, 11025), kernel="radix2_env")
    # mel basis, Slaney
    add("mel20_0_11025", ("broad", 2, nc(40, 128)), mel=(20, 0, 11025))
    add("mel256", ("broad", 2, nc(40, 128)), mel=(256, 0, 11025))
    add("mel1", ("broad", 2, nc(40, 128)), mel=(1, 80, 7600))
    add("fs48000_mel80_full", ("broad", 2, nc(40, 128)), fs=48000, mel=(80, 0, 24000))
    # mel basis, synthetic
    # ("ends" has single-bin filters on bin 0 and on Nyquist, where the broad signal has almost nothing: cells 1e-4 of the
    # frame's largest, outside the condition of the log10 metric - the linear one alone)
    for b in ("fill40", "fill_exact", "run64_65", "empty", "ends"):
        m = ("lin",) if b == "ends" else ("lin", "log")
        add(f"basis_{b}", ("broad", 2, nc(40, 128)), basis=b, metrics=m)
        add(f"r1024_env_basis_{b}", ("broad", 2, nc(40, 128)), basis=b, kernel="radix2_env", metrics=m)
    add("r512_basis_ends", ("broad", 2, nc(40, 128, 512)), n_fft=512, basis="ends", metrics=("lin",))
    # frames and batch
    add("T1", ("broad", 1, nc(1, 128)))
    add("T2", ("broad", 1, nc(2, 128) + 127))
    add("T3", ("broad", 1, nc(3, 128)))
    add("T37_B3", ("broad", 3, nc(37, 128) + 5))
    add("r512_T37_B3", ("broad", 3, nc(37, 128, 512) + 5), n_fft=512)
    add("B64_bench", ("broad", 64, 65023), host_rows=(0, 21, 42, 63))
    add("B270_ppw_cap", ("broad", 270, 65023), host_rows=(0, 133, 269))
    add("B5_T129_hop1024", ("broad", 5, nc(129, 1024)), hop=1024)
    # centred (offline extraction)
    for n in (513, 600, 1500, 9999):
        add(f"centred_{n}", ("broad", 1, n), center=True)
    add("centred_B4", ("broad", 4, 5000), center=True)
    add("centred_60s_24k", ("broad", 1, 60 * 24000), fs=24000, hop=240, center=True)
    add("r512_centred_B3", ("broad", 3, 3001), n_fft=512, hop=100, center=True)
    # scaler
    add("scaler_broad", ("broad", 2, nc(60, 128)), scaler=True)
    add("scaler_silence", ("silence", 2, nc(9, 128)), scaler=True, metrics=())
    add("scaler_centred", ("broad", 2, 3000), center=True, scaler=True)
    # other signals.  Tones are seen through a basis that covers bins 0 .. n_fft / 2 (the recipe's starts at 80 Hz)
    add("tones", ("tones", 5, nc(9, 128)), mel=(80, 0, 11025), metrics=("lin",))
    add("tones_basis_ends", ("tones", 4, nc(9, 128)), basis="ends", metrics=("lin",))  # (without bin 37: no filter there)
    add("r512_tones", ("tones", 5, nc(9, 128, 512)), n_fft=512, mel=(80, 0, 11025), metrics=("lin",))
    add("impulses", ("impulses", 2, nc(60, 128)))
    add("impulses_hop221", ("impulses", 2, nc(40, 221)), hop=221)
    add("r512_impulses", ("impulses", 2, nc(60, 128, 512)), n_fft=512)
    add("sweep_hamming", ("sweep", 1024, 1024), window="hamming")
    add("sweep_win800", ("sweep", 1024, 1024), window="hamming", win=800)  # (rows outside the window: silent frames)
    add("r512_sweep_hamming", ("sweep", 512, 512), n_fft=512, window="hamming")
    add("silence", ("silence", 2, nc(9, 128)), metrics=())
    add("r512_silence", ("silence", 2, nc(9, 128, 512)), n_fft=512, metrics=())
    add("broad_1e4", ("broad_1e4", 2, nc(40, 128)))
    add("broad_clamp", ("broad_clamp", 2, nc(40, 128)))
    add("r512_broad_clamp", ("broad_clamp", 2, nc(40, 128, 512)), n_fft=512)
    # the waveform and configuration of the two log-mel tests of tests/test_gpu_ops.py.  Its quietest cells are 1.4e-4 of
    # their frame's largest, outside the condition of the log10 metric: those tests keep their log10 tolerance and get
    # the linear metric next to it
    add("fixture", ("fixture", 1, 22050), metrics=("lin",))
    add("fixture_scaler", ("fixture", 1, 22050), scaler=True, metrics=("lin",))
    for n in (22050, 9999, 1500, 513):
        add(f"fixture_centred_{n}", ("fixture", 1, n), center=True, metrics=("lin",))
    assert len({c["name"] for c in out}) == len(out)
    return out


def n_frames(case, n=None):
    n = case["sig"][2] if n is None else n
    return 1 + n // case["hop"] if case["center"] else 1 + (n - case["n_fft"]) // case["hop"]


# -------------------------------------------------------------------------------------------------------- reference
def window64(case):
    """The window in float64, zero-padded to n_fft around its centre (win_length < n_fft: torch.stft's rule)."""
    w = getattr(torch, f"{case['window']}_window")(case["win"], dtype=torch.float64).numpy()
    out = np.zeros(case["n_fft"])
    lpad = (case["n_fft"] - case["win"]) // 2
    out[lpad:lpad + case["win"]] = w
    return out


def mel_energies(case, x):
    """float64 (B, T, n_mels) mel energies before the clamp, of float32 rows x."""
    n_fft, hop = case["n_fft"], case["hop"]
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    T = n_frames(case, x.shape[1])
    w = window64(case)
    fb = basis_of(case).astype(np.float64)
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    out = np.empty((x.shape[0], T, fb.shape[1]))
    for b in range(x.shape[0]):
        row = x[b].astype(np.float64)
        if case["center"]:
            row = np.pad(row, n_fft // 2, mode="reflect")  # mirrored without repeating the edge sample
        out[b] = np.abs(np.fft.rfft(row[idx] * w, axis=-1)) @ fb
    return out


def finish(case, energies):
    v = np.log10(np.maximum(energies, EPS))
    if case["scaler"]:
        mean, std = Scaler().mean_std32()
        v = (v - mean.astype(np.float64)) / std.astype(np.float64)
    return v


def reference(case, rows=None):
    """float64 (B, T, n_mels): what the layer returns, computed in double precision from the float32 samples."""
    return finish(case, mel_energies(case, signal(case, rows)))


def metrics(case, got, ref_energies):
    """(lin, log) of float32 results against the float64 mel energies of the same rows; None where a metric does not
    apply to the case."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref_energies.shape, (got.shape, ref_energies.shape)
    lin = log = None
    live = ~silent_frames(ref_energies)  # (silent frames are compared exactly, with silent_value())
    got, ref_energies = got[live], ref_energies[live]
    if got.size == 0:
        return lin, log
    if "lin" in case["metrics"]:
        g = got
        if case["scaler"]:
            mean, std = Scaler().mean_std32()
            g = g * std.astype(np.float64) + mean.astype(np.float64)
        r = np.maximum(ref_energies, EPS)
        lin = float((np.abs(10.0 ** g - r) / r.max(-1, keepdims=True)).max())
    if "log" in case["metrics"]:
        log = float(np.abs(got - finish(case, ref_energies)).max())
    return lin, log


def silent_frames(ref_energies):
    """(B, T) bool: frames whose windowed samples are all zero (every float64 mel energy is exactly 0)."""
    return (ref_energies == 0.0).all(-1)


def oracle(case):
    """OracleLogMel of the case (float32, CPU); a synthetic basis replaces the Slaney one it was built with."""
    n_mels, fmin, fmax = case.get("mel", (1, 0, None))
    o = OracleLogMel(fs=case["fs"], hop_size=case["hop"], fft_size=case["n_fft"], win_length=case["win"],
                     window=case["window"], center=case["center"], n_mels=n_mels, fmin=fmin, fmax=fmax,
                     scaler=Scaler() if case["scaler"] else None, eps=EPS)
    if "basis" in case:
        o.mel_basis = torch.from_numpy(basis_of(case))
    return o


def host_rows(case):
    return case["host_rows"]  # None: every row


def oracle_error(case):
    """(lin, log) of the fp32 oracle against the float64 reference, on the case's host rows."""
    x = signal(case, host_rows(case))
    with torch.no_grad():
        got = oracle(case)(torch.from_numpy(x)).numpy()
    return metrics(case, got, mel_energies(case, x))


def bounds(name):
    return tuple(None if e is None else FACTOR * e + FLOOR for e in ERRORS[name])


def silent_value(case):
    """What a frame of digital silence must return, bit for bit: log10(eps) = -10, standardised in float32."""
    v = np.full(basis_of(case).shape[1], -10.0, np.float32)
    if case["scaler"]:
        mean, std = Scaler().mean_std32()
        v = (v - mean) / std
    return v


# ------------------------------------------------------------------------------------------------------------ edges
def edges_reached(cs):
    """Host-side facts asserted before anything runs on the GPU: every edge the cases are meant to reach is reached."""
    by = {c["name"]: c for c in cs}

    def lens(name):
        return [max(hi - lo, 0) for lo, hi in filter_runs(basis_of(by[name]))]

    def table(name):  # the wave kernel's packing: runs of up to LM_RUN bins side by side while they fit LM_WTAB words
        off, where = 0, []
        for ln in lens(name):
            fits = ln <= LM_RUN and off + ln <= LM_WTAB
            where.append(off if fits else -1)
            off += ln if fits else 0
        return off, where

    def pairs(name):  # ceil(T / 2) * B: the launcher gives a wave ceil(pairs / 2048) frame pairs, at most 32
        c = by[name]
        return (n_frames(c) + 1) // 2 * c["sig"][1]

    facts = {}
    facts["recipe_basis_short_runs"] = max(lens("fs22050_hop128")) <= LM_RUN and sum(lens("fs22050_hop128")) <= LM_WTAB
    facts["runs_above_64"] = sum(ln > LM_RUN for ln in lens("mel20_0_11025")) == 5 and lens("mel1")[0] > LM_RUN
    facts["mel256_fits"] = sum(lens("mel256")) <= LM_WTAB and len(lens("mel256")) == 256
    ln = lens("basis_run64_65")
    facts["runs_of_64_and_65"] = sorted(set(ln)) == [LM_RUN, LM_RUN + 1] and table("basis_run64_65")[1].count(-1) == 4
    off, where = table("basis_fill40")
    facts["table_overflows"] = sum(lens("basis_fill40")) == 2560 and off == 2040 and where[50] >= 0 and where[51:] == [-1] * 13
    off, where = table("basis_fill_exact")
    facts["table_fills_exactly"] = off == LM_WTAB and where[64] == 2040 and where[65] == -1
    facts["empty_filter"] = filter_runs(basis_of(by["basis_empty"]))[1] == (513, 0) and lens("basis_empty")[0] > 0 < lens("basis_empty")[2]
    fb = basis_of(by["basis_ends"])
    facts["bins_0_and_nyquist"] = bool(fb[0].any() and fb[-1].any() and (fb[:, 1] != 0).sum() == 1 and (fb[:, 4] != 0).sum() == 1)
    facts["ppw_1"] = pairs("T37_B3") <= LM_WAVES_PER_ROUND
    facts["ppw_8"] = -(-pairs("B64_bench") // LM_WAVES_PER_ROUND) == 8
    facts["ppw_capped"] = pairs("B270_ppw_cap") > LM_WAVES_PER_ROUND * LM_PPW_CAP and pairs("B270_ppw_cap") == 67500
    facts["waves_past_T"] = n_frames(by["B5_T129_hop1024"]) == 129 and n_frames(by["T37_B3"]) % 2 == 1
    facts["lpad"] = all((by[n]["n_fft"] - by[n]["win"]) // 2 > 0 for n in ("win800_hamming", "win2", "r512_win400", "r2048_hop300_win1200"))
    facts["lpad_rounds_to_0"] = (1024 - by["win1023"]["win"]) // 2 == 0
    facts["hop_above_n_fft"] = by["hop1500"]["hop"] > by["hop1500"]["n_fft"]
    # centred, 513 samples, frame 1: samples -384 .. 639 of a signal of 513 - mirrored at both ends
    c = by["centred_513"]
    facts["mirrors_at_both_ends"] = c["hop"] - c["n_fft"] // 2 < 0 and c["hop"] + c["n_fft"] // 2 - 1 >= c["sig"][2] and n_frames(c) == 5
    e = mel_energies(by["broad_clamp"], signal(by["broad_clamp"]))
    facts["clamp_edge"] = 0.1 < float((e < EPS).mean()) < 0.9
    facts["radix2_sizes"] = {c["n_fft"] for c in cs if c["kernel"] == "radix2"} == {256, 512, 2048}
    facts["sixty_seconds"] = n_frames(by["centred_60s_24k"]) == 6001
    return facts


if __name__ == "__main__":
    print("ERRORS = {")
    for c in cases():
        lin, log = oracle_error(c)
        f = lambda v: "None" if v is None else f"{v:.3e}"  # noqa: E731
        print(f'    "{c["name"]}": ({f(lin)}, {f(log)}),')
    print("}")
