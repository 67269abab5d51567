"""Seeded synthetic inputs of the Griffin-Lim tests (CPU and GPU): no fixture files.

A case is a dict: name, fs, hop, win (win_length), T (frames), kind, and from ``materialise``: ``mlfb`` ((T, 80) log-mel, or
None for a spectrum given directly), ``S`` ((T, 513) magnitudes the iteration starts from) and ``angles`` ((T, 513) initial
unit phasors).  Hops 128 / 220 / 221 / 240, win_length 1024 and 800, fs 22050 and 24000, lengths from the shortest admissible
(hop * (T - 1) > 512) to 400 frames, a silent utterance, an all-zero spectrum, a log-mel whose linear spectrum has negative
cells, and log-mels taken from a harmonic + noise signal through the project's own mel basis.
"""
import functools

import numpy as np

from tests import griffin_lim_ref as R

N_MELS, FMIN, FMAX = 80, 80, 7600
KS = (1, 10, 100)

CASES = [
    dict(name="hop128_harmonic_400", fs=22050, hop=128, win=1024, T=400, kind="harmonic"),
    dict(name="hop220_smooth_150", fs=22050, hop=220, win=1024, T=150, kind="smooth"),
    dict(name="hop221_win800_120", fs=22050, hop=221, win=800, T=120, kind="smooth"),
    dict(name="hop240_fs24k_harmonic_200", fs=24000, hop=240, win=1024, T=200, kind="harmonic"),
    dict(name="hop240_win800_silent_60", fs=24000, hop=240, win=800, T=60, kind="silent"),
    dict(name="hop128_silent_90", fs=22050, hop=128, win=1024, T=90, kind="silent"),
    dict(name="hop128_shortest_6", fs=22050, hop=128, win=1024, T=6, kind="smooth"),
    dict(name="hop240_win800_shortest_4", fs=24000, hop=240, win=800, T=4, kind="smooth"),
    dict(name="hop128_negative_80", fs=22050, hop=128, win=1024, T=80, kind="rough"),
    dict(name="hop128_zero_20", fs=22050, hop=128, win=1024, T=20, kind="zero"),
]


def config_key(case):
    """Cases with the same key run through one GriffinLim object as one ragged batch."""
    return (case["fs"], case["hop"], case["win"])


@functools.lru_cache(maxsize=None)
def mel_basis(fs):
    from crank_amd.net.module.mlfb import slaney_mel_basis

    return slaney_mel_basis(fs, R.N, N_MELS, FMIN, FMAX).astype(np.float64)


@functools.lru_cache(maxsize=None)
def pinv_basis(fs):
    return np.ascontiguousarray(np.linalg.pinv(mel_basis(fs)))


def harmonic_signal(n, fs, rng):
    t = np.arange(n) / fs
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 1.5 * t)
    phase = 2 * np.pi * np.cumsum(f0) / fs
    y = sum(rng.uniform(0.02, 0.2) / h * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 20))
    return y + 0.01 * rng.standard_normal(n)


def _mlfb(case, rng):
    T, kind = case["T"], case["kind"]
    if kind == "silent":
        return np.full((T, N_MELS), -10.0)
    if kind == "harmonic":  # the log-mel of a signal, as the recipe's feature extraction forms it
        x = harmonic_signal(case["hop"] * (T - 1), case["fs"], rng)
        spc = np.abs(R.stft(x, case["hop"], case["win"]))
        return np.log10(np.maximum(1e-10, spc @ mel_basis(case["fs"]).T))
    if kind == "smooth":  # slowly varying in time and over the mels
        a = rng.standard_normal((T + 8, N_MELS + 8))
        a = np.cumsum(np.cumsum(a, 0), 1)
        a = (a[8:, 8:] - a[:-8, 8:] - a[8:, :-8] + a[:-8, :-8]) / 64.0
        return -2.0 + 0.8 * a
    if kind == "rough":  # independent cells: the pseudo-inverse turns neighbouring mels of unlike level into negative cells
        return -2.0 + 1.0 * rng.standard_normal((T, N_MELS))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def materialise(name):
    idx = [c["name"] for c in CASES].index(name)
    case = dict(CASES[idx])
    rng = np.random.default_rng(100 + idx)
    if case["kind"] == "zero":
        case["mlfb"], case["spc"] = None, np.zeros((case["T"], R.K))
    else:
        case["mlfb"] = _mlfb(case, rng)
        case["spc"] = R.linear_spectrum(case["mlfb"], pinv_basis(case["fs"]))
    case["S"] = np.abs(case["spc"])
    case["angles"] = R.initial_angles(case["T"], 1000 + idx)
    return case


@functools.lru_cache(maxsize=None)
def snapshots(name, transform_index):
    """{k: waveform} of the restatement for k in KS (and 0), one run of 100 iterations with transform TRANSFORMS[index]."""
    c = materialise(name)
    return R.griffin_lim_snapshots(c["S"], c["angles"], (0,) + KS, c["hop"], c["win"], R.TRANSFORMS[transform_index])


def all_snapshots():
    """{(name, transform index): snapshots} for every case and transform, computed on a process pool (the 100-iteration runs
    dominate the tests' CPU time)."""
    import concurrent.futures as cf
    import os

    jobs = [(c["name"], i) for c in CASES for i in range(len(R.TRANSFORMS))]
    todo = [j for j in jobs if j not in _DONE]
    if todo:
        workers = max(1, min(16, len(todo), len(os.sched_getaffinity(0))))
        import multiprocessing as mp

        # fresh interpreters, not forks: the parent may hold an initialised GPU runtime
        with cf.ProcessPoolExecutor(workers, mp_context=mp.get_context("spawn")) as ex:
            for j, res in zip(todo, ex.map(_job, todo)):
                _DONE[j] = res
    return {j: _DONE[j] for j in jobs}


_DONE = {}


def _job(j):
    import torch

    torch.set_num_threads(1)
    return snapshots(*j)
