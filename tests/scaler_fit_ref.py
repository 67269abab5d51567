"""numpy mirror of what the scaler-fit kernels compute, and the layout of tests/golden/scaler_fit.npz.

``utt_moments`` is the per-block half of sklearn's ``_incremental_mean_and_var`` (sklearn/utils/extmath.py) as numpy
evaluates it for a float32 block: float64 sum, T = sum / n, corrected two-pass sum of squares.  ``merge`` is the other
half, the Chan / Golub / LeVeque update, walked over per-utterance moments in order, every operation in numpy float64 in
sklearn's order: fed sklearn-style moments it reproduces ``StandardScaler.partial_fit``'s ``mean_`` / ``var_`` bit for bit
(tests/test_scaler_fit_cpu.py).  ``scale_rule`` is sklearn's ``_is_constant_feature`` + ``_handle_zeros_in_scale``.

The fixture (written by tests/golden/make_golden_scaler.py where sklearn is installed) holds, for every block of BLOCKS:
``<b>_x`` the float32 rows, ``<b>_n`` / ``<b>_sum`` / ``<b>_m2`` the per-utterance moments as numpy forms them,
``<b>_xsum`` / ``<b>_xm2`` the exact ones (integer arithmetic over the float32 values, rounded once to float64), and for
every group of GROUPS ``<b>_<g>_mean`` / ``_var`` / ``_scale`` / ``_count`` (sklearn) and ``_xmean`` / ``_xvar`` (exact).
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaler_fit.npz")

# file order: three interleaved speakers; "C" owns a single 1-frame utterance (variance 0, scale 1)
LENS = [63, 1, 2, 64, 65, 255, 256, 257, 700]
SPKS = ["A", "C", "B", "A", "B", "A", "B", "A", "B"]
GROUPS = ["all", "A", "B", "C"]
# name -> (ld, col0, D)
BLOCKS = {"lcf0": (1, 0, 1), "d5": (5, 0, 5), "d80": (80, 0, 80), "win": (12, 3, 5)}
CONST_COL, ZERO_COL = 7, 33  # of d80: constant at -10.0, all zero


def group_members(g):
    return [u for u, s in enumerate(SPKS) if g == "all" or s == g]


def starts():
    return np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)


def split(x):
    s = starts()
    return [x[s[u]:s[u + 1]] for u in range(len(LENS))]


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def window(name, fx=None):
    """The (F, D) window of a block that its scalers are fitted on."""
    fx = fixture() if fx is None else fx
    ld, col0, D = BLOCKS[name]
    return fx[f"{name}_x"][:, col0:col0 + D]


def utt_moments(X):
    """(n, sum, m2) of one utterance X (n, D) float32, as sklearn / numpy form them."""
    n = X.shape[0]
    new_sum = np.sum(X, axis=0, dtype=np.float64)
    T = new_sum / n
    temp = X - T
    correction = np.sum(temp, axis=0)
    temp **= 2
    m2 = np.sum(temp, axis=0)
    m2 -= correction**2 / n
    return n, new_sum, m2


def merge(ns, sums, m2s):
    """sklearn's running (mean, var, count) after the utterances whose moments are given, in that order."""
    D = np.asarray(sums[0]).shape[0]
    mean, var = np.zeros(D), np.zeros(D)
    count = np.zeros(D, dtype=np.int64)
    for n, new_sum, new_m2 in zip(ns, sums, m2s):
        new_count = np.full(D, int(n), dtype=np.int64)
        last_sum = mean * count
        updated_count = count + new_count
        updated_mean = (last_sum + new_sum) / updated_count
        last_m2 = var * count
        with np.errstate(divide="ignore", invalid="ignore"):
            r = count / new_count
            updated_m2 = last_m2 + new_m2 + r / updated_count * (last_sum / r - new_sum) ** 2
        zeros = count == 0
        updated_m2[zeros] = np.asarray(new_m2)[zeros]
        mean, var, count = updated_mean, updated_m2 / updated_count, updated_count
    return mean, var, int(count[0])


def scale_rule(mean, var, n):
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return scale


def bounds_mean_var(X, xmean, xvar):
    """The end-to-end bounds of a group's rows X: worst-case float64 summation, N 2^-53 mean|x| for the mean and
    N 2^-53 (var + mean^2) for the variance."""
    N = X.shape[0]
    u = 2.0**-53
    X = X.astype(np.float64)
    return N * u * np.mean(np.abs(X), axis=0), N * u * (xvar + xmean**2)


def bounds_moments(X, xsum):
    """The per-utterance bounds: n 2^-53 sum|x| for the sum, (n + 8) 2^-52 sum (x - m)^2 for m2."""
    n = X.shape[0]
    X = X.astype(np.float64)
    m = xsum / n
    return n * 2.0**-53 * np.sum(np.abs(X), axis=0), (n + 8) * 2.0**-52 * np.sum((X - m) ** 2, axis=0)
