"""Writes tests/golden/scaler_fit.npz: ragged float32 utterances, sklearn's StandardScaler fitted on them exactly as the
reference's ``Scaler.fit`` does (one ``partial_fit`` per utterance in file order), the per-utterance moments as numpy forms
them, and the exact statistics.  Needs scikit-learn (written with 1.7.2); the tests read the file only.

    python tests/golden/make_golden_scaler.py
"""
import os
import sys
from fractions import Fraction

import numpy as np
from sklearn.preprocessing import StandardScaler

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import scaler_fit_ref as R  # noqa: E402

SHIFT = 149  # every float32 is an integer multiple of 2^-149


def as_ints(col):
    """A float32 column as exact Python integers in units of 2^-149."""
    m, e = np.frexp(col.astype(np.float64))
    mi = np.round(m * 2.0**24).astype(np.int64)
    assert np.array_equal(mi / 2.0**24, m)
    return [int(a) << (int(b) - 24 + SHIFT) for a, b in zip(mi, e)]


def exact(X):
    """Per column of X (n, D) float32: exact sum, sum of squared deviations from the exact mean, mean and variance, each
    rounded once to float64."""
    n, D = X.shape
    out = np.zeros((4, D))
    for d in range(D):
        v = as_ints(X[:, d])
        sx, sxx = sum(v), sum(a * a for a in v)
        m2 = Fraction(sxx * n - sx * sx, n << (2 * SHIFT))
        out[:, d] = (float(Fraction(sx, 1 << SHIFT)), float(m2), float(Fraction(sx, n << SHIFT)), float(m2 / n))
    return out


def main():
    rng = np.random.default_rng(20201)
    F = sum(R.LENS)
    blocks = {
        "lcf0": (5.0 + 0.3 * rng.standard_normal((F, 1))).astype(np.float32),
        "d5": (rng.standard_normal((F, 5)) * [0.1, 1.0, 3.0, 10.0, 0.5] + [0.0, -2.0, 5.0, 100.0, 1e-3]).astype(np.float32),
        "d80": (rng.standard_normal((F, 80)) * rng.uniform(0.2, 4.0, 80) + rng.uniform(-8.0, 2.0, 80)).astype(np.float32),
        "win": (rng.standard_normal((F, 12)) * 2.0 + 1.0).astype(np.float32),
    }
    blocks["d80"][:, R.CONST_COL] = -10.0
    blocks["d80"][:, R.ZERO_COL] = 0.0
    out = {}
    for name, x in blocks.items():
        ld, col0, D = R.BLOCKS[name]
        assert x.shape == (F, ld)
        out[f"{name}_x"] = x
        parts = R.split(np.ascontiguousarray(x[:, col0:col0 + D]))
        mom = [R.utt_moments(p) for p in parts]
        out[f"{name}_n"] = np.asarray([m[0] for m in mom], np.int64)
        out[f"{name}_sum"] = np.stack([m[1] for m in mom])
        out[f"{name}_m2"] = np.stack([m[2] for m in mom])
        ex = [exact(p) for p in parts]
        out[f"{name}_xsum"] = np.stack([e[0] for e in ex])
        out[f"{name}_xm2"] = np.stack([e[1] for e in ex])
        for g in R.GROUPS:
            members = R.group_members(g)
            ss = StandardScaler()
            for u in members:
                ss.partial_fit(parts[u])
            out[f"{name}_{g}_mean"], out[f"{name}_{g}_var"], out[f"{name}_{g}_scale"] = ss.mean_, ss.var_, ss.scale_
            out[f"{name}_{g}_count"] = np.asarray(int(ss.n_samples_seen_), np.int64)
            e = exact(np.concatenate([parts[u] for u in members]))
            out[f"{name}_{g}_xmean"], out[f"{name}_{g}_xvar"] = e[2], e[3]
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
