"""CPU restatement of the one chain every codebook search kernel forms (crank_amd/csrc/vq_common.h), in numpy float32:
w2 and x2 as d-ordered sums of separately rounded squares, the dot product as a d-ordered chain of fused multiply-adds,
dist = (w2 - 2 dot) + x2, the first index on equal values."""
import numpy as np

F = np.float32


def sq_norm(v):
    """Row norms of v (rows, D): s = fl(s + fl(v_d * v_d)), d ascending."""
    s = np.zeros(v.shape[0], F)
    for d in range(v.shape[1]):
        s = s + v[:, d] * v[:, d]  # float32 arrays: the product and the sum each round to float32
    return s


def fma_dot(x, w):
    """dot[n, k] = fma(x[n, d], w[k, d], dot[n, k]) for d = 0, 1, ...; returns (dot, clean).  A step is emulated through
    float64: the product of two float32 values is exact there, the sum rounds to float64 and then to float32.  Where the
    float64 sum is exact (Knuth's two-sum gives a zero error term) the float32 rounding is the only one and the step IS the
    fma.  Where it is not, the two roundings differ from the fma's single one only if the float64 sum sits on a float32
    rounding midpoint (low 29 bits of the significand 1 0...0); clean[n] is False for a row with such a step (the caller
    leaves those rows out)."""
    dot = np.zeros((x.shape[0], w.shape[0]), F)
    clean = np.ones(x.shape[0], bool)
    for d in range(x.shape[1]):
        a, b = dot.astype(np.float64), x[:, d, None].astype(np.float64) * w[None, :, d].astype(np.float64)
        s = a + b
        bv = s - a
        inexact = ((a - (s - bv)) + (b - bv)) != 0
        midpoint = (s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
        clean &= ~(inexact & midpoint).any(axis=1)
        dot = s.astype(F)
    return dot, clean


def vq_search_ref(x, w):
    """x (N, D), w (K, D) float32 -> (indices (N,) int64, clean (N,) bool)."""
    x, w = np.ascontiguousarray(x, F), np.ascontiguousarray(w, F)
    dot, clean = fma_dot(x, w)
    dist = (sq_norm(w)[None, :] - F(2) * dot) + sq_norm(x)[:, None]
    assert dist.dtype == F
    return dist.argmin(axis=1).astype(np.int64), clean


def near_tie_case(D, K, N, seed):
    """Rows near a code that has a (1 + 1e-7) twin and a + 1e-7 twin (the near_ties construction of the split-f16 equality
    test), two thirds of the frames; the rest random."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((N, D)).astype(F)
    w = (0.5 * rs.standard_normal((K, D))).astype(F)
    c, t = 10, K // 2
    w[t] = w[c] * F(1 + 1e-7)
    w[t + 1] = w[c] + F(1e-7)
    near = 2 * N // 3
    x[:near] = w[c] + F(0.05) * x[:near]
    return x, w


# (D, K) -> seed for which no frame of near_tie_case(D, K, 300, seed) is left out (tests/test_vq_search_cpu.py checks)
NEAR_TIE_SEEDS = {(D, K): 0 for D in (16, 32, 128) for K in (40, 600)}
NEAR_TIE_FRAMES = 300
