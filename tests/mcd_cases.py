"""Inputs of the MCD / FastDTW tests and what the oracle (oracle/mcd.py) alone says about them.

``cases()`` gives name -> (x, y), float64 arrays of VOICED frames, on the edges the smooth random walks of
tests/test_gpu_mcd.py::_pairs never reach:

* tie families (``const``, ``binary``, ``quad4``, ``identical_q``, ``stairs``): every distance is an exactly representable
  integer (D = 1 integer features, or D = 4 with four equal coordinates: 2 |a - b|), so equal predecessor costs are equal
  bit for bit whatever a ``sqrt`` does away from perfect squares, and the path is decided by the predecessor order
  (up, left, diag; the first minimum wins by strict <);
* wide-window families (``L_shape``, ``L_shape2``, their noisy variants, ``thin``, ``thin5`` and the transpose ``thin2``): rows of
  more than 64 cells (one wavefront), neighbouring windows of very different extent, long purely horizontal / vertical runs;
* dimension edges (``dim1``, ``dim25``, ``dim60``) next to the 35 of the existing tests;
* ``full_radius`` (radius 70 over 40 x 70: one level, the window is every cell, exhaustive DTW is a second reference);
* ``longest`` (6398 x 6398: the largest row capacity crk_mcd_fastdtw accepts).

``radii(name)`` are the radii a case is run at, ``masked(name)`` feeds it through f0 masks with unvoiced frames interleaved,
``reference(name, radius)`` is om.mcd of that, ``levels(name, radius)`` is the oracle's recursion level by level (windows, paths, ties), computed once and shared,
``edges_reached()`` asserts on the host that each case sits on the edge it is named for.
"""
import functools
import zlib

import numpy as np

from oracle import mcd as om

TIE = ("const", "binary", "quad4", "identical_q", "stairs")
WIDE = ("L_shape", "L_shape_noisy", "L_shape2", "L_shape2_noisy", "thin", "thin5")
LONGEST = 6398  # 3 rows of LONGEST + 2 doubles are exactly the 150 KB of dynamic LDS the entry point allows
FULL_RADIUS = 70


def cells_max(nx, ny, radius):
    """Back-pointer capacity of a pair, as mcd_dtw_kernel / mcd_scratch_stride (crank_amd/csrc/mcd_kernels.hip) size it."""
    return 4 * (2 * radius + 1) * (2 * radius + 1) * (nx // 2 + ny // 2 + 2) + (radius + 2) * (nx + ny) + 64


def _step(n, at, dim, height=5.0):
    v = np.zeros((n, dim))
    v[at:] = height
    return v


def walk_pair(rs, nx, ny, dim):
    t = np.cumsum(rs.standard_normal((max(nx, ny) + 40, dim)) * 0.3, 0)
    a = t[np.sort(rs.choice(len(t), nx, replace=True))] + 0.05 * rs.standard_normal((nx, dim))
    b = t[np.sort(rs.choice(len(t), ny, replace=True))] + 0.05 * rs.standard_normal((ny, dim))
    return a, b


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (x, y), read-only."""
    rs = np.random.RandomState(1871)
    out = {}
    out["const"] = np.zeros((37, 2)), np.zeros((50, 2))
    out["binary"] = rs.randint(0, 2, (61, 1)).astype(np.float64), rs.randint(0, 2, (45, 1)).astype(np.float64)
    out["quad4"] = (np.repeat(rs.randint(0, 4, (80, 1)), 4, 1).astype(np.float64),
                    np.repeat(rs.randint(0, 4, (97, 1)), 4, 1).astype(np.float64))
    q = np.repeat(rs.randint(0, 5, 20), 3).astype(np.float64)[:, None]
    out["identical_q"] = q, q.copy()
    out["stairs"] = (np.repeat(np.arange(6), 30).astype(np.float64)[:, None],
                     np.repeat(np.arange(6), [5, 60, 5, 60, 5, 45]).astype(np.float64)[:, None])
    out["L_shape"] = _step(150, 10, 4), _step(130, 120, 4)
    out["L_shape2"] = _step(200, 190, 4), _step(70, 5, 4)
    for name in ("L_shape", "L_shape2"):
        x, y = out[name]
        out[name + "_noisy"] = x + 0.01 * rs.standard_normal(x.shape), y + 0.01 * rs.standard_normal(y.shape)
    out["thin"] = rs.standard_normal((3, 4)), np.cumsum(rs.standard_normal((300, 4)) * 0.3, 0)
    out["thin5"] = rs.standard_normal((5, 4)), np.cumsum(rs.standard_normal((300, 4)) * 0.3, 0)  # radius 2 and 3 recurse too
    out["thin2"] = np.cumsum(rs.standard_normal((300, 4)) * 0.3, 0), rs.standard_normal((2, 4))
    out["dim1"] = walk_pair(rs, 31, 40, 1)
    out["dim25"] = walk_pair(rs, 45, 52, 25)
    out["dim60"] = walk_pair(rs, 70, 33, 60)
    out["full_radius"] = rs.randint(0, 4, (40, 2)).astype(np.float64), rs.randint(0, 4, (70, 2)).astype(np.float64)
    x = np.cumsum(rs.standard_normal((LONGEST, 2)) * 0.3, 0)
    out["longest"] = x, x[np.sort(rs.choice(LONGEST, LONGEST, replace=True))] + 0.01 * rs.standard_normal((LONGEST, 2))
    for x, y in out.values():
        x.setflags(write=False)
        y.setflags(write=False)
    return out


def radii(name):
    """1, 2 and 3 wherever the shorter side has radius + 2 frames (the recursion happens at all); the two special cases
    at the one radius they are about."""
    if name == "full_radius":
        return (FULL_RADIUS,)
    if name == "longest":
        return (1,)
    x, y = cases()[name]
    return tuple(r for r in (1, 2, 3) if min(len(x), len(y)) >= r + 2) or (1,)


def runs():
    """Every (name, radius) of the small cases; ``longest`` is kept apart (it alone takes about a second of oracle time)."""
    return [(n, r) for n in cases() if n != "longest" for r in radii(n)]


@functools.lru_cache(maxsize=None)
def masked(name):
    """(mcep, f0, mcep, f0) of a case: its frames are the voiced ones (f0 > 0), unvoiced frames of other content are
    interleaved, as tests/test_gpu_mcd.py::_pairs does."""
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)

    def with_unvoiced(seq):
        n = len(seq)
        total = n + rs.randint(1, 7)
        f0 = np.zeros(total)
        f0[rs.choice(total, n, replace=False)] = 100.0 + rs.uniform(size=n)
        full = 3.0 + rs.standard_normal((total, seq.shape[1]))
        full[f0 > 0] = seq
        full.setflags(write=False)
        f0.setflags(write=False)
        return full, f0

    x, y = cases()[name]
    return with_unvoiced(x) + with_unvoiced(y)


@functools.lru_cache(maxsize=None)
def reference(name, radius):
    """om.mcd of the masked case: (mcd in dB, path).  Computed once, shared by the tests that compare against it."""
    val, path = om.mcd(*masked(name), radius=radius)
    return val, tuple(path)


def _decided_ties(x, y, window, path):
    """Cells of the path whose minimum two or three finite predecessor costs share: there the predecessor order, not
    the costs, picks the path.  The cost table is om.windowed_dtw's, recomputed (it does not return it)."""
    inf = float("inf")
    D = {(0, 0): 0.0}
    on_path = {(i + 1, j + 1) for i, j in path}
    n = 0
    for i0, j0 in window:
        i, j = i0 + 1, j0 + 1
        dt = om.euclidean(x[i0], y[j0])
        c = [D.get(k, inf) + dt for k in ((i - 1, j), (i, j - 1), (i - 1, j - 1))]
        D[i, j] = min(c)
        if (i, j) in on_path and D[i, j] < inf and c.count(D[i, j]) > 1:
            n += 1
    return n


@functools.lru_cache(maxsize=None)
def levels(name, radius):
    """The oracle's recursion on a case, finest level first: dicts of nx, ny, window (None: the full rectangle of the base
    level), cells, width (widest row), cost, path, ties.  levels(...)[0]["path"] is om.fastdtw's path."""
    x, y = cases()[name]
    xs, ys = [[v for v in x]], [[v for v in y]]
    while len(xs[-1]) >= radius + 2 and len(ys[-1]) >= radius + 2:
        xs.append(om.reduce_by_half(xs[-1]))
        ys.append(om.reduce_by_half(ys[-1]))
    out, path = [], None
    for xl, yl in zip(reversed(xs), reversed(ys)):
        nx, ny = len(xl), len(yl)
        window = None if path is None else om.expand_window(path, nx, ny, radius)
        cost, path = om.windowed_dtw(xl, yl, window)
        full = window if window is not None else [(i, j) for i in range(nx) for j in range(ny)]
        out.append(dict(nx=nx, ny=ny, window=window, cells=len(full), width=int(np.bincount([i for i, _ in full]).max()),
                        cost=cost, path=path, ties=_decided_ties(xl, yl, full, path)))
    return out[::-1]


def is_warping_path(path, nx, ny):
    return (path[0] == (0, 0) and path[-1] == (nx - 1, ny - 1)
            and all((c - a, d - b) in ((1, 0), (0, 1), (1, 1)) for (a, b), (c, d) in zip(path[:-1], path[1:])))


def edges_reached():
    """Every case sits on the edge it is named for (host only, from the oracle)."""
    cs = cases()
    for name, r in runs() + [("longest", 1)]:
        x, y = cs[name]
        lv = levels(name, r)
        # the kernel's back-pointer capacity holds at every level (it sizes it from the finest level's lengths)
        assert all(v["cells"] <= cells_max(len(x), len(y), r) for v in lv), (name, r)
    for name in TIE:
        x, y = cs[name]
        assert all(float(om.euclidean(u, v)).is_integer() for u in x[:12] for v in y[:12]), name
        for r in radii(name):
            assert levels(name, r)[0]["ties"] > 0, (name, r)
    assert levels("const", 1)[0]["cost"] == 0.0 and levels("identical_q", 1)[0]["cost"] == 0.0
    for name in WIDE:
        # a windowed (non-base) level with a row of more than one wavefront
        wide_at = [r for r in radii(name) if max(v["width"] for v in levels(name, r)[:-1]) > 64]
        assert wide_at == {"L_shape2_noisy": [2, 3]}.get(name, list(radii(name))), (name, wide_at)
    # thin2 is thin's transpose: the pyramid stops at once as well, but its one level is 300 rows of 2 cells
    assert len(levels("thin2", 1)) == 1 and levels("thin2", 1)[0]["width"] == 2
    for name in ("L_shape", "L_shape2"):
        # the noise leaves informative (pairwise different) distances beyond cell 64 of the wide rows
        x, y = cs[name + "_noisy"]
        assert len({om.euclidean(x[0], v) for v in y[64:]}) == len(y) - 64
        # long purely horizontal and purely vertical runs
        p = np.array(levels(name, 1)[0]["path"])
        d = np.diff(p, axis=0)
        assert _longest_run(d[:, 0] == 0) >= 50 and _longest_run(d[:, 1] == 0) >= 50, name
    assert levels("thin", 1)[0]["width"] == 300 and len(levels("thin", 1)) == 2
    assert all(levels("thin5", r)[0]["width"] == 300 and len(levels("thin5", r)) == 2 for r in (2, 3))
    assert {cs[n][0].shape[1] for n in cs} >= {1, 2, 4, 25, 60}
    assert len(levels("full_radius", FULL_RADIUS)) == 1 and levels("full_radius", FULL_RADIUS)[0]["cells"] == 40 * 70
    assert levels("full_radius", FULL_RADIUS)[0]["ties"] > 0
    x, y = cs["longest"]
    assert len(x) == len(y) == LONGEST and 3 * (LONGEST + 2) * 8 == 150 * 1024
    return True


def _longest_run(mask):
    best = n = 0
    for m in mask:
        n = n + 1 if m else 0
        best = max(best, n)
    return best


if __name__ == "__main__":
    for name, r in runs() + [("longest", 1)]:
        lv = levels(name, r)
        x, y = cases()[name]
        print(f"{name:16s} r={r:2d} {len(x):4d} x {len(y):4d} D={x.shape[1]:2d} levels={len(lv)} widest={max(v['width'] for v in lv):4d} "
              f"cells={max(v['cells'] for v in lv):7d} of {cells_max(len(x), len(y), r):7d} ties={lv[0]['ties']}")
    print(edges_reached())
