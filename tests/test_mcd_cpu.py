"""oracle/mcd.py (the FastDTW restatement, parity unpinned: the package is absent) checked for what can be
checked without it: against an exhaustive DTW where the window covers everything, path validity, and
against an interval formulation of the same algorithm (per-row [lo, hi] windows, rolling cost rows, one
back pointer per cell) that the device kernel crk_mcd_fastdtw implements line for line."""
import numpy as np
import pytest

from oracle import mcd as om
from tests import mcd_cases as C


def exact_dtw_cost(x, y):
    n, m = len(x), len(y)
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = om.euclidean(x[i - 1], y[j - 1]) + min(D[i - 1, j], D[i, j - 1], D[i - 1, j - 1])
    return D[n, m]


def interval_fastdtw(x, y, radius=1):
    """The device kernel's formulation (crank_amd/csrc/mcd_kernels.hip) in Python."""
    x = [np.asarray(v, dtype=np.float64) for v in x]
    y = [np.asarray(v, dtype=np.float64) for v in y]
    xs, ys = [x], [y]
    while len(xs[-1]) >= radius + 2 and len(ys[-1]) >= radius + 2:
        xs.append(om.reduce_by_half(xs[-1]))
        ys.append(om.reduce_by_half(ys[-1]))
    L = len(xs) - 1
    lo, hi = [0] * len(xs[L]), [len(ys[L]) - 1] * len(xs[L])
    path = None
    for l in range(L, -1, -1):
        xl, yl = xs[l], ys[l]
        nx, ny = len(xl), len(yl)
        back, prev, plo, phi = [], None, 0, -1
        for i in range(nx):
            cur, brow = [], []
            for c, j in enumerate(range(lo[i], hi[i] + 1)):
                dt = om.euclidean(xl[i], yl[j])
                if i == 0:
                    up, diag = np.inf, (0.0 if j == 0 else np.inf)
                else:
                    up = prev[j - plo] if plo <= j <= phi else np.inf
                    diag = prev[j - 1 - plo] if plo <= j - 1 <= phi else np.inf
                left = cur[c - 1] if c > 0 else np.inf
                best, bp = up + dt, 0
                if left + dt < best:
                    best, bp = left + dt, 1
                if diag + dt < best:
                    best, bp = diag + dt, 2
                cur.append(best)
                brow.append(bp)
            back.append(brow)
            prev, plo, phi = cur, lo[i], hi[i]
        i, j, path = nx - 1, ny - 1, []
        while i >= 0 and j >= 0:
            path.append((i, j))
            bp = back[i][j - lo[i]]
            if bp == 0:
                i -= 1
            elif bp == 1:
                j -= 1
            else:
                i, j = i - 1, j - 1
        path.reverse()
        if l > 0:
            jmin, jmax = [10 ** 9] * nx, [-1] * nx
            for ci, cj in path:
                jmin[ci], jmax[ci] = min(jmin[ci], cj), max(jmax[ci], cj)
            nxf, nyf = len(xs[l - 1]), len(ys[l - 1])
            lo, hi, start_j = [], [], 0
            for fi in range(nxf):
                ci = fi >> 1
                rows = [cr for cr in range(ci - radius, ci + radius + 1) if 0 <= cr < nx and jmax[cr] >= 0]
                e0, e1 = min(jmin[cr] for cr in rows) - radius, max(jmax[cr] for cr in rows) + radius
                f0, f1 = max(2 * e0, start_j), min(2 * e1 + 1, nyf - 1)
                lo.append(f0)
                hi.append(f1)
                start_j = f0
    return path


@pytest.mark.parametrize("seed", range(6))
def test_fastdtw_restatement_properties(seed):
    rs = np.random.RandomState(seed)
    for nx, ny in [(1, 1), (1, 7), (2, 9), (3, 3), (5, 4), (17, 40), (64, 33), (101, 96), (37, 150)]:
        D = 4
        base = np.cumsum(rs.standard_normal((max(nx, ny) + 8, D)), 0)
        x = base[rs.choice(len(base), nx, replace=True)][np.argsort(rs.uniform(size=nx))] if seed % 2 else base[:nx] + 0.1 * rs.standard_normal((nx, D))
        y = base[:ny] + 0.1 * rs.standard_normal((ny, D))
        cost, path = om.fastdtw(x, y, radius=1)
        # a valid warping path: ends fixed, steps in {(1,0),(0,1),(1,1)}
        assert path[0] == (0, 0) and path[-1] == (nx - 1, ny - 1)
        for (a, b), (c, d) in zip(path[:-1], path[1:]):
            assert (c - a, d - b) in ((1, 0), (0, 1), (1, 1))
        # its cost is the sum along the path and can only exceed the exhaustive optimum
        assert np.isclose(cost, sum(om.euclidean(x[i], y[j]) for i, j in path), rtol=1e-12)
        opt = exact_dtw_cost(x, y)
        assert cost >= opt * (1 - 1e-12)
        # with a radius as large as the sequences the window covers every cell: exact
        cost_full, _ = om.fastdtw(x, y, radius=max(nx, ny))
        assert np.isclose(cost_full, opt, rtol=1e-12)
        # the interval formulation the kernel uses gives the same path, cell for cell
        assert interval_fastdtw(x, y, radius=1) == path, (nx, ny)
        if min(nx, ny) >= 4:
            assert interval_fastdtw(x, y, radius=2) == om.fastdtw(x, y, radius=2)[1]


def test_mcd_formula_and_voiced_selection():
    rs = np.random.RandomState(3)
    cv, gt = rs.standard_normal((30, 5)), rs.standard_normal((26, 5))
    f0c, f0g = (rs.uniform(size=30) < 0.8) * 120.0, (rs.uniform(size=26) < 0.8) * 110.0
    val, path = om.mcd(cv, f0c, gt, f0g)
    a, b = cv[f0c > 0], gt[f0g > 0]
    ref = np.mean([10.0 / np.log(10.0) * np.sqrt(2 * np.sum((a[i] - b[j]) ** 2)) for i, j in path])
    assert np.isclose(val, ref, rtol=1e-13)
    # identical sequences: zero distortion along the diagonal
    val0, path0 = om.mcd(cv, np.ones(30), cv, np.ones(30))
    assert val0 == 0.0 and path0 == [(i, i) for i in range(30)]


# ------------------------------------------------------------------------------------------------ tests/mcd_cases.py
# ties, rows wider than a wavefront, dimension / radius edges, the full window and the longest accepted pair


@pytest.mark.parametrize("name,radius", C.runs() + [("longest", 1)], ids=lambda v: str(v))
def test_interval_formulation_equals_oracle_on_the_edge_cases(name, radius):
    x, y = C.cases()[name]
    cost, path = om.fastdtw(x, y, radius=radius)
    assert C.is_warping_path(path, len(x), len(y))
    assert C.levels(name, radius)[0]["path"] == path  # the level-by-level view the edge assertions read is the oracle's
    assert interval_fastdtw(x, y, radius=radius) == path
    if name == "full_radius":
        assert np.isclose(cost, exact_dtw_cost(x, y), rtol=1e-12, atol=0)
    if name in ("const", "identical_q"):
        assert cost == 0.0 and om.mcd(x, np.ones(len(x)), y, np.ones(len(y)), radius=radius)[0] == 0.0


def test_mcd_cases_sit_on_their_edges():
    assert C.edges_reached()


def test_masked_cases_select_the_voiced_frames():
    for name in C.cases():
        cv, f0c, gt, f0g = C.masked(name)
        x, y = C.cases()[name]
        assert len(cv) > len(x) and len(gt) > len(y)
        assert np.array_equal(cv[f0c > 0], x) and np.array_equal(gt[f0g > 0], y)


CRK_ERR_ARG, CRK_ERR_UNSUPPORTED = 1, 3
FAKE = 0x1000  # never dereferenced: every call below is refused before anything is launched


def _entry(P=1, D=2, radius=1, max_nx=10, max_ny=10, **null):
    from crank_amd import _lib

    names = ("cv", "cv_off", "gt", "gt_off", "mcd", "path_len", "path_out", "scratch", "status")
    assert set(null) <= set(names)
    p = {n: (None if n in null else FAKE + 64 * k) for k, n in enumerate(names)}
    return _lib.lib().crk_mcd_fastdtw(p["cv"], p["cv_off"], p["gt"], p["gt_off"], P, D, radius, max_nx, max_ny, p["mcd"],
                                      p["path_len"], p["path_out"], 2 * (max_nx + max_ny), p["scratch"], p["status"], None)


def test_mcd_entry_points_refuse_bad_arguments_before_any_launch():
    from crank_amd import _lib

    header = open(__file__.replace("tests/test_mcd_cpu.py", "include/crank_hip.h")).read()
    assert f"#define CRK_ERR_ARG {CRK_ERR_ARG}\n" in header and f"#define CRK_ERR_UNSUPPORTED {CRK_ERR_UNSUPPORTED}\n" in header
    for n in ("cv", "cv_off", "gt", "gt_off", "mcd", "path_len", "scratch", "status"):  # path_out alone is optional
        assert _entry(**{n: True}) == CRK_ERR_ARG, n
    for bad in (dict(P=0), dict(P=-1), dict(D=0), dict(D=-3), dict(radius=0), dict(radius=-1), dict(max_nx=0), dict(max_ny=-5)):
        assert _entry(**bad) == CRK_ERR_ARG, bad
    # the LDS envelope: three rows of max(max_nx, max_ny) + 2 doubles in 150 KB.  It is judged before the pointers, so a
    # null pointer shows which side of it a size lies on without a launch
    for big in (dict(max_nx=6399), dict(max_ny=6399), dict(max_nx=6399, max_ny=6399), dict(max_nx=2 ** 31 - 1)):
        assert _entry(**big) == CRK_ERR_UNSUPPORTED, big
        assert _entry(status=True, **big) == CRK_ERR_UNSUPPORTED, big
    for ok in (dict(max_nx=6398), dict(max_ny=6398), dict(max_nx=6398, max_ny=6398)):
        assert _entry(status=True, **ok) == CRK_ERR_ARG, ok


def test_mcd_scratch_bytes_refuses_and_grows():
    from crank_amd import _lib

    sb = _lib.lib().crk_mcd_scratch_bytes
    for bad in ((0, 10, 10, 2, 1), (-1, 10, 10, 2, 1), (1, 0, 10, 2, 1), (1, 10, 0, 2, 1), (1, 10, -1, 2, 1), (1, 10, 10, 0, 1),
                (1, 10, 10, 2, 0), (1, 10, 10, 2, -1)):
        assert sb(*bad) == -1, bad
    grid = [(nx, ny, D, r) for nx in (1, 2, 3, 64, 65, 6398) for ny in (1, 2, 5, 300, 6398) for D in (1, 25, 60) for r in (1, 2, 3)]
    for nx, ny, D, r in grid:
        b = sb(1, nx, ny, D, r)
        # holds what the kernel lays out for a pair of exactly these lengths (mcd_dtw_kernel's `need`), 256-byte granules
        need = 8 * D * (nx + ny) + 4 * (3 * nx + 1 + 2 * (nx + ny)) + C.cells_max(nx, ny, r)
        assert b % 256 == 0 and need <= b < need + 256, (nx, ny, D, r)
        assert sb(7, nx, ny, D, r) == 7 * b
        assert sb(1, nx + 1, ny, D, r) >= b and sb(1, nx, ny + 1, D, r) >= b and sb(1, nx, ny, D + 1, r) >= b
        assert sb(1, nx, ny, D, r + 1) >= b
        # before the 256-byte rounding every step up is a strict increase: 64 more frames always cost more
        assert sb(1, nx + 64, ny, D, r) > b and sb(1, nx, ny + 64, D, r) > b


def test_mcd_wrapper_host_checks():
    """All of these are raised before anything is uploaded: no device is needed."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw

    m, f = np.zeros((5, 3)), np.ones(5)
    with pytest.raises(ValueError):
        mcd_fastdtw([m, m], [f, f], [m], [f])  # unequal list lengths
    with pytest.raises(ValueError):
        mcd_fastdtw([m], [f, f], [m], [f])
    with pytest.raises(ValueError):
        mcd_fastdtw([], [], [], [])
    with pytest.raises(ValueError):
        mcd_fastdtw([m, np.zeros((5, 4))], [f, f], [m, m], [f, f])  # mixed D
    with pytest.raises(ValueError):
        mcd_fastdtw([m], [f], [np.zeros((5, 2))], [f])
    with pytest.raises(ValueError):
        mcd_fastdtw([m, m], [f, np.zeros(5)], [m, m], [f, f])  # an utterance with no voiced frame
    with pytest.raises(ValueError):
        mcd_fastdtw([m], [f], [m], [-f])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_mcd_wrapper_refuses_non_finite_voiced_frames(bad):
    """The package dies in its backtrack on these (every < is false, all predecessors are `up`, the walk leaves column
    ny - 1 at row 0: KeyError), and so does the oracle; the kernel would hand back a truncated path and a NaN."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw

    rs = np.random.RandomState(4)
    m, g, f = rs.standard_normal((9, 3)), rs.standard_normal((7, 3)), np.ones(9)
    f[4] = 0.0
    for where in ("cv", "gt"):
        a, b = m.copy(), g.copy()
        (a if where == "cv" else b)[2, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            mcd_fastdtw([a], [f], [b], [np.ones(7)])
    with pytest.raises(KeyError):
        a = m.copy()
        a[2, 1] = np.nan
        om.mcd(a, f, g, np.ones(7))
