"""crk_mcd_fastdtw (MCD with FastDTW alignment on the device) against oracle/mcd.py:
identical warping paths, MCD to 1e-12 relative (the mean is a wave-order sum), ragged batch with the
degenerate lengths (1, 2, 3 frames; odd / even; very different lengths).  tests/mcd_cases.py adds the inputs smooth random
walks never give: exact ties, rows wider than a wavefront, D = 1 / 25 / 60, radius 1 to 3, a window that covers every cell,
the longest pair the entry point accepts, and pairs longer than the maxima the library was told (refused, not run)."""
import time

import numpy as np
import pytest

from oracle import mcd as om
from tests import mcd_cases as C
from tests.test_mcd_cpu import exact_dtw_cost

pytestmark = pytest.mark.gpu


def _pairs(rs, shapes, D):
    cv, gt, f0c, f0g = [], [], [], []
    for nx, ny in shapes:
        t = np.cumsum(rs.standard_normal((max(nx, ny) + 40, D)) * 0.3, 0)
        # voiced masks drop ~20 % of the frames; lengths above are the VOICED counts
        def with_unvoiced(seq, n):
            total = n + rs.randint(0, 6)
            f0 = np.zeros(total)
            f0[rs.choice(total, n, replace=False)] = 100.0 + rs.uniform(size=n)
            full = rs.standard_normal((total, D))
            full[f0 > 0] = seq
            return full, f0
        a = t[np.sort(rs.choice(len(t), nx, replace=True))] + 0.05 * rs.standard_normal((nx, D))
        b = t[np.sort(rs.choice(len(t), ny, replace=True))] + 0.05 * rs.standard_normal((ny, D))
        A, fa = with_unvoiced(a, nx)
        B, fb = with_unvoiced(b, ny)
        cv.append(A); f0c.append(fa); gt.append(B); f0g.append(fb)
    return cv, f0c, gt, f0g


def test_mcd_fastdtw_matches_oracle_paths_and_values():
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw

    rs = np.random.RandomState(0)
    shapes = [(1, 1), (1, 9), (2, 2), (3, 2), (3, 3), (4, 7), (5, 5), (33, 64), (97, 100), (128, 31), (201, 255), (400, 377)]
    cv, f0c, gt, f0g = _pairs(rs, shapes, 35)
    vals, paths = mcd_fastdtw(cv, f0c, gt, f0g, return_paths=True)
    for p, (nx, ny) in enumerate(shapes):
        ref, rpath = om.mcd(cv[p], f0c[p], gt[p], f0g[p])
        assert [tuple(v) for v in paths[p].tolist()] == rpath, (nx, ny)
        assert np.isclose(vals[p], ref, rtol=1e-12, atol=0), (nx, ny, vals[p], ref)
    # radius 2 as well (wider windows, other base-level sizes)
    vals2, paths2 = mcd_fastdtw(cv[6:10], f0c[6:10], gt[6:10], f0g[6:10], radius=2, return_paths=True)
    for k, p in enumerate(range(6, 10)):
        ref, rpath = om.mcd(cv[p], f0c[p], gt[p], f0g[p], radius=2)
        assert [tuple(v) for v in paths2[k].tolist()] == rpath
        assert np.isclose(vals2[k], ref, rtol=1e-12)


def test_mcd_fastdtw_evaluation_sized_batch():
    """560 pairs of ~600 voiced frames x 35 coefficients (VCC2018: 35 utterances x 4 x 4 speaker pairs):
    one launch; identical sequences give 0 dB along the diagonal; prints the time."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw
    import torch

    rs = np.random.RandomState(1)
    shapes = [(int(n), int(m)) for n, m in zip(rs.randint(400, 800, 560), rs.randint(400, 800, 560))]
    cv, f0c, gt, f0g = _pairs(rs, shapes, 35)
    cv[0], f0c[0] = gt[0].copy(), f0g[0].copy()
    vals = mcd_fastdtw(cv, f0c, gt, f0g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vals = mcd_fastdtw(cv, f0c, gt, f0g)
    dt = time.perf_counter() - t0
    assert vals[0] == 0.0 and all(np.isfinite(v) and v > 0 for v in vals[1:])
    for p in range(7, 560, 36):  # 16 pairs spread over the batch
        ref, _ = om.mcd(cv[p], f0c[p], gt[p], f0g[p])
        assert np.isclose(vals[p], ref, rtol=1e-12), (p, vals[p], ref)
    print(f"MCD + FastDTW of 560 pairs (~600 x 600 frames, D=35): {dt * 1e3:.1f} ms incl. host packing and upload")


# ---------------------------------------------------------------------------------------------------- tests/mcd_cases.py


def _tuples(path):
    return tuple(tuple(v) for v in path.tolist())


def _run(names, radius, **kw):
    """One ragged batch of the named cases, fed through their f0 masks."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw

    m = [C.masked(n) for n in names]
    return mcd_fastdtw([v[0] for v in m], [v[1] for v in m], [v[2] for v in m], [v[3] for v in m], radius=radius, **kw)


def _assert_matches_oracle(name, radius, val, path):
    ref, rpath = C.reference(name, radius)
    print(f"{name} r={radius}: {val!r} against {ref!r}, path of {len(path)} against {len(rpath)}")
    assert _tuples(path) == rpath, (name, radius)
    assert np.isclose(val, ref, rtol=1e-12, atol=0), (name, radius, val, ref)
    if ref == 0.0:
        assert val == 0.0, (name, radius, val)


@pytest.mark.parametrize("radius", [1, 2, 3, C.FULL_RADIUS])
def test_mcd_fastdtw_edge_cases_match_oracle(radius):
    """Every case of tests/mcd_cases.py at this radius, one ragged batch per feature dimension."""
    names = [n for n, r in C.runs() if r == radius]
    dims = sorted({C.cases()[n][0].shape[1] for n in names})
    assert dims == ([2] if radius == C.FULL_RADIUS else [1, 2, 4, 25, 60])
    for D in dims:
        batch = [n for n in names if C.cases()[n][0].shape[1] == D]
        vals, paths = _run(batch, radius, return_paths=True)
        for n, v, p in zip(batch, vals, paths):
            _assert_matches_oracle(n, radius, v, p)
        # path_out == NULL: the same distortions, bit for bit
        assert _run(batch, radius) == vals, (radius, D)


def test_mcd_fastdtw_full_radius_is_the_exhaustive_optimum():
    x, y = C.cases()["full_radius"]
    vals, paths = _run(["full_radius"], C.FULL_RADIUS, return_paths=True)
    path = _tuples(paths[0])
    assert C.is_warping_path(list(path), len(x), len(y))
    assert np.isclose(sum(om.euclidean(x[i], y[j]) for i, j in path), exact_dtw_cost(x, y), rtol=1e-12, atol=0)


@pytest.mark.parametrize("radius", [1, 2])
def test_mcd_fastdtw_batch_independence(radius):
    """A pair's result does not depend on its neighbours, its place, or on whose lengths size the rows and the scratch."""
    # the longest x (200, L_shape2) and the longest y (130, L_shape_noisy) are in different pairs, max_nx > max_ny; then
    # every D = 4 case, where thin / thin5 (y of 300) and thin2 (x of 300) set the maxima
    for batch in (["L_shape2", "L_shape_noisy", "quad4"], [n for n, (x, _) in C.cases().items() if x.shape[1] == 4]):
        lens = [(len(C.cases()[n][0]), len(C.cases()[n][1])) for n in batch]
        ix, iy = int(np.argmax([a for a, _ in lens])), int(np.argmax([b for _, b in lens]))
        assert ix != iy
        if len(batch) == 3:
            assert lens[ix][0] > lens[iy][1]
        vals, paths = _run(batch, radius, return_paths=True)
        for n, v, p in zip(batch, vals, paths):
            _assert_matches_oracle(n, radius, v, p)
        rvals, rpaths = _run(batch[::-1], radius, return_paths=True)
        assert rvals[::-1] == vals and [_tuples(p) for p in rpaths[::-1]] == [_tuples(p) for p in paths]
        for n, v, p in zip(batch, vals, paths):
            v1, p1 = _run([n], radius, return_paths=True)
            assert v1[0] == v and _tuples(p1[0]) == _tuples(p), (n, radius)


def test_mcd_fastdtw_longest_accepted_pair():
    """6398 x 6398 voiced frames: three rows of 6400 doubles, all of the 150 KB of LDS the entry point allows; one frame more
    is refused by the wrapper."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw

    vals, paths = _run(["longest"], 1, return_paths=True)
    _assert_matches_oracle("longest", 1, vals[0], paths[0])
    x, y = C.cases()["longest"]
    more = np.concatenate([x, x[-1:]])
    for a, b in ((more, y), (x, np.concatenate([y, y[-1:]]))):
        with pytest.raises(RuntimeError, match="unsupported"):
            mcd_fastdtw([a], [np.ones(len(a))], [b], [np.ones(len(b))])


def test_mcd_fastdtw_ignores_unvoiced_content():
    """Only voiced frames are judged (and must be finite): an unvoiced frame may hold anything."""
    from crank_amd.bin.evaluate_mcd import mcd_fastdtw

    cv, f0c, gt, f0g = (np.array(v) for v in C.masked("dim25"))
    cv[f0c == 0] = np.nan
    gt[f0g == 0] = np.inf
    vals, paths = mcd_fastdtw([cv], [f0c], [gt], [f0g], return_paths=True)
    _assert_matches_oracle("dim25", 1, vals[0], paths[0])


# (nx, ny) of the middle pair; the library is told max_nx = max_ny = 100, which the two other pairs keep
UNDERSTATED = {
    "rows": (300, 300),    # ny + 2 > wmax: a row of costs would not fit the LDS reservation
    "scratch": (300, 50),  # rows fit, the pair's own scratch layout does not (need > scratch_stride)
}


def _understated(kind):
    rs = np.random.RandomState(11)
    shapes = [(100, 80), UNDERSTATED[kind], (60, 100)]
    return shapes, [C.walk_pair(rs, nx, ny, 4) for nx, ny in shapes]


@pytest.mark.parametrize("kind", list(UNDERSTATED))
def test_mcd_fastdtw_refuses_a_pair_beyond_the_stated_maxima(kind):
    """The kernel sizes a pair's rows and scratch from the pair's own lengths and checks both against what the host
    reserved before its first write: a pair longer than max_nx / max_ny is reported, not run, and its neighbours are
    untouched."""
    import torch
    from crank_amd import _lib
    from crank_amd._ragged import offsets

    D, radius, stated = 4, 1, 100
    shapes, pairs = _understated(kind)
    L = _lib.lib()
    per_pair = L.crk_mcd_scratch_bytes(1, stated, stated, D, radius)
    nx, ny = shapes[1]
    if kind == "rows":
        assert ny + 2 > stated + 2
    else:  # the pair's layout is at least what the host would reserve for exactly its lengths, less the 256-byte rounding
        assert ny + 2 <= stated + 2 and L.crk_mcd_scratch_bytes(1, nx, ny, D, radius) - 256 > per_pair
    dev = torch.device("cuda")
    x = torch.as_tensor(np.concatenate([a for a, _ in pairs]), device=dev)
    y = torch.as_tensor(np.concatenate([b for _, b in pairs]), device=dev)
    xo, yo = offsets([a for a, _ in shapes], dev), offsets([b for _, b in shapes], dev)
    scratch = torch.zeros(3 * per_pair, dtype=torch.uint8, device=dev)
    mcd = torch.full((3,), -1.0, dtype=torch.float64, device=dev)
    plen = torch.full((3,), -1, dtype=torch.int32, device=dev)
    status = torch.full((3,), -1, dtype=torch.int32, device=dev)
    stride = 2 * (stated + stated)
    paths = torch.full((3, stride), -1, dtype=torch.int32, device=dev)
    rc = L.crk_mcd_fastdtw(x.data_ptr(), xo.data_ptr(), y.data_ptr(), yo.data_ptr(), 3, D, radius, stated, stated, mcd.data_ptr(),
                           plen.data_ptr(), paths.data_ptr(), stride, scratch.data_ptr(), status.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert status.tolist() == [0, 1, 0] and plen[1].item() == 0 and np.isnan(mcd[1].item())
    assert (paths[1] == -1).all()  # nothing written for the refused pair
    assert not scratch[per_pair:2 * per_pair].any()  # nor into its scratch
    for p in (0, 2):
        a, b = pairs[p]
        ref, rpath = om.mcd(a, np.ones(len(a)), b, np.ones(len(b)), radius=radius)
        n = plen[p].item()
        assert [tuple(v) for v in paths[p, :2 * n].cpu().numpy().reshape(-1, 2).tolist()] == rpath
        assert np.isclose(mcd[p].item(), ref, rtol=1e-12, atol=0)


def test_mcd_fastdtw_wrapper_raises_on_a_refused_pair(monkeypatch):
    """The wrapper states the true maxima, so a refusal cannot come about through it; here the library it calls is told
    100 / 100 in its place, and the status the kernel reports must surface as RuntimeError."""
    from crank_amd import _lib
    from crank_amd.bin import evaluate_mcd

    real = _lib.lib()

    class Understating:
        def __getattr__(self, name):
            return getattr(real, name)

        def crk_mcd_fastdtw(self, *a):
            return real.crk_mcd_fastdtw(*a[:7], 100, 100, *a[9:])

    _, pairs = _understated("rows")
    args = ([a for a, _ in pairs], [np.ones(len(a)) for a, _ in pairs], [b for _, b in pairs], [np.ones(len(b)) for _, b in pairs])
    vals = evaluate_mcd.mcd_fastdtw(*args)
    assert all(np.isfinite(v) and v > 0 for v in vals)
    monkeypatch.setattr(evaluate_mcd._lib, "lib", lambda: Understating())
    with pytest.raises(RuntimeError, match="exceeded"):
        evaluate_mcd.mcd_fastdtw(*args)
