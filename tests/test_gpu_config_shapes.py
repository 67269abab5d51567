"""GPU parity at the configuration values the default step never builds (default.yml:88-106 at other settings):
quantizers off (D, K) = (64, 512) - the frame-per-lane search kernel with its codebook in LDS chunks, the composed path
behind the fused search, the per-quantizer EMA - and generator stacks at the channel counts, kernel sizes, conditioning
widths and lengths of the other configurations."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import QUANTIZER_SHAPES, golden, quantizer_shape_inputs
from tests.test_gpu_nets import _check_split_forward, _check_standalone, _GenStack, _generator_stack_case
from tests.test_gpu_ops import _make_quantizer, cu

pytestmark = pytest.mark.gpu

# two codes whose fp64 distances to a frame differ by less than this fraction of the terms of the reference's expression
# (sum(w^2) + 2 |x.w| + sum(x^2)) cannot be ordered by an fp32 evaluation of it: either index is a correct answer there
TIE_MARGIN = 1e-6


def _vq_chunk(D, K):
    """The codebook chunk vq_forward_kernel<D> stages in LDS (crk_vq_forward's launcher: halve until it fits)."""
    max_floats = (150 * 1024 - 4 * 128 * 8) // 4
    kchunk = K
    while kchunk * (D + 1) > max_floats:
        kchunk = (kchunk + 1) // 2
    return kchunk


def _search_fp32(x, w):
    """The reference's search on the CPU: fp32 sum(w^2) - 2 x.w^T + sum(x^2), argmin (lowest index on equal values)."""
    x, w = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(w, dtype=torch.float32)
    d = (w * w).sum(1)[None] - 2 * (x @ w.t()) + (x * x).sum(1, keepdim=True)
    return d.argmin(1).numpy()


def _check_indices(got, ref, x, w, what, cap=None):
    """got must equal ref, except at frames where the two chosen codes are an fp64 tie within TIE_MARGIN - at most `cap`
    of them (default: one per thousand frames); returns the number of frames that exception covers (printed)."""
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    diff = np.flatnonzero(got != ref)
    if diff.size:
        x64, w64 = np.asarray(x, np.float64)[diff], np.asarray(w, np.float64)
        wa, wb = w64[got[diff]], w64[ref[diff]]
        da = ((x64 - wa) ** 2).sum(1)
        db = ((x64 - wb) ** 2).sum(1)
        scale = (x64 ** 2).sum(1) + np.maximum((wa ** 2).sum(1), (wb ** 2).sum(1)) + 2 * np.abs(x64 * wa).sum(1)
        far = diff[np.abs(da - db) > TIE_MARGIN * scale]
        assert far.size == 0, (what, far[:8], got[far[:8]], ref[far[:8]])
    print(f"{what}: {got.size} frames, {diff.size} resolved differently as fp64 ties within {TIE_MARGIN:g} of scale")
    assert diff.size <= (max(2, got.size // 1000) if cap is None else cap), (what, diff.size)
    return diff.size


def _frames(x_bdt):
    return x_bdt.transpose(0, 2, 1).reshape(-1, x_bdt.shape[1])


# ------------------------------------------------------------------------------------------------ quantizer search
@pytest.mark.parametrize("D,K", QUANTIZER_SHAPES)
def test_vq_at_other_shapes_matches_reference_quantizer(D, K):
    """quantizer_shapes.npz: the library's Quantizer through three EMA calls and a search after them (8 000 frames each):
    every index against the reference's (fp64 ties aside, counted), e the chosen code rows and qx = x + (e - x) exactly,
    and the EMA state (ema_size, ema_w, the blended codebook at the probed and dead codes, every code's sum) within fp32
    rounding of the reference's."""
    fx = golden("quantizer_shapes.npz")
    tag = f"D{D}_K{K}"
    w0, size0, ema_w0, xs, probe = quantizer_shape_inputs(D, K)
    h, q = _make_quantizer(K, D)
    q.weight.copy_(cu(w0))
    q.ema_size.copy_(cu(size0))
    q.ema_w.copy_(cu(ema_w0))
    for it, x in enumerate(xs):
        w = q.weight.cpu().numpy()
        e, qx, idx = q(cu(x), use_ema=it < 3)
        torch.cuda.synchronize()
        got = idx.cpu().numpy()
        _check_indices(got, fx[f"{tag}/idx{it}"], _frames(x), w, f"{tag} call {it}")
        ef = e.cpu().numpy().reshape(-1, D)
        assert np.array_equal(ef, w[got.reshape(-1)])
        xt = x.transpose(0, 2, 1)
        assert np.array_equal(qx.cpu().numpy(), (xt + (ef.reshape(xt.shape) - xt)).transpose(0, 2, 1))
        if it == 2:
            np.testing.assert_allclose(q.ema_size.cpu().numpy(), fx[f"{tag}/ema_size"], rtol=2e-5, atol=1e-9)
            ew, wt = q.ema_w.cpu().numpy(), q.weight.cpu().numpy()
            np.testing.assert_allclose(ew[:, probe], fx[f"{tag}/ema_w_probe"], rtol=2e-5, atol=2e-6)
            ref = fx[f"{tag}/w_probe"]
            np.testing.assert_allclose(wt[probe], ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
            np.testing.assert_allclose(ew.astype(np.float64).sum(0), fx[f"{tag}/ema_w_sums"], rtol=1e-4, atol=1e-4)
            ref = fx[f"{tag}/w_sums"]
            np.testing.assert_allclose(wt.astype(np.float64).sum(1), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())


@pytest.mark.parametrize("D,K", [(16, 2048), (32, 1024), (64, 4096), (128, 1000), (128, 1001), (64, 4095)])
def test_vq_search_ties_and_edges_at_other_shapes(D, K):
    """Adversarial codebooks for the frame-per-lane search (vq_forward_kernel<D>): exact duplicates in different LDS
    chunks and in different wave-group slices of one chunk (the lowest index wins: torch.argmin), zero codes and zero
    frames, codes 1e-7 apart, NaN / +-inf frames (pinned to code 0 like the D = 64 path), a ragged frame count and, for
    K = 1001 / 4095, a ragged last chunk - against the reference's fp32 search on the CPU."""
    from crank_amd import ops

    rs = np.random.RandomState(D * 7 + K)
    kc = _vq_chunk(D, K)
    per = (kc + 3) // 4  # the slice of a chunk each of the four wave groups scans
    nxt = kc if kc < K else per + 20  # the next chunk (one chunk: inside the next wave group's slice)
    w = (0.5 * rs.standard_normal((K, D))).astype(np.float32)
    dup = [3, 2 * per + 1, nxt + 3, K - 1]  # slice 0 / slice 2 of chunk 0, the next chunk (or slice), the last code
    zero = [per + 5, nxt + 5, K - 2]
    near = [(10, nxt + 10), (11, 3 * per + 2)]  # a code and a copy 1e-7 away, later in the book
    used = dup + zero + [k for p in near for k in p]
    assert len(set(used)) == len(used) and max(used) < K, used
    for k in dup[1:]:
        w[k] = w[3]
    w[zero] = 0.0
    for a, b in near:
        w[b] = w[a] + np.float32(1e-7) * rs.choice([-1.0, 1.0], D).astype(np.float32)
    B, T = 3, 333  # 999 frames: not a multiple of the 128-frame workgroup
    x = rs.standard_normal((B * T, D)).astype(np.float32)
    x[:40] = w[3] + 1e-2 * rs.standard_normal((40, D)).astype(np.float32)
    x[40:48] = w[3]
    x[48:56] = 0.0
    x[56:72] = w[10] + 1e-3 * rs.standard_normal((16, D)).astype(np.float32)
    x[72:88] = w[11] + 1e-3 * rs.standard_normal((16, D)).astype(np.float32)
    bad = [100, 101, 102, 103]
    x[100] = np.nan
    x[101, D // 2] = np.inf
    x[102, 0] = -np.inf
    x[103, D - 1] = np.nan
    e, qx, idx = ops.vq_apply(cu(x.reshape(B, T, D)), cu(w))
    torch.cuda.synchronize()
    got = idx.cpu().numpy().reshape(-1)
    assert (got[40:48] == 3).all(), got[40:48]          # the duplicates: the lowest index, across chunks and slices
    assert (got[:40][np.isin(got[:40], dup)] == 3).all(), got[:40]
    assert (got[48:56] == zero[0]).all(), got[48:56]    # zero frames: the first zero code (distance exactly 0)
    assert (got[bad] == 0).all(), got[bad]              # non-finite frames: code 0
    np.testing.assert_array_equal(e.cpu().numpy().reshape(-1, D), w[got])
    ok = np.setdiff1d(np.arange(B * T), bad)
    # (the 32 frames at the 1e-7 pairs are ties by construction)
    ties = _check_indices(got[ok], _search_fp32(x[ok], w), x[ok], w, f"D={D} K={K} chunk {kc}", cap=32 + 2)
    # the 1e-7 pairs: the later copy only where fp32 cannot tell them apart
    for (a, b), sl in zip(near, (slice(56, 72), slice(72, 88))):
        assert np.isin(got[sl], [a, b]).all(), got[sl]
    print(f"D={D} K={K}: chunk {kc}, duplicates {dup}, zero codes {zero}, 1e-7 pairs {near}, fp64 ties {ties}")


def test_vq_fused_and_composed_paths_at_the_frame_limit():
    """D = 64, K = 512: N = 131 072 frames is the fused search's limit (1024 workgroups of 128), one frame more takes
    the composed path (input sum, search, loss pass).  Both: indices against the exact fp32 search (fp64 ties aside),
    x + add bit for bit, e the chosen rows, the commitment loss against float64 within fp32 summation order; and the two
    paths agree bit for bit on the frames they share."""
    from crank_amd import ops

    rs = np.random.RandomState(17)
    D, K = 64, 512
    w = (0.8 * rs.standard_normal((K, D))).astype(np.float32)
    N1 = 131073
    x = rs.standard_normal((1, N1, D)).astype(np.float32)
    a = (0.1 * rs.standard_normal((1, N1, D))).astype(np.float32)
    xs = x + a
    ref = _search_fp32(xs[0], w)
    res = {}
    for N in (131072, N1):
        e, qx, idx, commit, xin = ops.vq_commit_apply(cu(x[:, :N]), cu(w), None, add=cu(a[:, :N]))
        torch.cuda.synchronize()
        got = idx.cpu().numpy().reshape(-1)
        _check_indices(got, ref[:N], xs[0, :N], w, f"vq_commit_apply N={N}")
        assert np.array_equal(xin.cpu().numpy(), xs[:, :N])
        ev = e.cpu().numpy()[0]
        assert np.array_equal(ev, w[got])
        c64 = ((xs[0, :N].astype(np.float64) - ev) ** 2).mean()
        assert abs(float(commit) - c64) <= 1e-5 * c64, (N, float(commit), c64)
        res[N] = (got, qx.cpu().numpy(), float(commit))
    n0 = 131072
    assert np.array_equal(res[n0][0], res[N1][0][:n0])
    assert np.array_equal(res[n0][1], res[N1][1][:, :n0])


# ------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize("D,K", [(32, 100), (128, 100), (32, 1024), (128, 1024), (32, 4096), (128, 4096)])
def test_vq_ema_at_other_shapes_against_the_oracle(D, K):
    """The per-quantizer EMA path (crk_vq_ema_stats / crk_vq_ema_partial + reduce, crk_vq_ema_apply) at K = 100, 1024,
    4096 and D = 32, 128: counts and the 2^-28 fixed-point sums exactly (against an int64 recount on the CPU, and the
    two statistic paths bit for bit), then three blends against oracle/modules.py vq_ema_update within fp32 rounding,
    dead codes (Laplace smoothing, quirk Q2) included."""
    from crank_amd import ops
    from oracle.modules import vq_ema_update

    rs = np.random.RandomState(D + K)
    N = 5000
    size = np.where(np.arange(K) < K - K // 5, rs.uniform(1, 30, K), 0.0).astype(np.float32)
    ema_w = rs.standard_normal((D, K)).astype(np.float32)
    st = [cu(size), cu(ema_w), torch.zeros(K, D, device="cuda")]
    orac = [torch.from_numpy(size), torch.from_numpy(ema_w)]
    for it in range(3):
        x = (rs.standard_normal((N, D)) * (1.0 + it)).astype(np.float32)
        idx = rs.randint(0, K - K // 5, N).astype(np.int64)  # the last fifth of the codes stays dead
        counts = torch.empty(K, device="cuda", dtype=torch.int32)
        sums = torch.empty(D * K, device="cuda", dtype=torch.int64)
        ops.vq_ema_stats(cu(x), cu(idx), counts, sums)
        c2 = torch.empty_like(counts)
        s2 = torch.empty_like(sums)
        part = ops.vq_ema_partial(cu(x), cu(idx), D, K)
        ops.vq_ema_reduce_multi([part[0]], [part[1]], [D], [K], [c2], [s2])
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), np.bincount(idx, minlength=K))
        fixed = np.rint(x.astype(np.float64) * 2.0 ** 28).astype(np.int64)
        ref_sums = np.zeros((D, K), np.int64)
        np.add.at(ref_sums.T, idx, fixed)
        assert np.array_equal(sums.cpu().numpy().reshape(D, K), ref_sums)
        assert torch.equal(counts, c2) and torch.equal(sums, s2)
        ops.vq_ema_apply(counts, sums, st[0], st[1], st[2], 0.99, 1e-5)
        s, ew, cb = vq_ema_update(torch.from_numpy(x)[None], torch.from_numpy(idx)[None], orac[0], orac[1])
        orac = [s, ew]
        torch.cuda.synchronize()
        np.testing.assert_allclose(st[0].cpu().numpy(), s.numpy(), rtol=2e-5, atol=1e-9)
        np.testing.assert_allclose(st[1].cpu().numpy(), ew.numpy(), rtol=2e-5, atol=2e-6 * (1 + it))
        cbg = st[2].cpu().numpy()
        np.testing.assert_allclose(cbg, cb.numpy(), rtol=1e-4, atol=1e-5 * np.abs(cb.numpy()).max())
        assert np.abs(cbg[K - K // 5:]).max() > 1e3  # dead codes: ema_w over a smoothed size of ~1e-5


# (D, K, N): 9 chunks (one unrolled group of 8 and a tail of 1) | 2 chunks, K no multiple of 16 | one frame, 8 dim slices |
# the 64-chunk cap, a padded last image tile | slice width 4, four codes per lane in the size kernel
EMA_EXACT_SHAPES = [(64, 512, 1100), (32, 100, 129), (128, 1024, 1), (64, 500, 8200), (32, 4096, 300)]
EMA_DECAY, EMA_EPS = 0.99, 1e-5


def _ema_mix_exact(decay, a, omd, b):
    """ema_mix of vq_kernels.hip on fp32 arrays: fl32(omd * b), then decay * a + t with ONE rounding (a fused
    multiply-add).  Formed in float64, where the product is exact, and rounded to fp32: that differs from the single
    rounding only where the float64 sum lies exactly on an fp32 midpoint.  Returns (values, number of such elements)."""
    t = omd * b
    assert t.dtype == np.float32
    v = np.float64(decay) * a.astype(np.float64) + t.astype(np.float64)
    return v.astype(np.float32), int(np.count_nonzero((v.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)))


@functools.lru_cache(maxsize=None)
def _ema_exact_case(D, K, N):
    """Inputs of three EMA updates in a row (drawn as in test_vq_ema_at_other_shapes_against_the_oracle, the last fifth
    of the codes dead) and what the kernels must leave after each, restated on the CPU in the kernels' rounding order:
    [(x, idx, counts, sums, ema_size, ema_w, codebook)], the initial (ema_size, ema_w), and the midpoint count."""
    f32 = np.float32
    rs = np.random.RandomState(1000 + D + K + N)
    size = np.where(np.arange(K) < K - K // 5, rs.uniform(1, 30, K), 0.0).astype(f32)
    ema_w = rs.standard_normal((D, K)).astype(f32)
    init, steps, mid = (size, ema_w), [], 0
    decay, omd, eps, keps = f32(EMA_DECAY), f32(1.0 - EMA_DECAY), f32(EMA_EPS), f32(K * EMA_EPS)
    for it in range(3):
        x = (rs.standard_normal((N, D)) * (1.0 + it)).astype(f32)
        idx = rs.randint(0, K - K // 5, N).astype(np.int64)
        counts = np.bincount(idx, minlength=K).astype(np.int32)
        sums = np.zeros((D, K), np.int64)
        np.add.at(sums.T, idx, np.rint(x.astype(np.float64) * 2.0 ** 28).astype(np.int64))
        # cluster sizes: 1024 lanes add their codes k = lane, lane + 1024, ... in turn, a tree adds the lanes
        v, m = _ema_mix_exact(decay, size, omd, counts.astype(f32))
        mid += m
        lanes = np.zeros(-(-K // 1024) * 1024, f32)
        lanes[:K] = v
        red = np.zeros(1024, f32)
        for row in lanes.reshape(-1, 1024):
            red = red + row
        o = 512
        while o > 0:
            red[:o] = red[:o] + red[o:2 * o]
            o >>= 1
        n = red[0]
        den = n + keps
        size = (v + eps) / den * n
        # blend
        es = sums.astype(f32) * f32(2.0 ** -28)
        ema_w, m = _ema_mix_exact(decay, ema_w, omd, es)
        mid += m
        cb = np.ascontiguousarray((ema_w / size[None, :]).T)
        assert size.dtype == ema_w.dtype == cb.dtype == f32
        for a in (x, idx, counts, sums, size, ema_w, cb):
            a.setflags(write=False)
        steps.append((x, idx, counts, sums, size, ema_w, cb))
    return steps, init, mid


@pytest.mark.parametrize("shapes", [[s] for s in EMA_EXACT_SHAPES] + [EMA_EXACT_SHAPES[:4]],
                         ids=lambda ss: "+".join("x".join(map(str, s)) for s in ss))
def test_vq_ema_every_entry_point_equals_an_exact_cpu_restatement(shapes):
    """Every EMA entry point against a NumPy restatement of the kernels' arithmetic in their rounding order, bit for
    bit - counts, fixed-point sums, ema_size, ema_w and codebook after each of three updates in a row: (A) stats + apply,
    (B) partial + reduce_multi + apply_multi, (C) partial_multi + reduce_size_multi + blend_multi, (D, for D = 64 and
    K <= 512) the same with the blend that leaves the search image current, which must equal vq_image_build of the new
    codebook; then four shapes in one nq = 4 call through (B) and (C).  The oracle tests pin this arithmetic to 2e-5
    only, and the batched-equals-single tests compare one kernel with itself; this is the exact anchor."""
    from crank_amd import ops

    def dev(a):  # (a copy: the shared reference arrays are read-only)
        return torch.tensor(a, device="cuda")

    cases = [_ema_exact_case(*s) for s in shapes]
    assert sum(c[2] for c in cases) == 0  # no element on an fp32 midpoint: the restatement is exact for these inputs
    Ds, Ks = [s[0] for s in shapes], [s[1] for s in shapes]
    single = len(shapes) == 1
    paths = ["B", "C"] + (["A"] if single else []) + (["D"] if single and Ds[0] == 64 and Ks[0] <= 512 else [])
    for path in paths:
        size = [dev(c[1][0]) for c in cases]
        ema_w = [dev(c[1][1]) for c in cases]
        cb = [torch.zeros(K, D, device="cuda") for D, K in zip(Ds, Ks)]
        for it in range(3):
            xs = [dev(c[0][it][0]) for c in cases]
            idxs = [dev(c[0][it][1]) for c in cases]
            counts = [torch.empty(K, device="cuda", dtype=torch.int32) for K in Ks]
            sums = [torch.empty(D * K, device="cuda", dtype=torch.int64) for D, K in zip(Ds, Ks)]
            img = None
            if path == "A":
                ops.vq_ema_stats(xs[0], idxs[0], counts[0], sums[0])
                ops.vq_ema_apply(counts[0], sums[0], size[0], ema_w[0], cb[0], EMA_DECAY, EMA_EPS)
            elif path == "B":
                parts = [ops.vq_ema_partial(x, i, D, K) for x, i, D, K in zip(xs, idxs, Ds, Ks)]
                ops.vq_ema_reduce_multi([p[0] for p in parts], [p[1] for p in parts], Ds, Ks, counts, sums)
                ops.vq_ema_apply_multi(counts, sums, size, ema_w, cb, Ds, Ks, EMA_DECAY, EMA_EPS)
            else:
                parts = ops.vq_ema_partial_multi(xs, idxs, Ds, Ks)
                ops.vq_ema_reduce_size_multi([p[0] for p in parts], [p[1] for p in parts], Ds, Ks, counts, sums, size,
                                             EMA_DECAY, EMA_EPS)
                if path == "D":
                    img = [torch.full((ops.vq_image_bytes(Ks[0], 64),), 0x5A, device="cuda", dtype=torch.uint8)]
                assert ops.vq_ema_blend_multi(sums, size, ema_w, cb, Ds, Ks, EMA_DECAY, images=img) is (path == "D")
            if img is not None:
                built = [torch.full_like(img[0], 0xA5)]
                ops.vq_image_build(cb, built)
                assert torch.equal(img[0], built[0]), (path, it)
            torch.cuda.synchronize()
            for q, c in enumerate(cases):
                _, _, r_counts, r_sums, r_size, r_w, r_cb = c[0][it]
                got = (counts[q], sums[q].view(Ds[q], Ks[q]), size[q], ema_w[q], cb[q])
                for name, g, r in zip(("counts", "sums", "ema_size", "ema_w", "codebook"), got, (r_counts, r_sums, r_size, r_w, r_cb)):
                    g = g.cpu().numpy()
                    # (bytes, so that neither a NaN nor the sign of a zero can hide)
                    assert g.tobytes() == r.tobytes(), (path, shapes[q], it, name, int(np.count_nonzero(g != r)), g[g != r][:4], r[g != r][:4])


def test_generator_ema_of_quantizers_of_different_shapes_equals_each_alone():
    """Two quantizers of different (D, K) sharing one statistics message: flush_ema's multi entry points take them in
    one launch (the blend that would refresh the search images refuses these shapes and the plain blend runs) - the
    result equals each quantizer updated alone, bit for bit, indices included."""
    from crank_amd import parallel
    from crank_amd.net.module.vqvae2 import flush_ema

    dims = [(32, 1024), (128, 256)]
    rs = np.random.RandomState(5)
    init = [((0.8 * rs.standard_normal((K, D))).astype(np.float32), rs.uniform(0, 20, K).astype(np.float32),
             rs.standard_normal((D, K)).astype(np.float32)) for D, K in dims]
    xs = [[rs.standard_normal((2, D, 700)).astype(np.float32) for _ in range(2)] for D, _ in dims]

    def setup():
        qs = []
        for (D, K), (w, s, ew) in zip(dims, init):
            h, q = _make_quantizer(K, D)
            q.weight.copy_(cu(w))
            q.ema_size.copy_(cu(s))
            q.ema_w.copy_(cu(ew))
            qs.append(q)
        return qs

    together = setup()
    bucket = parallel.EmaBucket(dims, "cuda")
    for i, q in enumerate(together):
        q.bucket, q.slot = bucket, i
    alone = setup()
    for it in range(2):
        pending, idx_t = [], []
        for q, x in zip(together, xs):
            idx_t.append(q.quantize(cu(x[it]).transpose(1, 2), pending=pending)[2])
        flush_ema(pending)
        idx_a = [q(cu(x[it]))[2] for q, x in zip(alone, xs)]
        torch.cuda.synchronize()
        for qa, qb, ia, ib in zip(together, alone, idx_t, idx_a):
            assert torch.equal(ia, ib)
            for a, b in ((qa.weight, qb.weight), (qa.ema_size, qb.ema_size), (qa.ema_w, qb.ema_w)):
                assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ generator stacks
# (in, out, k, layers, stacks, aux, causal, T) of the stacks other configurations build, and the kernel generation
# crk_debug_net_paths must report for them.  bit 0 (route_of, net.hip) needs in and out a multiple of 8, a kernel
# of 3 or 5 and no conditioning on a kernel-3 stack (stack2_fwd_plan); none of these shapes exceeds its other limits.
# Where it fails, bit 1 (the bf16x3f split forward) cannot hold either and the stack runs the frame-split kernels.
GEN_CASES = {
    "vq_level3": ((64, 64, 3, 4, 2, 0, False, 500), True),
    "emb_dim32": ((32, 32, 3, 6, 3, 0, False, 500), True),
    "mcep24k_enc0": ((36, 64, 5, 8, 4, 0, False, 500), False),
    "mcep24k_dec0": ((128, 36, 5, 8, 4, 34, False, 500), False),
    "mcep22k_dec0": ((128, 34, 5, 8, 4, 34, False, 500), False),
    "dec0_no_f0": ((128, 80, 5, 8, 4, 32, False, 500), True),
    "dec0_onehot14_f0": ((128, 80, 5, 8, 4, 16, False, 500), True),
    "causal_enc0": ((80, 64, 5, 8, 4, 0, True, 500), True),
    "causal_enc1": ((64, 64, 3, 6, 3, 0, True, 333), True),
}


def _gen_cfg(case):
    (cin, cout, k, layers, stacks, aux, causal, T), split = GEN_CASES[case]
    cfg = dict(in_channels=cin, out_channels=cout, kernel_size=k, layers=layers, stacks=stacks, aux_channels=aux)
    if causal:
        cfg["use_causal_conv"] = True
    return cfg, T, split


def _paths(cfg, B, T):
    from crank_amd import _lib

    prod = _GenStack(**cfg)
    return int(_lib.lib().crk_debug_net_paths(prod.stack.net.handle, B, T))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", list(GEN_CASES))
def test_generator_stack_at_other_configurations(case, precision):
    """Forward, dx, dc and every parameter gradient against the fp32 oracle (bf16x3, 2e-4 of scale) and the bf16
    emulation (bf16) - with the kernel generation the case is meant to cover pinned first."""
    cfg, T, split = _gen_cfg(case)
    paths = _paths(cfg, 2, T)
    print(case, "crk_debug_net_paths", paths)
    assert bool(paths & 1) == split, (case, paths)
    if not split:
        assert not paths & 2, (case, paths)
    _generator_stack_case(cfg, T, precision, B=2)


@pytest.mark.parametrize("case", [c for c, (_, split) in GEN_CASES.items() if split])
def test_generator_stack_split_forward_at_other_configurations(case):
    """bf16x3f where the channel-split path applies: as test_generator_stack_split_forward_plain_backward."""
    from oracle import pwg

    cfg, T, _ = _gen_cfg(case)
    prod = _GenStack(**cfg)
    orac = pwg.ParallelWaveGANGenerator(**cfg, upsample_conditional_features=False)
    aux = cfg["aux_channels"]
    _check_split_forward(prod, orac, cfg["in_channels"], aux, 2, T, f"{case} k{cfg['kernel_size']} aux {aux}",
                         orac_call=(None if aux else (lambda x: orac(x, None))))
