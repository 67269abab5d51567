"""The loss kernels of csrc/loss_kernels.hip (masked L1 / MSE means, cross entropy, the fused reconstruction / STFT loss,
the speaker-embedding gather and its table gradient) against float64 references at the sizes where their scale-only code
runs: grids at the LOSS_MAX_BLOCKS cap with grid-stride loops that go round more than once and finishing loops over more
than 256 partials, the reconstruction loss's group loop, the embedding gradient's 32- and 8-wide reductions and tables
that do not fit one workgroup's LDS (100 and more speakers).  Where the host picks between two paths for one input
(16-byte or scalar masked losses, register or generic cross entropy), the same values go through both.  Every case first
restates, on the host, the predicate that sends it to its edge or path.  The C ABI is called directly wherever the ops
wrappers would copy or re-stride an input and so hide the path."""
import numpy as np
import pytest
import torch

from crank_amd import _lib
from crank_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu

LOSS_MAX_BLOCKS = 1024  # loss_kernels.hip
EMB_FRAMES, EMB_LDS = 256, 60 * 1024


def L():
    return _lib.lib()


def blocks(items):
    """loss_blocks(): workgroups of a grid-stride launch over `items` work items, 256 per workgroup."""
    return max(1, min(LOSS_MAX_BLOCKS, (items + 255) // 256))


def strided(vals, ld, off=0):
    """A (N, D) device view of vals with row stride ld, starting `off` floats into its allocation; the columns between D
    and ld and the floats in front hold 1e30, so a read of them shows in any sum."""
    N, D = vals.shape
    buf = torch.full((off + N * ld + 4,), 1e30, dtype=torch.float32, device="cuda")
    v = buf[off: off + N * ld].view(N, ld)[:, :D]
    v.copy_(vals)
    return v


def ld_of(t):
    return 0 if t is None else t.stride(0)


def vec4_ok(D, *ts):
    """loss_vec4_ok(): the pointers 16-byte aligned, D and the row strides multiples of 4."""
    return all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in ts) and D % 4 == 0


def scratch():
    return torch.empty(L().crk_loss_scratch_floats(), dtype=torch.float32, device="cuda")


def dscal(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------ A. masked L1 / MSE
def ml_fwd(x, y, mask, mode, yconst=0.0):
    N, D = x.shape
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    check(L().crk_masked_loss_fwd(ptr(x), ld_of(x), ptr(y), ld_of(y), yconst, ptr(mask), N, D, mode, ptr(out), ptr(scratch()),
                                  stream_ptr()), "crk_masked_loss_fwd")
    return out


def ml_both(x, y, mask):
    N, D = x.shape
    out = torch.empty(4, dtype=torch.float32, device="cuda")
    check(L().crk_masked_loss_both_fwd(ptr(x), ld_of(x), ptr(y), ld_of(y), ptr(mask), N, D, ptr(out), ptr(scratch()),
                                       stream_ptr()), "crk_masked_loss_both_fwd")
    return out


def ml_bwd(x, y, mask, mode, stat, g, yconst=0.0, add=None, add_scale=None, want_dy=False):
    N, D = x.shape
    dx = torch.empty(N, D, dtype=torch.float32, device="cuda")
    dy = torch.empty(N, D, dtype=torch.float32, device="cuda") if want_dy else None
    check(L().crk_masked_loss_bwd_acc(ptr(x), ld_of(x), ptr(y), ld_of(y), yconst, ptr(mask), N, D, mode, ptr(stat), ptr(g),
                                      ptr(dx), D, ptr(dy), D, ptr(add), ld_of(add), ptr(add_scale), stream_ptr()),
          "crk_masked_loss_bwd_acc")
    return dx, dy


def bwd4_taken(x, y, dx, add, want_dy):
    """crk_masked_loss_bwd_acc's choice of masked_loss_bwd<4>: y a tensor, dx wanted, dy not, 16-byte pointers, D and the
    row strides multiples of 4."""
    ts = [t for t in (x, y, dx, add) if t is not None]
    return y is not None and not want_dy and vec4_ok(x.shape[1], *ts)


def ref_masked(x, y, yconst, mask):
    """(L1 mean, MSE mean, count, float64 difference, selected frames) of the masked pair."""
    xd = x.detach().cpu().double()
    d = xd - (y.detach().cpu().double() if y is not None else yconst)
    sel = mask.cpu().bool() if mask is not None else torch.ones(x.shape[0], dtype=torch.bool)
    cnt = int(sel.sum()) * x.shape[1]
    return float(d[sel].abs().sum()) / cnt if cnt else float("nan"), float((d[sel] ** 2).sum()) / cnt if cnt else float("nan"), \
        cnt, d, sel


def make_mask(kind, N, gen):
    if kind == "none":
        return None
    if kind == "random":
        m = torch.rand(N, generator=gen) > 0.3
    elif kind == "single":
        m = torch.zeros(N, dtype=torch.bool)
        m[N // 3] = True
    else:
        m = torch.zeros(N, dtype=torch.bool)
    return m.to(torch.uint8).cuda()


# name: (N, D, ldx, ldy, pointer offset of x in floats, 16-byte path expected, items above one full pass of the grid)
ML_CASES = {
    "bench-64x500x80": (32000, 80, 80, 80, 0, True, True),   # 640 000 four-wide items: 2.4 passes, 1024 partials
    "scalar-64x500x35": (32000, 35, 35, 35, 0, False, True),  # 1 120 000 elements
    "d1": (300001, 1, 1, 1, 0, False, True),
    "d3": (300001, 3, 3, 3, 0, False, True),
    "d4": (300001, 4, 4, 4, 0, True, True),
    "stride83": (32000, 80, 83, 80, 0, False, True),          # a row stride above D, not a multiple of 4
    "offset1": (32000, 80, 80, 80, 1, False, True),           # x one float past 16-byte alignment
}


# every case without a mask and with a random one; a single frame and no frame at all on the two paths' benchmark shapes
ML_RUNS = [(n, m) for n in ML_CASES for m in ("none", "random")] + \
    [(n, m) for n in ("bench-64x500x80", "scalar-64x500x35", "d1") for m in ("single", "empty")]


@pytest.mark.parametrize("name,mask_kind", ML_RUNS)
def test_masked_losses_vs_float64(name, mask_kind):
    N, D, ldx, ldy, off, v4, multi = ML_CASES[name]
    gen = torch.Generator().manual_seed(hash((N, D, ldx)) % 1000)
    xh = torch.randn(N, D, generator=gen)
    yh = xh + 0.5 * torch.randn(N, D, generator=gen)
    x, y = strided(xh, ldx, off), strided(yh, ldy)
    mask = make_mask(mask_kind, N, gen)
    # the path and the edge, on the host
    assert vec4_ok(D, x, y) == v4
    items = N * D // 4 if v4 else N * D
    assert (items > LOSS_MAX_BLOCKS * 256) == multi and blocks(items) == LOSS_MAX_BLOCKS  # > 256 partials to finish
    l1r, mser, cnt, d, sel = ref_masked(x, y, 0.0, mask)
    o1, o2 = ml_fwd(x, y, mask, 0).cpu(), ml_fwd(x, y, mask, 1).cpu()
    both = ml_both(x, y, mask).cpu()
    assert float(o1[1]) == cnt and float(o2[1]) == cnt, (float(o1[1]), cnt)
    if cnt == 0:
        assert torch.isnan(o1[0]) and torch.isnan(o2[0])
    else:
        np.testing.assert_allclose(float(o1[0]), l1r, rtol=1e-5)
        np.testing.assert_allclose(float(o2[0]), mser, rtol=1e-5)
    # masked_loss_both_*: "the same loop and reduction order as the single-mode kernels"
    assert torch.equal(both[:2], o1) or (cnt == 0 and float(both[1]) == 0), (both, o1)
    assert torch.equal(both[2:], o2) or (cnt == 0 and float(both[3]) == 0), (both, o2)
    # backward: L1 exactly sign(x - y) * fp32(g / count), MSE against 2 (x - y) g / count
    g = dscal(1.7)
    selc = sel.cuda()[:, None]
    gc = (torch.tensor(1.7, dtype=torch.float32) / torch.tensor(float(cnt), dtype=torch.float32)).item()
    for mode, stat in ((0, ml_fwd(x, y, mask, 0)), (1, ml_fwd(x, y, mask, 1))):
        dx, _ = ml_bwd(x, y, mask, mode, stat, g)
        assert bwd4_taken(x, y, dx, None, False) == v4
        if mode == 0:
            want = torch.where(selc, torch.sign(x - y) * gc, torch.zeros_like(dx))
            assert torch.equal(dx, want), float((dx - want).abs().max())
        else:
            want = torch.where(sel[:, None], 2.0 * d * 1.7 / max(cnt, 1), torch.zeros_like(d)).numpy()
            np.testing.assert_allclose(dx.cpu().numpy(), want, rtol=1e-6, atol=0)
        if cnt == 0:
            assert not dx.abs().max() > 0


def test_masked_loss_paths_agree_on_the_same_values():
    """One (64 x 500 x 80) pair through the 16-byte kernels and, copied to row stride 83, through the scalar ones: the
    same count, means within 1e-6, and the backward kernels (masked_loss_bwd<4> against <1>; the scalar one again with dy
    wanted) bit for bit, with and without add / add_scale."""
    gen = torch.Generator().manual_seed(11)
    N, D = 32000, 80
    xh = torch.randn(N, D, generator=gen)
    yh = xh + 0.5 * torch.randn(N, D, generator=gen)
    ah = torch.randn(N, D, generator=gen)
    mask = make_mask("random", N, gen)
    xv, yv = xh.cuda(), yh.cuda()
    xs, ys = strided(xh, 83), strided(yh, 83)
    assert vec4_ok(D, xv, yv) and not vec4_ok(D, xs, ys)
    for mode in (0, 1):
        fv, fs = ml_fwd(xv, yv, mask, mode), ml_fwd(xs, ys, mask, mode)
        assert float(fv[1]) == float(fs[1])
        np.testing.assert_allclose(float(fv[0]), float(fs[0]), rtol=1e-6)
        bv, bs = ml_both(xv, yv, mask), ml_both(xs, ys, mask)
        assert torch.equal(bv[2 * mode: 2 * mode + 2], fv) and torch.equal(bs[2 * mode: 2 * mode + 2], fs)
        g, sc = dscal(-0.8), dscal(0.37)
        for add, add_s, asc in ((None, None, None), (ah.cuda(), strided(ah, 81), sc), (ah.cuda(), strided(ah, 81), None)):
            d4, _ = ml_bwd(xv, yv, mask, mode, fv, g, add=add, add_scale=asc)
            d1, _ = ml_bwd(xs, ys, mask, mode, fv, g, add=add_s, add_scale=asc)
            dd, dy = ml_bwd(xv, yv, mask, mode, fv, g, add=add, add_scale=asc, want_dy=True)
            assert bwd4_taken(xv, yv, d4, add, False) and not bwd4_taken(xs, ys, d1, add_s, False)
            assert not bwd4_taken(xv, yv, dd, add, True)
            assert torch.equal(d4, d1), (mode, float((d4 - d1).abs().max()))
            assert torch.equal(d4, dd), (mode, float((d4 - dd).abs().max()))
            r, _ = ml_bwd(xv, yv, mask, mode, fv, g)
            assert torch.equal(dy, -r)
            # against float64: dx = add * add_scale + d loss / dx
            cnt = float(fv[1])
            dd64 = (xh.double() - yh.double())
            sel = mask.cpu().bool()[:, None]
            rr = torch.where(sel, torch.sign(dd64) if mode == 0 else 2.0 * dd64, torch.zeros_like(dd64)) * (-0.8 / cnt)
            want = rr + (ah.double() * (0.37 if asc is not None else 1.0) if add is not None else 0.0)
            tol = 1e-6 * float(want.abs().max())
            np.testing.assert_allclose(d4.cpu().numpy(), want.numpy(), rtol=1e-6, atol=tol)


@pytest.mark.parametrize("yconst", [1.0, 0.0])
@pytest.mark.parametrize("mask_kind", ["none", "random", "empty"])
def test_lsgan_constant_target_at_the_benchmark_size(yconst, mask_kind):
    """y = NULL with the LSGAN targets 1 and 0 on 64 x 500 x 1 (always the scalar kernels): mean, count, gradient."""
    gen = torch.Generator().manual_seed(3)
    N = 32000
    xh = torch.randn(N, 1, generator=gen) * 0.6 + 0.5
    x = xh.cuda()
    mask = make_mask(mask_kind, N, gen)
    assert blocks(N) == 125
    l1r, mser, cnt, d, sel = ref_masked(x, None, yconst, mask)
    for mode, ref in ((0, l1r), (1, mser)):
        o = ml_fwd(x, None, mask, mode, yconst)
        assert float(o[1]) == cnt
        if cnt:
            np.testing.assert_allclose(float(o[0]), ref, rtol=1e-5)
        else:
            assert torch.isnan(o[0])
        dx, _ = ml_bwd(x, None, mask, mode, o, dscal(2.0), yconst=yconst)
        gc = (torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(cnt), dtype=torch.float32)).item()
        selc = sel.cuda()[:, None]
        if mode == 0:
            assert torch.equal(dx, torch.where(selc, torch.sign(x - yconst) * gc, torch.zeros_like(dx)))
        else:
            want = torch.where(sel[:, None], 2.0 * d * 2.0 / max(cnt, 1), torch.zeros_like(d)).numpy()
            np.testing.assert_allclose(dx.cpu().numpy(), want, rtol=1e-6, atol=0)


# ------------------------------------------------------------------ B. cross entropy
def ce_fwd(logits, target, C):
    N = target.shape[0]
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    dl = torch.empty(N, C, dtype=torch.float32, device="cuda")
    check(L().crk_ce_fwd(ptr(logits), logits.stride(0), ptr(target), N, C, -100, ptr(out), ptr(dl), ptr(scratch()),
                         stream_ptr()), "crk_ce_fwd")
    return out, dl


def ce_bwd(dl, stat, g):
    N, C = dl.shape
    res = torch.empty(N, C, dtype=torch.float32, device="cuda")
    check(L().crk_ce_bwd(ptr(dl), N, C, ptr(stat), ptr(g), ptr(res), stream_ptr()), "crk_ce_bwd")
    return res


def rows8(logits, dl, C):
    """crk_ce_fwd's choice of ce_partial_regs (for C = 12 / 14): contiguous rows, both pointers 8-byte aligned."""
    return logits.stride(0) == C and logits.data_ptr() % 8 == 0 and dl.data_ptr() % 8 == 0


def ce_inputs(N, C, seed):
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.rand(N, C, generator=gen) * 2 - 1) * 80.0
    t = torch.randint(0, C, (N,), generator=gen)
    t[torch.rand(N, generator=gen) < 0.1] = -100
    t[:3] = torch.tensor([0, C - 1, -100])
    return logits, t


def ce_ref(logits, t):
    ld = logits.double()
    keep = t != -100
    lse = torch.logsumexp(ld, 1)
    rows = lse[keep] - ld[keep, t[keep]]
    p = torch.softmax(ld, 1)
    p[keep, t[keep]] -= 1.0
    p[~keep] = 0.0
    return float(rows.mean()), int(keep.sum()), p


@pytest.mark.parametrize("N", [32000, 300001])
@pytest.mark.parametrize("C", [2, 12, 13, 14, 16, 100])
def test_cross_entropy_vs_float64(C, N):
    """Targets 0 and C - 1, -100 rows, logits over +-80 (most expf terms underflow); N = 300 001 runs the grid-stride
    loop of the capped grid and a finishing loop over 1024 partials."""
    logits, t = ce_inputs(N, C, 7 * C + N % 5)
    assert (t == 0).any() and (t == C - 1).any() and (t == -100).any()
    assert blocks(N) == (125 if N == 32000 else LOSS_MAX_BLOCKS) and (N > LOSS_MAX_BLOCKS * 256) == (N == 300001)
    # a large share of the exp terms underflow (fp32 expf is 0 below -103.97)
    assert float(((logits.max(1, keepdim=True).values - logits) > 104.0).float().mean()) > (0.1 if C > 2 else 0.02)
    lg, tg = logits.cuda(), t.cuda()
    out, dl = ce_fwd(lg, tg, C)
    assert rows8(lg, dl, C)  # (ce_partial_regs for C = 12 / 14, ce_partial otherwise)
    ref, cnt, gref = ce_ref(logits, t)
    assert float(out[1]) == cnt
    np.testing.assert_allclose(float(out[0]), ref, rtol=1e-5)
    keep = (t != -100)
    dlc = dl.cpu()
    assert not dlc[~keep].abs().max() > 0
    np.testing.assert_allclose(dlc.numpy(), gref.numpy(), rtol=2e-5, atol=2e-5)
    # the backward scales the saved gradient by fp32(g / count), nothing else
    g = dscal(3.0)
    res = ce_bwd(dl, out, g)
    gc = torch.tensor(3.0, dtype=torch.float32) / out[1].cpu()
    assert torch.equal(res.cpu(), dlc * gc)


def test_cross_entropy_of_an_all_ignored_batch():
    """Every target -100: loss NaN and count 0 (torch's mean over nothing), gradient 0 (torch's too), on both kernels."""
    for C, ldl in ((14, 14), (14, 16), (100, 100)):
        N = 3000
        logits = strided(torch.randn(N, C), ldl)
        t = torch.full((N,), -100, dtype=torch.long, device="cuda")
        out, dl = ce_fwd(logits, t, C)
        assert rows8(logits, dl, C) == (ldl == C)
        assert torch.isnan(out[0]) and float(out[1]) == 0.0
        assert not dl.abs().max() > 0
        res = ce_bwd(dl, out, dscal(1.0))
        assert torch.equal(res, torch.zeros_like(res)), (C, ldl, res.abs().max())


@pytest.mark.parametrize("C", [12, 14])
@pytest.mark.parametrize("N", [32000, 300001])
def test_cross_entropy_register_and_generic_paths_are_bit_identical(C, N):
    """The same logits through ce_partial_regs (contiguous, 8-byte aligned rows) and through ce_partial (row stride C + 2,
    and contiguous rows one float off 8-byte alignment): loss, count and unscaled gradient bit for bit."""
    logits, t = ce_inputs(N, C, 100 + C)
    tg = t.cuda()
    lc = logits.cuda()
    ref = ce_fwd(lc, tg, C)
    assert rows8(lc, ref[1], C)
    for lv in (strided(logits, C + 2), strided(logits, C, off=1)):
        out, dl = ce_fwd(lv, tg, C)
        assert not rows8(lv, dl, C)
        assert torch.equal(out, ref[0]), (out, ref[0])
        assert torch.equal(dl, ref[1]), float((dl - ref[1]).abs().max())


# ------------------------------------------------------------------ C. reconstruction / STFT
def stft_pair(B, T, D, gen):
    """x and y = 2 x + 0.01 noise: every bin's |X| - |Y| is about -|X|, so no sign(|X| - |Y|) of the STFT gradient is left
    to rounding.  (With y = x + 0.3 noise, 30 of the 2.56 M gradient elements at this size sit next to such a near tie and
    differ from float64 by the flipped term, in the kernels and in any fp32 evaluation alike.)"""
    xh = torch.randn(B, T, D, generator=gen)
    return xh, 2.0 * xh + 0.01 * torch.randn(B, T, D, generator=gen)


def _recon_groups(B, T, D, res):
    return [(B * (1 + T // hop) * D + 63) // 64 for _, hop, _ in res]


@pytest.mark.parametrize("res", [[(64, 64, 16), (128, 128, 32)], [(64, 19, 16)]], ids=["step", "groups2160"])
def test_recon_loss_at_the_benchmark_size(res, monkeypatch):
    """64 x 500 x 80 with a mask, fused and dense (cfg.recon_dense) against torch.stft in float64 (the tolerances of
    test_recon_loss_fused_vs_torch_and_dense_path).  (64, 19, 16) gives 27 frames and 2160 groups of 64 items: every
    workgroup of the capped grid runs two or three groups across the barriers of recon_stft_body's group loop."""
    from crank_amd import config, ops
    from tests.test_gpu_ops import _torch_recon

    B, T, D = 64, 500, 80
    groups = _recon_groups(B, T, D, res)
    assert ops.recon_supported(T, res)
    if len(res) == 1:
        assert groups == [2160] and groups[0] > 2 * LOSS_MAX_BLOCKS
    else:
        assert groups == [640, 320]
    gen = torch.Generator().manual_seed(21)
    xh, yh = stft_pair(B, T, D, gen)
    mh = torch.rand(B, T, generator=gen) > 0.2
    wts = (2.0, 0.5, 1.0)
    windows = [torch.hann_window(w, dtype=torch.float32, device="cuda") for _, _, w in res]

    def run(dense):
        monkeypatch.setattr(config.cfg, "recon_dense", bool(dense))
        leaf = xh.cuda().requires_grad_(True)
        vals = ops.recon_loss(leaf, yh.cuda(), mh.cuda(), res, windows, 0.0)
        sum(w * v for w, v in zip(wts, vals)).backward()
        return [v.item() for v in vals], leaf.grad.cpu().numpy()

    vf, gf = run(False)
    vd, gd = run(True)
    xr = xh.clone().double().requires_grad_(True)
    ref = _torch_recon(xr, yh, mh, res, 0.0)
    sum(w * v for w, v in zip(wts, ref)).backward()
    gr = xr.grad.numpy()
    np.testing.assert_allclose(vf, [v.item() for v in ref], rtol=3e-5)
    np.testing.assert_allclose(vf, vd, rtol=2e-6)
    np.testing.assert_allclose(gf, gr, rtol=2e-3, atol=3e-5 * np.abs(gr).max())
    np.testing.assert_allclose(gf, gd, rtol=2e-3, atol=2e-6 * np.abs(gr).max())
    a = run(False)
    assert a[0] == vf and np.array_equal(a[1], gf)


@pytest.mark.parametrize("sliced", [False, True])
def test_recon_fused_l1_mse_equal_masked_loss_both_bitwise(sliced):
    """The fused kernel's L1 / MSE run masked_sums, the loop of masked_loss_partial<4, 2> / <1, 2>: the same four
    values as crk_masked_loss_both_fwd on the same pair, bit for bit, on the 16-byte path and (row stride 83) the scalar
    one."""
    from crank_amd.ops import _iarr, _parr, _stft_tables

    B, T, D = 64, 500, 80
    res = [(64, 64, 16), (128, 128, 32)]
    gen = torch.Generator().manual_seed(4)
    xh = torch.randn(B * T, D, generator=gen)
    yh = xh + 0.3 * torch.randn(B * T, D, generator=gen)
    mask = make_mask("random", B * T, gen)
    x, y = (strided(xh, 83), strided(yh, 83)) if sliced else (xh.cuda(), yh.cuda())
    assert vec4_ok(D, x, y) == (not sliced)
    assert blocks(B * T * D // (1 if sliced else 4)) == LOSS_MAX_BLOCKS
    windows = [torch.hann_window(w, dtype=torch.float32, device="cuda") for _, _, w in res]
    tabs = _stft_tables(res, windows)
    ia = [_iarr([r[i] for r in res]) for i in range(3)]
    out5 = torch.empty(5, dtype=torch.float32, device="cuda")
    check(L().crk_recon_loss_fwd(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(mask), B, T, D, 2, ia[0], ia[1], ia[2],
                                 _parr(tabs), 0.0, ptr(out5), None, ptr(scratch()), stream_ptr()), "crk_recon_loss_fwd")
    both = ml_both(x, y, mask)
    assert torch.equal(out5[:4], both), (out5[:4], both)


def test_stft_losses_at_the_benchmark_size():
    """CustomFeatureLoss(loss_type="stft") with default.yml's stft_params at 64 x 500 x 80 (quirk Q1: 16- and 32-tap
    windows, the multi-resolution frame kernels, loss and gradient in one pass), and an 80-tap window on a 128-point
    frame (STFTLoss built directly: the single-resolution stft_loss_kernel with its atomics, 5.3 M (signal, frame, bin)
    items on the capped grid), against torch.stft in float64.  (default.yml's 128-point entries are n_fft and the
    effective hop; its windows have 16 and 32 taps, and the trainers never build a window above 64 taps.)"""
    from crank_amd.net.module.loss import CustomFeatureLoss, STFTLoss
    from crank_amd.utils import load_yaml
    from tests.test_gpu_ops import _torch_recon

    B, T, D = 64, 500, 80
    gen = torch.Generator().manual_seed(8)
    xh, yh = stft_pair(B, T, D, gen)
    sp = load_yaml(None)["stft_params"]
    crit = CustomFeatureLoss(loss_type="stft", stft_params=sp)
    res = crit.loss_func.resolutions
    assert res == [(64, 64, 16), (128, 128, 32)] and all(w <= 64 for _, _, w in res)
    direct = STFTLoss(fft_size=128, win_size=80, hop_size=32)
    assert direct.resolutions == [(128, 32, 80)]  # win > 64: not stft_multi_kernel; 2 * 65 * 80 twiddles fit in 60 KB of LDS
    assert B * D * (1 + T // 32) * 65 > LOSS_MAX_BLOCKS * 256
    for lossf, r, rtol_v in ((crit, res, 3e-5), (direct, direct.resolutions, 5e-5)):
        leaf = xh.cuda().requires_grad_(True)
        v = lossf(leaf, yh.cuda())
        (1.5 * v).backward()
        xr = xh.clone().double().requires_grad_(True)
        ref = _torch_recon(xr, yh, None, r, 0.0)[2]
        (1.5 * ref).backward()
        g, gr = leaf.grad.cpu().numpy(), xr.grad.numpy()
        np.testing.assert_allclose(v.item(), ref.item(), rtol=rtol_v)
        np.testing.assert_allclose(g, gr, rtol=2e-3, atol=5e-5 * np.abs(gr).max())


THREE_TILES = [(16, 5, 9), (32, 10, 20), (128, 70, 40)]  # (n_fft, hop, win) as torch.stft receives them
STFT_PATHS = {
    # name: (resolutions, passes)
    "three-tiles-one-pass": (THREE_TILES, 1),
    "three-tiles-two-pass": (THREE_TILES, 2),
    "five-resolutions": (THREE_TILES + [(16, 16, 16), (64, 19, 33)], 1),
    "mixed": ([(16, 5, 9), (128, 32, 80)], 1),
}


def _tile(win):
    return 16 if win <= 16 else 32 if win <= 32 else 64


@pytest.mark.parametrize("logratio", [0.0, 0.3])
@pytest.mark.parametrize("path", list(STFT_PATHS))
def test_stft_loss_paths_outside_the_step(path, logratio, monkeypatch):
    """The STFT-loss paths the training step never takes, at 2 x 130 x 3 against torch.stft in float64 (the bars of
    test_stft_losses_at_the_benchmark_size).  "three tiles": windows shorter than their 16-, 32- and 64-tap tiles in one
    launch (the 64-tap instantiation's dispatch), overlapping frames, both reflect edges, item counts that are no
    multiple of 8 and six workgroups for the first resolution - loss and gradient in one pass, and as two passes
    (cfg.stft_two_pass: the loss-only and the gradient-only modes), the two against each other at the fused-against-dense
    bars.  "five resolutions": more than LOSS_MAX_RES, so crk_stft_loss_fwd / _bwd run per resolution and accumulate.
    "mixed": a window above 64 taps sends the whole list there; the 9-tap resolution takes stft_multi_kernel with nres = 1, the
    80-tap one stft_loss_kernel, accumulated onto the first."""
    from crank_amd import config
    from crank_amd.net.module.loss import MultiSizeSTFTLoss
    from tests.test_gpu_ops import _torch_recon

    B, T, D = 2, 130, 3
    res, passes = STFT_PATHS[path]
    items = [B * (1 + T // hop) * D for _, hop, _ in res]
    multi = len(res) <= 4 and all(win <= 64 for _, _, win in res)  # _STFTLossFn's choice of the one-launch kernels
    if path.startswith("three-tiles"):
        assert multi and [_tile(w) for _, _, w in res] == [16, 32, 64] and all(w < _tile(w) for _, _, w in res)
        assert items == [162, 84, 12] and all(i % 8 for i in items) and blocks(items[0] * 8) == 6
        assert all(hop < win for _, hop, win in res[:2])  # overlapping frames: more than two atomics per sample
    elif path == "five-resolutions":
        assert len(res) > 4 and all(win <= 64 for _, _, win in res)
    else:
        assert len(res) <= 4 and any(win > 64 for _, _, win in res) and any(win <= 64 for _, _, win in res)
        assert not multi
    assert all(n_fft // 2 < T and win <= n_fft for n_fft, _, win in res) and T % 2 == 0
    gen = torch.Generator().manual_seed(31)
    xh, yh = stft_pair(B, T, D, gen)
    # MultiSizeSTFTLoss takes (fft, hop, win) lists in the reference's swapped order (quirk Q1)
    crit = MultiSizeSTFTLoss(fft_sizes=[r[0] for r in res], win_sizes=[r[1] for r in res], hop_sizes=[r[2] for r in res],
                             logratio=logratio)
    assert crit.resolutions == res

    def run(two_pass):
        monkeypatch.setattr(config.cfg, "stft_two_pass", bool(two_pass))
        leaf = xh.cuda().requires_grad_(True)
        v = crit(leaf, yh.cuda())
        (1.5 * v).backward()
        return v.item(), leaf.grad.cpu().numpy()

    xr = xh.clone().double().requires_grad_(True)
    ref = _torch_recon(xr, yh, None, res, logratio)[2]
    (1.5 * ref).backward()
    gr = xr.grad.numpy()
    v, g = run(passes == 2)
    np.testing.assert_allclose(v, ref.item(), rtol=5e-5)
    np.testing.assert_allclose(g, gr, rtol=2e-3, atol=5e-5 * np.abs(gr).max())
    if passes == 2:
        v1, g1 = run(False)
        np.testing.assert_allclose(v1, v, rtol=2e-6)
        np.testing.assert_allclose(g1, g, rtol=2e-3, atol=2e-6 * np.abs(gr).max())


# ------------------------------------------------------------------ D. speaker embedding
def emb_plan(E, n_rows):
    """crk_embed_bwd_run's host plan: (frame lanes per column, rows per window, windows)."""
    wrows = min(n_rows, EMB_LDS // (4 * E))
    nsub = min(256 // E, EMB_LDS // (4 * E * wrows))
    return nsub, wrows, -(-n_rows // wrows)


EMB_SHAPES = [(32, 14), (32, 60), (32, 61), (32, 100), (32, 1024), (1, 3), (3, 7), (100, 5), (256, 60), (256, 61)]


def test_embedding_plans_reach_their_edges():
    """Which of the shapes keeps 256 / E frame lanes (every shape the library took before), which needs fewer, and which
    needs row windows."""
    plans = {s: emb_plan(*s) for s in EMB_SHAPES}
    for (E, rows), (nsub, wrows, nwin) in plans.items():
        assert nsub >= 1 and nsub * wrows * E * 4 <= EMB_LDS
        old_fit = (256 // E) * rows * E * 4 <= EMB_LDS  # the only shapes accepted before
        assert (nsub == 256 // E and nwin == 1) == old_fit, (E, rows)
    assert plans[(32, 60)] == (8, 60, 1) and plans[(32, 61)] == (7, 61, 1) and plans[(32, 100)] == (4, 100, 1)
    assert plans[(256, 60)] == (1, 60, 1) and plans[(256, 61)] == (1, 60, 2) and plans[(32, 1024)] == (1, 480, 3)


def _emb_inputs(E, n_rows, N, run, seed):
    """dcat with the embedding at column c0 of rows wider than the concatenation, labels (run = T: one per utterance, read
    at n - n % T) with and without -100 pads, and a non-zero starting table gradient."""
    gen = torch.Generator().manual_seed(seed)
    c0 = 2 + seed % 3
    ld = c0 + E + 3
    dcat = torch.randn(N, ld, generator=gen)
    if run == 1:
        lab = torch.randint(0, n_rows, (N,), generator=gen)
    else:
        lab = torch.randint(0, n_rows, (N // run, 1), generator=gen).expand(-1, run).reshape(-1)
    if run == 1:  # the first and the last row of the table
        lab[: min(2, N)] = torch.tensor([0, n_rows - 1])[: min(2, N)]
    padded = lab.clone()
    pad = torch.rand(N, generator=gen) < 0.15
    if run > 1:
        pad = pad.view(-1, run)[:, :1].expand(-1, run).reshape(-1)
    padded[pad] = -100
    table = torch.randn(n_rows, E, generator=gen)
    dt0 = torch.randn(n_rows, E, generator=gen)
    return c0, ld, dcat, lab, padded, table, dt0


@pytest.mark.parametrize("E,n_rows", EMB_SHAPES)
def test_speaker_embedding_gather_and_table_gradient(E, n_rows):
    """crk_concat_embed_run: bitwise table[idx] (plus the concatenated sources); crk_embed_bwd_run: the table gradient
    within 1e-5 of a float64 index_add, scaled per element by the float64 sum of absolute contributions and the starting
    value (the reduction adds to what dtable held), identical bits from two calls.  N = 1 / 255 / 257 / 32 000 frames and one
    not a multiple of 8 nsub; run = T (stride-0 labels) at 64 x 500; -100 pads only in the backward."""
    nsub, wrows, nwin = emb_plan(E, n_rows)
    odd = 8 * nsub * 37 + 5
    cases = [(1, 1), (255, 1), (257, 1), (32000, 1), (odd, 1), (32000, 500)]
    assert odd % (8 * nsub) and -(-32000 // EMB_FRAMES) == 125  # 125 partial tables: the 32- and 8-wide loops and the tail
    for k, (N, run) in enumerate(cases):
        c0, ld, dcat, lab, padded, table, dt0 = _emb_inputs(E, n_rows, N, run, 1000 * E + n_rows + k)
        dc, tb = dcat.cuda(), table.cuda()
        ik = lab.cuda().contiguous()
        # the gather, with the embedding behind a 2-column source at c0 = 2 of a wider row
        a = torch.randn(N, ld, generator=torch.Generator().manual_seed(k)).cuda()
        out = torch.full((N, 2 + E + 1), 7.0, device="cuda")
        check(L().crk_concat_embed_run(ptr(a), ld, 2, None, 0, 0, ptr(tb), E, ptr(ik), run, N, ptr(out), 2 + E + 1,
                                       stream_ptr()), "crk_concat_embed_run")
        want = torch.cat([a[:, :2], tb[lab.cuda()]], 1)
        assert torch.equal(out[:, : 2 + E], want), (E, n_rows, N, run)
        assert torch.equal(out[:, 2 + E], torch.full((N,), 7.0, device="cuda"))
        # the table gradient
        ip = padded.cuda().contiguous()
        scr = torch.empty(L().crk_embed_bwd_scratch_floats(N, E, n_rows), dtype=torch.float32, device="cuda")

        def bwd():
            dt = dt0.cuda()
            check(L().crk_embed_bwd_run(ptr(dc), ld, c0, E, ptr(ip), run, N, n_rows, ptr(dt), ptr(scr), stream_ptr()),
                  "crk_embed_bwd_run")
            return dt

        got, again = bwd(), bwd()
        assert torch.equal(got, again), (E, n_rows, N, run)
        keep = padded != -100
        contrib = dcat[:, c0: c0 + E].double()[keep]
        ref = dt0.double().index_add(0, padded[keep], contrib)
        scale = dt0.double().abs().index_add(0, padded[keep], contrib.abs())
        err = (got.cpu().double() - ref).abs()
        assert bool((err <= 1e-5 * scale + 1e-30).all()), (E, n_rows, N, run, float((err / scale.clamp_min(1e-30)).max()))
