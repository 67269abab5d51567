"""The per-layer conv kernels (conv_tile_kernel<MODE_PLAIN | MODE_RESFWD | MODE_BWDA>, the table weight-gradient kernel)
at configurations that route to them ON THEIR OWN - no process switch: stacks the fused planners refuse because a tap
offset, the halo or the conditioning width is beyond what their windows hold.  Every case first pins the route it got (the
library's launch recorder), then goes through the same oracle comparisons, at the same tolerances, as the fused kernels
do in test_gpu_nets.py.

B = 2, T = 150 everywhere but the length edges: one full 128-frame conv tile plus a 22-frame tail that is shorter than the
32-frame halo of the dilation-16 / 32 convs (the tail tile reads back across the tile boundary and past the utterance's
end), three 64-frame weight-gradient chunks with a ragged last one, and a second utterance that a leaking halo would reach.

| case       | in, out, k, layers, stacks, aux | what the fused planners refuse                         | bf16      | bf16x3    |
| dil16_k5   | 80, 64, 5, 5, 1, 0              | tap offset 32 > the 16 guard rows                      | per-layer | per-layer |
| dil32_k3   | 64, 64, 3, 6, 1, 0              | tap offset 32; tap span 64 > the weight gradient's 32  | per-layer | per-layer |
| halo240    | 80, 64, 5, 16, 4, 0             | halo 240 > 256 - 32 (16 blocks: the deepest table)     | per-layer | per-layer |
| onehot100  | 128, 80, 5, 8, 4, 102           | conditioning wider than 64 (100 speakers one-hot + f0) | per-layer | refused   |
| aux65/128  | 128, 80, 5, 8, 4, 65 / 128      | the same, at its two edges                             | per-layer | refused   |
| aux64      | 128, 80, 5, 8, 4, 64            | nothing: the last width that stays fused (control)     | fused     | fused     |
| mixed_8x2  | 80, 64, 5, 8, 2, 0              | halo 120 > 128 - 32 in the split-operand window only   | fused     | per-layer |
| mixed_12x4 | 64, 64, 5, 12, 4, 0             | halo 112, the same                                     | fused     | per-layer |
| disc_dil16 | kind 1: 37, 1, 5, 5, 1          | as dil16_k5 (dropout 0 and 0.25)                       | per-layer | per-layer |

"refused": with hi + lo operand planes the gated per-layer kernel's tiles of a conditioning chunk wider than 64 channels
do not fit the 160 KB of LDS (pwg.py per_layer_gated_lds_bytes), so such a stack runs in plain bf16 only and says so when
it is called in another arithmetic (HipStack.__call__)."""
import ctypes

import pytest
import torch

from tests.helpers import fill_models
from tests.test_gpu_nets import _check_split_forward, _check_standalone, _generator_stack_case, _GenStack

pytestmark = pytest.mark.gpu

B, T = 2, 150


def _gen(cin, cout, k, layers, stacks, aux):
    return dict(in_channels=cin, out_channels=cout, kernel_size=k, layers=layers, stacks=stacks, aux_channels=aux)


GEN = {
    "dil16_k5": _gen(80, 64, 5, 5, 1, 0),
    "dil32_k3": _gen(64, 64, 3, 6, 1, 0),
    "halo240": _gen(80, 64, 5, 16, 4, 0),
    "onehot100": _gen(128, 80, 5, 8, 4, 102),
    "aux65": _gen(128, 80, 5, 8, 4, 65),
    "aux128": _gen(128, 80, 5, 8, 4, 128),
    "aux64": _gen(128, 80, 5, 8, 4, 64),
    "mixed_8x2": _gen(80, 64, 5, 8, 2, 0),
    "mixed_12x4": _gen(64, 64, 5, 12, 4, 0),
}
DISC = dict(in_channels=37, out_channels=1, kernel_size=5, layers=5, stacks=1)
# the kernel family of a case in (plain bf16, bf16x3); None: refused (see the module docstring)
ROUTE = {
    "dil16_k5": ("per-layer", "per-layer"),
    "dil32_k3": ("per-layer", "per-layer"),
    "halo240": ("per-layer", "per-layer"),
    "onehot100": ("per-layer", None),
    "aux65": ("per-layer", None),
    "aux128": ("per-layer", None),
    "aux64": ("fused", "fused"),
    "mixed_8x2": ("fused", "per-layer"),
    "mixed_12x4": ("fused", "per-layer"),
    "disc_dil16": ("per-layer", "per-layer"),
}
_PREC = ("bf16", "bf16x3")
PER_LAYER = [(c, p) for c in ROUTE for i, p in enumerate(_PREC) if ROUTE[c][i] == "per-layer"]
REFUSED = [(c, p) for c in ROUTE for i, p in enumerate(_PREC) if ROUTE[c][i] is None]


def _models(case, dropout=0.0):
    """(HIP model, oracle, input channels, conditioning channels) of a case."""
    from crank_amd.net.module.pwg import ResidualParallelWaveGANDiscriminator
    from oracle import pwg

    if case == "disc_dil16":
        return (ResidualParallelWaveGANDiscriminator(**DISC, dropout=dropout),
                pwg.ResidualParallelWaveGANDiscriminator(**DISC, dropout=0.0), DISC["in_channels"], 0)
    cfg = GEN[case]
    return (_GenStack(**cfg), pwg.ParallelWaveGANGenerator(**cfg, upsample_conditional_features=False), cfg["in_channels"],
            cfg["aux_channels"])


def _report():
    from crank_amd import _lib

    L = _lib.lib()
    out = {}
    for cls in range(7):
        cnt, ms, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        assert L.crk_prof_report(cls, ctypes.byref(cnt), ctypes.byref(ms), ctypes.byref(fl)) == 0
        if cnt.value:
            out[cls] = cnt.value
    return out


def _launches(prod, cin, aux, precision):
    """{launch class: count} of ONE forward and of ONE backward of `prod` at (B, T) in `precision`, from the library's launch
    recorder (classes: 0 conv_tile_kernel, 1 gated forward, 2 gated data-gradient chain, 3 table weight gradient, 4 plain
    chains, 5 gated weight gradient, 6 plain-conv weight gradient)."""
    from crank_amd import _lib, ops

    L = _lib.lib()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, cin, T, generator=g).cuda().requires_grad_(True)
    c = torch.randn(B, aux, T, generator=g).cuda().requires_grad_(True) if aux else None
    ops.set_precision(precision)
    try:
        prod.zero_grad()
        L.crk_prof_enable(1)
        y = prod(x, c) if aux else prod(x)
        fwd = _report()
        L.crk_prof_enable(1)
        y.sum().backward()
        bwd = _report()
    finally:
        L.crk_prof_enable(0)
        ops.set_precision("bf16")
    torch.cuda.synchronize()
    return fwd, bwd


def _family(fwd, bwd):
    """("per-layer" | "fused" | "mixed") of the forward and of the backward."""
    def one(n, per_layer, fused):
        if all(n.get(k, 0) > 0 for k in per_layer) and not any(n.get(k, 0) for k in fused):
            return "per-layer"
        if any(n.get(k, 0) for k in fused) and not any(n.get(k, 0) for k in per_layer):
            return "fused"
        return "mixed"

    return one(fwd, (0,), (1, 4)), one(bwd, (0, 3), (2, 4, 5, 6))


@pytest.mark.parametrize("precision", _PREC)
@pytest.mark.parametrize("case", [c for c in ROUTE])
def test_route(case, precision):
    """What one forward and one backward launch: a per-layer case conv_tile_kernel in both directions, the table weight
    gradient once and no fused chain; a fused case the reverse; a refused case says why."""
    want = ROUTE[case][_PREC.index(precision)]
    prod, _, cin, aux = _models(case)
    if want is None:
        with pytest.raises(NotImplementedError, match="conditioning channels: .* plain bf16 only"):
            _launches(prod, cin, aux, precision)
        return
    fwd, bwd = _launches(prod, cin, aux, precision)
    print(f"[route {case} {precision}] forward {fwd} backward {bwd}")
    assert _family(fwd, bwd) == (want, want), (case, precision, fwd, bwd)
    if want == "per-layer":
        assert bwd.get(3) == 1 and not fwd.get(4) and not bwd.get(4), (fwd, bwd)
    else:
        assert not fwd.get(0) and not bwd.get(0) and not bwd.get(3), (fwd, bwd)


@pytest.mark.parametrize("case,precision", PER_LAYER + [("mixed_8x2", "bf16"), ("mixed_12x4", "bf16")])
def test_parity(case, precision):
    """y, dx, dc and every parameter gradient against the oracle, as test_generator_stack / test_residual_discriminator:
    bf16x3 within TOL["bf16x3"] of the fp32 oracle, bf16 as close to the float64-accumulated bf16 emulation as three times
    the CPU fp32 evaluations' own error.  (mixed_* in bf16: the fused 8-wave window at a halo of 120 / 112 frames.)"""
    if case == "disc_dil16":
        prod, orac, cin, _ = _models(case)
        _check_standalone(prod, orac, cin, B=B, T=T, precision=precision)
    else:
        _generator_stack_case(GEN[case], T, precision, B=B)


@pytest.mark.parametrize("Tn", [1, 31, 128, 129])
def test_length_edges(Tn):
    """dil16_k5 below one tap offset, below the receptive field (125), at exactly one tile and one frame past it."""
    _generator_stack_case(GEN["dil16_k5"], Tn, "bf16x3", B=B)


@pytest.mark.parametrize("case", ["mixed_8x2", "mixed_12x4"])
def test_split_forward_and_plain_backward_take_one_kernel_family(case):
    """bf16x3f on a stack whose two arithmetics disagree about the fused kernels: the split-operand forward (which reads the
    bf16x3 route) and the plain backward (which reads the bf16 route) must run the same family - the per-layer forward
    writes fp32 planes only, the fused backward reads bf16 planes - and then meet _check_split_forward's bars."""
    from oracle import pwg

    cfg = GEN[case]
    prod = _GenStack(**cfg)
    fwd, bwd = _launches(prod, cfg["in_channels"], 0, "bf16x3f")
    print(f"[route {case} bf16x3f] forward {fwd} backward {bwd}")
    fam = _family(fwd, bwd)
    assert fam[0] == fam[1] and fam[0] != "mixed", (fam, fwd, bwd)
    orac = pwg.ParallelWaveGANGenerator(**cfg, upsample_conditional_features=False)
    _check_split_forward(prod, orac, cfg["in_channels"], 0, B, T, f"gated {cfg['kernel_size']}x{cfg['layers']} {case}",
                         orac_call=lambda x: orac(x, None))


def _fd_discrepancy(prod, x, v, eps, seed):
    """|central difference - <dx, v>| / max(1, |<dx, v>|) of sum(prod(x)) along v, the dropout mask pinned by `seed`."""
    def run(inp):
        if seed is not None:
            prod.stack.net.reseed(seed)
        return prod(inp)

    xb = x.detach().clone().requires_grad_(True)
    gb, = torch.autograd.grad(run(xb).sum(), xb)
    fd = ((run(x.detach() + eps * v).double().sum() - run(x.detach() - eps * v).double().sum()) / (2 * eps)).item()
    an = (gb.double() * v.double()).sum().item()
    return abs(fd - an) / max(1.0, abs(an)), fd, an


def test_dropout_mask_is_one_mask_in_every_per_layer_kernel():
    """disc_dil16 with dropout 0.25 (load_src's dropout branch in the forward, the epilogue's in the data gradient, the
    weight-gradient kernel's): the identities of test_dropout_mask_is_consistent_between_forward_and_backward.  The bound
    of the directional derivative is measured, not fixed: the same net, x, v and eps with dropout 0.0 - whose gradients
    test_parity has validated - gives the discrepancy the LeakyReLU / gate curvature alone causes, and the dropout run may
    be twice that.  The direction is the dropout net's own input gradient, scaled to unit rms like a random one: along a
    random direction the derivative of this net nearly cancels (-0.17 against 1440 here) and any bound relative to
    max(1, |derivative|) passes whatever the mask.
    Measured on MI355X (eps 2e-3; profiles/per_layer_tests.txt): dropout 0.0 finite difference 457.920 against 458.659,
    discrepancy 1.61e-3; dropout 0.25 1445.854 against 1449.357, 2.42e-3, bound 3.22e-3; with the analytic side taken
    under another seed's mask (measured apart) 317.2 against 1436.8, a discrepancy of 3.5."""
    from crank_amd import ops

    ops.set_precision("bf16x3")
    try:
        prod = _models("disc_dil16", dropout=0.25)[0]
        plain = _models("disc_dil16", dropout=0.0)[0]
        fill_models({"D": prod})
        fill_models({"D": plain})
        g = torch.Generator().manual_seed(0)
        x = torch.randn(B, DISC["in_channels"], T, generator=g).cuda().requires_grad_(True)
        eps = 2e-3
        y = prod(x)
        g1, = torch.autograd.grad(y.sum(), x, retain_graph=True)
        g2, = torch.autograd.grad(y.sum(), x)
        assert torch.isfinite(y).all() and torch.isfinite(g1).all()
        assert torch.equal(g1, g2)
        y2 = prod(x)  # new seed -> different mask
        assert (y - y2).abs().max().item() > 0
        prod.stack.net.reseed(7)
        ya = prod(x.detach())
        prod.stack.net.reseed(7)
        yb = prod(x.detach())
        assert torch.equal(ya, yb)
        prod.stack.net.reseed(7)
        v, = torch.autograd.grad(prod(x).sum(), x)
        v = v / v.norm() * v.numel() ** 0.5
        base, fd0, an0 = _fd_discrepancy(plain, x, v, eps, None)
        drop, fd1, an1 = _fd_discrepancy(prod, x, v, eps, 7)
        print(f"[dropout disc_dil16] directional derivative: dropout 0.0 fd {fd0:.6f} analytic {an0:.6f} discrepancy {base:.3e}; "
              f"dropout 0.25 fd {fd1:.6f} analytic {an1:.6f} discrepancy {drop:.3e} (bound {2 * base:.3e})")
        assert drop <= 2 * base, (drop, base)
    finally:
        ops.set_precision("bf16")


@pytest.mark.parametrize("case,precision", REFUSED)
def test_refused(case, precision):
    """A conditioning chunk wider than 64 channels in split-operand arithmetic: refused with its reason, in bf16x3 and in
    bf16x3f, by the stack itself: the library is not called."""
    from crank_amd import ops

    prod, _, cin, aux = _models(case)
    x, c = torch.zeros(B, cin, T, device="cuda"), torch.zeros(B, aux, T, device="cuda")
    for mode in (precision, "bf16x3f"):
        ops.set_precision(mode)
        try:
            with pytest.raises(NotImplementedError, match="conditioning channels: .* plain bf16 only"):
                prod(x, c)
        finally:
            ops.set_precision("bf16")
