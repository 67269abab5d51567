"""GPU parity UNDER DROPOUT: every stack kernel that regenerates the keep mask (frame-split and channel-split forward and
data-gradient chain, the per-layer load / epilogue, the gated and the table weight gradient, the saved dropped plane)
against the oracle evaluated under the very mask the kernels draw (tests/dropout_ref.py restates the integer hash).

The comparisons are the dropout-free ones of test_gpu_nets.py (_check_standalone, _check_split_forward, the exact pin),
at their tolerances; tests/test_dropout_cpu.py shows on the CPU that a mask shifted by a layer or a lane, a keep scale of
1 / p, a weight gradient on the undropped input, or (exact pin) ONE flipped mask element exceeds these bounds more than
tenfold.  Cases and shapes: tests/dropout_cases.py.  Every case first asserts the route it got, then compares.

Measured on MI355X (profiles/dropout_pin_tests.txt, beside the dropout-free tests of the same session): bf16x3 1.1e-5 ...
2.7e-5 of scale (bound 2e-4); plain bf16 0.8 ... 2.7 x the CPU fp32 evaluations' own error (bound 3 x); the p = 0.5 pin cases
bit-identical in y and dx, parameter gradients <= 1.7e-4 of scale (bound 3e-4).  Their first run found two stacks the
channel-split forward's plan accepted without having a kernel for them (k = 3 with dropout: no mask in the forward, y off
by 0.57 relative L2; conditioning with dropout: refused at launch) - profiles/dropout_before_plan_fix.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dropout_cases as C
from tests import dropout_ref as R
from tests.helpers import REPO
from tests.test_gpu_nets import (_check_split_forward, _check_standalone, _compare_standalone, _load_same, _pin_metrics, _pin_oracle)
from tests.test_gpu_per_layer import _family, _report

pytestmark = pytest.mark.gpu


def _pin_seed(prod, v):
    """reseed(v), read the seed the next forward will draw, and hand back the hook that restarts the sequence in front
    of that forward."""
    net = prod.stack.net
    net.reseed(v)
    seed = int(net.next_seed().item())
    assert seed == C.first_seed(v), (seed, C.first_seed(v))
    net.reseed(v)
    return seed, (lambda: net.reseed(v))


def _route(prod, cfg, T, precision, want):
    """Assert (and print) the kernel family ONE forward and ONE backward of `prod` launch at (B, T): the library's launch
    recorder (classes: test_gpu_per_layer._launches) and crk_debug_net_paths."""
    from crank_amd import _lib, ops

    L = _lib.lib()
    aux = C.aux_of(cfg)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(C.B, cfg["in_channels"], T, generator=g).cuda().requires_grad_(True)
    c = torch.randn(C.B, aux, T, generator=g).cuda() if aux else None
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
    prod.zero_grad()
    paths = L.crk_debug_net_paths(prod.stack.net.handle, C.B, T)
    fam = _family(fwd, bwd)
    print(f"[route {precision} T={T} want {want}] paths {paths} family {fam} forward {fwd} backward {bwd}")
    if want == "per-layer":
        assert fam == ("per-layer", "per-layer") and bwd.get(3) == 1, (fam, fwd, bwd)
        return paths
    assert fam == ("fused", "fused") and not bwd.get(3), (fam, fwd, bwd)
    if want == "split":  # channel-split discriminator: forward + chain, saved dropped plane, gated weight gradient
        assert paths & 4, paths
        assert (fwd.get(1), fwd.get(4)) == (1, 2) and [bwd.get(k) for k in (2, 5, 6, 4)] == [1, 1, 1, 2], (fwd, bwd)
    elif want == "frame-gen":  # a generator-kind stack with dropout never takes the channel-split kernels
        assert paths == 0, paths
    elif want == "frame-disc":
        assert not paths & 4, paths
    return paths


def test_seed_sequence_is_the_restated_one():
    from crank_amd import ops

    net = ops.HipNet(kind=1, in_ch=16, out_ch=1, kernel_size=5, layers=2, stacks=1, res_ch=64, gate_ch=128, skip_ch=64, aux_ch=0,
                     conv_ch=64, causal=0, use_bias=1, slope=0.2, dropout=0.25)
    net.reseed(1001)
    got = [int(net.next_seed().item()) for _ in range(3)]
    print("[seed sequence after reseed(1001)]", got)
    assert got == R.seed_sequence(1001, 3)


@pytest.mark.parametrize("name", list(C.PARITY))
def test_parity_under_the_kernels_own_mask(name):
    """y, dx, dc and every parameter gradient at p = 0.25 (generator kind: 0.1) against the masked oracle, through
    _check_standalone / _check_split_forward at their dropout-free tolerances."""
    kind, cfg, p, T, precision, v, route = C.PARITY[name]
    if precision != "bf16x3f":
        v = C.parity_reference(name)[0]  # (chosen from the CPU emulations alone: see there)
    prod, orac = C.product_of(kind, cfg, p), C.oracle_of(kind, cfg, p)
    want = {"frame": "frame-gen" if kind == "gen" else None}.get(route, route)
    _route(prod, cfg, T, precision, want)
    seed, pre_run = _pin_seed(prod, v)
    masks = C.masks_of(seed, cfg, T, p)
    ctx = lambda: R.masked(orac, masks, p=p)  # noqa: E731
    aux = C.aux_of(cfg)
    print(f"[dropout parity {name}] p {p} reseed {v} seed {seed}")
    if precision == "bf16x3f":
        _check_split_forward(prod, orac, cfg["in_channels"], aux, C.B, T, f"dropout {name}", mask_ctx=ctx, pre_run=pre_run)
    elif aux:
        _check_standalone(prod, orac, cfg["in_channels"], B=C.B, T=T, precision=precision, aux_ch=aux,
                          prod_call=lambda x, c: prod(x, c), mask_ctx=ctx, pre_run=pre_run)
    else:
        _check_standalone(prod, orac, cfg["in_channels"], B=C.B, T=T, precision=precision, mask_ctx=ctx, pre_run=pre_run)


# ---- the lsgan D under process switches ------------------------------------------------------------------------------------
_SWITCHES = {"CRK_SK_V=1": "frame-disc", "CRK_DISC_SPLIT=0": "frame-disc", "CRK_NO_FUSE=1": "per-layer"}
_SWITCH_V = 1011


def _run(prod, x, c, dy, keys):
    xp = x.cuda().requires_grad_(True)
    cp = c.cuda().requires_grad_(True) if c is not None else None
    prod.zero_grad()
    yp = prod(xp, cp) if c is not None else prod(xp)
    (yp * dy.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {"y": yp.detach(), "dx": xp.grad}
    if c is not None:
        got["dc"] = cp.grad
    for k in keys:
        if k not in got:
            got[k] = prod.grad_view(k[1:])
    return {k: got[k].detach().cpu().clone() for k in keys}


def _switch_child(path_in, path_out, want, v):
    """In a fresh process (the switches are read once): the lsgan D with dropout on inputs from `path_in`, route asserted,
    tensors dumped to `path_out`."""
    from crank_amd import ops

    kind, cfg, p, T, _, _, _ = C.PARITY["lsgan_bf16"]
    inp = np.load(path_in)
    prod, orac = C.product_of(kind, cfg, p), C.oracle_of(kind, cfg, p)
    ops.set_precision("bf16")
    _load_same(prod, orac)
    paths = _route(prod, cfg, T, "bf16", want)
    seed, pre_run = _pin_seed(prod, v)
    pre_run()
    keys = [str(k) for k in inp["keys"]]
    got = _run(prod, torch.from_numpy(inp["x"]), None, torch.from_numpy(inp["dy"]), keys)
    np.savez(path_out, paths=paths, seed=np.uint64(seed), **{k: v.numpy() for k, v in got.items()})


@pytest.mark.parametrize("switch", list(_SWITCHES))
def test_lsgan_discriminator_parity_under_a_process_switch(switch, tmp_path):
    """The older kernel generations a switch routes the lsgan D to draw the same mask: one fresh child per switch (one after
    another, each with a timeout) runs forward and backward and dumps its tensors; compared here as _check_standalone does."""
    kind, cfg, p, T, _, _, _ = C.PARITY["lsgan_bf16"]
    v, _, _, (x, c, dy, ref, e32, e32p, margin) = C.parity_reference("lsgan_bf16", _SWITCH_V)
    pin, pout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(pin, x=x.numpy(), dy=dy.numpy(), keys=np.array(list(ref)))
    var, val = switch.split("=")
    code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_dropout import _switch_child; _switch_child(%r, %r, %r, %d)"
            % (REPO, pin, pout, _SWITCHES[switch], v))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{var: val}), capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(pout)
    assert int(out["seed"]) == C.first_seed(v)
    got = {k: torch.from_numpy(out[k]) for k in ref}
    _compare_standalone(f"lsgan D @{switch} paths {int(out['paths'])}", got, ref, e32, e32p, margin, "bf16", C.B, T)


# ---- the exact pin at p = 0.5 ------------------------------------------------------------------------------------------------
def _pin_models(name, n_seeds=1):
    from crank_amd import ops

    kind, cfg, _ = C.PIN[name]
    v, ulps, where = C.pin_reseed(name, n_seeds)  # (chosen from the CPU emulation alone: see there)
    print(f"[dropout pin {name}] reseed {v}: every gate output >= {ulps} fp32 ulps from a bf16 rounding boundary "
          f"(closest: block, utterance, frame {where})")
    ops.set_precision("bf16")
    orac, cfg, vals = C.pin_oracle(name)
    prod = C.product_of(kind, cfg, C.PIN_P, C.PIN_SLOPE)
    prod.load_state_dict({k: torch.from_numpy(vals[k]) for k in orac.state_dict()})
    return kind, cfg, v, prod, orac


def _pin_check(tag, got, ref):
    bad, worst = {}, ("", 0.0)
    for k in ref:
        m = _pin_metrics(got[k], ref[k])
        if m["max"] > worst[1]:
            worst = (k, m["max"])
        if not C.pin_ok(k, m):
            bad[k] = m
    my, mx = _pin_metrics(got["y"], ref["y"]), _pin_metrics(got["dx"], ref["dx"])
    ey = (got["y"].detach().cpu().double() - ref["y"].double()).abs().amax(dim=1)
    if float(ey.max()) > 0:
        print(f"[dropout pin {tag}] y differs in {int((ey > 0).sum())} frames, most at (utterance, frame) "
              f"{divmod(int(ey.argmax()), ey.shape[1])}")
    print(f"[dropout pin {tag}] y max {my['max']:.1e} rl2 {my['rl2']:.1e} frac>2e-5 {my['frac>2e-5']:.1e}; dx max {mx['max']:.1e} "
          f"rl2 {mx['rl2']:.1e} frac>2e-5 {mx['frac>2e-5']:.1e}; worst max-norm {worst[0]} {worst[1]:.1e} "
          f"(bounds: activations 2e-5 on 98 %, rl2 5e-5, 2e-3 everywhere; parameters 3e-4, rl2 1e-4)")
    assert not bad, bad


@pytest.mark.parametrize("name", list(C.PIN))
def test_bf16_exact_pin_with_dropout_one_half(name):
    """Plain bf16, p = 0.5 (scale 2.0 adds no rounding), exactly representable operands: against the float64-accumulated
    masked emulation at the fixed bounds of test_bf16_single_layer_deterministic_pin.  One flipped mask element breaks the
    2e-3 "everywhere" bound more than tenfold (test_dropout_cpu.py): this is the bit-level check of the mask."""
    kind, cfg, v, prod, orac = _pin_models(name)
    _route(prod, cfg, C.PIN_T, "bf16", "split" if kind == "disc" else "frame-gen")
    seed, pre_run = _pin_seed(prod, v)
    masks = C.masks_of(seed, cfg, C.PIN_T, C.PIN_P)
    x, c, dy = C.pin_inputs(cfg)
    with R.masked(orac, masks, p=C.PIN_P):
        ref = _pin_oracle(orac, C.pin_call, x, c, dy, "fp64")
    pre_run()
    _pin_check(name, _run(prod, x, c, dy, list(ref)), ref)


# ---- one mask across calls -------------------------------------------------------------------------------------------------
def test_each_forward_draws_the_next_seed_and_a_late_backward_keeps_its_own():
    """Two forwards after one reseed match the masked emulation under the first and the second seed of the sequence; the
    backward of the FIRST forward, run after the second, still regenerates the first seed's mask.  The exact residual-D case
    on the channel-split kernels, at the pin's bounds."""
    name = "residual_d_two_blocks"
    kind, cfg, v, prod, orac = _pin_models(name, 2)
    _route(prod, cfg, C.PIN_T, "bf16", "split")
    s1, s2 = R.seed_sequence(v, 2)
    x, c, dy = C.pin_inputs(cfg)
    refs = []
    for s in (s1, s2):
        with R.masked(orac, C.masks_of(s, cfg, C.PIN_T, C.PIN_P), p=C.PIN_P):
            refs.append(_pin_oracle(orac, C.pin_call, x, c, dy, "fp64"))
    assert not torch.equal(refs[0]["y"], refs[1]["y"])
    prod.stack.net.reseed(v)
    prod.zero_grad()
    xa = x.cuda().requires_grad_(True)
    xb = x.cuda().requires_grad_(True)
    ya = prod(xa)
    yb = prod(xb)
    (ya * dy.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {"y": ya.detach(), "dx": xa.grad}
    for k in refs[0]:
        if k not in got:
            got[k] = prod.grad_view(k[1:])
    _pin_check(name + " first forward, backward after the second forward", got, refs[0])
    m = _pin_metrics(yb.detach(), refs[1]["y"])
    cross = _pin_metrics(yb.detach(), refs[0]["y"])
    print(f"[dropout pin {name} second forward] y max {m['max']:.1e} rl2 {m['rl2']:.1e} frac>2e-5 {m['frac>2e-5']:.1e} "
          f"(against the first seed's emulation: max {cross['max']:.1e}; bounds 2e-5 on 98 %, 2e-3 everywhere)")
    # The second forward has no backward behind it and its bounds are the pin's two that do not move with the NUMBER of gate
    # outputs the hardware's exp / rcp round the other way (each moves one frame by a bf16 ulp: <= 2e-3 of scale, and 2 % of
    # the entries is six whole frames); the relative-L2 bound stays with the first forward.  Under the first seed's mask y is
    # off by O(1) of scale on most entries.
    assert m["frac>2e-5"] <= 2e-2 and m["max"] <= 2e-3, m
    assert cross["max"] > 0.1 and cross["frac>2e-5"] > 0.5, cross
