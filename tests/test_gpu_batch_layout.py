"""The conv stacks at the batch layouts the benchmark runs: weight-gradient groups that walk several 64-frame chunks, begin
and end inside utterances, and the data-gradient chain's 192-row window (ft = 3).

Every case first asserts crk_debug_net_layout == tests/net_layout.py == the edge it is named after (test_net_layout_cpu.py
pins the restatement), so a plan that changes later fails a precondition instead of silently testing another layout.

Part 1 (test_oracle_*): the oracle comparisons of test_gpu_nets.py, criteria unchanged, at the smallest shapes that reach
those layouts.  Part 2 (test_benchmark_shape_*): the step's six nets at the benchmark's shapes against the same utterances
run two at a time and one at a time - layouts in which every chunk of the generic region is its own group and no group of
the gated region holds more than one utterance, which are the layouts the oracle tests pin."""
import ctypes

import pytest
import torch

from tests import net_layout as nl
from tests.net_layout import NETS, ORACLE_CASES
from tests.test_gpu_nets import _check_split_forward, _check_standalone, _generator_stack_case, _GenStack, _load_same

pytestmark = pytest.mark.gpu

_PLAIN_KW = dict(conv_channels=64, dilation_factor=1, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, bias=True, use_weight_norm=True)


def _cfg(name):
    net = NETS[name]
    keys = {"generator": ("in_channels", "out_channels", "kernel_size", "layers", "stacks", "aux_channels"),
            "discriminator": ("in_channels", "out_channels", "kernel_size", "layers", "stacks"),
            "plain": ("in_channels", "out_channels", "kernel_size", "layers")}[net["kind"]]
    return {k: net[k] for k in keys}


def _build(name):
    """(HIP model, oracle module) of one of the step's nets; both take (B, C, T) and, dec0, the conditioning."""
    from crank_amd.net.module.pwg import ParallelWaveGANDiscriminator, ResidualParallelWaveGANDiscriminator
    from oracle import pwg

    kind, cfg = NETS[name]["kind"], _cfg(name)
    if kind == "plain":
        return ParallelWaveGANDiscriminator(**cfg, **_PLAIN_KW), pwg.ParallelWaveGANDiscriminator(**cfg, **_PLAIN_KW)
    if kind == "discriminator":
        return (ResidualParallelWaveGANDiscriminator(**cfg, dropout=0.0),
                pwg.ResidualParallelWaveGANDiscriminator(**cfg, dropout=0.0))
    return _GenStack(**cfg), pwg.ParallelWaveGANGenerator(**cfg, upsample_conditional_features=False)


def _report(prod, B, T):
    """crk_debug_net_layout of the model's stack at (B, T) (reserved here if it was not): ({key: value}, forward rows)."""
    from crank_amd import _lib

    net = prod.stack.net
    net.saved_bytes(B, T)
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.lib().crk_debug_net_layout(net.handle, B, T, out), "crk_debug_net_layout")
    return dict(zip(nl.KEYS, list(out)[:6])), out[6]


def _assert_layout(name, prod, B, T, want=None):
    got, rows = _report(prod, B, T)
    print(f"[layout {name} B={B} T={T}] {got} forward rows {rows}")
    assert got == nl.layout(NETS[name], B, T), (got, nl.layout(NETS[name], B, T))
    if want is not None:
        assert got == want, (got, want)
    return got


@pytest.fixture(autouse=True)
def _plain_precision_afterwards():
    """(_check_standalone leaves its precision set when it fails)"""
    from crank_amd import ops

    yield
    ops.set_precision("bf16")


def _pick_utterances_away_from_kinks(orac, B, cin, T, n_seeds=24, extra=None):
    """test_gpu_nets._pick_input_away_from_kinks for batches of dozens of utterances.  That function keeps, of n_seeds whole
    batches, the one whose smallest hidden |pre-activation| is largest; the smallest of the 2.8e6 pre-activations of the
    classifier at B = 33, T = 193 is then ~1e-6, below the forward's error (~1e-5), units flip their LeakyReLU branch and
    the gradients move by O(1e-3) of scale without an error on either side (the case that function exists to avoid).
    Utterances do not see each other, so the choice is made per batch row here: row i is taken from the seed whose row i
    has the largest margin - same seeds, same number of oracle forwards, a margin one to two orders larger.  The margin
    of a unit is measured in units of its layer's rms pre-activation: the forward's error grows with the layer's scale, and
    the absolute minimum protects the layers of small scale only (chosen by it, one unit of row 6 of that case still
    flipped: dx off by 4e-2 over exactly one receptive field, 89 frames, in every batch layout and alone).  The
    conditioning (`extra`) stays with its row."""
    import numpy as np

    mins = []

    def hook(_m, inp):
        a = inp[0].detach()
        mins.append(a.abs().flatten(1).min(dim=1).values / a.pow(2).mean().sqrt())

    hs = [m.register_forward_pre_hook(hook) for m in orac.modules() if isinstance(m, (torch.nn.LeakyReLU, torch.nn.ReLU))]
    xs, margins = [], []
    for seed in range(n_seeds):
        x = torch.from_numpy(np.random.RandomState(100 + seed).standard_normal((B, cin, T)).astype(np.float32))
        mins.clear()
        with torch.no_grad():
            orac(x) if extra is None else orac(x, extra)
        xs.append(x)
        margins.append(torch.stack(mins).min(dim=0).values if mins else torch.ones(B))
    for h in hs:
        h.remove()
    best = torch.stack(margins).max(dim=0)  # per row: the margin and the seed that has it
    x = torch.stack([xs[int(s)][i] for i, s in enumerate(best.indices)])
    return x, float(best.values.min())


# --------------------------------------------------------------------------------------------------------------------
# Part 1: oracle parity where groups walk several chunks and ft = 3 is planned
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name,B,T,want", ORACLE_CASES, ids=[f"{n}-{b}x{t}" for n, b, t, _ in ORACLE_CASES])
def test_oracle_parity_at_multi_chunk_groups_and_192_row_windows(name, B, T, want, precision, monkeypatch):
    """test_net_layout_cpu.py::test_oracle_case_edges names each case's edge.  Forward, dx, dc and every parameter gradient
    against the fp32 oracle ("bf16x3") and the bf16-emulating one ("bf16"), by _check_standalone's criteria; the bf16x3 input
    is chosen away from the activations' kinks row by row (_pick_utterances_away_from_kinks)."""
    import tests.test_gpu_nets as nets

    monkeypatch.setattr(nets, "_pick_input_away_from_kinks", _pick_utterances_away_from_kinks)
    prod, orac = _build(name)
    _assert_layout(name, prod, B, T, want)
    if NETS[name]["kind"] == "generator":
        _generator_stack_case(_cfg(name), T, precision, B=B)
    else:
        _check_standalone(prod, orac, NETS[name]["in_channels"], B=B, T=T, precision=precision)


@pytest.mark.parametrize("name,T", [("enc0", 100), ("dec0", 100), ("enc1", 120)])
def test_oracle_parity_split_forward_plain_backward_at_192_row_windows(name, T):
    """`bf16x3f` at B = 129: the plain-bf16 chain at ft = 3 reads the planes the split-operand forward wrote."""
    B = 129
    prod, orac = _build(name)
    assert _assert_layout(name, prod, B, T)["ft"] == 3
    aux = NETS[name]["aux_channels"]
    _check_split_forward(prod, orac, NETS[name]["in_channels"], aux, B, T, f"{name} B={B}",
                         orac_call=(None if aux else (lambda x: orac(x, None))))


# --------------------------------------------------------------------------------------------------------------------
# Part 2: the benchmark's shapes against sub-batches of two and of one
SHAPES = [(64, 500), (128, 500), (65, 449), (33, 500)]
MODES = ["bf16", "bf16x3f", "bf16x3"]
SINGLES_AT = (33, 500)  # the shape at which the test also runs the utterances one at a time (every net, every arithmetic)
# Relative L2 of a parameter-gradient tensor of the whole batch against the float64 sum of the sub-batch runs' gradients:
# 4x (rounded up) the largest value measured in each arithmetic over every net and shape, see the docstring of
# test_benchmark_shape_equals_its_sub_batches.  A difference above 1e-4 would not be reassociation (test_gpu_cond_sums.py).
BOUND = {"bf16": 6e-6, "bf16x3f": 6e-6, "bf16x3": 5e-5}


def _inputs(name, B, T):
    net = NETS[name]
    g = torch.Generator("cuda").manual_seed(1000 + B + T)
    x = torch.randn(B, net["in_channels"], T, device="cuda", generator=g)
    c = torch.randn(B, net["aux_channels"], T, device="cuda", generator=g) if net["aux_channels"] else None
    dy = torch.randn(B, net["out_channels"], T, device="cuda", generator=g)
    return x, c, dy


def _run(prod, x, c, dy):
    xp = x.clone().requires_grad_(True)
    cp = c.clone().requires_grad_(True) if c is not None else None
    prod.zero_grad()
    y = prod(xp, cp) if c is not None else prod(xp)
    (y * dy).sum().backward()
    prod.finish_grads()
    out = {"y": y.detach().clone(), "dx": xp.grad.clone(), "gp": prod.grad_flat.double()}
    if c is not None:
        out["dc"] = cp.grad.clone()
    return out


def _split_run(prod, x, c, dy, step):
    """The batch `step` utterances at a time: rows of y / dx / dc put back together, float64 sum of the parameter gradients."""
    parts, gp = [], None
    for i in range(0, x.shape[0], step):
        r = _run(prod, x[i: i + step], None if c is None else c[i: i + step], dy[i: i + step])
        gp = r.pop("gp") if gp is None else gp + r.pop("gp")
        parts.append(r)
    out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    out["gp"] = gp
    return out


def _tensor_errors(prod, a, b):
    """{tensor: relative L2 of a against b} over the model's parameter-gradient tensors (float64 flat blocks)."""
    errs = {}
    for k, off, shp in prod._entries:
        n = 1
        for s in shp:
            n *= int(s)
        ra, rb = a[off: off + n], b[off: off + n]
        nb = float(rb.norm())
        if nb == 0.0:  # (the last block's 1x1 out conv never gets a gradient)
            assert not bool(ra.any()), k
            continue
        errs[k] = float((ra - rb).norm()) / nb
    return errs


def benchmark_shape_case(name, B, T, mode, singles):
    """One case of test_benchmark_shape_equals_its_sub_batches; returns the measured figures."""
    from crank_amd import ops

    ops.set_precision("bf16")
    prod, orac = _build(name)
    _load_same(prod, orac)
    ncpu = nl.chunks_per_utt(T)
    whole_layout = _assert_layout(name, prod, B, T)
    for sub in (2, 1) if singles or B % 2 else (2,):
        got = _assert_layout(name, prod, sub, T)
        # every chunk of the generic region its own group, no group of the gated region beyond one utterance
        assert got["cpg"] == 1 and (got["cpg_s"] == 0 or ncpu % got["cpg_s"] == 0), got
    x, c, dy = _inputs(name, B, T)
    ops.set_precision(mode)
    try:
        whole = _run(prod, x, c, dy)
        pairs = _split_run(prod, x, c, dy, 2)
        ones = _split_run(prod, x, c, dy, 1) if singles else None
        torch.cuda.synchronize()
    finally:
        ops.set_precision("bf16")
    from crank_amd import _lib

    x3f = [bool(_lib.lib().crk_debug_net_paths(prod.stack.net.handle, b, T) & 2) for b in (B, 2, 1)]
    # the whole batch's bf16x3f forward runs stack2x_fwd_kernel and a sub-batch's does not (or the reverse)
    fig = {"layout": whole_layout, "rows": _report(prod, B, T)[1], "exact": {},
           "other_forward": mode == "bf16x3f" and (x3f[0] != x3f[1] or x3f[0] != x3f[2])}
    for ref_name, ref in (("pairs", pairs), ("singles", ones)):
        if ref is None:
            continue
        for k in ("y", "dx", "dc"):
            if k in whole:
                same = torch.equal(whole[k], ref[k])
                fig["exact"][f"{k} vs {ref_name}"] = same if same else float((whole[k] - ref[k]).abs().max() / ref[k].abs().max())
    fig["err"] = _tensor_errors(prod, whole["gp"], pairs["gp"])
    if ones is not None:
        fig["err1"] = _tensor_errors(prod, whole["gp"], ones["gp"])
        fig["dist"] = _tensor_errors(prod, pairs["gp"], ones["gp"])
    worst = max(fig["err"], key=fig["err"].get)
    line = f"[batch layout {name} {mode} B={B} T={T}] rows equal: " + ", ".join(f"{k}: {v}" for k, v in fig["exact"].items())
    line += f"; parameter gradients vs float64 pair sums: worst {worst} {fig['err'][worst]:.3e}"
    if ones is not None:
        w1, wd = max(fig["err1"], key=fig["err1"].get), max(fig["dist"], key=fig["dist"].get)
        line += f", vs single sums {w1} {fig['err1'][w1]:.3e}; pair sums vs single sums {wd} {fig['dist'][wd]:.3e}"
    print(line)
    return fig


_CHILD = ("import sys, json; sys.path.insert(0, %r); from tests.test_gpu_batch_layout import benchmark_shape_case as f; "
          "print('FIG ' + json.dumps(f(%r, %d, %d, %r, singles=%r)))")


def _case_with_the_forward_window_pinned(name, B, T, mode, singles, rows):
    """The case in a process of its own with CRK_S2_CFG set to the window the whole batch's forward planned by itself (the
    switch is read once per process): the whole batch launches what it launches without the switch, and the sub-batches'
    forwards take the same kernel."""
    import json
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CRK_S2_CFG={192: "32", 160: "322"}[rows])
    r = subprocess.run([sys.executable, "-c", _CHILD % (repo, name, B, T, mode, singles)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout, end="")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FIG ")][-1][4:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,T", SHAPES, ids=[f"{b}x{t}" for b, t in SHAPES])
@pytest.mark.parametrize("name", list(NETS))
def test_benchmark_shape_equals_its_sub_batches(name, B, T, mode):
    """One forward and backward of the whole batch against the same utterances two at a time (every case) and one at a time
    (B = 33): rows of y, dx and dc bit for bit (a frame's sums do not depend on the window or on the batch), every
    parameter-gradient tensor against the float64 sum of the sub-batch runs' gradients (the weight-norm backward is linear
    in dW, so the sum is exact up to fp32 reassociation).

    Measured on an MI355X with pairs AND singles at every shape (profiles/batch_layout_tests.txt), worst tensor per case,
    relative L2, range over the nets and shapes:

        arithmetic   whole vs pair sums     whole vs single sums   pair sums vs single sums
        bf16         2.4e-7 ... 1.1e-6      2.4e-7 ... 1.5e-6      1.6e-7 ... 4.1e-7
        bf16x3f      2.4e-7 ... 1.1e-6      2.7e-7 ... 1.5e-6      1.4e-7 ... 3.8e-7
        bf16x3       3.6e-7 ... 8.2e-6      3.5e-7 ... 1.1e-5      1.6e-7 ... 3.3e-6

    y, dx and dc rows: equal to the bit in every case.  The whole batch adds 8 to 32 chunks per group in fp32 where the
    references add 1 to 8, so it lies 3 to 14 times further from either reference than they lie from each other: four
    times their distance bounds the references, not a 32-chunk sum.  Every value is reassociation-sized - the largest are
    the bias of D's one-channel head, the plain sum of dy over all frames, which cancels to 1e-2 of its terms - and a
    dropped chunk is 2e-3 (profiles/batch_layout_tests.txt: two drop-work mutants).  BOUND is 4x the largest value of each
    arithmetic, rounded up.

    Seven `bf16x3f` cases (enc0 and dec0 at 64 x 500 and 128 x 500, enc1 at 64 x 500, 128 x 500 and 65 x 449) are compared in
    a child process that pins the forward's window (CRK_S2_CFG).  Without the pin the whole batch's forward runs
    stack2x_fwd_kernel - planned only where stack2_fwd_plan picks its 192- or 160-row window, which depends on B - and a
    sub-batch's runs stack_fwd_kernel<PRECISE>: the same sums in the same order, but hardware exp2 / rcp in the gate
    against libm expf and an IEEE division (stack2x_kernels.hip, header).  y then differs by 6.1e-6 ... 9.3e-6 of scale
    (asserted here: inside _compare_standalone's 2e-4), and the plain-bf16 backward, rounding planes that differ in the
    last bit, gives dx 0.9e-2 ... 1.0e-1 of scale, dc 8e-2 ... 1.2e-1 and parameter gradients 3.8e-3 ... 6.2e-3 from the
    sub-batch runs: bf16 rounding noise (oracle/pwg.py), not a sum gone wrong, and no reference for one.  With the window
    pinned to what the whole batch planned, the whole batch launches exactly what it launches without the pin, the
    sub-batches take the same forward kernel, and every assertion below holds as in the other 65 cases."""
    singles = (B, T) == SINGLES_AT
    fig = benchmark_shape_case(name, B, T, mode, singles)
    if fig["other_forward"]:
        far = {k: v for k, v in fig["exact"].items() if k.startswith("y ") and v is not True and not v < 2e-4}
        assert not far, far
        fig = _case_with_the_forward_window_pinned(name, B, T, mode, singles, fig["rows"])
        assert not fig["other_forward"]
    bad = {k: v for k, v in fig["exact"].items() if v is not True}
    assert not bad, bad
    bound = BOUND[mode]
    assert bound is not None and bound <= 1e-4
    for key in ("err", "err1"):
        over = {k: v for k, v in fig.get(key, {}).items() if not v <= bound}
        assert not over, (key, over, bound)
