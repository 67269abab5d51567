"""The dropout cases tests/test_gpu_dropout.py runs on the GPU and tests/test_dropout_cpu.py qualifies on the CPU (what a
wrong mask would do to the oracle, against the bounds the GPU test uses): one table, so both files speak of the same
nets, seeds and inputs.  B = 2 everywhere (the second utterance makes the global frame base non-zero); T = 150 is one
128-frame tile and a 22-frame tail that is shorter than the halo, T = 257 three tiles."""
import functools

import numpy as np
import torch

from tests import dropout_ref as R
from tests.helpers import deterministic_state

B = 2
LSGAN_D = dict(in_channels=113, out_channels=1, kernel_size=5, layers=8, stacks=4)  # D (train.py:108-118)
GEN_DROP = dict(in_channels=80, out_channels=64, kernel_size=5, layers=4, stacks=2, aux_channels=34)
DISC_DIL16 = dict(in_channels=37, out_channels=1, kernel_size=5, layers=5, stacks=1)  # test_gpu_per_layer.py

# name: (kind, cfg, dropout, T, precision, reseed value, route)
# route: "split" crk_debug_net_paths & 4 (channel-split discriminator), "frame" fused frame-split kernels (paths without
# bit 2 / bit 0), "per-layer" conv_tile_kernel + the table weight gradient
PARITY = {
    "lsgan_bf16": ("disc", LSGAN_D, 0.25, 150, "bf16", 1001, "split"),
    "lsgan_bf16_T257": ("disc", LSGAN_D, 0.25, 257, "bf16", 1002, "split"),
    "lsgan_bf16x3": ("disc", LSGAN_D, 0.25, 150, "bf16x3", 1003, "frame"),
    "lsgan_bf16x3f": ("disc", LSGAN_D, 0.25, 150, "bf16x3f", 1004, "frame"),
    "d67_k3_bf16": ("disc", dict(in_channels=67, out_channels=15, kernel_size=3, layers=2, stacks=1), 0.25, 150, "bf16", 1005, None),
    "d69_bf16": ("disc", dict(in_channels=69, out_channels=1, kernel_size=5, layers=8, stacks=4), 0.25, 150, "bf16", 1006, None),
    "gen_bf16": ("gen", GEN_DROP, 0.1, 150, "bf16", 1007, "frame"),
    "gen_bf16x3": ("gen", GEN_DROP, 0.1, 150, "bf16x3", 1008, "frame"),
    "dil16_bf16": ("disc", DISC_DIL16, 0.25, 150, "bf16", 1009, "per-layer"),
    "dil16_bf16x3": ("disc", DISC_DIL16, 0.25, 150, "bf16x3", 1010, "per-layer"),
}
# exact pin at p = 0.5 (scale 2.0: no rounding added): name: (kind, cfg, reseed value).  The residual D has 32 output
# channels, of the order of the generator-kind cases: the pin's relative-L2 bounds allow for the rare gate value that the hardware's
# exp / rcp put on the other side of a bf16 rounding boundary (test_gpu_nets.py: about one in 3e4, it moves one frame's
# outputs), and with ONE output channel one such frame of 300 is 1 / sqrt(300) of the whole tensor, not 1 / sqrt(300 * 32).
PIN = {
    "gated_k3_one_block": ("gen", dict(in_channels=64, out_channels=64, kernel_size=3, layers=1, stacks=1, aux_channels=0), 2001),
    "gated_k5_dil12_aux34": ("gen", dict(in_channels=128, out_channels=80, kernel_size=5, layers=2, stacks=1, aux_channels=34), 2002),
    "residual_d_two_blocks": ("disc", dict(in_channels=128, out_channels=32, kernel_size=5, layers=2, stacks=1), 2003),
}
PIN_P = 0.5
PIN_T = 150
PIN_SLOPE = 0.25  # LeakyReLU of the residual-D pin case: 0.2 is no power of two (see test_dropout_cpu.py)


class _GenOracle(torch.nn.Module):
    """oracle generator stack called (x) or (x, c) like the HIP _GenStack."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, c=None):
        return self.m(x, c)

    def state_dict(self, *a, **k):
        return self.m.state_dict(*a, **k)

    def load_state_dict(self, sd, strict=True):
        return self.m.load_state_dict(sd, strict)

    def named_parameters(self, *a, **k):
        return self.m.named_parameters(*a, **k)


def oracle_of(kind, cfg, dropout, slope=0.2):
    from oracle import pwg

    if kind == "disc":
        return pwg.ResidualParallelWaveGANDiscriminator(**cfg, dropout=dropout, nonlinear_activation_params={"negative_slope": slope})
    return _GenOracle(pwg.ParallelWaveGANGenerator(**cfg, dropout=dropout, upsample_conditional_features=False))


def product_of(kind, cfg, dropout, slope=0.2):
    from crank_amd.net.module.pwg import ResidualParallelWaveGANDiscriminator
    from tests.test_gpu_nets import _GenStack

    if kind == "disc":
        return ResidualParallelWaveGANDiscriminator(**cfg, dropout=dropout, nonlinear_activation_params={"negative_slope": slope})
    return _GenStack(**cfg, dropout=dropout)


def load_oracle(orac, seed=99):
    """The state tests.test_gpu_nets._load_same gives both sides."""
    sd = orac.state_dict()
    vals = deterministic_state({k: tuple(v.shape) for k, v in sd.items()}, seed)
    orac.load_state_dict({k: torch.from_numpy(vals[k]) for k in sd})


def masks_of(seed, cfg, T, p):
    return R.layer_masks(seed, cfg["layers"], B, T, p)


def aux_of(cfg):
    return max(cfg.get("aux_channels", 0), 0)


def pin_inputs(cfg):
    """x, c, dy in eighths, as test_bf16_single_layer_deterministic_pin's (B = 2)."""
    from tests.test_gpu_nets import _eighths

    rs = np.random.RandomState(17)
    aux = aux_of(cfg)
    x = _eighths(rs, (B, cfg["in_channels"], PIN_T))
    c = _eighths(rs, (B, aux, PIN_T)) if aux else None
    dy = _eighths(rs, (B, cfg["out_channels"], PIN_T))
    return x, c, dy


def pin_oracle(name, slope=None):
    """(oracle loaded with the exact +-1/4 state, cfg, call) of a pin case."""
    from tests.test_gpu_nets import _exact_state

    kind, cfg, _ = PIN[name]
    orac = oracle_of(kind, cfg, PIN_P, PIN_SLOPE if slope is None else slope)
    sd = orac.state_dict()
    vals = _exact_state({k: tuple(v.shape) for k, v in sd.items()}, 321)
    orac.load_state_dict({k: torch.from_numpy(vals[k]) for k in sd})
    return orac, cfg, vals


def pin_call(m, x, c):
    return m(x, c) if c is not None else m(x)


def gate_margin(orac, cfg, masks, x, c):
    """How far the gate outputs z = tanh * sigmoid of the masked bf16 emulation stay from a bf16 rounding boundary, in fp32
    ulps (the smallest over all blocks and elements; 0: a tie), and the (block, utterance, frame) of that element.  The 1x1
    convs behind the gate round z to bf16; the kernels' exp / rcp differ from libm in the last fp32 bit or two, so a z
    that close to a boundary rounds the other way on the GPU and moves its whole frame by a bf16 ulp."""
    from oracle import pwg as opwg

    seen = []
    hs = [b.conv1x1_skip.register_forward_pre_hook(lambda _m, inp: seen.append(inp[0].detach().clone())) for b in R._blocks(orac)]
    try:
        with R.masked(orac, masks, p=PIN_P), opwg.bf16_emulation(accumulate="fp64"), torch.no_grad():
            pin_call(orac, x, c)
    finally:
        for h in hs:
            h.remove()
    best = (1 << 16, None)
    for l, z in enumerate(seen):
        d = np.abs((z.numpy().view(np.uint32) & 0xFFFF).astype(np.int64) - 0x8000)
        k = int(d.argmin())
        if int(d.reshape(-1)[k]) < best[0]:
            b, _, t = np.unravel_index(k, z.shape)
            best = (int(d.reshape(-1)[k]), (l, int(b), int(t)))
    return best


def pin_sums_exact(orac, masks, x, c, dy):
    """Do the float64, fp32 and permuted-fp32 emulations of a pin case agree BIT FOR BIT in y and dx?  That agreement is
    the sign that every sum in front of a rounding is exact, i.e. that the kernel's own summation order cannot matter.
    (dc, where a case has it, is a sum over 128 gate channels per block and agrees to an fp32 ulp only, under any mask.)"""
    from tests.test_gpu_nets import _pin_oracle

    with R.masked(orac, masks, p=PIN_P):
        out = [_pin_oracle(orac, pin_call, x, c, dy, a) for a in ("fp64", "fp32", "fp32-permuted")]
    return all(torch.equal(o[k], out[0][k]) for o in out[1:] for k in ("y", "dx"))


@functools.lru_cache(maxsize=None)
def pin_reseed(name, n_seeds=1):
    """The reseed value of a pin case, from the CPU emulation alone (the analogue of _pick_input_away_from_kinks): of
    v, v + 100, ... (16 candidates) the one whose masks keep the gate outputs furthest from a bf16 rounding boundary
    (gate_margin, over the first `n_seeds` seeds of the sequence) among those under which every sum is exact
    (pin_sums_exact: a data-gradient sum of bf16 values that span more than 13 binary orders is not, and which elements
    meet in a sum depends on the mask).  About five of the 4e4 gate outputs of a case lie within 6 fp32 ulps of a boundary
    under any mask, ties included; the best of 16 masks keeps 2 - 4 ulps.
    Returns (reseed value, margin in fp32 ulps, (block, utterance, frame) of the closest element)."""
    kind, cfg, v = PIN[name]
    orac, cfg, _ = pin_oracle(name)
    x, c, dy = pin_inputs(cfg)
    for batch in range(4):  # (libm differs between hosts in the last bit: should none of 16 be exact, the next 16)
        cand = []
        for i in range(16 * batch, 16 * batch + 16):
            vi = v + 100 * i
            m = min(gate_margin(orac, cfg, masks_of(s, cfg, PIN_T, PIN_P), x, c) for s in R.seed_sequence(vi, n_seeds))
            cand.append((-m[0], i, vi, m))
        for _, _, vi, m in sorted(cand):
            if all(pin_sums_exact(orac, masks_of(s, cfg, PIN_T, PIN_P), x, c, dy) for s in R.seed_sequence(vi, n_seeds)):
                return vi, m[0], m[1]
    raise AssertionError(name)


def pin_ok(k, m):
    """The fixed bounds of test_bf16_single_layer_deterministic_pin's gated cases on _pin_metrics `m` of tensor `k`."""
    if k in ("y", "dx", "dc"):
        return m["frac>2e-5"] <= 2e-2 and m["rl2"] <= 5e-5 and m["max"] <= 2e-3
    return m["max"] <= 3e-4 and m["rl2"] <= 1e-4


@functools.lru_cache(maxsize=None)
def first_seed(v):
    return R.seed_sequence(v, 1)[0]


@functools.lru_cache(maxsize=None)
def parity_reference(name, v0=None):
    """(reseed value, oracle, masks, _standalone_refs(...)) of a parity case, chosen from the CPU emulations ALONE.

    Plain bf16 is accepted within 3x the larger deviation of two fp32 CPU evaluations from the float64-accumulated one.
    For a tensor of many entries that two-sample figure is stable.  The weight_g gradient of a one-row conv (the head of a
    discriminator with one output channel) is ONE number, <v, dW> / ||v||, which here cancels to 1 - 10 % of ||dW||: its two
    CPU deviations are two draws of a Gaussian, and the larger of two draws is below a third of the next draw once in 15
    (measured: 3e-4 to 1.5e-1 of the scalar across reseed values, with ||dW|| steady at 2e-3).  The row itself gives an
    independent estimate of that Gaussian's width - the deviation of dW projected on one direction, ||delta dW|| /
    sqrt(row length) - so the reseed value of a case is the first of v, v + 100, ... at which the two-sample figure of every
    such scalar is at least that width.  Nothing the kernels compute enters the choice."""
    from tests.test_gpu_nets import _rl2, _standalone_refs

    kind, cfg, p, T, precision, v, _ = PARITY[name]
    v = v if v0 is None else v0
    assert precision in ("bf16", "bf16x3")
    orac = oracle_of(kind, cfg, p)
    load_oracle(orac)
    for i in range(16):
        vi = v + 100 * i
        masks = masks_of(first_seed(vi), cfg, T, p)
        refs = _standalone_refs(orac, cfg["in_channels"], B, T, precision, aux_of(cfg), mask_ctx=lambda: R.masked(orac, masks, p=p))
        ref, e32, e32p = refs[3], refs[4], refs[5]
        ok = True
        for k in (ref if precision == "bf16" else ()):
            kv = k[:-1] + "v"
            if k.endswith("weight_g") and ref[k].numel() == 1 and kv in ref:
                two = max(_rl2(e32[k], ref[k]), _rl2(e32p[k], ref[k])) * ref[k].abs().item()
                dv = max((e32[kv] - ref[kv]).norm().item(), (e32p[kv] - ref[kv]).norm().item())
                ok = ok and two >= dv / ref[kv].numel() ** 0.5
        if ok:
            return vi, orac, masks, refs
    raise AssertionError(name)
