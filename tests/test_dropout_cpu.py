"""CPU half of the dropout pin (tests/test_gpu_dropout.py is the GPU half).

1. The restated mask (tests/dropout_ref.py) behaves like a mask: keep rate, independence across layers, seeds and the
   four lanes of a quad.  These are conditions on the hash, not tolerances.
2. Discriminating power, from the oracle alone: for every GPU parity case, on that case's state and inputs, the masked
   oracle is evaluated with the mask or scale a subtly wrong kernel would use, and each such perturbation must move y, dx
   or a parameter gradient away from the unperturbed oracle by more than 10x the bound the GPU test applies to that
   tensor.  That is what makes the GPU bounds mean something.  A single flipped mask element is tried on the exact-pin
   cases, against their "everywhere" bound."""
import functools

import numpy as np
import pytest
import torch

from tests import dropout_cases as C
from tests import dropout_ref as R
from tests.test_gpu_nets import _cos, _oracle_run, _pin_metrics, _pin_oracle, _rel, _rl2, _x3_errors

SEED, ST_B, ST_T, ST_LAYERS = 1234, 2, 150, 8
SIGMA = 4.0


def _corr(a, b):
    a = a.reshape(-1).astype(np.float64)
    b = b.reshape(-1).astype(np.float64)
    a -= a.mean()
    b -= b.mean()
    return float((a @ b) / np.sqrt((a @ a) * (b @ b)))


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_restated_mask_statistics(p):
    masks = [R.keep_mask(SEED, l, ST_B, ST_T, 64, p) for l in range(ST_LAYERS)]
    n = masks[0].size
    assert masks[0].shape == (ST_B, 64, ST_T) and masks[0].dtype == np.bool_
    sd = np.sqrt(p * (1 - p) / n)
    rate = max(abs(m.mean() - (1 - p)) / sd for m in masks)
    layer = max(abs(_corr(masks[i], masks[j])) * np.sqrt(n) for i in range(ST_LAYERS) for j in range(i + 1, ST_LAYERS))
    seeds = R.seed_sequence(SEED, 4)
    sm = [R.keep_mask(s, 0, ST_B, ST_T, 64, p) for s in seeds]
    seedc = max(abs(_corr(sm[i], sm[i + 1])) * np.sqrt(n) for i in range(3))
    lane = 0.0
    for m in masks:
        q = m.transpose(0, 2, 1).reshape(-1, 4)  # (frame, quad) x lane
        for i in range(4):
            for j in range(i + 1, 4):
                lane = max(lane, abs(_corr(q[:, i], q[:, j])) * np.sqrt(q.shape[0]))
    print(f"[mask statistics p={p}] keep rate {rate:.2f} sigma, layers {layer:.2f}, consecutive seeds {seedc:.2f}, "
          f"lanes of a quad {lane:.2f} (all < {SIGMA})")
    assert rate < SIGMA and layer < SIGMA and seedc < SIGMA and lane < SIGMA


def test_restatement_constants():
    assert [R.threshold(p) for p in (0.1, 0.25, 0.5)] == [6554, 16384, 32768]
    assert float(R.keep_scale(0.5)) == 2.0 and R.keep_scale(0.25) == np.float32(4.0 / 3.0)
    s = R.seed_sequence(7, 3)
    assert len(set(s)) == 3 and all(0 <= v < 2 ** 62 for v in s) and R.seed_sequence(7, 2) == s[:2]
    # the element index is (global frame) * 64 + channel: utterance 1 continues utterance 0's frames
    two = R.keep_mask(SEED, 3, 2, 150, 64, 0.25)
    one = R.keep_mask(SEED, 3, 1, 300, 64, 0.25)
    assert np.array_equal(two[1], one[0][:, 150:]) and np.array_equal(two[0], one[0][:, :150])


def test_masked_oracle_is_the_oracle_times_the_mask():
    """masked() against the definition, in fp32 and inside the bf16 emulation: an all-kept mask of scale 1 is the
    dropout-free oracle bit for bit, and a real mask equals an oracle whose blocks multiply by it by hand."""
    from oracle import pwg as opwg

    kind, cfg, p, T, _, v, _ = C.PARITY["d67_k3_bf16"]
    orac = C.oracle_of(kind, cfg, p)
    C.load_oracle(orac)
    orac.eval()  # F.dropout is the identity: the dropout-free oracle
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((C.B, cfg["in_channels"], T)).astype(np.float32))
    ones = [np.ones((C.B, 64, T), dtype=bool)] * cfg["layers"]
    masks = C.masks_of(C.first_seed(v), cfg, T, p)
    for emu in (False, True):
        with opwg.bf16_emulation(on=emu, accumulate="fp64"):
            plain, dy = _oracle_run(orac, x, None, None, 0)
            with R.masked(orac, ones, scale=1.0):
                same, _ = _oracle_run(orac, x, None, dy, 0)
            with R.masked(orac, masks, p=p):
                got, _ = _oracle_run(orac, x, None, dy, 0)
            mult = [torch.from_numpy(m.astype(np.float32) * R.keep_scale(p)) for m in masks]
            hs = [b.conv.register_forward_pre_hook(lambda _m, inp, k=k: (inp[0] * mult[k],)) for k, b in enumerate(R._blocks(orac))]
            try:
                hand, _ = _oracle_run(orac, x, None, dy, 0)
            finally:
                for h in hs:
                    h.remove()
        for k in plain:
            assert torch.equal(plain[k], same[k]), (emu, k)
            assert torch.equal(hand[k], got[k]), (emu, k)
        assert not torch.equal(plain["y"], got["y"])


# ---- discriminating power ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_reference(name):
    kind, cfg, p, T, precision, v, _ = C.PARITY[name]
    if precision != "bf16x3f":
        v, orac, masks, refs = C.parity_reference(name)
        return v, orac, masks, refs
    orac = C.oracle_of(kind, cfg, p)
    C.load_oracle(orac)
    masks = C.masks_of(C.first_seed(v), cfg, T, p)
    x = torch.from_numpy(np.random.RandomState(100).standard_normal((C.B, cfg["in_channels"], T)).astype(np.float32))  # _check_split_forward's
    with R.masked(orac, masks, p=p):
        ref, dy = _oracle_run(orac, x, None, None, 0)
    return v, orac, masks, (x, None, dy, ref, None, None, float("nan"))


def _margins(precision, pert, ref, e32, e32p):
    """{tensor: distance of `pert` from `ref` / the bound the GPU test applies to that tensor}."""
    if precision == "bf16x3":
        return {k: e / 2e-4 for k, e in _x3_errors(pert, ref).items()}
    if precision == "bf16x3f":  # y 2e-4 of scale; gradients relative L2 < 5e-2 and cosine > 0.998
        out = {"y": _rel(pert["y"], ref["y"]) / 2e-4}
        for k in ref:
            if k != "y":
                out[k] = max(_rl2(pert[k], ref[k]) / 5e-2, (1.0 - _cos(pert[k], ref[k])) / 2e-3)
        return out
    out = {}
    for k in ref:  # bf16: relative L2 within 3x the CPU fp32 evaluations' own + 2e-4
        noise = max(_rl2(e32[k], ref[k]), _rl2(e32p[k], ref[k]))
        out[k] = _rl2(pert[k], ref[k]) / (3.0 * noise + 2e-4)
    return out


@pytest.mark.parametrize("name", list(C.PARITY))
def test_wrong_masks_exceed_ten_times_the_gpu_bounds(name):
    """(b) block l given block l + 1's mask, (c) channels permuted within each quad, (d) scale 1 / p, (e) the dilated
    conv's weight gradient taken on the undropped block input: each moves some tensor by more than 10x its GPU bound."""
    from oracle import pwg as opwg

    kind, cfg, p, T, precision, _, _ = C.PARITY[name]
    v, orac, masks, (x, c, dy, ref, e32, e32p, _) = _parity_reference(name)
    seed, aux = C.first_seed(v), C.aux_of(cfg)
    extra = R.keep_mask(seed, cfg["layers"], C.B, T, 64, p)
    perts = {
        "(b) next layer's mask": dict(masks=R.shift_layers(masks, extra), p=p),
        "(c) quad lanes permuted": dict(masks=R.permute_quads(masks), p=p),
        "(d) scale 1/p": dict(masks=masks, scale=1.0 / p),
        "(e) wgrad on undropped input": dict(masks=masks, p=p, wgrad_undropped=True),
    }
    line = []
    for tag, kw in perts.items():
        with R.masked(orac, **kw), opwg.bf16_emulation(on=(precision == "bf16"), accumulate="fp64"):
            pert, _ = _oracle_run(orac, x, c, dy, aux)
        if tag.startswith("(e)"):  # everything but the block convs' parameter gradients is untouched
            for k in ref:
                if not (k.endswith(".conv.weight_v") or k.endswith(".conv.weight_g") or k.endswith(".conv.bias")):
                    assert torch.equal(pert[k], ref[k]), k
        m = _margins(precision, pert, ref, e32, e32p)
        worst = max(m, key=m.get)
        line.append(f"{tag}: {m[worst]:.0f}x ({worst})")
        assert m[worst] > 10.0, (name, tag, worst, m[worst])
    print(f"[dropout power {name} p={p} {precision} reseed {v}] margin over the GPU bound: " + "; ".join(line))


# ---- the exact pin ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pin_reference(name, accumulate="fp64", slope=None):
    v = C.pin_reseed(name)[0]
    orac, cfg, _ = C.pin_oracle(name, slope)
    masks = C.masks_of(C.first_seed(v), cfg, C.PIN_T, C.PIN_P)
    x, c, dy = C.pin_inputs(cfg)
    with R.masked(orac, masks, p=C.PIN_P):
        ref = _pin_oracle(orac, C.pin_call, x, c, dy, accumulate)
    return orac, masks, (x, c, dy), ref


@pytest.mark.parametrize("name", list(C.PIN))
def test_pin_cases_are_exact_in_every_summation_order(name):
    """Every pin case, under the masks of its reseed value: the float64, fp32 and permuted-fp32 emulations agree bit for bit
    in y and dx - every sum is exact, so the GPU comparison has no summation-order noise to allow for - and to 3e-6 of
    scale in dc (a sum over 128 gate channels per block) and the parameter gradients (fp32 sums over B * T frames; their
    bound is 3e-4).  The residual D is built with
    LeakyReLU slope 0.25: with the reference's 0.2 (no power of two) the activations agree only to an fp32 ulp."""
    refs = {a: _pin_reference(name, a)[3] for a in ("fp64", "fp32", "fp32-permuted")}
    act = ("y", "dx")
    for a in ("fp32", "fp32-permuted"):
        for k in act:
            assert torch.equal(refs[a][k], refs["fp64"][k]), (a, k)
    worst = max(_pin_metrics(refs[a][k], refs["fp64"][k])["max"] for a in ("fp32", "fp32-permuted") for k in refs["fp64"])
    v, ulps, where = C.pin_reseed(name)
    note = ""
    if C.PIN[name][0] == "disc":
        s02 = {a: _pin_reference(name, a, 0.2)[3] for a in ("fp64", "fp32", "fp32-permuted")}
        n02 = sum(int((s02[a][k] != s02["fp64"][k]).sum()) for a in ("fp32", "fp32-permuted") for k in act)
        note = f"; with slope 0.2: {n02} entries of y, dx differ between the three"
    print(f"[pin {name} reseed {v}, gate outputs >= {ulps} fp32 ulps from a rounding boundary] y, dx bit-identical in fp64 / fp32 / "
          f"fp32-permuted, dc and parameter gradients within {worst:.1e} of scale{note}")
    assert worst <= 3e-6


@pytest.mark.parametrize("name", list(C.PIN))
def test_one_flipped_mask_element_trips_the_everywhere_bound(name):
    """(a) one mask element of one layer flipped, on the exact-pin cases: y or dx leaves the unperturbed emulation by more
    than 10x the 2e-3 of scale the pin allows everywhere - the pin is a bit-level check of the mask."""
    kind, cfg, v = C.PIN[name]
    orac, masks, (x, c, dy), ref = _pin_reference(name)
    # the element: second utterance, the tail behind the 128-frame tile, where the block's input is largest (what a flip
    # changes is +-2 x that input; a flip at an input of zero changes nothing, whatever the bound)
    seen = []
    hs = [b.register_forward_pre_hook(lambda _m, inp: seen.append(inp[0].detach()[1, :, 128:].abs())) for b in R._blocks(orac)]
    with R.masked(orac, masks, p=C.PIN_P), torch.no_grad():
        C.pin_call(orac, x, c)
    for h in hs:
        h.remove()
    line = []
    for layer in range(cfg["layers"]):
        ch, t = divmod(int(seen[layer].argmax()), seen[layer].shape[1])
        flipped = R.flip_one(masks, layer, 1, ch, 128 + t)
        with R.masked(orac, flipped, p=C.PIN_P):
            pert = _pin_oracle(orac, C.pin_call, x, c, dy, "fp64")
        m = {k: _pin_metrics(pert[k], ref[k])["max"] / 2e-3 for k in ("y", "dx")}
        worst = max(m, key=m.get)
        line.append(f"layer {layer}: {m[worst]:.0f}x ({worst})")
        assert m[worst] > 10.0, (name, layer, m)
    print(f"[dropout power {name} p={C.PIN_P}] (a) one flipped element over the 2e-3 everywhere bound: " + "; ".join(line))
