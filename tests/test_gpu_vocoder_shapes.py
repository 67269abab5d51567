"""Parallel WaveGAN vocoder inference (crk_voc_*, csrc/vocoder_kernels.hip) against the CPU restatement
tests/pwg_vocoder_ref.py beyond the configurations of tests/test_gpu_vocoder.py: hops that put utterance edges and the
batch end inside a wave's 32-sample tile, batches long enough that every workgroup walks several tiles, aux widths
1 / 36 / 127 / 128, aux context windows 0 and 5, one- and two-layer stacks and one 30-layer stack, upsample scales of
1, 16 and eight stages, and bf16x3f.  Each case asserts, on the host, that it reaches the edge it is named after; the
tolerances are those of tests/test_gpu_vocoder.py."""
import functools

import numpy as np
import pytest
import torch

from oracle.pwg import bf16_emulation
from tests.pwg_vocoder_ref import checkpoint_of, random_generator

pytestmark = pytest.mark.gpu

TILE = 32  # samples per wave of voc_layer_kernel
WAVES = 8  # waves per workgroup
SMALL = dict(layers=6, stacks=2)


def _tile_walk_lens(hop, n_cu):
    """Frames of a ragged batch (1- and 2-frame utterances among them) whose N exceeds 2 * CUs * 8 waves * 32 samples:
    the grid is capped at the CU count, so the tile loop takes a third trip."""
    need = 2 * n_cu * WAVES * TILE // hop + 1
    big = -(-(need - 3) // 3)
    return [1, big + 7, 2, big, big - 5]


# name -> (generator_params, frames per utterance or None for a tile-walking batch, seed)
CASES = {
    "hop240": (dict(upsample_params={"upsample_scales": [4, 5, 3, 4]}), [4, 5, 3, 4, 1, 2], 21),
    "hop30": (dict(SMALL, upsample_params={"upsample_scales": [2, 3, 5]}), [5, 3, 2, 1], 22),
    "walk_small_hop300": (dict(SMALL, upsample_params={"upsample_scales": [4, 5, 3, 5]}), None, 23),
    "walk_default_hop256": (dict(upsample_params={"upsample_scales": [4, 4, 4, 4]}), None, 24),
    "aux1": (dict(SMALL, aux_channels=1, upsample_params={"upsample_scales": [2, 4, 4]}), [3, 1, 6, 2], 25),
    "aux36": (dict(SMALL, aux_channels=36, upsample_params={"upsample_scales": [2, 4, 4]}), [3, 1, 6, 2], 26),
    "aux127": (dict(SMALL, aux_channels=127, upsample_params={"upsample_scales": [2, 4, 4]}), [3, 1, 6, 2], 27),
    "aux128": (dict(SMALL, aux_channels=128, upsample_params={"upsample_scales": [2, 4, 4]}), [3, 1, 6, 2], 28),
    "window0": (dict(SMALL, aux_context_window=0, upsample_params={"upsample_scales": [2, 4, 4]}), [1, 4, 1, 2], 29),
    "window5": (dict(SMALL, aux_context_window=5, upsample_params={"upsample_scales": [2, 4, 4]}), [1, 4, 1, 2], 30),
    "layers1": (dict(layers=1, stacks=1, upsample_params={"upsample_scales": [2, 4, 4]}), [2, 5, 1], 31),
    "layers2": (dict(layers=2, stacks=1, upsample_params={"upsample_scales": [2, 4, 4]}), [2, 5, 1], 32),
    "layers30_stack1": (dict(layers=30, stacks=1, upsample_params={"upsample_scales": [2, 4, 4]}), [2, 5, 1, 9], 33),
    "scales_1_4_8": (dict(SMALL, upsample_params={"upsample_scales": [1, 4, 8]}), [1, 2, 5, 3], 34),
    "scales_16_16": (dict(SMALL, upsample_params={"upsample_scales": [16, 16]}), [1, 2, 5, 3], 35),
    "scales_2x8": (dict(SMALL, upsample_params={"upsample_scales": [2] * 8}), [1, 2, 5, 3], 36),
}


def _hop(name):
    return int(np.prod(CASES[name][0]["upsample_params"]["upsample_scales"]))


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lens(name):
    lens = CASES[name][1]
    return list(lens) if lens is not None else _tile_walk_lens(_hop(name), _n_cu())


@functools.lru_cache(maxsize=None)
def _case(name):
    """(restated generator without weight norm, vocoder, features, noises, fp32 waveforms)."""
    from crank_amd.vocoder import ParallelWaveGANVocoder

    params, _, seed = CASES[name]
    g = random_generator(seed, **params)
    hop = _hop(name)
    voc = ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(g), {"generator_params": params, "hop_size": hop},
                                                 device="cuda")
    g.remove_weight_norm()
    gen = torch.Generator().manual_seed(seed)
    A = g.aux_channels
    cs = [torch.randn(T, A, generator=gen) for T in _lens(name)]
    xs = [torch.randn(T * hop, generator=gen) for T in _lens(name)]
    with torch.no_grad():
        ref = [g.inference(c, x) for c, x in zip(cs, xs)]
    return g, voc, cs, xs, ref


@functools.lru_cache(maxsize=None)
def _emulated(name):
    g, _, cs, xs, _ = _case(name)
    with torch.no_grad(), bf16_emulation():
        return [g.inference(c, x) for c, x in zip(cs, xs)]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _run(name, prec, cs, xs):
    from crank_amd import ops

    voc = _case(name)[1]
    ops.set_precision(prec)
    try:
        out = voc.inference_batch(cs, xs)
        torch.cuda.synchronize()
    finally:
        ops.set_precision("bf16")
    return out


# ---- what each case reaches
def _reach(name):
    """Host-side assertions that the case reaches the edge its name gives."""
    params, _, _ = CASES[name]
    voc = _case(name)[1]
    hop, lens = _hop(name), _lens(name)
    bounds = np.cumsum(lens) * hop
    N = int(bounds[-1])
    assert 1 in lens and 2 in lens, lens
    if name in ("hop240", "hop30", "walk_small_hop300"):
        assert hop % TILE != 0 and any(b % TILE for b in bounds[:-1]), bounds  # an utterance edge inside a tile
    if name in ("hop240", "hop30"):
        assert N % TILE != 0, N  # a partial last tile
    if name.startswith("walk"):
        assert N > 2 * _n_cu() * WAVES * TILE, (N, _n_cu())
    if name.startswith("aux"):
        A = int(name[3:])
        assert voc.aux_channels == A and voc.params["aux_channels"] == A
        assert (A % 16 != 0) == (A in (1, 36, 127))  # zero-padded auxp channels, or none at the 128 limit
    if name.startswith("window"):
        w = int(name[6:])
        assert voc.params["aux_context_window"] == w
        assert w == 0 or 2 * w + 1 > min(lens) == 1  # replicate padding wider than a 1-frame utterance
    if name.startswith("layers"):
        L, S = params["layers"], params["stacks"]
        assert (voc.params["layers"], voc.params["stacks"]) == (L, S)
        if L == 30:
            assert 2 ** (L // S - 1) > N  # dilation longer than any utterance
    if name.startswith("scales"):
        sc = params["upsample_params"]["upsample_scales"]
        assert voc.scales == sc and (1 in sc or 16 in sc or len(sc) == 8)


@pytest.mark.parametrize("name", list(CASES))
def test_aux_path_alone_matches_fp32_restatement(name):
    _reach(name)
    g, voc, cs, _, _ = _case(name)
    got = voc.upsample_batch(cs)
    torch.cuda.synchronize()
    hop = _hop(name)
    for c, u in zip(cs, got):
        with torch.no_grad():
            r = g.upsample_aux(c)
        assert u.shape == r.shape
        assert _rel(u, r) <= 1e-5, (len(c), _rel(u, r))
        assert _rel(u[:hop], r[:hop]) <= 1e-5 and _rel(u[-hop:], r[-hop:]) <= 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_bf16x3_waveform_within_1e3_of_fp32(name):
    _reach(name)
    _, _, cs, xs, ref = _case(name)
    got = _run(name, "bf16x3", cs, xs)
    for T, y, r in zip(_lens(name), got, ref):
        assert y.shape == (T * _hop(name),)
        assert _rel(y, r) <= 1e-3, (T, _rel(y, r))


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_waveform_error_within_twice_the_emulation_error(name):
    _reach(name)
    _, _, cs, xs, ref = _case(name)
    got = _run(name, "bf16", cs, xs)
    for T, y, r, e in zip(_lens(name), got, ref, _emulated(name)):
        assert torch.isfinite(y).all()
        assert _rel(y, r) <= 2 * _rel(e, r), (T, _rel(y, r), _rel(e, r))


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["hop240", "hop30", "walk_small_hop300", "walk_default_hop256", "window5", "layers1"])
def test_ragged_batch_is_bit_identical_alone_and_reordered(name, prec):
    _reach(name)
    _, _, cs, xs, _ = _case(name)
    batch = _run(name, prec, cs, xs)
    alone = [_run(name, prec, [c], [x])[0] for c, x in zip(cs, xs)]
    order = list(range(len(cs)))[::-1]
    order = order[1:] + order[:1]  # reversed, then rotated: no utterance keeps its place or its offset
    shuffled = _run(name, prec, [cs[i] for i in order], [xs[i] for i in order])
    for i in range(len(cs)):
        assert torch.equal(batch[i], alone[i]), i
        assert torch.equal(batch[order[i]], shuffled[i]), i


@pytest.mark.parametrize("name", ["hop240", "walk_small_hop300"])
def test_bf16x3f_is_bit_identical_to_bf16x3(name):
    _, _, cs, xs, _ = _case(name)
    a = _run(name, "bf16x3", cs, xs)
    b = _run(name, "bf16x3f", cs, xs)
    plain = _run(name, "bf16", cs, xs)
    assert not all(torch.equal(x, y) for x, y in zip(a, plain))  # the flag is on in both
    for x, y in zip(a, b):
        assert torch.equal(x, y)
