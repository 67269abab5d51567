"""Host restatement of the kernels' dropout mask, and the oracle evaluated under that mask.

The HIP stack kernels never store a keep mask: every kernel that needs it (forward, data gradient, weight gradient, of
every kernel family) regenerates it from dropout_scale(layer_seed(seed, layer), frame * 64 + channel, p) of
crank_amd/csrc/common.h, each from its own lane layout.  The mask is a pure integer hash, so it is restated here in numpy
- unsigned integers up to the final compare - and handed to the oracle's ResidualBlock through oracle.pwg.dropout_hook:
every oracle comparison then becomes a comparison under dropout, at the tolerances of the dropout-free one.

  keep_mask(seed, layer, B, T, channels, p)  bool (B, channels, T): hash32, dropout_scale, layer_seed (net.hip)
  seed_sequence(start, n)                    the seeds crk_seed_next hands to n consecutive forward calls after reseed(start)
  keep_scale(p)                              the fp32 value 1 / (1 - p) a kept element is multiplied by
  masked(orac, masks, ...)                   context manager: block `l` of `orac` multiplies its input by masks[l] * scale
"""
import contextlib

import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)
GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def _hash32(x):
    """common.h hash32 on uint64 arrays that hold 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def layer_seed(seed, layer):
    """net.hip layer_seed: seed + GOLDEN * (layer + 1) modulo 2^64 (python ints)."""
    return (int(seed) + GOLDEN * (int(layer) + 1)) & _M64


def threshold(p):
    """common.h: (uint32_t)(p * 65536.f + 0.5f) - round(p * 65536) for every p a config uses."""
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    assert thr == int(round(float(p) * 65536)), (p, thr)
    return thr


def keep_scale(p):
    """common.h: 1.f / (1.f - p) in fp32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def element_bits(seed, idx):
    """The 16 bits dropout_scale compares with the threshold, for element indices `idx` (uint64 array) under the 64-bit
    `seed` (already layer_seed'ed): four consecutive elements share two hashes and take one half each."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & _M64
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    quad = idx >> np.uint64(2)
    ln = idx & np.uint64(3)
    q32 = (quad ^ (quad >> np.uint64(32))) & _M32
    h = _hash32((((q32 * np.uint64(0x9E3779B9)) & _M32) + lo) & _M32)
    h = _hash32(h ^ hi)
    h2 = _hash32((h + np.uint64(0x68BC21EB)) & _M32)
    w = np.where((ln & np.uint64(2)) != 0, h2, h)
    return np.where((ln & np.uint64(1)) != 0, w >> np.uint64(16), w & np.uint64(0xFFFF))


def keep_mask(seed, layer, B, T, channels=64, p=0.25):
    """bool (B, channels, T): element (b, c, t) of block `layer`'s input is kept.  Element index (b * T + t) * channels + c:
    the kernels' (global frame) * 64 + channel."""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    c = np.arange(channels, dtype=np.uint64)[None, :, None]
    t = np.arange(T, dtype=np.uint64)[None, None, :]
    idx = (b * np.uint64(T) + t) * np.uint64(channels) + c
    return element_bits(layer_seed(seed, layer), idx) >= np.uint64(threshold(p))


def seed_sequence(start, n):
    """net.hip seed_next_kernel: splitmix64 of a Weyl sequence from `start`, cut to 62 bits."""
    out, state = [], int(start) & _M64
    for _ in range(n):
        state = (state + GOLDEN) & _M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        out.append((z ^ (z >> 31)) & 0x3FFFFFFFFFFFFFFF)
    return out


def layer_masks(seed, layers, B, T, p, channels=64):
    return [keep_mask(seed, l, B, T, channels, p) for l in range(layers)]


def _blocks(orac):
    from oracle import pwg as opwg

    return [m for m in orac.modules() if isinstance(m, opwg.ResidualBlock)]


@contextlib.contextmanager
def masked(orac, masks, p=None, scale=None, wgrad_undropped=False):
    """Under this context block `l` of `orac` (its ResidualBlocks in order: layers are counted per forward call) multiplies
    its input by masks[l] * scale in fp32 instead of calling F.dropout.  scale defaults to keep_scale(p).  It composes with
    oracle.pwg.bf16_emulation: the product is formed before the dilated conv rounds its operand.

    wgrad_undropped=True is a deliberately WRONG oracle (tests/test_dropout_cpu.py measures that the GPU bounds tell it
    apart): values and data gradients as above, the dilated conv's weight and bias gradients taken on the undropped input."""
    from oracle import pwg as opwg

    blocks = _blocks(orac)
    assert len(masks) == len(blocks), (len(masks), len(blocks))
    s = float(keep_scale(p) if scale is None else np.float32(scale))
    mult = {id(b): torch.from_numpy(np.asarray(m, dtype=np.float32) * np.float32(s)) for b, m in zip(blocks, masks)}

    def hook(block, x):
        m = mult[id(block)]
        assert tuple(m.shape) == tuple(x.shape) and x.dtype == torch.float32, (m.shape, x.shape, x.dtype)
        block._undropped = x
        return x * m

    def wrong_conv(block):
        conv = block.conv

        def forward(xm):
            b = conv.bias
            good = conv.conv_with(xm, conv.weight.detach(), None if b is None else b.detach())  # value, dx
            bad = conv.conv_with(block._undropped.detach(), conv.weight, b)  # weight / bias gradient only
            return good + (bad - bad.detach())

        return forward

    try:
        if wgrad_undropped:
            for b in blocks:
                b.conv.forward = wrong_conv(b)
        with opwg.dropout_hook(hook):
            yield
    finally:
        for b in blocks:
            b.conv.__dict__.pop("forward", None)
            b.__dict__.pop("_undropped", None)


# ---- perturbed masks: what a subtly wrong kernel would draw -----------------------------------------------------------
def flip_one(masks, layer, b, c, t):
    out = [m.copy() for m in masks]
    out[layer][b, c, t] ^= True
    return out


def shift_layers(masks, extra):
    """block l takes block l + 1's mask (`extra`: the mask of the block after the last one)."""
    return [m.copy() for m in masks[1:]] + [extra]


def permute_quads(masks):
    """channels rotated by one inside each quad: lane j takes lane (j + 1) % 4's bit."""
    C = masks[0].shape[1]
    perm = np.arange(C).reshape(-1, 4)[:, [1, 2, 3, 0]].reshape(-1)
    return [m[:, perm].copy() for m in masks]
