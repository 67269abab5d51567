"""The per-layer fallback kernels (conv_tile_kernel, the table weight-gradient kernel: what runs for shapes the
fused stack / chain kernels refuse, and under CRK_NO_FUSE=1) against the fused kernels on the same weights and
inputs: generator with all four gated stacks, the 1x1 chains and the conditioning input (bf16x3), and three of its stacks
on their own (both arithmetics: through the quantizers 0.8 % of the codes of a plain-bf16 forward differ between the
families - bf16 noise on a nearest-neighbour search - and the decoder then sees other inputs, decoded 7.8e-2 / gradients
2.4e-1 in relative L2, which says nothing about a kernel); the gated discriminator, without
dropout and - the two families hash (seed, layer, frame * 64 + channel) alike, so under one seed they draw one mask - with
dropout 0.25; the plain conv chains (whose per-layer path, fwd_chain_layers / bwd_chain_layers, only the switch reaches),
at 90 frames and at 150 (a full tile and a ragged one).

In bf16x3 both families are ~fp32 accurate: every tensor within 1e-3 in the max norm and in relative L2.  In plain bf16 the
two families round the same operands but sum in other orders: every tensor within the bar _check_split_forward
(test_gpu_nets.py) sets for gradients of one arithmetic computed two ways, relative L2 < 5e-2 and cosine > 0.998.

tests/test_gpu_per_layer.py runs the per-layer kernels where they run on their own, against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import REPO

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import sys, torch, numpy as np
sys.path.insert(0, %r)
from crank_amd import ops
from crank_amd.bin.train import get_model
from crank_amd.net.module.pwg import ParallelWaveGANDiscriminator, ResidualParallelWaveGANDiscriminator
from crank_amd.utils import load_yaml
from tests.helpers import fill_models, make_batch
from tests.test_gpu_nets import _GenStack
out = {}
for prec in ("bf16x3", "bf16"):
    ops.set_precision(prec)
    gen = torch.Generator().manual_seed(2)
    if prec == "bf16x3":
        conf = load_yaml(None, batch_size=2, batch_len=96)
        G = get_model(conf, 3, "cuda")["G"].train()
        fill_models({"G": G})
        b = make_batch(2, 96, 3, device="cuda", seed=5)
        dec_h = torch.cat([b["lcf0"], b["uv"]], -1)
        h = b["org_h"].clone(); h[:, :] = h[:, 0:1]
        x = b["in_feats"].clone().requires_grad_(True)
        o = G(x, None, dec_h, spkrvec=h, use_ema=False)
        (o["decoded"] * torch.randn(o["decoded"].shape, generator=gen).cuda()).sum().backward()
        torch.cuda.synchronize()
        out[prec + ":G_decoded"], out[prec + ":G_dx"], out[prec + ":G_gp"] = o["decoded"].detach().cpu().numpy(), x.grad.cpu().numpy(), G.grad_flat.cpu().numpy()
        out[prec + ":G_qidx"] = torch.stack(o["qidx"]).cpu().numpy()
    # G's gated stacks on their own (no quantizer between them)
    for name, cfg in [("dec0", dict(in_channels=128, out_channels=80, kernel_size=5, layers=8, stacks=4, aux_channels=34)),
                      ("enc0", dict(in_channels=80, out_channels=64, kernel_size=5, layers=8, stacks=4, aux_channels=0)),
                      ("enc1", dict(in_channels=64, out_channels=64, kernel_size=3, layers=6, stacks=3, aux_channels=0))]:
        S = _GenStack(**cfg)
        fill_models({name: S})
        xx = torch.randn(2, cfg["in_channels"], 96, generator=gen).cuda().requires_grad_(True)
        cc = torch.randn(2, cfg["aux_channels"], 96, generator=gen).cuda().requires_grad_(True) if cfg["aux_channels"] else None
        y = S(xx, cc)
        (y * torch.randn(y.shape, generator=gen).cuda()).sum().backward()
        torch.cuda.synchronize()
        out[prec + ":" + name + "_y"], out[prec + ":" + name + "_dx"], out[prec + ":" + name + "_gp"] = y.detach().cpu().numpy(), xx.grad.cpu().numpy(), S.grad_flat.cpu().numpy()
        if cc is not None:
            out[prec + ":" + name + "_dc"] = cc.grad.cpu().numpy()
    chain = dict(conv_channels=64)
    for name, net, cin, T in [("D", ResidualParallelWaveGANDiscriminator(in_channels=37, out_channels=1, kernel_size=5, layers=4, stacks=2, dropout=0.0), 37, 90),
                              ("Ddrop", ResidualParallelWaveGANDiscriminator(in_channels=37, out_channels=1, kernel_size=5, layers=4, stacks=2, dropout=0.25), 37, 90),
                              ("C", ParallelWaveGANDiscriminator(in_channels=20, out_channels=6, kernel_size=3, layers=4), 20, 90),
                              ("C_T150", ParallelWaveGANDiscriminator(in_channels=20, out_channels=6, kernel_size=3, layers=4), 20, 150),
                              ("spkr_T150", ParallelWaveGANDiscriminator(in_channels=80, out_channels=14, kernel_size=5, layers=8, **chain), 80, 150),
                              ("adv_T150", ParallelWaveGANDiscriminator(in_channels=128, out_channels=14, kernel_size=3, layers=3, **chain), 128, 150)]:
        fill_models({name: net})
        xx = torch.randn(2, cin, T, generator=gen).cuda().requires_grad_(True)
        if name == "Ddrop":
            net.stack.net.reseed(7)
        y = net(xx)
        (y * torch.randn(y.shape, generator=gen).cuda()).sum().backward()
        torch.cuda.synchronize()
        out[prec + ":" + name + "_y"], out[prec + ":" + name + "_dx"], out[prec + ":" + name + "_gp"] = y.detach().cpu().numpy(), xx.grad.cpu().numpy(), net.grad_flat.cpu().numpy()
ops.set_precision("bf16")
np.savez(sys.argv[1], **out)
"""


def test_per_layer_fallback_kernels_agree_with_the_fused_ones(tmp_path):
    outs = {}
    for mode in ("0", "1"):
        f = tmp_path / f"nofuse{mode}.npz"
        r = subprocess.run([sys.executable, "-c", _SCRIPT % REPO, str(f)], env=dict(os.environ, CRK_NO_FUSE=mode),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[mode] = np.load(f)
    bad = {}
    for k in outs["0"].files:
        prec, name = k.split(":")
        a, b = outs["0"][k], outs["1"][k]
        if name == "G_qidx":
            same = float((a == b).mean())
            print(k, "equal codes", same)
            assert same > 0.999
            continue
        assert np.isfinite(b).all(), k
        a64, b64 = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
        err = float(np.abs(a - b).max() / (np.abs(a).max() + 1e-30))
        rl2 = float(np.linalg.norm(b64 - a64) / (np.linalg.norm(a64) + 1e-30))
        cos = float(a64 @ b64 / (np.linalg.norm(a64) * np.linalg.norm(b64) + 1e-30))
        print(f"{k}: max norm {err:.2e} relative L2 {rl2:.2e} cosine {cos:.6f}")
        if prec == "bf16x3":
            if not (err < 1e-3 and rl2 < 1e-3):
                bad[k] = (err, rl2)
        elif not (rl2 < 5e-2 and cos > 0.998):
            bad[k] = (rl2, cos)
    assert not bad, bad
