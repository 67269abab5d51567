"""The speaker-adversarial net's and the speaker classifier's updates as one set of launches (config.cfg.overlap_c = 3,
VQVAETrainer.update_speaker_nets): the two updates read nothing of each other, so every value of the step is the one the
separate updates (overlap_c = 0) compute, to the bit.  Below that, the launches that serve several nets at once against
the single-net launches: the plain convs' weight gradients on their per-group partial sums, Adam over several blocks."""
import ctypes

import pytest
import torch

from tests.helpers import fill_models, make_batch
from crank_amd.utils import load_yaml

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- trainer level
def _run_trainer(conf, n_spkrs, B, T, mode, monkeypatch, wrap_step_of=None):
    """(state, losses, joint calls) of three eager steps, the capture of the step and two replays in mode `mode`."""
    from crank_amd import config
    from crank_amd.bin.train import build_trainer
    from crank_amd.net.trainer.trainer_vqvae import VQVAETrainer

    monkeypatch.setattr(config.cfg, "overlap_c", mode)
    calls = []
    joint = VQVAETrainer.update_speaker_nets
    monkeypatch.setattr(VQVAETrainer, "update_speaker_nets", lambda self, *a, **k: (calls.append(1), joint(self, *a, **k))[1])
    torch.manual_seed(7)
    trainer = build_trainer(conf, n_spkrs, "/tmp/crank_amd_speaker_nets_joint")
    fill_models(trainer.model)
    trainer.steps = 1
    trainer.check_custom_start()
    for opt in trainer.optimizer.values():
        opt.clear_grads = False
    seen = []
    if wrap_step_of:  # a caller with a hook in front of the update, the way tests/helpers.py looks at the gradients there
        opt, real = trainer.optimizer[wrap_step_of], trainer.optimizer[wrap_step_of].step
        opt.step = lambda *a, **k: (seen.append(1), real(*a, **k))[1]
    if mode == 3:  # in line: no second stream, so a captured step is a single chain without a fork or a join
        assert trainer._classifier_stream(make_batch(B, T, n_spkrs, seed=50, device="cuda"), "train") is None
    losses = []
    for step in range(6):  # (three eager steps, the capture, replays)
        batch = make_batch(B, T, n_spkrs, seed=50 + step, device="cuda", full_length=True)
        v = trainer.train_graphed(batch)
        losses.append({k: float(x) for k, x in v.items()})
    torch.cuda.synchronize()
    assert any(slot[1] is not None for slot in trainer._graphs.values()), "no step was captured"
    assert getattr(trainer, "_c_stream", None) is None
    state = {k: (m.grad_flat.clone(), m.flat.detach().clone(), trainer.optimizer[k].exp_avg.clone(),
                 trainer.optimizer[k].exp_avg_sq.clone(), trainer.optimizer[k].step_dev.clone())
             for k, m in trainer.model.items()}
    qs = trainer.model["G"].quantizers
    state["ema"] = (torch.cat([q.ema_size for q in qs]), torch.cat([q.weight.reshape(-1) for q in qs]),
                    torch.cat([q.ema_w.reshape(-1) for q in qs]))
    monkeypatch.setattr(VQVAETrainer, "update_speaker_nets", joint)
    assert not wrap_step_of or len(seen) >= 4, seen  # the wrapper ran: in the three eager steps and in the capture
    return state, losses, len(calls)


def _assert_same(a, la, b, lb):
    assert la == lb, (la, lb)
    assert set(a) == set(b)
    for k in a:
        names = ("codebook sizes", "codebooks", "EMA sums") if k == "ema" else ("gradients", "parameters", "exp_avg", "exp_avg_sq", "step count")
        for i, what in enumerate(names):
            assert torch.equal(a[k][i], b[k][i]), f"{what} of {k} differ: {float((a[k][i] - b[k][i]).abs().max())}"
        if k != "ema":
            assert a[k][0].abs().max() > 0, f"{k}: no gradient"


_TRAINERS = {
    "vqvae": dict(trainer_type="vqvae"),
    "vqvae_cyclic": dict(trainer_type="vqvae", use_cyclic_training=True, n_steps_cycle_start=0),  # C is read by G's update
    "lsgan": dict(trainer_type="lsgan", n_steps_gan_start=0),
}


@pytest.mark.parametrize("shape", [(4, 160, 5), (3, 97, 14)], ids=["B4_T160_S5", "B3_T97_S14"])
@pytest.mark.parametrize("kind", list(_TRAINERS))
def test_joint_speaker_updates_leave_every_value_unchanged(kind, shape, monkeypatch):
    """Mode 3 against mode 0: parameters, gradients, Adam moments and step counts of every model, codebooks, EMA sums and
    sizes and every loss value, over three eager steps, a captured step and its replays.  (3, 97, 14): T is no multiple
    of the 64-frame chunk and a weight-gradient group crosses an utterance boundary."""
    from crank_amd import ops

    ops.set_precision("bf16")
    B, T, S = shape
    conf = load_yaml(None, batch_size=B, batch_len=T, hip_graph=True, **_TRAINERS[kind])
    assert conf["use_spkr_classifier"] and conf["use_spkradv_training"]
    a, la, joint_a = _run_trainer(conf, S, B, T, 3, monkeypatch)
    b, lb, joint_b = _run_trainer(conf, S, B, T, 0, monkeypatch)
    assert joint_a > 0 and joint_b == 0, (joint_a, joint_b)
    _assert_same(a, la, b, lb)


@pytest.mark.parametrize("case", ["clip_C", "clip_SPKRADV", "radam_C", "radam_SPKRADV", "wrapped_C"])
def test_joint_speaker_updates_fall_back_to_the_separate_ones(case, monkeypatch):
    """Gradient clipping on one model, an optimizer that is not FlatAdam, or one whose step() a caller has wrapped: mode 3
    takes the separate updates (the wrapper runs) and still matches mode 0."""
    from crank_amd import ops

    ops.set_precision("bf16")
    what, name = case.split("_")
    conf = load_yaml(None, batch_size=4, batch_len=160, hip_graph=True, trainer_type="vqvae")
    if what == "clip":
        conf["optim"][name]["clip_grad_norm"] = 0.5
    elif what == "radam":
        conf["optim"][name]["type"] = "radam"
    wrap = name if what == "wrapped" else None
    a, la, joint_a = _run_trainer(conf, 5, 4, 160, 3, monkeypatch, wrap_step_of=wrap)
    b, lb, joint_b = _run_trainer(conf, 5, 4, 160, 0, monkeypatch, wrap_step_of=wrap)
    assert joint_a == 0 and joint_b == 0, (joint_a, joint_b)
    _assert_same(a, la, b, lb)


# ----------------------------------------------------------------------------------------------------- kernel level
_BASE = dict(kind=2, stacks=1, res_ch=64, gate_ch=128, skip_ch=64, aux_ch=0, conv_ch=64, causal=0, use_bias=1, slope=0.2, dropout=0.0)
_ADV = dict(_BASE, in_ch=128, out_ch=14, kernel_size=3, layers=3)  # 24 tiles a conv at most: six per wave, 64 groups
_CLS = dict(_BASE, in_ch=80, out_ch=14, kernel_size=5, layers=8)   # 30 tiles in the first conv (eight per wave), 20 after; 32 groups
_DEFER_WNORM = 8


def _chain_backward(L, net, d, B, T, seed, flags):
    """One forward and one backward of a plain net on seeded data; (gradient block, what must outlive a deferred launch)."""
    from crank_amd._lib import ptr, stream_ptr

    N = B * T
    g = torch.Generator().manual_seed(seed)
    params = (0.1 * torch.randn(net.n_params, generator=g)).abs().add_(0.05).cuda()
    x = torch.randn(N, d["in_ch"], generator=g).cuda()
    dy = torch.randn(N, d["out_ch"], generator=g).cuda()
    y = torch.empty(N, d["out_ch"], device="cuda")
    grads = torch.zeros_like(params)
    assert L.crk_net_reserve(net.handle, B, T) == 0
    saved = torch.empty(L.crk_net_saved_bytes(net.handle, B, T) // 4 + 1, device="cuda")
    assert L.crk_net_forward(net.handle, ptr(params), 1, ptr(x), d["in_ch"], None, 0, ptr(y), d["out_ch"], ptr(saved), B, T, 0, 0,
                             stream_ptr()) == 0
    assert L.crk_net_backward(net.handle, ptr(params), 1, ptr(grads), ptr(x), d["in_ch"], None, 0, ptr(dy), d["out_ch"], None, 0,
                              1.0, None, 0, ptr(saved), B, T, flags, 0, stream_ptr()) == 0
    return grads, (params, x, dy, y, saved)


def _partials(L, net, B, T):
    from crank_amd._lib import ptr, stream_ptr

    n = L.crk_debug_net_partials(net.handle, B, T, None, 0, stream_ptr())
    assert n > 0
    out = torch.empty(n, device="cuda")
    assert L.crk_debug_net_partials(net.handle, B, T, ptr(out), n, stream_ptr()) == n
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", [(3, 97), (9, 450)], ids=["B3_T97", "B9_T450"])
def test_weight_gradients_of_two_plain_nets_in_one_launch_match_the_single_net_launches(shape):
    """A 3-conv k = 3 net (64 groups) and an 8-conv k = 5 net (32 groups) whose backward calls deferred their weight
    gradients, finished by ONE crk_nets_wnorm_bwd: the per-group partial sums and the gradients equal, bit for bit, those
    of each net finishing alone (the single-net launch).  (3, 97): six chunks, one per group in both nets, T no multiple of
    64; (9, 450): 72 chunks - 36 groups of two against 24 groups of three, so the two nets differ in depth, taps, tile
    count AND group count inside the grid, and groups cross utterance boundaries."""
    from crank_amd import _lib, ops
    from crank_amd._lib import stream_ptr

    ops.set_precision("bf16")
    L = _lib.lib()
    B, T = shape
    nets = [(ops.HipNet(**d), d) for d in (_ADV, _CLS)]
    assert all(L.crk_debug_net_paths(n.handle, B, T) & 8 for n, _ in nets), "the chains do not run fused"
    alone = []
    for i, (net, d) in enumerate(nets):  # each net on its own: weight gradients in the backward call, its own launch
        grads, keep = _chain_backward(L, net, d, B, T, 11 + i, 0)
        alone.append((_partials(L, net, B, T), grads.clone()))
        del keep
    for i, (net, d) in enumerate(nets):  # ... and deferred and finished alone: still the single-net launch
        grads, keep = _chain_backward(L, net, d, B, T, 11 + i, _DEFER_WNORM)
        assert L.crk_nets_wnorm_bwd(1, (ctypes.c_void_p * 1)(net.handle), stream_ptr()) == 0
        assert torch.equal(_partials(L, net, B, T), alone[i][0]) and torch.equal(grads, alone[i][1])
        del keep
    for order in ((0, 1), (1, 0)):
        out = {}
        for i in order:
            net, d = nets[i]
            out[i] = _chain_backward(L, net, d, B, T, 11 + i, _DEFER_WNORM)
            assert float(out[i][0].abs().max()) == 0.0, "a deferred backward wrote parameter gradients"
        arr = (ctypes.c_void_p * 2)(*[nets[i][0].handle for i in order])
        assert L.crk_nets_wnorm_bwd(2, arr, stream_ptr()) == 0
        for i in order:
            p = _partials(L, nets[i][0], B, T)
            assert p.numel() == alone[i][0].numel()
            assert torch.equal(p, alone[i][0]), f"net {i}, order {order}: partial sums differ in {int((p != alone[i][0]).sum())} places"
            assert torch.equal(out[i][0], alone[i][1]), f"net {i}, order {order}: gradients differ"
            assert float(out[i][0].abs().max()) > 0


def test_adam_over_three_blocks_in_one_launch_matches_three_launches():
    """crk_adam_step_multi over blocks of 5, 4096 and 40 003 elements (one short workgroup; whole workgroups; a tail) with
    their own lr and step counts against crk_adam_step per block: parameters, cleared gradients and both moments to the
    bit, over two steps, and every step count advanced once per step - by the call, or (clear_grads bit 1) left alone."""
    from crank_amd import ops

    sizes, lrs, steps0 = (5, 4096, 40003), (1e-3, 2e-4, 5e-2), (0.0, 7.0, 123.0)
    g = torch.Generator().manual_seed(3)

    def blocks():
        out = []
        for n, lr, st in zip(sizes, lrs, steps0):
            gg = torch.Generator().manual_seed(n)
            out.append([torch.randn(n, generator=gg).cuda(), torch.randn(n, generator=gg).cuda(), torch.zeros(n, device="cuda"),
                        torch.zeros(n, device="cuda"), torch.tensor([lr], device="cuda"), torch.tensor([st], device="cuda")])
        return out

    for clear in (True, False):
        one, many = blocks(), blocks()
        for step in range(2):
            fresh = [torch.randn(n, generator=g).cuda() for n in sizes]
            for b, m, f in zip(one, many, fresh):
                if step:
                    b[1].copy_(f); m[1].copy_(f)
                ops.adam_step(*b, clear_grads=clear)
            ops.adam_step_multi([tuple(m) for m in many], clear_grads=clear)
            torch.cuda.synchronize()
            for i, (b, m) in enumerate(zip(one, many)):
                for j, what in enumerate(("parameters", "gradients", "exp_avg", "exp_avg_sq", "lr", "step count")):
                    assert torch.equal(b[j], m[j]), f"block {i} ({sizes[i]}), step {step}: {what} differ"
                assert float(m[5]) == steps0[i] + step + 1
                assert float(m[1].abs().max()) == 0.0 if clear else float(m[1].abs().max()) > 0
        ops.adam_step_multi([tuple(m) for m in many], clear_grads=clear, defer_bump=True)
        torch.cuda.synchronize()
        assert [float(m[5]) for m in many] == [s + 2 for s in steps0]


def test_step_counts_of_two_models_advance_in_the_preparation_launch():
    """crk_nets_prepare_models over the nets of two models: each net prepared for its own model's version (a second call
    with the same versions launches nothing and advances nothing twice), both step counts advanced once."""
    from crank_amd import _lib, ops
    from crank_amd._lib import ptr, stream_ptr

    ops.set_precision("bf16")
    L = _lib.lib()
    nets = [ops.HipNet(**d) for d in (_ADV, _CLS)]
    params = [(0.1 * torch.randn(n.n_params, generator=torch.Generator().manual_seed(5))).abs().add_(0.05).cuda() for n in nets]
    steps = [torch.tensor([3.0], device="cuda"), torch.tensor([9.0], device="cuda")]
    ops.nets_prepare_models(nets, [ptr(p) for p in params], [4, 17], steps)
    torch.cuda.synchronize()
    assert [float(s) for s in steps] == [4.0, 10.0]
    # the prepared planes serve a forward at those versions: same output as a net prepared by its own first call
    B, T = 2, 70
    for net, d, p, ver in zip(nets, (_ADV, _CLS), params, (4, 17)):
        ref = ops.HipNet(**d)
        x = torch.randn(B * T, d["in_ch"], generator=torch.Generator().manual_seed(6)).cuda()
        ys = []
        for h in (net, ref):
            assert L.crk_net_reserve(h.handle, B, T) == 0
            y = torch.empty(B * T, d["out_ch"], device="cuda")
            assert L.crk_net_forward(h.handle, ptr(p), ver, ptr(x), d["in_ch"], None, 0, ptr(y), d["out_ch"], None, B, T, 4, 0,
                                     stream_ptr()) == 0
            ys.append(y)
        torch.cuda.synchronize()
        assert torch.equal(ys[0], ys[1])
    ops.nets_prepare_models(nets, [ptr(p) for p in params], [4, 17], steps)  # nothing to prepare: the counts still advance
    torch.cuda.synchronize()
    assert [float(s) for s in steps] == [5.0, 11.0]
