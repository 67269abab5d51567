"""The speaker table's gradient from per-utterance sums (crk_net_backward_embed; ops.concat_embed_owned, switch
cfg.cond_sums) against the per-frame path it replaces on the training step (crk_net_backward's dc, then crk_embed_bwd_run).

The two paths share every launch of the forward and every gradient except the table's, so everything but the table must
agree to the bit.  The table's gradient is the same sum in another order: over the frames of an utterance first (the bf16
dG planes, fp32, inside stack_wgrad_kernel), then through Waux^T (fp32), against Waux^T per frame (bf16 MFMA, fp32
accumulate) and then over frames.  Both are compared with a float64 sum over frames of the per-frame path's dc."""
import numpy as np
import pytest
import torch

from tests.helpers import fill_models, make_batch
from crank_amd.utils import load_yaml

pytestmark = pytest.mark.gpu

MODES = ["bf16", "bf16x3f", "bf16x3"]


def _rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _conf(blocks):
    """The default generator; blocks = 6: a last decoder of 3 x 2 gated blocks, whose weight-gradient groups (256 / 6 = 42 >
    32 groups of whole utterances) begin and end inside utterances."""
    conf = load_yaml(None)
    if blocks == 6:
        conf["n_layers_stacks"] = [3] + list(conf["n_layers_stacks"][1:])
    assert conf["n_layers"][0] * conf["n_layers_stacks"][0] == blocks
    return conf


def _run(conf, B, T, S, mode, owned, labels="stride0", seed=5):
    """One forward / backward of VQVAE2 on seeded inputs.  owned: the switch.  Returns forward values, the whole flat
    gradient, the table's slice of it, the per-frame conditioning gradient where that path produced one, and whether the
    decoder's net op owned the table gradient."""
    from crank_amd import ops
    from crank_amd.config import override
    from crank_amd.net.module.vqvae2 import VQVAE2

    ops.set_precision(mode)
    try:
        torch.manual_seed(7)
        prod = VQVAE2(conf, spkr_size=S).train()
        fill_models({"G": prod})
        batch = make_batch(B, T, S, seed=seed, device="cuda")
        x = batch["in_feats"]
        base = batch["org_h"].clone()
        base[:, :] = base[:, 0:1]
        h = base[:, 0:1].expand(-1, T) if labels == "stride0" else base
        seen = {}
        orig = prod._get_dec_h

        def spy(dec_h, spkrvec):
            out = orig(dec_h, spkrvec)
            seen["owned"] = getattr(out, "_crk_embed", None) is not None
            if out.requires_grad:
                out.register_hook(lambda g: seen.__setitem__("dc", g.detach().clone()))
            return out

        prod._get_dec_h = spy
        w = torch.from_numpy(np.random.RandomState(0).standard_normal((B, T, conf["output_size"])).astype(np.float32)).cuda()
        with override(cond_sums=owned):
            po = prod(x, None, (batch["lcf0"], batch["uv"]), spkrvec=h, use_ema=False)
            prod.zero_grad()
            loss = (po["decoded"] * w).sum() + sum(((po["encoded"][n] - po["emb_idx"][n].detach()) ** 2).mean() for n in range(2))
            loss.backward()
            if hasattr(prod, "finish_grads"):
                prod.finish_grads()
        torch.cuda.synchronize()
        o, E = prod.emb_offset, prod.emb_size
        flat = prod.grad_flat.detach().cpu().numpy().copy()
        return {
            "fwd": [po["decoded"].detach().cpu().numpy()] + [e.detach().cpu().numpy() for e in po["encoded"]]
                   + [q.cpu().numpy() for q in po["qidx"]],
            "flat": flat, "table": flat[o: o + S * E].reshape(S, E).copy(), "span": (o, o + S * E),
            "dc": seen.get("dc"), "owned": seen["owned"], "labels": base[:, 0].cpu().numpy(), "c0": 2,
        }
    finally:
        ops.set_precision("bf16")


def _table_f64(run, S, E):
    """float64 sum over frames of the per-frame conditioning gradient, per speaker."""
    dc = run["dc"].cpu().numpy().astype(np.float64)[..., run["c0"]: run["c0"] + E].sum(axis=1)  # [B, E]
    ref = np.zeros((S, E))
    for u, r in enumerate(run["labels"]):
        ref[int(r)] += dc[u]
    return ref


CASES = [
    # (blocks, B, T, speakers)
    (8, 64, 500, 14),    # the benchmark's shape: 32 groups of two whole utterances
    (8, 64, 500, 100),   # ... at the recipe's 100 speakers
    (6, 64, 500, 14),    # 40 groups of 13 chunks: groups begin and end inside utterances
    (6, 5, 333, 14),     # T not a multiple of 64; 30 chunks over 42 slots: every chunk its own group, 6 segments an utterance
    (8, 3, 140, 3),      # T not a multiple of 64, whole utterances per group
    (8, 65, 193, 14),    # cond_embed_bwd_kernel gathers the utterance list in passes of 64: two passes, the second of one utterance
    (8, 129, 100, 14),   # three passes
]
# fp32 reassociation over <= 500 frames x 8 blocks.  The assertion is 4x (rounded up) the largest value measured in each
# arithmetic, see the docstring below; a difference above 1e-4 would not be reassociation and needs an explanation.
BOUND = {"bf16": 1.5e-6, "bf16x3f": 1.5e-6, "bf16x3": 1.6e-5}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocks,B,T,S", CASES)
def test_table_gradient_from_sums_equals_the_per_frame_one(mode, blocks, B, T, S):
    """Measured on an MI355X, relative L2 over the whole table gradient (|gradient| 1.3e2 ... 1.3e3), every case of CASES:

        arithmetic   frame path vs f64   sums path vs f64      sums vs frame path
        bf16         1.0e-7 ... 1.5e-7   2.2e-7 ... 2.7e-7     2.4e-7 ... 3.2e-7
        bf16x3f      1.1e-7 ... 1.5e-7   2.1e-7 ... 2.7e-7     2.3e-7 ... 3.1e-7
        bf16x3       1.1e-7 ... 1.5e-7   2.8e-6 ... 3.9e-6     2.8e-6 ... 3.9e-6

    (f64 = the float64 sum over frames of the per-frame path's dc.)  The largest value of each arithmetic is the case of
    3 utterances x 140 frames or of 5 x 333 in six segments each; 64 x 500 gives 2.7e-7 / 3.0e-7 / 3.1e-6 at 14 speakers
    and the same at 100.  The two cases that take two and three passes of cond_embed_bwd_kernel's utterance list (65 x 193,
    129 x 100; added after the table) sit at its lower end: frame path 9.9e-8 ... 1.1e-7, sums path 2.2e-7 / 2.2e-7 /
    2.6e-6, sums vs frame 2.3e-7 ... 2.5e-7 and 2.6e-6.  In bf16x3 the sums path multiplies (Waux_hi + Waux_lo) by the fp32 sum of dG_hi + dG_lo, which
    contains the lo x lo products the chain's three MFMAs (hi.hi + lo.hi + hi.lo) leave out - 2^-18 of a product at most,
    the size of the difference; the float64 reference is built from the chain's dc and inherits its omission.  Against the
    fp32 oracle the table's gradient sits at 1.4e-5 of scale (test_sums_path_parameter_gradients_vs_oracle_bf16x3), inside
    the 6e-5 ... 7e-5 of the worst parameter gradient."""
    conf = _conf(blocks)
    E = conf["spkr_embedding_size"]
    old = _run(conf, B, T, S, mode, owned=False)
    new = _run(conf, B, T, S, mode, owned=True)
    assert not old["owned"] and old["dc"] is not None
    assert new["owned"] and new["dc"] is None, "the decoder's net op did not take the table gradient"
    # forward values and every other gradient: the same launches, bit for bit
    for a, b in zip(old["fwd"], new["fwd"]):
        assert np.array_equal(a, b)
    lo, hi = old["span"]
    assert np.array_equal(old["flat"][:lo], new["flat"][:lo]) and np.array_equal(old["flat"][hi:], new["flat"][hi:])
    ref = _table_f64(old, S, E)
    e_old, e_new, e_pair = _rel_l2(old["table"], ref), _rel_l2(new["table"], ref), _rel_l2(new["table"], old["table"])
    print(f"cond_sums {mode} blocks {blocks} B {B} T {T} S {S}: rel L2 vs float64 frame sum: frame path {e_old:.3e}, "
          f"sums path {e_new:.3e}; sums vs frame {e_pair:.3e}; |table grad| {np.linalg.norm(ref):.3e}")
    assert np.linalg.norm(ref) > 0
    # rows of speakers without an utterance stay untouched
    absent = sorted(set(range(S)) - set(int(r) for r in new["labels"]))
    assert not np.any(new["table"][absent])
    bound = BOUND[mode]
    assert bound is not None and bound <= 1e-4
    assert e_pair <= bound and e_new <= bound, (e_pair, e_new, bound)


@pytest.mark.parametrize("mode", MODES)
def test_per_frame_labels_keep_the_per_frame_path(mode):
    """A filled contiguous label tensor (run = 1, as _vqvae2_vs_oracle passes it) is not one label per utterance as far as
    the library can tell: the per-frame path runs with the switch on, and gives what it gives with the switch off."""
    conf = _conf(8)
    a = _run(conf, 4, 200, 5, mode, owned=True, labels="filled")
    b = _run(conf, 4, 200, 5, mode, owned=False, labels="filled")
    c = _run(conf, 4, 200, 5, mode, owned=False, labels="stride0")
    assert not a["owned"] and a["dc"] is not None
    for other in (b, c):
        assert np.array_equal(a["flat"], other["flat"])
        for x, y in zip(a["fwd"], other["fwd"]):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("S", [3, 100])
def test_sums_path_parameter_gradients_vs_oracle_bf16x3(S):
    """The bar of test_vqvae2_forward_backward_vs_oracle (every G parameter gradient within 1e-3 of OracleVQVAE2, bf16x3)
    with one label per utterance as the trainers pass it, so that the table's gradient comes from the sums."""
    from crank_amd import ops
    from crank_amd.net.module.vqvae2 import VQVAE2
    from oracle.modules import OracleVQVAE2

    ops.set_precision("bf16x3")
    try:
        conf = load_yaml(None)
        B, T = 2, 140
        orac = OracleVQVAE2(conf, spkr_size=S).train()
        prod = VQVAE2(conf, spkr_size=S).train()
        fill_models({"G": orac})
        fill_models({"G": prod})
        batch = make_batch(B, T, S, seed=5)
        x = batch["in_feats"]
        dec_h = torch.cat([batch["lcf0"], batch["uv"]], -1)
        h = batch["org_h"].clone()
        h[:, :] = h[:, 0:1]
        hg = batch["org_h"].cuda().contiguous()[:, 0:1].expand(-1, T)
        seen = {}
        orig = prod._get_dec_h
        prod._get_dec_h = lambda d, s: seen.setdefault("out", orig(d, s))
        oo = orac(x, None, dec_h, spkrvec=h, use_ema=False)
        po = prod(x.cuda(), None, dec_h.cuda(), spkrvec=hg, use_ema=False)
        assert getattr(seen["out"], "_crk_embed", None) is not None, "the sums path did not run"
        w = torch.from_numpy(np.random.RandomState(0).standard_normal((B, T, 80)).astype(np.float32))

        def objective(o, wt):
            return (o["decoded"] * wt).sum() + sum(((o["encoded"][n] - o["emb_idx"][n].detach()) ** 2).mean() for n in range(2))

        objective(oo, w).backward()
        prod.zero_grad()
        objective(po, w.cuda()).backward()
        torch.cuda.synchronize()
        worst, table = ("", 0.0), None
        for k, p in orac.named_parameters():
            if p.grad is None:
                continue
            a, b = prod.grad_view(k).cpu().numpy().astype(np.float64), p.grad.numpy().astype(np.float64)
            e = np.abs(a - b).max() / (np.abs(b).max() + 1e-12)
            if "spkr_embedding" in k:
                table = e
            if e > worst[1]:
                worst = (k, e)
        print("cond_sums vs oracle, bf16x3,", S, "speakers: worst G parameter-gradient error", worst, "| speaker table", table)
        assert table is not None
        assert worst[1] < 1e-3, worst
    finally:
        ops.set_precision("bf16")


@pytest.mark.parametrize("ttype,extra,steps", [
    ("vqvae", {}, 5),
    ("cyclegan", {"use_cyclic_training": True, "n_steps_cycle_start": 0, "n_steps_gan_start": 0}, 12),
])
def test_sums_path_replayed_from_a_graph_equals_eager_bit_for_bit(ttype, extra, steps, monkeypatch):
    """The trainers' steps with the table gradient from the sums: enqueued eagerly and replayed from captured graphs, the
    loss values of every step, the parameters and the codebooks at the end agree to the bit."""
    from crank_amd import ops
    from tests.test_gpu_step import _assert_same_run, _run_steps

    ops.set_precision("bf16")
    calls = []
    real = ops.concat_embed_owned
    monkeypatch.setattr(ops, "concat_embed_owned", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    conf = load_yaml(None, batch_size=4, batch_len=160, trainer_type=ttype, **extra)
    shapes = [(4, 160)] * steps
    eager = _run_steps(dict(conf), 14, False, shapes)
    assert calls, "the steps did not take the sums path"
    graphed = _run_steps(dict(conf, hip_graph=True), 14, True, shapes)
    tr = graphed[3]
    assert tr._graphs and any(slot[1] is not None for slot in tr._graphs.values()), "no step was captured"
    _assert_same_run(eager, graphed, exact=True)
