"""Streaming conversion on the GPU (crank_amd.stream.StreamingConverter, csrc/stream_kernels.hip): chunk invariance and
stream independence bit for bit, the offline forwards (CPU oracle fp32, the package's own bf16x3), the exact search's
indices, reset, parameter / codebook updates, graph capture, the configurations off the default and the refused shapes.
Inputs: tests/stream_inputs.py (S = 3 streams of T = 150 frames, more than the 132-frame receptive chain)."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import stream_inputs as SI
from tests.helpers import REPO

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = 12345.0, -7  # what output rows past n_valid must still hold after a push
T, S = SI.T, SI.S


def build_model(fx):
    from crank_amd.net.module.vqvae2 import VQVAE2

    G = VQVAE2(fx.conf, spkr_size=SI.N_SPK).eval()
    G.load_state_dict(fx.state)
    return G


class Dev:
    """A fixture's inputs on the device and a generator holding its parameters (built once per configuration)."""

    _made = {}

    def __init__(self, fx):
        self.fx, self.G = fx, build_model(fx)
        self.x, self.lcf0, self.uv, self.spk = fx.x.cuda(), fx.lcf0.cuda(), fx.uv.cuda(), fx.spk.cuda()
        self.enc_cond = None if fx.enc_cond is None else fx.enc_cond.cuda()
        self._base = None

    @classmethod
    def of(cls, **over):
        fx = SI.fixture(**over)
        if id(fx) not in cls._made:
            cls._made[id(fx)] = cls(fx)
        return cls._made[id(fx)]

    def converter(self, n_streams, max_chunk, G=None):
        from crank_amd.stream import StreamingConverter

        return StreamingConverter(self.G if G is None else G, n_streams, max_chunk)

    def baseline(self):
        """All three streams pushed 40 frames at a time: what every other schedule must reproduce."""
        if self._base is None:
            self._base = run(self.converter(S, 64), self, [(c,) * S for c in SI.SCHEDULES["c40"]], range(S))
        return self._base


def run(conv, dev, plan, rows, start=None):
    """plan: per push, the frames each converter row takes (0: the row sits the push out); rows: the fixture stream feeding
    each row; start: the first frame of each row (default 0).  Returns per row {"decoded", "qidx", "encoded"} of its
    frames in order, after checking that no push wrote an output row at or past n_valid."""
    rows = list(rows)
    R, nst = len(rows), dev.fx.nst
    at = [0] * R if start is None else list(start)
    got = [dict(decoded=[], qidx=[[] for _ in range(nst)], encoded=[[] for _ in range(nst)]) for _ in rows]
    spk = dev.spk[rows].contiguous()
    clean = torch.ones((), dtype=torch.bool, device="cuda")
    for counts in plan:
        C = max(counts)
        if C == 0:
            continue
        feats = torch.zeros(R, C, dev.x.shape[-1], device="cuda")
        lcf0, uv = torch.zeros(R, C, 1, device="cuda"), torch.zeros(R, C, 1, device="cuda")
        econd = None if dev.enc_cond is None else torch.zeros(R, C, 2, device="cuda")
        for r, (s, c) in enumerate(zip(rows, counts)):
            feats[r, :c], lcf0[r, :c], uv[r, :c] = dev.x[s, at[r]: at[r] + c], dev.lcf0[s, at[r]: at[r] + c], dev.uv[s, at[r]: at[r] + c]
            if econd is not None:
                econd[r, :c] = dev.enc_cond[s, at[r]: at[r] + c]
        out = conv.empty_outputs(R, C)
        out["decoded"].fill_(SENT_F)
        for n in range(nst):
            out["qidx"][n].fill_(SENT_I)
            out["encoded"][n].fill_(SENT_F)
        res = conv.push(feats, lcf0, uv, spk, n_valid=torch.tensor(counts, device="cuda"), enc_lcf0_uv=econd, out=out)
        assert res is out
        for r, c in enumerate(counts):
            clean &= (out["decoded"][r, c:] == SENT_F).all()
            got[r]["decoded"].append(out["decoded"][r, :c])
            for n in range(nst):
                clean &= (out["qidx"][n][r, c:] == SENT_I).all() & (out["encoded"][n][r, c:] == SENT_F).all()
                got[r]["qidx"][n].append(out["qidx"][n][r, :c])
                got[r]["encoded"][n].append(out["encoded"][n][r, :c])
            at[r] += c
    assert bool(clean), "a push wrote output rows at or past n_valid"
    return [dict(decoded=torch.cat(g["decoded"]), qidx=[torch.cat(q) for q in g["qidx"]],
                 encoded=[torch.cat(e) for e in g["encoded"]]) for g in got]


def same(a, b, lo=0, hi=None):
    """Bit for bit: a's frames against b's frames [lo, hi)."""
    sl = slice(lo, hi)
    return (torch.equal(a["decoded"], b["decoded"][sl]) and all(torch.equal(p, q[sl]) for p, q in zip(a["qidx"], b["qidx"]))
            and all(torch.equal(p, q[sl]) for p, q in zip(a["encoded"], b["encoded"])))


def rel_err(got, ref, keep):
    """Largest difference on the kept frames relative to the reference's largest value: the golden-vector tests' measure."""
    keep = torch.as_tensor(keep)
    return float((got - ref)[keep].abs().max()) / float(ref.abs().max())


def check_offline(res, ref, fx, what):
    """res: run()'s result for the three streams; ref: an offline forward's dict.  qidx identical on every kept frame,
    decoded within 1e-3 on the kept frames; returns the measured decoded error."""
    assert fx.left_out <= SI.MAX_LEFT_OUT
    for n in range(fx.nst):
        q = torch.stack([r["qidx"][n] for r in res]).cpu()
        keep = torch.as_tensor(fx.keep_q[n])
        differ = int((q != ref["qidx"][n].cpu())[keep].sum())
        assert differ == 0, (what, n, differ)
    err = rel_err(torch.stack([r["decoded"] for r in res]).cpu(), ref["decoded"].cpu(), fx.keep_dec)
    print(f"{what}: decoded max |diff| / max |ref| = {err:.3e} on {int(fx.keep_dec.sum())} frames")
    assert err <= 1e-3, (what, err)
    return err


def offline_gpu(dev):
    """The package's own offline forward (what trainer.eval runs) in bf16x3 on the fixture."""
    from crank_amd import ops

    dec_h, h = dev.fx.dec_cond()
    ops.set_precision("bf16x3")
    try:
        with torch.no_grad():
            out = dev.G(dev.x, dev.enc_cond, None if dec_h is None else dec_h.cuda(), spkrvec=None if h is None else h.cuda(),
                        use_ema=False)
        torch.cuda.synchronize()
    finally:
        ops.set_precision("bf16")
    return out


# ---------------------------------------------------------------------------------------------------- 1 chunk invariance
def test_outputs_do_not_depend_on_the_chunk_schedule():
    dev = Dev.of()
    conv = dev.converter(1, 160)
    res = {}
    for name, sched in SI.SCHEDULES.items():
        conv.reset()
        res[name] = run(conv, dev, [(c,) for c in sched], [0])[0]
        assert res[name]["decoded"].shape == (T, dev.fx.conf["output_size"])
    for name in SI.SCHEDULES:
        assert same(res[name], res["whole"]), name
    assert same(res["whole"], dev.baseline()[0])  # ... nor on the converter's width or the stream's row


@pytest.mark.parametrize("sched", [[64, 64, 22], [17] * 8 + [14]])
def test_full_tile_and_one_frame_past_a_run(sched):
    """C = max_chunk = 64 exactly (a whole LDS tile) and C = 17 (two eight-frame runs of a thread and one frame)."""
    dev = Dev.of()
    conv = dev.converter(S, 64)
    res = run(conv, dev, [(c,) * S for c in sched], range(S))
    assert all(same(res[s], dev.baseline()[s]) for s in range(S))


# ---------------------------------------------------------------------------------------------------- 2 independence
_RAGGED = [(5, 0, 12, 1), (16, 3, 0), (7, 7, 40, 0, 2)]  # frames per push of each stream, repeated


def _ragged_plan():
    pats = _RAGGED
    left, plan, i = [T] * S, [], 0
    while any(left):
        counts = tuple(min(pats[s][i % len(pats[s])], left[s]) for s in range(S))
        left = [l - c for l, c in zip(left, counts)]
        plan.append(counts)
        i += 1
    return plan


def test_streams_are_independent_and_rows_past_n_valid_are_untouched():
    dev = Dev.of()
    plan = _ragged_plan()
    assert any(0 in p and max(p) > 0 for p in plan) and len({p for p in plan}) > 4
    last = [[p[s] for p in plan if p[s]][-1] for s in range(S)]
    assert any(last[s] not in pats for s, pats in enumerate(_RAGGED))  # a stream's last push is cut short
    together = run(dev.converter(S, 64), dev, plan, range(S))
    for s in range(S):
        alone = run(dev.converter(1, 64), dev, [(p[s],) for p in plan], [s])[0]
        assert same(together[s], alone), s
        assert same(together[s], dev.baseline()[s]), s
    # rows in another order, another speaker per row: a row's result follows its inputs only
    swapped = run(dev.converter(S, 64), dev, [(c,) * S for c in SI.SCHEDULES["c16"]], [2, 0, 1])
    assert same(swapped[0], dev.baseline()[2]) and same(swapped[1], dev.baseline()[0]) and same(swapped[2], dev.baseline()[1])


# ---------------------------------------------------------------------------------------------------- 3 offline
def test_streaming_equals_the_offline_forwards():
    """Against the oracle's causal forward on the CPU (fp32) and the package's offline GPU forward in bf16x3: identical
    indices on every frame the oracle's margins keep, decoded within 1e-3.
    Measured on the MI355X, all 450 frames kept: 5.1e-7 against the oracle, 1.6e-5 against bf16x3."""
    dev = Dev.of()
    check_offline(dev.baseline(), dev.fx.ref, dev.fx, "streaming vs CPU oracle fp32")
    check_offline(dev.baseline(), offline_gpu(dev), dev.fx, "streaming vs offline GPU bf16x3")
    for n in range(dev.fx.nst):
        enc = torch.stack([r["encoded"][n] for r in dev.baseline()]).cpu()
        assert rel_err(enc, dev.fx.ref["encoded"][n], np.ones((S, T), bool)) <= 1e-3


# ---------------------------------------------------------------------------------------------------- 4 exact search
def test_indices_are_the_exact_searchs_with_ties_to_the_first_index():
    from crank_amd import ops

    dev = Dev.of()
    fx = dev.fx
    G = build_model(fx)
    used = np.bincount(fx.ref["qidx"][0].numpy().reshape(-1), minlength=fx.conf["emb_size"][0])
    K = len(used)
    order = [int(k) for k in np.argsort(-used) if 0 < k < K - 1]
    a, b = order[0], order[1]
    assert used[a] > 0 and used[b] > 0
    with torch.no_grad():
        w = G.quantizers[0].weight
        w[K - 1] = w[a]  # a copy behind the code: the code itself must win
        w[0] = w[b]      # a copy in front of it: the copy must win
    G.touch_codebook()
    res = run(dev.converter(S, 64, G=G), dev, [(c,) * S for c in SI.SCHEDULES["c40"]], range(S))
    q0 = torch.stack([r["qidx"][0] for r in res])
    assert int((q0 == a).sum()) > 0 and int((q0 == K - 1).sum()) == 0
    assert int((q0 == 0).sum()) > 0 and int((q0 == b).sum()) == 0
    for n in range(fx.nst):
        enc = torch.stack([r["encoded"][n] for r in res]).contiguous()
        e, qx, idx = ops.vq_apply(enc, G.quantizers[n].weight)
        assert torch.equal(idx, torch.stack([r["qidx"][n] for r in res])), n


# ---------------------------------------------------------------------------------------------------- 5 reset
def test_reset_restarts_one_stream_and_leaves_the_others():
    dev = Dev.of()
    conv = dev.converter(S, 64)
    run(conv, dev, [(40,) * S], range(S))
    conv.reset([1])
    res = run(conv, dev, [(40,) * S], range(S), start=[40, 0, 40])
    base = dev.baseline()
    assert same(res[1], base[1], 0, 40)
    assert same(res[0], base[0], 40, 80) and same(res[2], base[2], 40, 80)
    conv.reset()
    assert all(same(r, b, 0, 40) for r, b in zip(run(conv, dev, [(40,) * S], range(S)), base))


# ---------------------------------------------------------------------------------------------------- 6 updates
def test_parameter_and_codebook_updates_are_followed():
    dev = Dev.of()
    G = build_model(dev.fx)
    conv = dev.converter(S, 64, G=G)
    first = run(conv, dev, [(16,) * S], range(S))
    assert same(first[0], dev.baseline()[0], 0, 16)
    with torch.no_grad():
        G.flat.data[: G.quantizers[0].cb_offset].mul_(1.02)  # every conv parameter, in place
    G.touch()
    conv.reset()
    after = run(conv, dev, [(16,) * S], range(S))
    fresh = run(dev.converter(S, 64, G=G), dev, [(16,) * S], range(S))
    assert all(same(a, f) for a, f in zip(after, fresh)) and not torch.equal(after[0]["decoded"], first[0]["decoded"])
    with torch.no_grad():
        G.quantizers[0].weight.mul_(1.05)
    G.touch_codebook()
    conv.reset()
    after2 = run(conv, dev, [(16,) * S], range(S))
    fresh2 = run(dev.converter(S, 64, G=G), dev, [(16,) * S], range(S))
    assert all(same(a, f) for a, f in zip(after2, fresh2)) and not torch.equal(after2[0]["decoded"], after[0]["decoded"])


# ---------------------------------------------------------------------------------------------------- 7 capture
def capture_and_replay(dev, warm):
    """Two streams, 16 frames per push: one push captured on static buffers and replayed over 5 chunks against the eager
    run; returns (replayed results, eager results, allocations by the library, bytes by torch) - the last two across
    every push after the reserve."""
    from crank_amd import _lib

    R, C, nch = 2, 16, 5
    conv = dev.converter(R, C)
    st = dict(feats=torch.zeros(R, C, dev.x.shape[-1], device="cuda"), lcf0=torch.zeros(R, C, 1, device="cuda"),
              uv=torch.zeros(R, C, 1, device="cuda"), spk=dev.spk[:R].contiguous(), out=conv.empty_outputs(R, C))
    if warm:
        conv.push(st["feats"], st["lcf0"], st["uv"], st["spk"], out=st["out"])
        conv.reset()
    torch.cuda.synchronize()
    allocs0, bytes0 = _lib.lib().crk_debug_alloc_count(), None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        conv.push(st["feats"], st["lcf0"], st["uv"], st["spk"], out=st["out"])
    conv.reset()  # (a capture runs nothing; the state is still zero - this only says so)
    torch.cuda.synchronize()
    bytes0 = torch.cuda.memory_allocated()
    replayed = [dict(decoded=[], qidx=[[] for _ in range(dev.fx.nst)], encoded=[[] for _ in range(dev.fx.nst)]) for _ in range(R)]
    keep = []
    for i in range(nch):
        st["feats"].copy_(dev.x[:R, i * C: (i + 1) * C])
        st["lcf0"].copy_(dev.lcf0[:R, i * C: (i + 1) * C])
        st["uv"].copy_(dev.uv[:R, i * C: (i + 1) * C])
        graph.replay()
        if i == 0:
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - bytes0
        keep.append({k: (v.clone() if k == "decoded" else [t.clone() for t in v]) for k, v in st["out"].items()})
    torch.cuda.synchronize()
    allocs = _lib.lib().crk_debug_alloc_count() - allocs0
    for r in range(R):
        replayed[r] = dict(decoded=torch.cat([k["decoded"][r] for k in keep]),
                           qidx=[torch.cat([k["qidx"][n][r] for k in keep]) for n in range(dev.fx.nst)],
                           encoded=[torch.cat([k["encoded"][n][r] for k in keep]) for n in range(dev.fx.nst)])
    eager = run(dev.converter(R, C), dev, [(C,) * R] * nch, range(R))
    return replayed, eager, allocs, grown


def test_push_is_capturable_and_allocates_nothing():
    dev = Dev.of()
    replayed, eager, allocs, grown = capture_and_replay(dev, warm=True)
    assert all(same(a, b) for a, b in zip(replayed, eager))
    assert all(same(a, b, 0, 80) for a, b in zip(eager, dev.baseline()))
    assert allocs == 0 and grown == 0, (allocs, grown)


def test_capture_as_a_process_first_push():
    """The same capture in a child process that has launched nothing of this family before it."""
    r = subprocess.run([sys.executable, "-m", "tests.stream_capture_child"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stream capture ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------- 8 other shapes
@pytest.mark.parametrize("name", sorted(SI.VARIANTS))
def test_configurations_off_the_default(name):
    """Each: one stream frame by frame against three streams 16 frames at a time, bit for bit; then the oracle's offline
    forward (fp32) and the package's offline GPU forward (bf16x3) under the same rules as the default shapes."""
    dev = Dev.of(**SI.VARIANTS[name])
    by16 = run(dev.converter(S, 64), dev, [(c,) * S for c in SI.SCHEDULES["c16"]], range(S))
    by1 = run(dev.converter(1, 64), dev, [(1,)] * T, [0])[0]
    assert same(by1, by16[0])
    check_offline(by16, dev.fx.ref, dev.fx, f"{name}: streaming vs CPU oracle fp32")
    check_offline(by16, offline_gpu(dev), dev.fx, f"{name}: streaming vs offline GPU bf16x3")


# ---------------------------------------------------------------------------------------------------- 9 refusals
def test_refused_shapes_return_status_3_without_a_launch():
    from crank_amd import _lib
    from crank_amd._lib import check

    L = _lib.lib()
    dev = Dev.of()
    conv = dev.converter(2, 64)
    conv._prepare()
    nst = dev.fx.nst

    def push(R, C):
        out = conv.empty_outputs(R, C)
        out["decoded"].fill_(SENT_F)
        feats = torch.zeros(R, C, dev.x.shape[-1], device="cuda")
        cond = torch.zeros(R, C, 2, device="cuda")
        ptrs = ctypes.c_void_p * nst
        rc = L.crk_stream_push(conv._handle, feats.data_ptr(), feats.shape[-1], cond.data_ptr(), 2, None, 2,
                               torch.zeros(R, dtype=torch.int64, device="cuda").data_ptr(), None, R, C,
                               out["decoded"].data_ptr(), ptrs(*[t.data_ptr() for t in out["qidx"]]),
                               ptrs(*[t.data_ptr() for t in out["encoded"]]), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    for R, C in ((2, 65), (3, 16), (2, 0), (0, 16)):
        rc, out = push(R, C)
        assert rc == 3, (R, C, rc)
        assert bool((out["decoded"] == SENT_F).all())
        with pytest.raises(RuntimeError, match="unsupported"):
            check(rc, "crk_stream_push")
    rc, out = push(2, 64)
    assert rc == 0 and not bool((out["decoded"] == SENT_F).any())
    assert L.crk_stream_reserve(conv._handle, 0, 64) == 3 and L.crk_stream_reserve(conv._handle, 2, 0) == 3
    # a descriptor the kernel does not take: refused at creation
    G = dev.G
    for field, value in (("emb_dim", 48), ("causal", 0), ("n_stacks", 4), ("in_ch", 200)):
        d = _lib.StreamDesc()
        d.n_stacks, d.in_ch, d.out_ch = nst, dev.fx.conf["input_size"], dev.fx.conf["output_size"]
        for n in range(nst):
            d.emb_dim[n], d.emb_size[n], d.cb_off[n] = 64, 512, G.quantizers[n].cb_offset
            d.enc_base[n], d.dec_base[n] = G.encoders[n].base, G.decoders[n].base
        d.causal, d.enc_f0, d.dec_f0, d.spk_dim, d.spk_onehot, d.n_spk, d.spk_off = 1, 0, 1, 32, 0, SI.N_SPK, G.emb_offset
        if field == "emb_dim":
            d.emb_dim[0] = value
        else:
            setattr(d, field, value)
        nets = ctypes.c_void_p * 3
        enc = nets(*([G.encoders[n].net.handle for n in range(nst)] + [None] * (3 - nst)))
        dec = nets(*([G.decoders[n].net.handle for n in range(nst)] + [None] * (3 - nst)))
        h = ctypes.c_void_p()
        assert L.crk_stream_create(ctypes.byref(d), enc, dec, ctypes.byref(h)) == 3, field
        assert not h.value


# ---------------------------------------------------------------------------------------------------- 10 one argument path
def _family(kind):
    """(the family's Dev of its small configuration - k333 causal, SMALL behind a look-ahead -, its converter class)."""
    from crank_amd.stream import LookaheadConverter, StreamingConverter
    from tests import stream_la_inputs as LI
    from tests.test_gpu_stream_la import LaDev

    if kind == "causal":
        return Dev.of(**SI.VARIANTS["k333"]), StreamingConverter
    return LaDev.of(**LI.SMALL), LookaheadConverter


_BAD_S, _BAD_C = 2, 3
_BAD_ARGS = {  # case -> (configuration keys on top of the family's, the message)
    "feats_dtype": ({}, "feats: a float32 (2, 3, 80) tensor on the GPU, got torch.float64 (2, 3, 80) on cuda:0"),
    "feats_width": ({}, "feats: a float32 (2, 3, 80) tensor on the GPU, got torch.float32 (2, 3, 79) on cuda:0"),
    "spkr_shape": ({}, "spkr: an int64 (2,) tensor on the GPU, got torch.int64 (3,) on cuda:0"),
    "n_valid_on_host": ({}, "n_valid: an integer (2,) tensor on the GPU"),
    "both_f0_forms": ({}, "lcf0_uv: the packed rows replace lcf0 and uv; give one form, not both"),
    "lcf0_uv_without_decoder_f0": (dict(decoder_f0=False), "lcf0_uv: this model has decoder_f0 = false and takes no F0 rows"),
    "missing_enc_lcf0_uv": (dict(encoder_f0=True), "enc_lcf0_uv is required by this configuration"),
    "no_streams": ({}, "n_streams = 0, max_chunk = 3: both must be at least 1"),
}


@pytest.mark.parametrize("case", sorted(_BAD_ARGS))
@pytest.mark.parametrize("kind", ["causal", "lookahead"])
def test_both_converters_refuse_the_same_bad_arguments(kind, case):
    """The same ValueError, word for word, from either class, and nothing launched: the output buffers keep their fill."""
    from crank_amd.net.module.vqvae2 import VQVAE2

    dev, cls = _family(kind)
    over, message = _BAD_ARGS[case]
    assert dev.fx.conf["input_size"] == 80
    G = VQVAE2(dict(dev.fx.conf, **over), spkr_size=SI.N_SPK).eval() if over else dev.G
    if case == "no_streams":
        with pytest.raises(ValueError) as e:
            cls(G, 0, _BAD_C)
        assert str(e.value) == message
        return
    conv = cls(G, _BAD_S, _BAD_C)
    S, C = _BAD_S, _BAD_C
    z = lambda *shape, **kw: torch.zeros(*shape, device="cuda", **kw)  # noqa: E731
    args = dict(feats=z(S, C, 80), lcf0=z(S, C, 1), uv=z(S, C, 1), spkr=z(S, dtype=torch.int64))
    if case == "feats_dtype":
        args["feats"] = args["feats"].double()
    elif case == "feats_width":
        args["feats"] = z(S, C, 79)
    elif case == "spkr_shape":
        args["spkr"] = z(S + 1, dtype=torch.int64)
    elif case == "n_valid_on_host":
        args["n_valid"] = torch.full((S,), C, dtype=torch.int32)
    elif case == "both_f0_forms":
        args["lcf0_uv"] = z(S, C, 2)
    elif case == "lcf0_uv_without_decoder_f0":
        args.update(lcf0=None, uv=None, lcf0_uv=z(S, C, 2))
    out = conv.empty_outputs(S, C) if kind == "causal" else conv.empty_outputs(S)
    for t in [out["decoded"]] + out["qidx"] + out["encoded"]:
        t.fill_(SENT_I)
    with pytest.raises(ValueError) as e:
        conv.push(out=out, **args)
    assert str(e.value) == message
    torch.cuda.synchronize()
    assert all(bool((t == SENT_I).all()) for t in [out["decoded"]] + out["qidx"] + out["encoded"])


def test_a_reset_with_an_id_out_of_range_zeroes_nothing():
    """reset([0, n_streams]): RuntimeError, and stream 0 goes on as if nobody had asked - every id is checked before the
    first row is zeroed.  5 frames, the refused reset, 5 more, against a converter that was never reset, bit for bit."""
    dev, _ = _family("causal")
    plan = [(3, 3), (2, 2)]
    conv = dev.converter(2, 3)
    head = run(conv, dev, plan, range(2))
    with pytest.raises(RuntimeError):
        conv.reset([0, 2])
    rest = run(conv, dev, plan, range(2), start=[5, 5])
    whole = run(dev.converter(2, 3), dev, plan + plan, range(2))
    assert all(same(head[r], whole[r], 0, 5) and same(rest[r], whole[r], 5, 10) for r in range(2))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_a_converter_on_a_second_device_after_one_on_the_first():
    """The push kernel's dynamic-LDS limit is raised per reserve, on the device the converter lives on: a converter on
    cuda:1 works in a process whose first converter was made on cuda:0.  Both against tests/stream_ref.py's float64
    streaming reference under test_streaming_equals_the_offline_forwards' rules: identical indices, decoded and the
    quantizers' inputs within 1e-3 of the largest reference value."""
    from crank_amd.net.module.vqvae2 import VQVAE2
    from crank_amd.stream import StreamingConverter
    from tests.stream_ref import StreamRef

    dev, _ = _family("causal")
    fx, S2, C = dev.fx, 2, 3
    dec_h, h = fx.dec_cond()
    ref = []
    for s in range(S2):
        cond = torch.cat([dec_h[s, :C], fx.orac.spkr_embedding(h[s, :C]).detach()], -1)
        ref.append(StreamRef(fx.orac).push(fx.x[s, :C], cond))
    for name in ("cuda:0", "cuda:1"):
        with torch.cuda.device(name):
            G = VQVAE2(fx.conf, spkr_size=SI.N_SPK, device=name).eval()
            G.load_state_dict(fx.state)
            assert G.flat.device == torch.device(name)
            conv = StreamingConverter(G, S2, C, device=name)
            to = lambda t: t[:S2, :C].to(name).contiguous()  # noqa: E731
            out = conv.push(to(fx.x), to(fx.lcf0), to(fx.uv), fx.spk[:S2].to(name))
            torch.cuda.synchronize()
        for s in range(S2):
            d, q, e = ref[s]
            assert fx.keep_dec[s, :C].any()
            assert rel_err(out["decoded"][s].cpu().double(), d, fx.keep_dec[s, :C]) <= 1e-3, (name, s)
            for n in range(fx.nst):
                keep = torch.as_tensor(fx.keep_q[n][s, :C])
                assert torch.equal(out["qidx"][n][s].cpu()[keep], q[n][keep]), (name, s, n)
                assert rel_err(out["encoded"][n][s].cpu().double(), e[n], np.ones(C, bool)) <= 1e-3, (name, s, n)
