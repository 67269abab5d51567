"""Look-ahead streaming conversion on the GPU (crank_amd.stream.LookaheadConverter, csrc/stream_la_kernels.hip): a
non-causal generator followed at its look-ahead.  Chunk invariance, utterances back to back, stream independence and reset
bit for bit; the offline forwards of the whole utterances (CPU oracle fp32, the package's own bf16x3); the exact search's
indices; parameter / codebook updates; graph capture; the configurations off the default; the refused shapes.
Inputs: tests/stream_la_inputs.py (the fixtures of tests/stream_inputs.py with causal: false)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stream_la_inputs as LI
from tests.test_gpu_stream import SENT_F, SENT_I, Dev, build_model, offline_gpu, rel_err, same

pytestmark = pytest.mark.gpu

T, S = LI.T, LI.S
MIXED = (1, 7, 16, 2, 33, 1)


class LaDev(Dev):
    """A non-causal fixture's inputs on the device and a generator holding its parameters (once per configuration)."""

    _made = {}

    @classmethod
    def of(cls, **over):
        fx = LI.fixture(**over)
        if id(fx) not in cls._made:
            cls._made[id(fx)] = cls(fx)
        return cls._made[id(fx)]

    def converter(self, n_streams, max_chunk, G=None):
        from crank_amd.stream import LookaheadConverter

        return LookaheadConverter(self.G if G is None else G, n_streams, max_chunk)

    def baseline(self):
        """All three streams pushed 40 frames at a time, the end flag on the last push: what every schedule must reproduce."""
        if self._base is None:
            self._base = [u[0] for u in drive(self.converter(S, 64), self, range(S), whole_plan([40, 40, 40, 30], S))]
        return self._base


def cut(sizes, total):
    out, done, i = [], 0, 0
    while done < total:
        out.append(min(sizes[i % len(sizes)], total - done))
        done += out[-1]
        i += 1
    return out


def whole_plan(sizes, R, end_alone=False):
    """Every row takes `sizes` frames push by push; the end flag on the last push, or on a further one without frames."""
    plan = [((c, False),) * R for c in sizes]
    return plan + [((0, True),) * R] if end_alone else plan[:-1] + [((sizes[-1], True),) * R]


def drive(conv, dev, rows, plan, start=None, taken=None):
    """plan: per push, (frames, end) for each converter row; rows: the fixture stream feeding each row; start: the first
    frame of each row (default 0); taken: the frames each row's open utterance holds already (default 0).  Returns per row
    the list of its utterances, each {"decoded", "qidx", "encoded", "n"} (an utterance the plan leaves open comes last, with
    "open": True), after checking per push that ``first`` counts the frames the utterance has emitted, that ``n_out`` is max(0, T - LA) - emitted (everything left under the end flag) and
    that no output row at or past ``n_out`` was written."""
    rows = list(rows)
    R, nst, la = len(rows), dev.fx.nst, conv.lookahead
    at = [0] * R if start is None else list(start)
    spk = dev.spk[rows].contiguous()
    outs, clean = [], torch.ones((), dtype=torch.bool, device="cuda")
    past = torch.arange(conv.max_out, device="cuda")[None]
    for push in plan:
        counts = [c for c, _ in push]
        C = max(max(counts), 1)
        feats = torch.zeros(R, C, dev.x.shape[-1], device="cuda")
        lcf0, uv = torch.zeros(R, C, 1, device="cuda"), torch.zeros(R, C, 1, device="cuda")
        econd = None if dev.enc_cond is None else torch.zeros(R, C, 2, device="cuda")
        for r, (s, c) in enumerate(zip(rows, counts)):
            feats[r, :c], lcf0[r, :c], uv[r, :c] = dev.x[s, at[r]: at[r] + c], dev.lcf0[s, at[r]: at[r] + c], dev.uv[s, at[r]: at[r] + c]
            if econd is not None:
                econd[r, :c] = dev.enc_cond[s, at[r]: at[r] + c]
            at[r] += c
        out = conv.empty_outputs(R)
        out["decoded"].fill_(SENT_F)
        for n in range(nst):
            out["qidx"][n].fill_(SENT_I)
            out["encoded"][n].fill_(SENT_F)
        res = conv.push(feats, lcf0, uv, spk, n_valid=torch.tensor(counts, device="cuda"),
                        end=torch.tensor([int(e) for _, e in push], device="cuda"), enc_lcf0_uv=econd, out=out)
        assert res is out
        keep = past >= out["n_out"][:, None]  # (R, max_out): rows that must still hold the sentinel
        clean &= (out["decoded"] == SENT_F).all(-1)[keep].all()
        for n in range(nst):
            clean &= (out["qidx"][n] == SENT_I)[keep].all() & (out["encoded"][n] == SENT_F).all(-1)[keep].all()
        outs.append(out)
    assert bool(clean), "a push wrote output rows at or past n_out"
    n_out = torch.stack([o["n_out"] for o in outs]).cpu().numpy()
    first = torch.stack([o["first"] for o in outs]).cpu().numpy()
    result = []
    for r in range(R):
        utts, cur, held = [], [], 0 if taken is None else taken[r]
        emitted = max(0, held - la)
        for i, push in enumerate(plan):
            c, end = push[r]
            held += c
            want = held if end else max(0, held - la)
            assert first[i, r] == emitted and n_out[i, r] == want - emitted, (r, i, first[i, r], n_out[i, r], emitted, want)
            emitted = want
            cur.append((outs[i], int(n_out[i, r])))
            if end:
                utts.append(_gather(cur, r, nst, held))
                cur, held, emitted = [], 0, 0
        if held:
            utts.append(dict(_gather(cur, r, nst, held), open=True))
        result.append(utts)
    return result


def _gather(parts, r, nst, n):
    return dict(decoded=torch.cat([o["decoded"][r, :k] for o, k in parts]),
                qidx=[torch.cat([o["qidx"][m][r, :k] for o, k in parts]) for m in range(nst)],
                encoded=[torch.cat([o["encoded"][m][r, :k] for o, k in parts]) for m in range(nst)], n=n)


def check_offline(res, ref, fx, what):
    """res: one whole utterance per fixture stream; ref: an offline forward's dict.  qidx identical on every kept frame
    (the fixture keeps all of them), decoded within 1e-3 (max |diff| / max |ref|); returns the measured decoded error."""
    assert fx.left_out <= LI.MAX_LEFT_OUT
    for n in range(fx.nst):
        q = torch.stack([r["qidx"][n] for r in res]).cpu()
        differ = int((q != ref["qidx"][n].cpu())[torch.as_tensor(fx.keep_q[n])].sum())
        assert differ == 0, (what, n, differ)
    err = rel_err(torch.stack([r["decoded"] for r in res]).cpu(), ref["decoded"].cpu(), fx.keep_dec)
    print(f"{what}: decoded max |diff| / max |ref| = {err:.3e} on {int(fx.keep_dec.sum())} frames")
    assert err <= 1e-3, (what, err)
    return err


# ---------------------------------------------------------------------------------------------------- 1 small, back to back
UTTS = (40, 12, 5, 1)  # frames: longer than the look-ahead of 12, equal to it, shorter, one


def _back_to_back(chunking, end_alone):
    plan = []
    for n in UTTS:
        plan += whole_plan(chunking(n), 1, end_alone)
    return plan


def test_small_configuration_utterances_back_to_back():
    """One stream, utterances of 40, 12 (= LA), 5 and 1 frames back to back, pushed a frame at a time, as (1, 7, 16, 2, 33,
    1, ...), each in one push, and with the end flag alone on a push of no frames: equal decoded, encoded, qidx and totals
    of n_out; first counts up from 0 per utterance (drive checks it per push); each utterance within the bar of the
    oracle's offline forward of it alone, with its indices."""
    dev = LaDev.of(**LI.SMALL)
    fx = dev.fx
    conv = dev.converter(1, 40)
    assert conv.lookahead == 12 and conv.max_out == 52
    runs = {}
    for name, chunking, end_alone in (("c1", lambda n: [1] * n, False), ("mixed", lambda n: cut(MIXED, n), False),
                                      ("whole", lambda n: [n], False), ("whole, end alone", lambda n: [n], True),
                                      ("c1, end alone", lambda n: [1] * n, True)):
        runs[name] = drive(conv, dev, [0], _back_to_back(chunking, end_alone))[0]
        assert [u["n"] for u in runs[name]] == list(UTTS) and not any("open" in u for u in runs[name])
        assert [u["decoded"].shape[0] for u in runs[name]] == list(UTTS)
    for name, utts in runs.items():
        assert all(same(a, b) for a, b in zip(utts, runs["whole"])), name
    lo = 0
    for u, n in zip(runs["whole"], UTTS):
        want = fx.offline_part(fx.orac, 0, lo, lo + n)
        for m in range(fx.nst):
            assert float(LI.margins(want["encoded"][m][0].numpy(), fx.codebooks[m]).min()) > LI.MARGIN
            assert torch.equal(u["qidx"][m].cpu(), want["qidx"][m][0]), (n, m)
        err = rel_err(u["decoded"].cpu(), want["decoded"][0], np.ones(n, bool))
        print(f"small, utterance of {n} frames vs CPU oracle fp32: {err:.3e}")
        assert err <= 1e-3
        lo += n


# ---------------------------------------------------------------------------------------------------- 2 default shapes
def test_one_push_of_a_whole_utterance_and_the_mixed_schedule():
    """max_chunk 160: 150 frames and the 66-frame flush in one launch (tiles of 64 inside it, the flush crossing a tile),
    against the mixed schedule and the baseline (40 frames a push)."""
    dev = LaDev.of()
    conv = dev.converter(S, 160)
    assert conv.lookahead == 66 and conv.max_out == 226
    whole = [u[0] for u in drive(conv, dev, range(S), whole_plan([T], S))]
    mixed = [u[0] for u in drive(conv, dev, range(S), whole_plan(cut(MIXED, T), S))]
    alone = [u[0] for u in drive(conv, dev, range(S), whole_plan(cut(MIXED, T), S, end_alone=True))]
    for s in range(S):
        assert whole[s]["decoded"].shape == (T, dev.fx.conf["output_size"])
        assert same(whole[s], dev.baseline()[s]) and same(mixed[s], dev.baseline()[s]) and same(alone[s], dev.baseline()[s]), s


_RAGGED = [(5, 0, 12, 1), (16, 3, 0), (7, 7, 40, 0, 2)]  # frames per push of each stream, repeated


def _ragged_plan():
    left, plan, i = [T] * S, [], 0
    while any(left):
        counts = [min(_RAGGED[s][i % len(_RAGGED[s])], left[s]) for s in range(S)]
        left = [l - c for l, c in zip(left, counts)]
        plan.append(tuple((c, l == 0 and c > 0) for c, l in zip(counts, left)))
        i += 1
    return plan


def test_streams_are_independent_and_rows_past_n_out_are_untouched():
    dev = LaDev.of()
    plan = _ragged_plan()
    assert any(0 in [c for c, _ in p] and max(c for c, _ in p) > 0 for p in plan)
    last = [[p[s][0] for p in plan if p[s][0]][-1] for s in range(S)]
    assert any(last[s] not in pats for s, pats in enumerate(_RAGGED))  # a stream's last push is cut short
    together = drive(dev.converter(S, 64), dev, range(S), plan)
    for s in range(S):
        assert len(together[s]) == 1
        alone = drive(dev.converter(1, 64), dev, [s], [(p[s],) for p in plan])[0]
        assert same(together[s][0], alone[0]), s
        assert same(together[s][0], dev.baseline()[s]), s
    # rows in another order, another speaker per row: a row's result follows its inputs only
    swapped = [u[0] for u in drive(dev.converter(S, 64), dev, [2, 0, 1], whole_plan(cut([16], T), S))]
    assert same(swapped[0], dev.baseline()[2]) and same(swapped[1], dev.baseline()[0]) and same(swapped[2], dev.baseline()[1])


def test_reset_restarts_one_stream_mid_utterance_and_leaves_the_others():
    dev = LaDev.of()
    conv = dev.converter(S, 64)
    head = drive(conv, dev, range(S), [((40, False),) * S, ((40, False),) * S])  # 80 frames in, 14 out
    assert all(u[0]["decoded"].shape[0] == 14 for u in head)
    conv.reset([1])
    tail = drive(conv, dev, range(S), whole_plan([40, 30], S), start=[80, 0, 80], taken=[80, 0, 80])
    base = dev.baseline()
    # stream 1 started over: its 70 frames are an utterance of their own, NOT the baseline's first 70 (the end differs)
    fresh = drive(dev.converter(1, 64), dev, [1], whole_plan([40, 30], 1))[0][0]
    assert same(tail[1][0], fresh) and tail[1][0]["decoded"].shape[0] == 70
    for s in (0, 2):  # the others went on: what they emitted before and after the reset is the whole utterance
        assert same(head[s][0], base[s], 0, 14) and same(tail[s][0], base[s], 14, T), s
    conv.reset()
    again = [u[0] for u in drive(conv, dev, range(S), whole_plan([40, 40, 40, 30], S))]
    assert all(same(a, b) for a, b in zip(again, base))


# ---------------------------------------------------------------------------------------------------- 3 offline
def test_lookahead_streaming_equals_the_offline_forwards():
    """All 450 frames against the oracle's non-causal forward on the CPU (fp32) and the package's offline GPU forward in
    bf16x3: identical indices, decoded within 1e-3; the quantizers' inputs within the same bar of the oracle's.
    Measured on the MI355X: see DESIGN.md section 6n."""
    dev = LaDev.of()
    check_offline(dev.baseline(), dev.fx.ref, dev.fx, "look-ahead streaming vs CPU oracle fp32")
    check_offline(dev.baseline(), offline_gpu(dev), dev.fx, "look-ahead streaming vs offline GPU bf16x3")
    for n in range(dev.fx.nst):
        enc = torch.stack([r["encoded"][n] for r in dev.baseline()]).cpu()
        assert rel_err(enc, dev.fx.ref["encoded"][n], np.ones((S, T), bool)) <= 1e-3


_VARIANT_SCHEDULE = {"nvq1": [T], "nvq3": cut(MIXED, T), "encf0": cut([16], T), "onehot": cut([40], T), "k333": cut([3], T),
                     "dim32": cut([64], T), "mcep35": cut(MIXED[::-1], T)}


@pytest.mark.parametrize("name", sorted(LI.VARIANTS))
def test_configurations_off_the_default(name):
    """Each with one schedule: the oracle's offline forward (fp32) and the package's offline GPU forward (bf16x3) under
    the rules of the default shapes."""
    dev = LaDev.of(**LI.VARIANTS[name])
    sched = _VARIANT_SCHEDULE[name]
    res = [u[0] for u in drive(dev.converter(S, max(sched)), dev, range(S), whole_plan(sched, S))]
    check_offline(res, dev.fx.ref, dev.fx, f"{name}: look-ahead streaming vs CPU oracle fp32")
    check_offline(res, offline_gpu(dev), dev.fx, f"{name}: look-ahead streaming vs offline GPU bf16x3")


# ---------------------------------------------------------------------------------------------------- 4 robustness
def test_returned_indices_are_the_exact_searchs_on_the_returned_rows():
    from crank_amd import ops

    dev = LaDev.of()
    for n in range(dev.fx.nst):
        enc = torch.stack([r["encoded"][n] for r in dev.baseline()]).contiguous()
        _, _, idx = ops.vq_apply(enc, dev.G.quantizers[n].weight)
        assert torch.equal(idx, torch.stack([r["qidx"][n] for r in dev.baseline()])), n


def test_parameter_and_codebook_updates_are_followed():
    dev = LaDev.of(**LI.SMALL)
    G = build_model(dev.fx)
    conv = dev.converter(S, 64, G=G)
    plan = whole_plan([16, 14], S)
    first = [u[0] for u in drive(conv, dev, range(S), plan)]
    with torch.no_grad():
        G.flat.data[: G.quantizers[0].cb_offset].mul_(1.02)  # every conv parameter, in place
    G.touch()
    after = [u[0] for u in drive(conv, dev, range(S), plan)]
    fresh = [u[0] for u in drive(dev.converter(S, 64, G=G), dev, range(S), plan)]
    assert all(same(a, f) for a, f in zip(after, fresh)) and not torch.equal(after[0]["decoded"], first[0]["decoded"])
    with torch.no_grad():
        G.quantizers[0].weight.mul_(1.05)
    G.touch_codebook()
    after2 = [u[0] for u in drive(conv, dev, range(S), plan)]
    fresh2 = [u[0] for u in drive(dev.converter(S, 64, G=G), dev, range(S), plan)]
    assert all(same(a, f) for a, f in zip(after2, fresh2)) and not torch.equal(after2[0]["decoded"], after[0]["decoded"])


def test_push_is_capturable_and_allocates_nothing():
    """Two streams of the small configuration, 16 frames per push: one push captured on static buffers and replayed over
    five chunks, the fifth carrying the end flag (set in the static flag tensor), against the eager run."""
    from crank_amd import _lib

    dev = LaDev.of(**LI.SMALL)
    R, C, nch = 2, 16, 5
    conv = dev.converter(R, C)
    st = dict(feats=torch.zeros(R, C, dev.x.shape[-1], device="cuda"), lcf0=torch.zeros(R, C, 1, device="cuda"),
              uv=torch.zeros(R, C, 1, device="cuda"), spk=dev.spk[:R].contiguous(),
              n_valid=torch.full((R,), C, dtype=torch.int32, device="cuda"), end=torch.zeros(R, dtype=torch.int32, device="cuda"),
              out=conv.empty_outputs(R))

    def push():
        return conv.push(st["feats"], st["lcf0"], st["uv"], st["spk"], n_valid=st["n_valid"], end=st["end"], out=st["out"])

    push()  # (warm: the first launch of the family, the effective weights)
    conv.reset()
    torch.cuda.synchronize()
    allocs0 = _lib.lib().crk_debug_alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        push()
    conv.reset()
    torch.cuda.synchronize()
    bytes0 = torch.cuda.memory_allocated()
    parts, grown = [], None
    for i in range(nch):
        st["feats"].copy_(dev.x[:R, i * C: (i + 1) * C])
        st["lcf0"].copy_(dev.lcf0[:R, i * C: (i + 1) * C])
        st["uv"].copy_(dev.uv[:R, i * C: (i + 1) * C])
        st["end"].fill_(int(i == nch - 1))
        graph.replay()
        if i == 0:
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - bytes0
        parts.append({k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in st["out"].items()})
    torch.cuda.synchronize()
    allocs = _lib.lib().crk_debug_alloc_count() - allocs0
    eager = drive(dev.converter(R, C), dev, range(R), whole_plan([C] * nch, R))
    for r in range(R):
        got = _gather([(p, int(p["n_out"][r])) for p in parts], r, dev.fx.nst, nch * C)
        assert [int(p["n_out"][r]) for p in parts] == [4, 16, 16, 16, 28]
        assert [int(p["first"][r]) for p in parts] == [0, 4, 20, 36, 52]
        assert same(got, eager[r][0]), r
    assert allocs == 0 and grown == 0, (allocs, grown)


def test_push_refuses_output_buffers_that_are_not_empty_outputs():
    """The kernel writes up to max_out rows per stream into every buffer of ``out``: each one is checked, not only decoded."""
    dev = LaDev.of(**LI.SMALL)
    conv = dev.converter(2, 16)
    args = (torch.zeros(2, 16, dev.x.shape[-1], device="cuda"), torch.zeros(2, 16, 1, device="cuda"),
            torch.zeros(2, 16, 1, device="cuda"), dev.spk[:2].contiguous())
    small = conv.empty_outputs(2)
    for key, bad in (("qidx", [t[:, :16].contiguous() for t in small["qidx"]]),
                     ("encoded", [t[:, :16].contiguous() for t in small["encoded"]]),
                     ("encoded", [t.double() for t in small["encoded"]]), ("qidx", small["qidx"][:1]),
                     ("n_out", small["n_out"].long()), ("first", small["first"].cpu()), ("decoded", small["decoded"][:, :16])):
        with pytest.raises(ValueError, match=key):
            conv.push(*args, out=dict(conv.empty_outputs(2), **{key: bad}))
    assert conv.push(*args, out=small) is small


def test_refused_shapes_return_status_3_without_a_write():
    from crank_amd import _lib
    from crank_amd._lib import check
    from crank_amd.net.module.vqvae2 import VQVAE2
    from tests.helpers import load_yaml

    L = _lib.lib()
    dev = LaDev.of()
    conv = dev.converter(2, 64)
    conv._prepare()
    nst = dev.fx.nst

    def push(R, C):
        out = {k: ([t.fill_(SENT_I if t.dtype == torch.int64 else SENT_F) for t in v] if isinstance(v, list) else
                   v.fill_(SENT_I if v.dtype == torch.int32 else SENT_F))
               for k, v in conv.empty_outputs(max(R, 1)).items()}
        feats = torch.zeros(max(R, 1), max(C, 1), dev.x.shape[-1], device="cuda")
        cond = torch.zeros(max(R, 1), max(C, 1), 2, device="cuda")
        ptrs = ctypes.c_void_p * nst
        rc = L.crk_lstream_push(conv._handle, feats.data_ptr(), feats.shape[-1], cond.data_ptr(), 2, None, 2,
                                torch.zeros(max(R, 1), dtype=torch.int64, device="cuda").data_ptr(), None, None, R, C,
                                conv.max_out, out["decoded"].data_ptr(), ptrs(*[t.data_ptr() for t in out["qidx"]]),
                                ptrs(*[t.data_ptr() for t in out["encoded"]]), out["n_out"].data_ptr(),
                                out["first"].data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    for R, C in ((2, 65), (3, 16), (2, 0), (0, 16)):
        rc, out = push(R, C)
        assert rc == 3, (R, C, rc)
        assert bool((out["decoded"] == SENT_F).all()) and bool((out["n_out"] == SENT_I).all()) and bool((out["first"] == SENT_I).all())
        with pytest.raises(RuntimeError, match="unsupported"):
            check(rc, "crk_lstream_push")
    rc, out = push(2, 64)  # (64 frames in, fewer than the look-ahead: the counters are written, no row is)
    assert rc == 0 and bool((out["n_out"] == 0).all()) and bool((out["first"] == 0).all()) and bool((out["decoded"] == SENT_F).all())
    assert L.crk_lstream_reserve(conv._handle, 0, 64) == 3 and L.crk_lstream_reserve(conv._handle, 2, 0) == 3

    def create(G, **fields):
        d = _lib.StreamDesc()
        d.n_stacks, d.in_ch, d.out_ch = nst, dev.fx.conf["input_size"], dev.fx.conf["output_size"]
        for n in range(nst):
            d.emb_dim[n], d.emb_size[n], d.cb_off[n] = 64, 512, G.quantizers[n].cb_offset
            d.enc_base[n], d.dec_base[n] = G.encoders[n].base, G.decoders[n].base
        d.causal, d.enc_f0, d.dec_f0, d.spk_dim, d.spk_onehot, d.n_spk, d.spk_off = 0, 0, 1, 32, 0, LI.N_SPK, G.emb_offset
        for field, value in fields.items():
            if field == "emb_dim":
                d.emb_dim[0] = value
            else:
                setattr(d, field, value)
        nets = ctypes.c_void_p * 3
        enc = nets(*([G.encoders[n].net.handle for n in range(nst)] + [None] * (3 - nst)))
        dec = nets(*([G.decoders[n].net.handle for n in range(nst)] + [None] * (3 - nst)))
        h = ctypes.c_void_p()
        rc = L.crk_lstream_create(ctypes.byref(d), enc, dec, ctypes.byref(h))
        if rc == 0:
            L.crk_lstream_destroy(h)
        else:
            assert not h.value
        return rc

    assert create(dev.G) == 0
    for fields in (dict(causal=1), dict(emb_dim=48), dict(n_stacks=4), dict(in_ch=200)):
        assert create(dev.G, **fields) == 3, fields
    # an even kernel size: the stacks of a causal generator with kernel_size 4 (a non-causal layer cannot pad 1.5 frames)
    even = VQVAE2(load_yaml(None, causal=True, kernel_size=[4, 3, 3]), spkr_size=LI.N_SPK).eval()
    assert create(even) == 3
    # and the causal entry point keeps refusing a non-causal descriptor
    d = _lib.StreamDesc()
    h = ctypes.c_void_p()
    nets = ctypes.c_void_p * 3
    d.n_stacks, d.causal = nst, 0
    assert L.crk_stream_create(ctypes.byref(d), nets(), nets(), ctypes.byref(h)) == 3


# ---------------------------------------------------------------------------------------------------- 10 a refused reset
def test_a_reset_with_an_id_out_of_range_zeroes_nothing():
    """reset([0, n_streams]): RuntimeError, and stream 0 keeps its history and its frame count - every id is checked
    before the first row of either is zeroed.  5 frames, the refused reset, 5 more with the end flag, against a converter
    that was never reset, bit for bit (a reset stream 0 would emit an utterance of 5 frames, not of 10)."""
    dev = LaDev.of(**LI.SMALL)
    head = [((3, False),) * 2, ((2, False),) * 2]
    tail = [((3, False),) * 2, ((2, True),) * 2]
    conv = dev.converter(2, 3)
    drive(conv, dev, range(2), head)
    with pytest.raises(RuntimeError):
        conv.reset([0, 2])
    rest = drive(conv, dev, range(2), tail, start=[5, 5], taken=[5, 5])
    whole = drive(dev.converter(2, 3), dev, range(2), head + tail)
    for r in range(2):
        assert len(rest[r]) == 1 and rest[r][0]["n"] == 10 and rest[r][0]["decoded"].shape[0] == 10
        assert same(rest[r][0], whole[r][0]), r
