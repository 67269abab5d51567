"""Streaming Parallel WaveGAN vocoding on the GPU (crank_amd.vocoder.StreamingVocoder, csrc/voc_stream_kernels.hip).  Every
comparison with the offline vocoder is ``torch.equal`` against ``inference_batch([c], [x])`` with the same noise: the
streamed samples are the offline samples bit for bit, in every precision and however an utterance is cut into pushes."""
import functools
import json

import numpy as np
import pytest
import torch

from tests.pwg_vocoder_ref import checkpoint_of, random_generator

pytestmark = pytest.mark.gpu

SENT = 12345.0  # what wave samples past n_out must still hold after a push
DEFAULT = dict(layers=30, stacks=3, aux_context_window=2, upsample_params={"upsample_scales": [4, 4, 4, 4]})
DEEP = dict(layers=10, stacks=1, aux_context_window=2, aux_channels=8, upsample_params={"upsample_scales": [2, 2]})


def hop_of(params):
    return int(np.prod(params["upsample_params"]["upsample_scales"]))


@functools.lru_cache(maxsize=None)
def vocoder(seed, spec):
    from crank_amd.vocoder import ParallelWaveGANVocoder

    params = json.loads(spec)
    g = random_generator(seed, **params)
    return ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(g), {"generator_params": params, "hop_size": hop_of(params)},
                                                  device="cuda")


def voc_of(params, seed=31):
    """One vocoder per configuration, built once per process."""
    return vocoder(seed, json.dumps(params, sort_keys=True))


def utterance(voc, T, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(T, voc.aux_channels, generator=gen).cuda(), torch.randn(T * voc.hop_size, generator=gen).cuda())


class precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        from crank_amd import ops

        ops.set_precision(self.prec)

    def __exit__(self, *exc):
        from crank_amd import ops

        ops.set_precision("bf16")


def offline(voc, c, x):
    return voc.inference_batch([c], [x])[0]


def drive(sv, utts, plan, C=None):
    """utts[r]: the (c, x) utterances row r vocodes, in order; plan: per push and row (frames taken, end flag).  Rows at and
    past n_valid hold NaN.  Checks at every push that n_out follows the rule - max(0, T - LA) frames emitted after T frames,
    everything at the end - and that no sample past n_out was written.  Returns per row the waveform of each utterance."""
    R, H, LA, A = len(utts), sv.hop_size, sv.lookahead, sv.aux_channels
    which, at = [0] * R, [0] * R
    got = [[[]] for _ in range(R)]
    for push in plan:
        Cp = max(1, max(n for n, _ in push)) if C is None else C
        c = torch.full((R, Cp, A), float("nan"), device="cuda")
        x = torch.full((R, Cp * H), float("nan"), device="cuda")
        want = []
        for r, (n, end) in enumerate(push):
            if n:
                uc, ux = utts[r][which[r]]
                assert at[r] + n <= len(uc)
                c[r, :n], x[r, :n * H] = uc[at[r]:at[r] + n], ux[at[r] * H:(at[r] + n) * H]
            t0, t1 = at[r], at[r] + n
            want.append(((t1 if end else max(0, t1 - LA)) - max(0, t0 - LA)) * H)
            at[r] = t1
        out = sv.empty_outputs(R, Cp)
        out["wave"].fill_(SENT)
        res = sv.push(c, x, n_valid=torch.tensor([n for n, _ in push], device="cuda", dtype=torch.int32),
                      end=torch.tensor([int(e) for _, e in push], device="cuda", dtype=torch.int32), out=out)
        assert res is out
        assert out["n_out"].tolist() == want, (out["n_out"].tolist(), want)
        for r, (n, end) in enumerate(push):
            assert bool((out["wave"][r, want[r]:] == SENT).all()), "a push wrote samples past n_out"
            got[r][-1].append(out["wave"][r, :want[r]].clone())
            if end:
                got[r].append([])
                which[r] += 1
                at[r] = 0
    return [[torch.cat(p) for p in row if p] for row in got]


def cut(T, sizes):
    """[(frames, end)] for one row: `sizes` cycled until T frames are taken, the end flag on the last push."""
    out, done, i = [], 0, 0
    while done < T:
        n = min(sizes[i % len(sizes)], T - done)
        done += n
        out.append((n, done == T))
        i += 1
    return out


def random_sizes(seed, lo, hi, n=4096):
    return [int(v) for v in np.random.RandomState(seed).randint(lo, hi + 1, size=n)]


# ------------------------------------------------------------------------------------------ 5 long history, ring wrap
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_history_longer_than_many_pushes_and_ring_wrap(prec):
    """10 layers in one stack (D = 1023, LA = 260 frames of 4 samples), 330 frames: pushed one frame at a time the last
    layers run 260 pushes behind the input and every ring wraps many times."""
    voc = voc_of(DEEP)
    c, x = utterance(voc, 330, 1)
    with precision(prec):
        ref = offline(voc, c, x)
        sv = voc.streaming(1, 8)
        assert sv.lookahead == 260
        ones = drive(sv, [[(c, x)]], [[p] for p in cut(330, [1])])[0][0]
        rand = drive(sv, [[(c, x)]], [[p] for p in cut(330, random_sizes(4, 1, 8))])[0][0]
        whole = drive(voc.streaming(1, 330), [[(c, x)]], [[(330, True)]])[0][0]
    assert ref.shape == (330 * 4,)
    assert torch.equal(ones, ref) and torch.equal(rand, ref) and torch.equal(whole, ref)


# ------------------------------------------------------------------------------------- 6 a frontier inside a tile
@pytest.mark.parametrize("win", [0, 5])
def test_frontiers_inside_a_32_sample_tile(win):
    """Hop 30 ([5, 6]): no frontier of any stage is a multiple of the 32-sample tile."""
    voc = voc_of(dict(layers=6, stacks=2, aux_context_window=win, aux_channels=8, upsample_params={"upsample_scales": [5, 6]}))
    c, x = utterance(voc, 41, 2)
    for prec in ("bf16", "bf16x3"):
        with precision(prec):
            ref = offline(voc, c, x)
            sv = voc.streaming(1, 7)
            assert sv.lookahead == win + 2
            for sizes in ([1], [3], random_sizes(9, 1, 7)):
                assert torch.equal(drive(sv, [[(c, x)]], [[p] for p in cut(41, sizes)])[0][0], ref), (prec, sizes[:4])


# --------------------------------------------------------------------------------------- 7 default config, 3 streams
def _three_stream_plan(lens):
    """Chunks of 3; row 1 starts two pushes late, row 2 four; every row sits some pushes out (n_valid = 0)."""
    rows = []
    for r, T in enumerate(lens):
        p = [(0, False)] * (2 * r)
        for i, step in enumerate(cut(T, [3])):
            if i % (4 + r) == 3:
                p.append((0, False))
            p.append(step)
        rows.append(p)
    n = max(len(p) for p in rows)
    rows = [p + [(0, False)] * (n - len(p)) for p in rows]
    return [list(push) for push in zip(*rows)]


def test_default_config_three_ragged_staggered_streams():
    voc = voc_of(DEFAULT)
    lens = [40, 31, 25]
    utts = [utterance(voc, T, 10 + r) for r, T in enumerate(lens)]
    other = [utts[0]] + [utterance(voc, T, 20 + r) for r, T in enumerate(lens)][1:]
    plan = _three_stream_plan(lens)
    for prec in ("bf16", "bf16x3"):
        with precision(prec):
            sv = voc.streaming(3, 3)
            assert sv.lookahead == 16
            got = drive(sv, [[u] for u in utts], plan, C=3)
            for r, (c, x) in enumerate(utts):
                assert torch.equal(got[r][0], offline(voc, c, x)), (prec, r)
            again = drive(sv, [[u] for u in other], plan, C=3)
            assert torch.equal(again[0][0], got[0][0])
            assert not torch.equal(again[1][0], got[1][0])


# ------------------------------------------------------------------------------------------------- 8 n_out, flushes
def test_n_out_rule_flush_with_no_frames_and_utterances_shorter_than_the_lookahead():
    """drive() checks n_out against the rule at every push.  Row 0: 30 frames, then the end flag on a push with
    n_valid = 0; row 1: utterances of 1 and 5 frames (< LA = 16), which come out whole on their end push."""
    voc = voc_of(DEFAULT)
    long_, one, five = utterance(voc, 30, 40), utterance(voc, 1, 41), utterance(voc, 5, 42)
    sv = voc.streaming(2, 4)
    plan = [[(4, False), (1, True)],
            [(4, False), (4, False)],
            [(4, False), (1, True)],
            [(4, False), (0, False)]] + [[(4, False), (0, False)]] * 3 + [[(2, False), (0, False)], [(0, True), (0, False)],
                                                                            [(0, True), (0, True)]]
    got = drive(sv, [[long_], [one, five]], plan, C=4)
    assert torch.equal(got[0][0], offline(voc, *long_))
    assert torch.equal(got[1][0], offline(voc, *one)) and got[1][0].shape == (256,)
    assert torch.equal(got[1][1], offline(voc, *five)) and got[1][1].shape == (5 * 256,)


# ------------------------------------------------------------------------------------------------- 9 end, reset
def test_end_then_a_new_utterance_and_reset_mid_utterance_equal_two_offline_runs():
    voc = voc_of(DEFAULT)
    a, b = utterance(voc, 23, 50), utterance(voc, 19, 51)
    ra, rb = offline(voc, *a), offline(voc, *b)
    sv = voc.streaming(2, 5)
    got = drive(sv, [[a, b], [b, a]], [list(p) for p in zip(cut(23, [5]) + cut(19, [4]) + [(0, False)],
                                                              cut(19, [4]) + cut(23, [5]) + [(0, False)])], C=5)
    assert torch.equal(got[0][0], ra) and torch.equal(got[0][1], rb)
    assert torch.equal(got[1][0], rb) and torch.equal(got[1][1], ra)
    # reset in the middle of an utterance: what was not emitted is dropped, the next frame is an utterance's first
    H = voc.hop_size
    for streams in (None, [0]):
        out = sv.push(a[0][None, :5].contiguous(), a[1][None, :5 * H].contiguous())
        assert out["n_out"].tolist() == [0]
        sv.reset(streams)
        assert torch.equal(drive(sv, [[b]], [[p] for p in cut(19, [5])])[0][0], rb)


# ------------------------------------------------------------------------------------------------- 10 capture
def test_captured_push_equals_eager_allocates_nothing_and_bf16x3f_is_bf16x3():
    from crank_amd import _lib

    voc = voc_of(DEFAULT)
    S, C, n_push = 2, 3, 9
    H, LA = voc.hop_size, 16
    utts = [utterance(voc, C * n_push, 60 + r) for r in range(S)]
    results = {}
    for prec in ("bf16x3", "bf16x3f"):
        with precision(prec):
            plan = [[(C, i + 1 == n_push)] * S for i in range(n_push)]
            eager = drive(voc.streaming(S, C), [[u] for u in utts], plan, C=C)
            sv = voc.streaming(S, C)
            st = dict(c=torch.zeros(S, C, voc.aux_channels, device="cuda"), x=torch.zeros(S, C * H, device="cuda"),
                      nv=torch.full((S,), C, dtype=torch.int32, device="cuda"), end=torch.zeros(S, dtype=torch.int32, device="cuda"),
                      out=sv.empty_outputs(S, C))
            sv.push(st["c"], st["x"], st["nv"], st["end"], out=st["out"])  # warm: every kernel of the family has launched once
            sv.reset()
            torch.cuda.synchronize()
            allocs0 = _lib.lib().crk_debug_alloc_count()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sv.push(st["c"], st["x"], st["nv"], st["end"], out=st["out"])
            sv.reset()
            pieces = [[] for _ in range(S)]
            for i in range(n_push):
                for r, (uc, ux) in enumerate(utts):
                    st["c"][r].copy_(uc[i * C:(i + 1) * C])
                    st["x"][r].copy_(ux[i * C * H:(i + 1) * C * H])
                st["end"].fill_(int(i + 1 == n_push))
                graph.replay()
                n = st["out"]["n_out"].tolist()
                assert n == [((C * n_push) if i + 1 == n_push else max(0, C * (i + 1) - LA)) * H - max(0, C * i - LA) * H] * S
                for r in range(S):
                    pieces[r].append(st["out"]["wave"][r, :n[r]].clone())
            torch.cuda.synchronize()
            assert _lib.lib().crk_debug_alloc_count() == allocs0
            for r in range(S):
                assert torch.equal(torch.cat(pieces[r]), eager[r][0]), (prec, r)
                assert torch.equal(eager[r][0], offline(voc, *utts[r])), (prec, r)
            results[prec] = [e[0] for e in eager]
    assert all(torch.equal(a, b) for a, b in zip(results["bf16x3"], results["bf16x3f"]))


# ------------------------------------------------------------------------------------------------- 11 refusals
def test_refused_calls_name_the_limit():
    voc = voc_of(DEEP)
    with pytest.raises(ValueError, match="both must be at least 1"):
        voc.streaming(0, 4)
    with pytest.raises(ValueError, match="both must be at least 1"):
        voc.streaming(2, 0)
    sv = voc.streaming(2, 4)
    assert sv.state_bytes > 0
    H = voc.hop_size
    c, x = torch.zeros(2, 4, 8, device="cuda"), torch.zeros(2, 4 * H, device="cuda")
    with pytest.raises(ValueError, match="max_chunk = 4"):
        sv.push(torch.zeros(2, 5, 8, device="cuda"), torch.zeros(2, 5 * H, device="cuda"))
    with pytest.raises(ValueError, match="n_streams = 2"):
        sv.push(torch.zeros(3, 4, 8, device="cuda"), torch.zeros(3, 4 * H, device="cuda"))
    with pytest.raises(ValueError, match="c: a float32"):
        sv.push(torch.zeros(2, 4, 9, device="cuda"), x)
    with pytest.raises(ValueError, match="c: a float32"):
        sv.push(c.double(), x)
    with pytest.raises(ValueError, match="c: a float32"):
        sv.push(c.cpu(), x)
    with pytest.raises(ValueError, match="c: a float32"):
        sv.push(c[0], x)
    with pytest.raises(ValueError, match="noise: a float32"):
        sv.push(c, x[:, :-1])
    with pytest.raises(ValueError, match="noise: a float32"):
        sv.push(c, x.cpu())
    with pytest.raises(ValueError, match="n_valid: an integer"):
        sv.push(c, x, n_valid=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="n_valid: an integer"):
        sv.push(c, x, n_valid=torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError, match="end: an integer"):
        sv.push(c, x, end=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="out: wave float32"):
        sv.push(c, x, out=sv.empty_outputs(2, 3))
    with pytest.raises(ValueError, match="stream ids are 0 .. 1"):
        sv.reset([2])
    # nothing above reached the device: the stream still starts an utterance, and drawn noise is reproducible
    voc.manual_seed(5)
    a = sv.push(c, end=torch.ones(2, dtype=torch.int32, device="cuda"))
    voc.manual_seed(5)
    b = sv.push(c, end=torch.ones(2, dtype=torch.int32, device="cuda"))
    assert a["n_out"].tolist() == [4 * H] * 2 and torch.equal(a["wave"][:, :4 * H], b["wave"][:, :4 * H])


# ------------------------------------------------------------------------------------------------- 12 the live loop
def test_streaming_converter_into_streaming_vocoder_equals_the_offline_vocoder():
    """A causal generator pushed through StreamingConverter, its decoded frames de-scaled with crank's scaler, normalised
    with the vocoder's statistics and pushed into StreamingVocoder: the waveform of the offline vocoder on the
    concatenated decoded frames."""
    from crank_amd.vocoder import ParallelWaveGANVocoder
    from tests.test_gpu_stream import Dev

    dev = Dev.of()
    D = dev.fx.conf["output_size"]
    params = dict(layers=6, stacks=2, aux_channels=D, upsample_params={"upsample_scales": [2, 4, 4]})
    rs = np.random.RandomState(3)
    stats = (rs.standard_normal(D).astype(np.float32), rs.uniform(0.5, 2.0, D).astype(np.float32))
    voc = ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(random_generator(6, **params)),
                                                 {"generator_params": params, "hop_size": 32}, stats=stats, device="cuda")
    mean_ = torch.from_numpy(rs.standard_normal(D).astype(np.float32)).cuda()  # crank's scaler["mlfb"]
    scale_ = torch.from_numpy(rs.uniform(0.5, 2.0, D).astype(np.float32)).cuda()
    R, C, n_push, H = 2, 16, 4, 32
    conv, sv = dev.converter(R, C), voc.streaming(R, C)
    noise = torch.randn(R, n_push * C * H, generator=torch.Generator().manual_seed(1)).cuda()
    frames, waves = [], [[] for _ in range(R)]
    for i in range(n_push + 1):
        last = i == n_push
        if not last:
            sl = slice(i * C, (i + 1) * C)
            dec = conv.push(dev.x[:R, sl].contiguous(), dev.lcf0[:R, sl].contiguous(), dev.uv[:R, sl].contiguous(),
                            dev.spk[:R].contiguous())["decoded"]
            frames.append(dec.clone())
            out = sv.push(voc.normalize(dec * scale_ + mean_), noise[:, i * C * H:(i + 1) * C * H].contiguous())
        else:  # nothing new: flush
            out = sv.push(torch.zeros(R, 1, D, device="cuda"), torch.zeros(R, H, device="cuda"),
                          n_valid=torch.zeros(R, dtype=torch.int32, device="cuda"), end=torch.ones(R, dtype=torch.int32, device="cuda"))
        n = out["n_out"].tolist()
        for r in range(R):
            waves[r].append(out["wave"][r, :n[r]].clone())
    dec = torch.cat(frames, dim=1)
    for r in range(R):
        ref = voc.inference_batch([voc.normalize(dec[r] * scale_ + mean_)], [noise[r]])[0]
        assert torch.equal(torch.cat(waves[r]), ref), r
