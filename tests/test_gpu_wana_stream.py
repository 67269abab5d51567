"""Streaming CheapTrick / mel-cepstrum analysis on the GPU (crank_amd.world.StreamingMcep, csrc/wana_stream_kernels.hip):
every frame bit for bit ``WorldAnalyzer.mcep_batch`` of the whole utterance under any cut of samples and F0 rows, ragged
streams, reuse and reset, ``feats`` against float64 numpy, the definition in sets (tests/wana_stream_ref.py) within the
offline tests' per-case bound, the flags, the refusals, graph capture, and the chain behind ``StreamingF0``."""
import functools

import numpy as np
import pytest
import torch

from tests import wana_stream_ref as W
from tests import world_analysis_cases as C
from tests import world_analysis_ref as A

pytestmark = pytest.mark.gpu

FS, SHIFT, DIM, ALPHA, LOW_CUT = 16000, 5.0, 24, 0.41, 70
HOP = 80  # samples per frame
LENS = (2400, 3300, 4000, 100)
LONGEST = W.REACH - 1  # the longest half window an F0 above the floor gives at 16 kHz
SENT = 12345.0  # what rows at and past n_frames must still hold after a push


@functools.lru_cache(maxsize=None)
def streams():
    """Three utterances and one of 100 samples and 2 rows (windows clamp at both ends).  Each contour has voiced runs,
    zeros, a frame just above the floor (the longest window: half = 510 at this rate - 1.5 fs / F0 reaches 510.5 only at
    the floor itself), one at fs / 4 and one exactly at the floor (analysed at 500 Hz)."""
    rng = np.random.default_rng(77)
    xs, f0s = [], []
    for i, n in enumerate(LENS):
        xs.append(C._harmonic(rng, n, FS, 120.0 + 30.0 * i).astype(np.float32))
        T = 2 if n == 100 else n // HOP + 1
        f0 = 140.0 + 25.0 * i + 30.0 * np.sin(np.arange(T) / 4.0) + rng.uniform(-3, 3, T)
        if T > 2:
            f0[3:6] = 0.0
            f0[T // 2:T // 2 + 2] = 0.0
            f0[9] = np.nextafter(A.f0_floor(FS), 1e9)
            f0[12] = FS / 4.0
            f0[15] = A.f0_floor(FS)
        f0s.append(f0)
    sh = A.frame_shapes(f0s[0], FS, SHIFT)
    assert sh["half"][9] == LONGEST and sh["f0"][15] == 500.0 and sh["half"][12] == 6
    return xs, f0s


def analyzer():
    from crank_amd.world import WorldAnalyzer

    return WorldAnalyzer(FS, shiftms=SHIFT)


@functools.lru_cache(maxsize=None)
def offline(low_cut=LOW_CUT):
    """(mceps, sps) of the whole utterances: the oracle, computed once."""
    xs, f0s = streams()
    return analyzer().mcep_batch(list(xs), list(f0s), DIM, ALPHA, low_cut, return_sp=True)


def make(n_streams, max_samples, max_f0_in, f0_capacity=64, ring_capacity=8192, low_cut=LOW_CUT, **kw):
    from crank_amd.world import StreamingMcep

    kw.setdefault("max_utt_frames", 64)
    return StreamingMcep(FS, SHIFT, n_streams, max_samples, max_f0_in, f0_capacity, ring_capacity, dim=DIM, alpha=ALPHA,
                         low_cut=low_cut, **kw)


def ints(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def run(sm, xs, f0s, scheds, bad_calls=()):
    """Streams one utterance per stream: scheds[s] is the list of (samples, rows) of stream s's pushes, the last of which
    takes whatever is left and carries the end flag; a stream with fewer pushes idles afterwards.  What a push does not
    bring is NaN.  Returns per stream mcep, sp, feats of its frames in order, the frames per push and the rows dropped,
    after checking that no push wrote a row at or past n_frames.  bad_calls: callables that must raise, run one between
    every two pushes."""
    S, P = sm.n_streams, max(len(s) for s in scheds)
    res = [dict(mcep=[], sp=[], feats=[], per_push=[], dropped=0) for _ in range(S)]
    at = [[0, 0] for _ in range(S)]
    out = sm.empty_outputs(S, sp=True)
    for p in range(P):
        counts = [[0, 0, 0] for _ in range(S)]
        for s in range(S):
            if p < len(scheds[s]):
                c, r = scheds[s][p]
                if p + 1 == len(scheds[s]):
                    c, r, counts[s][2] = len(xs[s]) - at[s][0], len(f0s[s]) - at[s][1], 1
                counts[s][0], counts[s][1] = min(c, len(xs[s]) - at[s][0]), min(r, len(f0s[s]) - at[s][1])
        Cm, Rm = max(c[0] for c in counts), max(c[1] for c in counts)
        x = np.full((S, Cm), np.nan, np.float32)
        f = np.full((S, Rm), np.nan)
        for s in range(S):
            x[s, :counts[s][0]] = xs[s][at[s][0]:at[s][0] + counts[s][0]]
            f[s, :counts[s][1]] = f0s[s][at[s][1]:at[s][1] + counts[s][1]]
            at[s][0] += counts[s][0]
            at[s][1] += counts[s][1]
        for k in ("mcep", "sp", "feats"):
            out[k].fill_(SENT)
        if bad_calls:
            with pytest.raises(ValueError):
                bad_calls[p % len(bad_calls)](out)
            assert all(bool((out[k] == SENT).all()) for k in ("mcep", "sp", "feats"))
        got = sm.push(torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda(), ints([c[0] for c in counts]),
                      ints([c[1] for c in counts]), ints([c[2] for c in counts]), out=out)
        assert got is out
        nf, first, nd = out["n_frames"].tolist(), out["first"].tolist(), out["n_dropped"].tolist()
        assert first == [sm.first] * S
        for s in range(S):
            assert 0 <= nf[s] <= sm.max_frames
            for k in ("mcep", "sp", "feats"):
                assert bool((out[k][s, nf[s]:] == SENT).all()), (p, s, k)
                res[s][k].append(out[k][s, :nf[s]].clone())
            res[s]["per_push"].append(nf[s])
            res[s]["dropped"] += nd[s]
    for s in range(S):
        assert at[s] == [len(xs[s]), len(f0s[s])]
        for k in ("mcep", "sp", "feats"):
            res[s][k] = torch.cat(res[s][k])
    return res


def late_rows(n_total, T, cuts, lag, block=1):
    """A schedule whose sample cuts cycle through ``cuts`` and whose rows come in blocks of ``block``, a block once the
    stream holds ``lag`` samples past the origin of its last frame."""
    sched, n, rows, i = [], 0, 0, 0
    while n < n_total:
        c = min(cuts[i % len(cuts)], n_total - n)
        i += 1
        n += c
        r = 0
        while rows + r + block <= T and (rows + r + block - 1) * HOP + lag <= n:
            r += block
        rows += r
        sched.append((c, r))
    return sched


def cut(name, n, T):
    if name == "single":
        return [(n, T)]
    if name == "pushes_of_160":
        return [(160, 2)] * (-(-n // 160))
    if name == "irregular_late_f0":  # rows in blocks of 16 that arrive 180 ms late
        return late_rows(n, T, (37, 1, 500, 3, 700), 180 * FS // 1000, 16)
    if name == "f0_first":  # rows wait for samples
        return [(0, T)] + [(333, 0)] * (-(-n // 333))
    raise KeyError(name)


SIZES = {"single": (4000, 64), "pushes_of_160": (160, 4), "irregular_late_f0": (700, 64), "f0_first": (333, 64)}


def check_equal(res, mceps, sps, which=None):
    """Every stream's frames are the offline call's, bit for bit, and as many as the rows given."""
    for s, r in enumerate(res):
        u = s if which is None else which[s]
        assert r["mcep"].shape[0] == mceps[u].shape[0] and r["dropped"] == 0, (s, r["mcep"].shape, r["dropped"])
        assert torch.equal(r["mcep"], mceps[u]), s
        assert torch.equal(r["sp"], sps[u]), s


# ---------------------------------------------------------------------------------------------------- 1, 2 any cut
@pytest.mark.parametrize("name", list(SIZES))
def test_streamed_frames_are_the_offline_bits_under_every_cut(name):
    xs, f0s = streams()
    mceps, sps = offline()
    sm = make(len(xs), *SIZES[name])
    res = run(sm, xs, f0s, [cut(name, len(x), len(f)) for x, f in zip(xs, f0s)])
    check_equal(res, mceps, sps)
    sm.status()
    if name == "pushes_of_160":  # frame i leaves with the push that completes origin_i + 512 samples
        want = [max(0, (160 * (p + 1) - 512) // HOP + 1) - max(0, (160 * p - 512) // HOP + 1) for p in range(14)]
        assert res[0]["per_push"][:14] == want
    if name == "f0_first":
        assert res[2]["per_push"][:3] == [0, 0, (666 - 512) // HOP + 1]
    assert max(res[3]["per_push"]) == 2 and sum(res[3]["per_push"]) == 2  # an end push with n < 512 emits all its frames


def test_without_a_low_cut_the_stream_is_the_offline_call_without_one():
    xs, f0s = streams()
    mceps, sps = offline(None)
    assert not torch.equal(mceps[0], offline()[0][0])
    sm = make(len(xs), 160, 4, low_cut=None)
    check_equal(run(sm, xs, f0s, [cut("pushes_of_160", len(x), len(f)) for x, f in zip(xs, f0s)]), mceps, sps)
    sm.status()


# ---------------------------------------------------------------------------------------------------- 3 ragged
def test_ragged_streams_together_equal_each_stream_alone():
    xs, f0s = streams()
    together = run(make(len(xs), 700, 64), xs, f0s, [cut("irregular_late_f0", len(x), len(f)) for x, f in zip(xs, f0s)])
    for s in range(len(xs)):
        alone = run(make(1, 700, 64), [xs[s]], [f0s[s]], [cut("irregular_late_f0", len(xs[s]), len(f0s[s]))])[0]
        for k in ("mcep", "sp", "feats"):
            assert torch.equal(alone[k], together[s][k]), (s, k)
        assert alone["mcep"].shape[0] == len(f0s[s])


# ---------------------------------------------------------------------------------------------------- 4 reuse, reset
def test_a_second_utterance_after_an_end_push_and_after_reset_equals_a_fresh_handle():
    xs, f0s = streams()
    mceps, sps = offline()
    sm = make(2, 160, 4)
    sched = lambda u: cut("pushes_of_160", len(xs[u]), len(f0s[u]))  # noqa: E731
    first = run(sm, [xs[0], xs[3]], [f0s[0], f0s[3]], [sched(0), sched(3)])
    check_equal(first, mceps, sps, which=[0, 3])
    assert first[1]["per_push"][0] == 2  # the 100-sample utterance: one end push with n < 512, both frames
    second = run(sm, [xs[1], xs[2]], [f0s[1], f0s[2]], [sched(1), sched(2)])
    check_equal(second, mceps, sps, which=[1, 2])
    # half an utterance, then reset of that stream alone while the other is in the middle of its own
    half = torch.from_numpy(np.stack([xs[1][:160], xs[2][:160]])).cuda()
    rows = torch.from_numpy(np.stack([f0s[1][:4], f0s[2][:4]])).cuda()
    for _ in range(5):
        sm.push(half, rows)
    sm.reset([0])
    sm.reset([1])
    third = run(sm, [xs[2], xs[0]], [f0s[2], f0s[0]], [sched(2), sched(0)])
    check_equal(third, mceps, sps, which=[2, 0])
    sm.status()
    assert sm.state_bytes > 2 * 8192 * 8


# ---------------------------------------------------------------------------------------------------- 5 feats
@pytest.mark.parametrize("use_0th", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_feats_are_the_float64_expression_rounded_once(scaled, use_0th):
    xs, f0s = streams()
    rng = np.random.default_rng(3)
    scaler = (rng.standard_normal(DIM + 1), rng.uniform(0.3, 2.0, DIM + 1)) if scaled else None
    sm = make(len(xs), 4000, 64, scaler=scaler, use_mcep_0th=use_0th)
    res = run(sm, xs, f0s, [cut("single", len(x), len(f)) for x, f in zip(xs, f0s)])
    check_equal(res, *offline())
    first = 0 if use_0th else 1
    assert sm.first == first
    for s, r in enumerate(res):
        m = r["mcep"].cpu().numpy()
        want = ((m - scaler[0]) / scaler[1] if scaled else m)[:, first:].astype(np.float32)
        assert r["feats"].dtype == torch.float32 and tuple(r["feats"].shape) == want.shape
        assert np.array_equal(r["feats"].cpu().numpy(), want), s
        assert np.array_equal(want, W.feats_of(m, first, scaler))


# ---------------------------------------------------------------------------------------------------- 6 the definition
@pytest.mark.parametrize("name", ["fs16000_shift5", "fs16000_shift5.33333"])
def test_against_the_definition_in_sets_within_the_offline_bound(name):
    """The CPU restatement streamed in pushes of 160 against the device streamed in another cut, on the float32 cast of a
    case of tests/world_analysis_cases.py, no low cut: within that file's bound for the case, 10 s + 1e-12."""
    from crank_amd.world import StreamingMcep
    from tests.test_gpu_world_analysis import _cases  # (built once for both files)

    c = _cases()[name]
    x, f0 = c["waves"][0].astype(np.float32), c["f0s"][0]
    n, T = len(x), len(f0)
    ref = W.McepStreamRef(c["fs"], c["shiftms"], c["dim"], c["alpha"], None, T, n + 1024, T)
    want = W.stream_utterance(ref, x, f0, [(160, 2)] * (n // 160) + [(0, 0)])
    assert ref.flags == 0 and want["index"] == list(range(T))
    sm = StreamingMcep(c["fs"], c["shiftms"], 1, 700, 64, 64, 8192, dim=c["dim"], alpha=c["alpha"], low_cut=None,
                       max_utt_frames=T)
    got = run(sm, [x], [f0], [late_rows(n, T, (37, 1, 500, 3, 700), 0)])[0]
    sm.status()
    assert got["mcep"].shape[0] == T and got["dropped"] == 0
    b_sp, b_mc = C.bounds(name)
    e_sp = float(np.abs(np.log(got["sp"].cpu().numpy()) - np.log(want["sp"])).max())
    e_mc = float(np.abs(got["mcep"].cpu().numpy() - want["mcep"]).max())
    print(f"{name}: log sp {e_sp:.3e} (bound {b_sp:.3e}), mcep {e_mc:.3e} (bound {b_mc:.3e})")
    assert e_sp <= b_sp and e_mc <= b_mc


# ---------------------------------------------------------------------------------------------------- 7 flags
def expect_flag(sm, flag, streams_set=(0,)):
    flags = sm.flags()
    assert [f for f in flags] == [flag if s in streams_set else 0 for s in range(sm.n_streams)], flags
    with pytest.raises(RuntimeError):
        sm.status()
    sm.reset()
    sm.status()


def test_a_ring_one_sample_below_what_the_latest_frame_needs_drops_it_and_keeps_the_other_bits():
    """analysis_capacities counts on a half window of 511; the longest a contour reaches at 16 kHz is 510, so the ring one
    step below what the worst history needs here is the helper's capacity less 2."""
    from crank_amd.world import analysis_capacities

    xs, f0s = streams()
    mceps, sps = offline()
    x, f0 = xs[2], f0s[2]
    lag = 100 * FS // 1000
    ring, queue = analysis_capacities(FS, SHIFT, 100.0, 160, 32)
    assert (ring, queue) == (lag - 1 + 160 + 511, 23)
    # frame 9 (the longest window) gets its row as late as the lag allows, in a push that began one sample short of origin + lag
    sched = late_rows(len(x), len(f0), (9 * HOP + lag - 1 - 14 * 160,) + (160,) * 40, lag)
    assert sched[0][0] == 79 and sched[15] == (160, 2) and sum(r for _, r in sched[:15]) == 9
    res = run(make(1, 160, 32, queue, ring), [x], [f0], [sched])[0]
    check_equal([res], [mceps[2]], [sps[2]])
    res = run(make(1, 160, 32, queue, ring - 1), [x], [f0], [sched])[0]  # (the sample the helper keeps in hand)
    check_equal([res], [mceps[2]], [sps[2]])
    sm = make(1, 160, 32, queue, ring - 1 - (W.REACH - LONGEST))
    res = run(sm, [x], [f0], [sched])[0]
    keep = [k for k in range(len(f0)) if k != 9]
    assert res["dropped"] == 1 and res["mcep"].shape[0] == len(keep)
    assert torch.equal(res["mcep"], mceps[2][keep]) and torch.equal(res["sp"], sps[2][keep])
    expect_flag(sm, 1)


def test_a_queue_one_row_short_sets_flag_2():
    from crank_amd.world import analysis_capacities

    xs, f0s = streams()
    x, f0 = xs[2], np.concatenate([f0s[2], [150.0]])  # 52 rows: the most the offline call takes for 4000 samples
    lag = 100 * FS // 1000
    ring, queue = analysis_capacities(FS, SHIFT, 100.0, 160, 32)
    want = analyzer().mcep_batch([x], [f0], DIM, ALPHA, LOW_CUT)[0]
    sched = late_rows(len(x), len(f0), (160,), lag)
    sm = make(1, 160, 32, queue, ring)
    res = run(sm, [x], [f0], [sched])[0]
    assert res["dropped"] == 0 and torch.equal(res["mcep"], want)
    sm.status()
    sm = make(1, 160, 32, queue - 1, ring)
    res = run(sm, [x], [f0], [sched])[0]
    assert res["dropped"] == 1 and torch.equal(res["mcep"], want[:-1])  # the newest row went
    expect_flag(sm, 2)


def test_flags_4_8_and_16():
    xs, f0s = streams()
    mceps, sps = offline()
    x, f0 = xs[0], f0s[0]
    # 4: a randn table of 4 frames' draws; every frame still leaves, the first four with the offline bits
    sm = make(1, 4000, 64, max_utt_frames=4)
    res = run(sm, [x], [f0], [[(len(x), len(f0))]])[0]
    assert res["mcep"].shape[0] == len(f0) and res["dropped"] == 0
    assert torch.equal(res["mcep"][:4], mceps[0][:4]) and bool(torch.isfinite(res["mcep"]).all())
    expect_flag(sm, 4)
    # 8: two rows more; the first is one shift past the end (taken), the second two shifts (refused)
    sm = make(1, 4000, 64)
    res = run(sm, [x], [np.concatenate([f0, [150.0, 150.0]])], [[(len(x), len(f0) + 2)]])[0]
    assert res["mcep"].shape[0] == len(f0) + 1 and res["dropped"] == 1
    assert torch.equal(res["mcep"][:len(f0)], mceps[0])
    expect_flag(sm, 8)
    # 8 again: rows and not one sample
    out = sm.push(torch.zeros(1, 0, device="cuda"), torch.full((1, 3), 150.0, dtype=torch.float64, device="cuda"),
                  end=ints([1]))
    assert out["n_frames"].tolist() == [0] and out["n_dropped"].tolist() == [3]
    expect_flag(sm, 8)
    # 16: NaN, a negative row and one above fs / 4 are analysed as 0
    bad = f0.copy()
    bad[[7, 20, 25]] = [np.nan, -1.0, np.nextafter(FS / 4.0, 1e9)]
    zeroed = bad.copy()
    zeroed[[7, 20, 25]] = 0.0
    want = analyzer().mcep_batch([x], [zeroed], DIM, ALPHA, LOW_CUT)[0]
    res = run(sm, [x], [bad], [[(len(x), len(f0))]])[0]
    assert res["dropped"] == 0 and torch.equal(res["mcep"], want)
    expect_flag(sm, 16)
    # and a flag is one stream's own
    sm = make(2, 4000, 64)
    res = run(sm, [x, x], [bad, zeroed], [[(len(x), len(f0))]] * 2)
    assert torch.equal(res[0]["mcep"], res[1]["mcep"])
    expect_flag(sm, 16, (0,))


# ---------------------------------------------------------------------------------------------------- 8 refusals
def test_refused_calls_leave_outputs_and_state_untouched():
    xs, f0s = streams()
    S = len(xs)
    sm = make(S, 160, 4)
    good_x, good_f = torch.zeros(S, 160, device="cuda"), torch.zeros(S, 4, dtype=torch.float64, device="cuda")
    bad = [lambda out: sm.push(good_x.double(), good_f, out=out),                       # wrong dtype
           lambda out: sm.push(good_x, good_f.float(), out=out),
           lambda out: sm.push(good_x.cpu(), good_f, out=out),                          # wrong device
           lambda out: sm.push(good_x, good_f.cpu(), out=out),
           lambda out: sm.push(torch.zeros(S, 161, device="cuda"), good_f, out=out),    # C > max_samples
           lambda out: sm.push(good_x, torch.zeros(S, 5, dtype=torch.float64, device="cuda"), out=out),  # rows > max_f0_in
           lambda out: sm.push(good_x, good_f, n_valid=[160] * S, out=out),             # host n_valid
           lambda out: sm.push(good_x, good_f, n_valid=torch.full((S,), 160, dtype=torch.int32), out=out),
           lambda out: sm.push(good_x, good_f, n_f0=ints([4] * S).long(), out=out),
           lambda out: sm.push(good_x[:-1], good_f[:-1], out=out),
           lambda out: sm.push(good_x, good_f, out=dict(out, mcep=out["mcep"][:, :-1]))]
    res = run(sm, xs, f0s, [cut("pushes_of_160", len(x), len(f)) for x, f in zip(xs, f0s)], bad_calls=bad)
    check_equal(res, *offline())
    sm.status()


# ---------------------------------------------------------------------------------------------------- 9 graph capture
def test_a_captured_push_replayed_over_an_utterance_equals_the_eager_bits():
    from crank_amd import _lib
    from tests.test_gpu_logmel_shapes import _capture

    xs, f0s = streams()
    x, f0 = xs[1], f0s[1]
    mceps, sps = offline()
    sm = make(1, 160, 4)
    out = sm.empty_outputs(1, sp=True)
    st = dict(x=torch.zeros(1, 160, device="cuda"), f=torch.zeros(1, 4, dtype=torch.float64, device="cuda"),
              nv=ints([0]), nf=ints([0]), end=ints([0]))
    sm.push(st["x"], st["f"], st["nv"], st["nf"], st["end"], out=out)  # (a warm-up that brings nothing)
    torch.cuda.synchronize()
    allocs0 = _lib.lib().crk_debug_alloc_count()
    graph, _ = _capture(lambda: sm.push(st["x"], st["f"], st["nv"], st["nf"], st["end"], out=out))
    sm.reset()  # (a capture runs nothing; the handle is at the start of an utterance either way)
    sched = cut("pushes_of_160", len(x), len(f0))
    pieces, a, b = dict(mcep=[], sp=[]), 0, 0
    for i in range(len(sched)):
        last = i + 1 == len(sched)
        c, r = (len(x) - a, len(f0) - b) if last else sched[i]
        st["x"].fill_(float("nan"))
        st["f"].fill_(float("nan"))
        st["x"][0, :c].copy_(torch.from_numpy(x[a:a + c]))
        st["f"][0, :r].copy_(torch.from_numpy(f0[b:b + r]))
        st["nv"].fill_(c)
        st["nf"].fill_(r)
        st["end"].fill_(int(last))
        a, b = a + c, b + r
        graph.replay()
        n = int(out["n_frames"][0])
        for k in pieces:
            pieces[k].append(out[k][0, :n].clone())
    assert _lib.lib().crk_debug_alloc_count() == allocs0
    assert torch.equal(torch.cat(pieces["mcep"]), mceps[1]) and torch.equal(torch.cat(pieces["sp"]), sps[1])
    sm.status()
    del graph


# ---------------------------------------------------------------------------------------------------- 10 the chain
def test_streaming_f0_feeds_streaming_mcep_with_no_flag_at_the_helper_capacities():
    from crank_amd.world import StreamingMcep, analysis_capacities
    from tests.test_gpu_f0_stream import SPK_MEAN, SPK_STD, spk, voiced_silence_voiced

    x = voiced_silence_voiced(FS, (300, 150, 350), (151.3, 0, 118.0), 1)  # voiced, digital silence, voiced
    n, P = len(x), 1280
    from crank_amd.world import StreamingF0

    sf = StreamingF0(FS, [70], [400], SPK_MEAN, SPK_STD, P, shiftms=5)
    ring, queue = analysis_capacities(FS, SHIFT, sf.ahead_ms + sf.block_ms + 80, P, sf.max_frames)
    sm = StreamingMcep(FS, SHIFT, 1, P, sf.max_frames, queue, ring, dim=DIM, alpha=ALPHA, low_cut=LOW_CUT,
                       max_utt_frames=n // HOP + 2)
    o, c = spk([0]), spk([1])
    f_out, m_out = sf.empty_outputs(1, raw=True), sm.empty_outputs(1, sp=True)
    raw, mc, sp, at = [], [], [], 0
    while at < n:
        k = min(P, n - at)
        xx = torch.zeros(1, P, device="cuda")
        xx[0, :k] = torch.from_numpy(x[at:at + k]).cuda()
        at += k
        end = int(at == n)
        sf.push(xx, o, c, n_valid=[k], end=[end], out=f_out)
        sm.push(xx, f_out["raw"], ints([k]), f_out["n_frames"], ints([end]), out=m_out)
        nf, nm = int(f_out["n_frames"][0]), int(m_out["n_frames"][0])
        assert m_out["n_dropped"].tolist() == [0]
        raw.append(f_out["raw"][0, :nf, 0].clone())
        mc.append(m_out["mcep"][0, :nm].clone())
        sp.append(m_out["sp"][0, :nm].clone())
    sf.status()
    sm.status()
    contour = torch.cat(raw)
    assert contour.numel() == n // HOP + 1 and bool((contour > 0).any()) and bool((contour == 0).any())
    want_mc, want_sp = analyzer().mcep_batch([x], [contour], DIM, ALPHA, LOW_CUT, return_sp=True)
    got = torch.cat(mc)
    assert got.shape[0] == contour.numel()
    assert torch.equal(got, want_mc[0]) and torch.equal(torch.cat(sp), want_sp[0])
