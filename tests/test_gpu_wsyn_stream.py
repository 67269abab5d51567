"""Streaming WORLD synthesis on the GPU (crank_amd.world.StreamingWorldSynthesizer, csrc/world_stream_kernels.hip;
DESIGN.md section 6p): the samples WorldSynthesizer.synthesis_batch writes for the whole utterance, bit for bit under
every cut, for four ragged streams of 60, 41, 33 and 2 frames at fs 16000, shiftms 5, 25 coefficients, 1 band.

One deviation from the set-up this was asked with: at 16 kHz and 5 ms no pulse interval can exceed 1024 samples (the
time base's floor is 16 Hz, 1000 samples a cycle, and the two half-frame ramps next to unvoiced rows add 20.5 at the
most: crank_amd.world.longest_pulse_interval gives 1021).  The 17 Hz rows next to zeros are there and their interval is
asserted above 700, and above 900 in the 60-frame stream; the min(ns, 1024) branch is reached by a test of its own at
22050 Hz and 30 ms frames, where the ramps are long enough (ns > 1024 asserted)."""
import functools

import numpy as np
import pytest
import torch

from tests import world_synth_ref as R
from tests import wsyn_stream_ref as W
from tests.world_inputs import with_f0
from tests.wsyn_inputs import ALPHA, FS, SHIFTMS, streams

pytestmark = pytest.mark.gpu

ORDER1, BANDS, SENT = 25, 1, -12345.0
NAN = float("nan")


def ints(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def utts():
    rng = np.random.default_rng(11)
    return [with_f0(rng, f0, ORDER1, BANDS) for f0 in streams()]


@functools.lru_cache(maxsize=None)
def synthesizer(fs=FS, shiftms=SHIFTMS):
    from crank_amd.world import WorldSynthesizer

    return WorldSynthesizer(fs, 1024, shiftms, ALPHA)


@functools.lru_cache(maxsize=None)
def offline(pm):
    u = utts()
    return synthesizer().synthesis_batch([x[0] for x in u], [x[1] for x in u], [x[2] for x in u],
                                         [x[3] for x in u] if pm else None)


def make(S, R_, pm, **kw):
    kw.setdefault("max_utt_samples", 8192)
    return synthesizer().streaming(S, R_, ORDER1, power_mod=pm, **kw)


def sched(kind, T, most=16):
    """A stream's pushes as (rows, end) pairs."""
    if kind == "single":
        return [(T, 1)]
    if kind == "one_row":
        return [(1, int(k == T - 1)) for k in range(T)]
    sizes, k, pat = [], 0, [3, 1, 7, 2, most, 5, 1, 1, 9, 4]
    while k < T:
        c = min(pat[len(sizes) % len(pat)], T - k)
        sizes.append(c)
        k += c
    if kind == "end_alone":
        return [(c, 0) for c in sizes] + [(0, 1)]
    assert kind == "irregular"
    return [(c, int(i == len(sizes) - 1)) for i, c in enumerate(sizes)]


def drive(sw, data, scheds, out=None, push=None):
    """Pushes each stream's rows by its schedule, all streams in lock-step; rows past a stream's count are NaN and y is
    filled with a sentinel before every push.  Returns per stream (samples, emitted counts per push)."""
    S, Rm, pm = sw.n_streams, sw.max_rows_in, sw.power_mod
    out = sw.empty_outputs() if out is None else out
    at, pieces, counts = [0] * S, [[] for _ in range(S)], [[] for _ in range(S)]
    for p in range(max(len(s) for s in scheds)):
        f0 = torch.full((S, Rm), NAN, dtype=torch.float64)
        mc, cap = torch.full((S, Rm, ORDER1), NAN, dtype=torch.float64), torch.full((S, Rm, BANDS), NAN, dtype=torch.float64)
        rm = torch.full((S, Rm, ORDER1), NAN, dtype=torch.float64)
        nr, en = [], []
        for s in range(S):
            c, e = scheds[s][p] if p < len(scheds[s]) else (0, 0)
            sl = slice(at[s], at[s] + c)
            for dst, src in ((f0, data[s][0]), (mc, data[s][1]), (cap, data[s][2]), (rm, data[s][3])):
                dst[s, :c] = torch.from_numpy(np.ascontiguousarray(src[sl]))
            at[s] += c
            nr.append(c)
            en.append(e)
        out["y"].fill_(SENT)
        args = (f0.cuda(), mc.cuda(), cap.cuda(), rm.cuda() if pm else None, ints(nr), ints(en))
        if push is None:
            sw.push(*args, out=out)
        else:
            push(*args)
        n = out["n_samples"].tolist()
        for s in range(S):
            assert bool((out["y"][s, n[s]:] == SENT).all()), "written at or past n_samples"
            pieces[s].append(out["y"][s, :n[s]].clone())
            counts[s].append(n[s])
    return [torch.cat(p) for p in pieces], counts


# ---------------------------------------------------------------------------------------------------- 0 the edges
def test_the_contours_reach_their_edges():
    f0s = streams()
    assert [len(f) for f in f0s] == [60, 41, 33, 2]
    floor = FS // 1024 + 1
    sets = [R.pulses(f, FS, 1024, SHIFTMS) for f in f0s]
    for f0, (pos, ns, shift, pvuv, ylen) in zip(f0s[:2], sets[:2]):
        assert ((f0 > 0) & (f0 < floor)).sum() == 1 and (f0 == 17.0).any() and (f0 == 800.0).sum() == 1
        assert np.count_nonzero(np.diff((f0 >= floor).astype(int))) >= 6  # runs entered and left from both sides
        assert ns.max() > 700, ns.max()  # (1021 is the most at this rate and shift: see the module's docstring)
        assert pos[0] < 512 and pos[-1] > ylen - 512
        assert (pvuv == 1).any() and (pvuv == 0).any()
    assert sets[0][1].max() > 900  # a whole cycle of the 17 Hz run
    assert tuple(f0s[1][-2:]) == (300.0, 100.0)  # the extrapolated knot is -100 Hz
    assert (f0s[2] == 0).all() and len(sets[2][0]) > 50
    for pos, ns, _, _, ylen in sets:
        assert pos[0] < 512 and pos[-1] > ylen - 512


# ---------------------------------------------------------------------------------------------------- 1 the bits
@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("kind", ["single", "one_row", "irregular", "end_alone"])
def test_streamed_samples_are_the_offline_bits_under_every_cut(kind, pm):
    data, want = utts(), offline(pm)
    sw = make(4, 60 if kind == "single" else 16, pm)
    got, counts = drive(sw, data, [sched(kind, len(u[0])) for u in data])
    sw.status()
    for s in range(4):
        assert sum(counts[s]) == R.y_length(len(data[s][0]), FS, SHIFTMS) == want[s].numel()
        assert torch.equal(got[s], want[s]), (s, float((got[s] - want[s]).abs().max()))


def test_the_long_interval_branch_at_30_ms_frames():
    fs, shiftms = 22050, 30.0
    rng = np.random.default_rng(0)
    lo = fs // 1024 + 1
    f0 = lo + rng.uniform(0, 1.5, 12)
    f0[rng.random(12) < 0.35] = 0.0
    f0, mc, cap, rmc = with_f0(rng, f0, ORDER1, R.n_bands(fs))
    ns = R.pulses(f0, fs, 1024, shiftms)[1]
    assert ns.max() > 1024, ns.max()
    ws = synthesizer(fs, shiftms)
    want = ws.synthesis(f0, mc, cap, rmc)
    sw = ws.streaming(1, 4, ORDER1, power_mod=True, max_utt_samples=1 << 14)
    pieces, k = [], 0
    for c in (3, 1, 4, 2, 2):
        end = int(k + c == 12)
        t = [torch.from_numpy(np.ascontiguousarray(a[k:k + c]))[None].cuda() for a in (f0, mc, cap, rmc)]
        out = sw.push(*t, end=ints([end]))
        pieces.append(out["y"][0, :int(out["n_samples"][0])].clone())
        k += c
    sw.status()
    assert torch.equal(torch.cat(pieces), want)


# ---------------------------------------------------------------------------------------------------- 2 ragged
def test_ragged_streams_together_equal_each_stream_alone():
    data = utts()
    together, _ = drive(make(4, 16, True), data, [sched("irregular", len(u[0])) for u in data])
    for s in (1, 3):
        alone, _ = drive(make(1, 16, True), [data[s]], [sched("irregular", len(data[s][0]))])
        assert torch.equal(alone[0], together[s])


# ---------------------------------------------------------------------------------------------------- 3 a second one
def test_a_second_utterance_after_an_end_push_and_after_reset_equals_a_fresh_handle():
    data, want = utts(), offline(False)
    sw = make(1, 16, False)
    first, _ = drive(sw, [data[3]], [sched("single", 2)])
    assert torch.equal(first[0], want[3])
    second, _ = drive(sw, [data[1]], [sched("irregular", 41)])
    assert torch.equal(second[0], want[1])
    drive(sw, [data[0]], [sched("irregular", 60)[:4]])  # an utterance left open
    sw.reset()
    third, _ = drive(sw, [data[1]], [sched("one_row", 41)])
    assert torch.equal(third[0], want[1])
    sw.status()


# ---------------------------------------------------------------------------------------------------- 4 the definition
@pytest.mark.parametrize("s,pm", [(0, True), (1, False)])
def test_against_the_definition_in_sets_within_the_offline_bound(s, pm):
    u = utts()[s]
    sc = sched("irregular", len(u[0]))
    got, counts = drive(make(1, 16, pm), [u], [sc])
    st = W.Stream(FS, SHIFTMS, ALPHA, pm)
    ref, rcounts = W.run(st, u[0], u[1], u[2], u[3] if pm else None, [c for c, _ in sc])
    assert counts[0] == rcounts
    err = np.linalg.norm(got[0].cpu().numpy() - ref) / np.linalg.norm(ref)
    print("relative L2 against the definition:", err)
    assert err < 1e-9, err


# ---------------------------------------------------------------------------------------------------- 5 the flags
def _victim_and_witness(victim_sched, victim_data, witness=1, kind="irregular", **kw):
    """Stream 0 runs `victim_sched`, stream 1 the utterance `witness`; returns (handle, outputs of the last push, the
    victim's (samples, counts)) after asserting the witness's bits."""
    data, want = utts(), offline(False)
    sw = make(2, 16, False, **kw)
    out = sw.empty_outputs()
    got, counts = drive(sw, [victim_data, data[witness]], [victim_sched, sched(kind, len(data[witness][0]))], out=out)
    assert torch.equal(got[1], want[witness])
    return sw, out, (got[0], counts[0])


def test_a_queue_one_row_short_sets_flag_2():
    from crank_amd.world import synthesis_capacities

    u = utts()[0]
    sc = sched("one_row", 60)  # (the rows held are most behind the 17 Hz run's pending pulse)
    caps = synthesis_capacities(FS, SHIFTMS, 16, 1000.0)
    st = W.Stream(FS, SHIFTMS, ALPHA, responses=False)
    need, k = 0, 0
    for c, e in sc:  # the most rows the queue holds on this schedule
        need = max(need, len(st.f0) - st.row_lo + c)
        st.push(u[0][k:k + c], end=bool(e))
        k += c
    assert need > 10  # the unvoiced witness, a row a push, holds 4 at the most: the shorter queue is short for the victim alone
    sw, _, (y, _) = _victim_and_witness(sc, u, witness=2, kind="one_row", capacities=dict(caps, rows=need))
    assert sw.flags() == [0, 0] and torch.equal(y, offline(False)[0])
    sw, _, _ = _victim_and_witness(sc, u, witness=2, kind="one_row", capacities=dict(caps, rows=need - 1))
    assert sw.flags() == [W.FLAG_QUEUE, 0]
    with pytest.raises(RuntimeError, match="row queue"):
        sw.status()


def test_a_noise_table_one_sample_short_sets_flag_4():
    u, want = utts()[0], offline(False)[0]
    sc = sched("irregular", 60)
    st = W.Stream(FS, SHIFTMS, ALPHA, responses=False)
    W.run(st, u[0], None, None, None, [c for c, _ in sc])
    need = max(off + min(ns, 1024) for _, ns, _, _, off in st.added if ns > 0)
    sw, _, (y, _) = _victim_and_witness(sc, u, max_utt_samples=need)
    assert sw.flags() == [0, 0] and torch.equal(y, want)
    sw, _, _ = _victim_and_witness(sc, u, max_utt_samples=need - 1)
    assert sw.flags() == [W.FLAG_NOISE, 0]


def test_bad_f0_rows_set_flag_16_and_are_synthesised_as_unvoiced():
    f0, mc, cap, rmc = utts()[1]
    bad, zeroed = f0.copy(), f0.copy()
    bad[[4, 20, 30]] = (NAN, -3.0, 1000.5)
    zeroed[[4, 20, 30]] = 0.0
    want = synthesizer().synthesis(zeroed, mc, cap)
    sw, _, (y, _) = _victim_and_witness(sched("irregular", 41), (bad, mc, cap, rmc))
    assert sw.flags() == [W.FLAG_F0, 0]
    assert torch.equal(y, want)


def test_an_end_with_one_row_sets_flag_8_and_an_end_on_an_empty_stream_none():
    u = utts()[0]
    sw, out, (y, counts) = _victim_and_witness([(0, 1), (1, 1)], u)
    assert sw.flags() == [W.FLAG_SHORT, 0] and y.numel() == 0 and sum(counts) == 0
    sw2 = make(1, 16, False)
    o = sw2.push(*[torch.from_numpy(np.ascontiguousarray(a[:1]))[None].cuda() for a in u[:3]], end=ints([1]))
    assert o["n_dropped"].tolist() == [1] and o["n_samples"].tolist() == [0]
    o = sw2.push(*[torch.from_numpy(np.ascontiguousarray(a[:0]))[None].cuda() for a in u[:3]], end=ints([1]))
    assert o["n_dropped"].tolist() == [0] and sw2.flags() == [W.FLAG_SHORT]
    sw2.reset()
    assert sw2.flags() == [0]
    got, _ = drive(sw2, [utts()[1]], [sched("irregular", 41)])  # the stream is at its start state
    assert torch.equal(got[0], offline(False)[1])


# ---------------------------------------------------------------------------------------------------- 6 refusals
def test_refused_calls_leave_outputs_and_state_untouched():
    u, want = utts()[1], offline(True)[1]
    sw = make(1, 16, True)
    plain = make(1, 16, False)
    out = sw.empty_outputs()
    sc = sched("irregular", 41)
    half = len(sc) // 2
    first, _ = drive(sw, [u], [sc[:half]], out=out)
    rows = sum(c for c, _ in sc[:half])
    t = [torch.from_numpy(np.ascontiguousarray(a[rows:rows + 4]))[None].cuda() for a in u]
    f0, mc, cap, rm = t
    for o in out.values():
        o.fill_(-7)
    refused = [lambda: sw.push(f0, mc, cap, None, out=out),                        # rmcep missing
               lambda: plain.push(f0, mc, cap, rm),                                # rmcep without power modification
               lambda: sw.push(f0, mc[:, :3], cap, rm, out=out),                   # shapes differ
               lambda: sw.push(f0, mc.float(), cap, rm, out=out),                  # dtype
               lambda: sw.push(f0.cpu(), mc, cap, rm, out=out),                    # device
               lambda: sw.push(f0, mc, cap[:, :, :0], rm, out=out),                # bands
               lambda: sw.push(f0, mc, cap, rm, n_rows=torch.tensor([4]), out=out),  # counts on the host
               lambda: sw.push(f0, mc, cap, rm, out=dict(out, y=out["y"][:, :-1])),
               lambda: sw.push(*[torch.cat([a] * 5, 1) for a in t], out=out)]      # 20 rows, max_rows_in is 16
    for call in refused:
        with pytest.raises(ValueError):
            call()
    assert all(bool((o == -7).all()) for o in out.values())
    rest, _ = drive(sw, [tuple(a[rows:] for a in u)], [sc[half:]], out=out)
    assert torch.equal(torch.cat([first[0], rest[0]]), want)
    sw.status()


# ---------------------------------------------------------------------------------------------------- 7 capture
def test_a_captured_push_replayed_over_an_utterance_equals_the_eager_bits():
    from crank_amd import _lib
    from tests.test_gpu_logmel_shapes import _capture

    u, want = utts()[1], offline(True)[1]
    sw = make(1, 16, True)
    out = sw.empty_outputs()
    st = dict(f0=torch.zeros(1, 16, dtype=torch.float64, device="cuda"),
              mc=torch.zeros(1, 16, ORDER1, dtype=torch.float64, device="cuda"),
              cap=torch.zeros(1, 16, BANDS, dtype=torch.float64, device="cuda"),
              rm=torch.zeros(1, 16, ORDER1, dtype=torch.float64, device="cuda"), nr=ints([0]), end=ints([0]))
    call = lambda: sw.push(st["f0"], st["mc"], st["cap"], st["rm"], st["nr"], st["end"], out=out)  # noqa: E731
    call()  # (a warm-up that brings nothing)
    torch.cuda.synchronize()
    allocs0 = _lib.lib().crk_debug_alloc_count()
    graph, _ = _capture(call)
    sw.reset()  # (a capture runs nothing; the handle is at the start of an utterance either way)

    def replay(f0, mc, cap, rm, nr, end):
        for k, v in (("f0", f0), ("mc", mc), ("cap", cap), ("rm", rm), ("nr", nr), ("end", end)):
            st[k].copy_(v)
        graph.replay()

    got, counts = drive(sw, [u], [sched("irregular", 41)], out=out, push=replay)
    assert _lib.lib().crk_debug_alloc_count() == allocs0
    assert sum(counts[0]) == want.numel() and torch.equal(got[0], want)
    sw.status()
    del graph


# ---------------------------------------------------------------------------------------------------- 8 the chain
def test_streaming_mcep_feeds_streaming_synthesis():
    from crank_amd.world import StreamingMcep, WorldAnalyzer, analysis_capacities

    dim, P, frames = ORDER1 - 1, 1280, 50
    rng = np.random.default_rng(5)
    n = frames * 80
    t = np.arange(n) / FS
    x = (0.3 * np.sin(2 * np.pi * 140.0 * t) + 0.1 * np.sin(2 * np.pi * 420.0 * t) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    T = n // 80 + 1
    f0 = np.full(T, 140.0)
    f0[20:26] = 0.0
    cap = np.where(f0[:, None] > 0, -20.0, 0.0)
    ring, queue = analysis_capacities(FS, SHIFTMS, 0.0, P, 17)
    sm = StreamingMcep(FS, SHIFTMS, 1, P, 17, queue, ring, dim=dim, alpha=ALPHA, max_utt_frames=T + 2)
    sw = make(1, sm.max_frames, True, max_utt_samples=n + 1024)
    m_out = sm.empty_outputs(1)
    pieces, at, row, frame = [], 0, 0, 0
    while at < n:
        k = min(P, n - at)
        xx = torch.zeros(1, P, device="cuda")
        xx[0, :k] = torch.from_numpy(x[at:at + k]).cuda()
        at += k
        end = int(at == n)
        r = T - row if end else min(16, T - row)
        ff = torch.zeros(1, 17, dtype=torch.float64, device="cuda")
        ff[0, :r] = torch.from_numpy(f0[row:row + r]).cuda()
        row += r
        sm.push(xx, ff, ints([k]), ints([r]), ints([end]), out=m_out)
        nm = int(m_out["n_frames"][0])
        F = sm.max_frames
        f_in = torch.zeros(1, F, dtype=torch.float64, device="cuda")
        c_in = torch.zeros(1, F, BANDS, dtype=torch.float64, device="cuda")
        f_in[0, :nm] = torch.from_numpy(f0[frame:frame + nm]).cuda()
        c_in[0, :nm] = torch.from_numpy(cap[frame:frame + nm]).cuda()
        frame += nm
        o = sw.push(f_in, m_out["mcep"], c_in, m_out["mcep"], n_rows=m_out["n_frames"], end=ints([end]))
        assert o["n_dropped"].tolist() == [0]
        pieces.append(o["y"][0, :int(o["n_samples"][0])].clone())
    sm.status()
    sw.status()
    assert frame == T
    mc = WorldAnalyzer(FS, 1024, SHIFTMS).mcep_batch([x], [f0], dim, ALPHA)[0]
    want = synthesizer().synthesis(f0, mc, cap, mc)
    assert torch.equal(torch.cat(pieces), want)
