"""Streaming F0 on the GPU (crank_amd.world.StreamingF0, csrc/f0_stream_kernels.hip): the raw contour bit for bit against
Harvest on host-cut windows of the whole signal's low cut, cut invariance, ragged streams with end / reuse / reset, the
conditioning values against float64 numpy, the carry path, the refusals, and the chain into StreamingConverter.
The grid and the expectation come from tests/f0_stream_ref.py with the GPU's own Harvest as the 1 ms estimator."""
import functools

import numpy as np
import pytest
import torch

from tests import f0_stream_ref as R

pytestmark = pytest.mark.gpu

N_SPK = 4
SPK_MEAN = np.array([4.9, 5.3, 4.6, 5.1])
SPK_STD = np.array([0.21, 0.17, 0.3, 0.25])
SCALER = (5.02, 0.31)
SENT = 12345.0


def _harmonics(rng, f0, n, fs):
    ph = 2 * np.pi * f0 * np.arange(n) / fs
    y = sum(rng.uniform(0.05, 0.3) * np.sin(h * ph + rng.uniform(0, 6.28)) for h in range(1, 9))
    return y + 1e-3 * rng.standard_normal(n)


def voiced_silence_voiced(fs, ms, f0s, seed):
    """Stretches of ms[i] milliseconds, voiced at f0s[i] Hz or digital silence where f0s[i] is 0; float32, odd length."""
    rng = np.random.default_rng(seed)
    parts = [np.zeros(m * fs // 1000) if f == 0 else _harmonics(rng, f, m * fs // 1000, fs) for m, f in zip(ms, f0s)]
    return np.concatenate(parts + [np.zeros(0) if f0s[-1] == 0 else _harmonics(rng, f0s[-1], 37, fs)]).astype(np.float32)


CASES = {
    "16k_shift5": dict(fs=16000, shiftms=5, hop=None, x=lambda: voiced_silence_voiced(16000, (300, 150, 350), (151.3, 0, 118.0), 1)),
    "22k_hop128": dict(fs=22050, shiftms=None, hop=128, x=lambda: voiced_silence_voiced(22050, (280, 140, 300), (203.7, 0, 171.0), 2)),
}


def make(fs, ranges, max_samples, shiftms=None, hop=None, scaler=SCALER, **kw):
    from crank_amd.world import StreamingF0

    return StreamingF0(fs, [r[0] for r in ranges], [r[1] for r in ranges], SPK_MEAN, SPK_STD, max_samples, shiftms=shiftms,
                       hop_size=hop, lcf0_scaler=scaler, **kw)


def spk(ids):
    return torch.tensor(ids, dtype=torch.int32, device="cuda")


def run(sf, xs, plan, org, cv, late_end=False):
    """xs: one float32 signal per stream; plan: per push the samples each stream takes (clipped to what it has left; the
    push that takes a stream's last sample carries its end flag, or with late_end an empty push behind it).  Returns per
    stream {lcf0, uv, raw, cv_f0} of its frames in order and the frames per push, after checking that no push wrote a row
    at or past n_frames."""
    S = len(xs)
    at, done = [0] * S, [len(x) == 0 for x in xs]
    got = [dict(lcf0=[], uv=[], raw=[], cv_f0=[], per=[]) for _ in xs]
    clean = torch.ones((), dtype=torch.bool, device="cuda")
    o, c = spk(org), spk(cv)
    for counts in plan:
        counts = [0 if done[s] else min(int(k), len(xs[s]) - at[s]) for s, k in enumerate(counts)]
        C = max(counts)
        x = np.zeros((S, C), np.float32)
        end = [0] * S
        for s, k in enumerate(counts):
            x[s, :k] = xs[s][at[s]:at[s] + k]
            at[s] += k
            if not done[s] and at[s] == len(xs[s]) and (not late_end or k == 0):
                end[s], done[s] = 1, True
        out = sf.empty_outputs(S, raw=True, cv_f0=True)
        for k in ("lcf0", "uv", "raw", "cv_f0"):
            out[k].fill_(SENT)
        res = sf.push(torch.from_numpy(x).cuda(), o, c, n_valid=counts, end=end, out=out)
        assert res is out
        nf = out["n_frames"].tolist()
        for s in range(S):
            assert 0 <= nf[s] <= sf.max_frames
            for k in ("lcf0", "uv", "raw", "cv_f0"):
                clean &= (out[k][s, nf[s]:] == SENT).all()
                got[s][k].append(out[k][s, :nf[s], 0].clone())
            got[s]["per"].append(nf[s])
        if all(done):
            break
    assert all(done) and bool(clean), "a push wrote rows at or past n_frames"
    sf.status()
    return [{k: (torch.cat(v).cpu().numpy() if k != "per" else v) for k, v in g.items()} for g in got]


def cut(n, sizes):
    return [(c,) for c in R.cut(n, sizes)]


def expect(x, fs, lo, hi, shiftms, hop, org, cv, scaler=SCALER, low_cut=70):
    """The definition with the GPU's own stages: WorldAnalyzer.low_cut_batch of the whole signal, every block's window cut
    on the host, HarvestF0(fs, 1).harvest of it alone; then float64 numpy to the conditioning values."""
    from crank_amd.world import HarvestF0, WorldAnalyzer
    from oracle.dataset import convert_f0

    y = torch.from_numpy(x).cuda().double() if low_cut is None else WorldAnalyzer(fs).low_cut_batch([torch.from_numpy(x).cuda()], low_cut)[0]
    hv = HarvestF0(fs, 1)
    est = lambda w: hv.harvest(torch.from_numpy(np.ascontiguousarray(w)).cuda(), lo, hi).cpu().numpy()  # noqa: E731
    raw, uv, cf0 = R.define(y.cpu().numpy(), R.Grid(fs, shiftms=shiftms, hop=hop), est, carry0=float(np.exp(SPK_MEAN[org])))
    cvl = convert_f0(np.log(cf0), SPK_MEAN[org], SPK_STD[org], SPK_MEAN[cv], SPK_STD[cv])
    lcf0 = (cvl - scaler[0]) / scaler[1] if scaler else cvl
    return dict(raw=raw, uv=uv, lcf0=lcf0, cv_f0=np.exp(cvl) * uv)


@functools.lru_cache(maxsize=None)
def case(name):
    """A case's signal, its expectation and the streamed baseline (pushes of 100 ms), computed once and left unchanged."""
    c = CASES[name]
    x, fs = c["x"](), c["fs"]
    want = expect(x, fs, 70, 400, c["shiftms"], c["hop"], 1, 2)
    sf = make(fs, [(70, 400)], len(x), c["shiftms"], c["hop"])
    got = run(sf, [x], cut(len(x), [fs // 10]), [1], [2])[0]
    return dict(x=x, fs=fs, want=want, got=got, sf=sf, **{k: c[k] for k in ("shiftms", "hop")})


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


# -------------------------------------------------------------------------------------------- 1 raw contour, 4 values
@pytest.mark.parametrize("name", list(CASES))
def test_raw_contour_is_harvest_of_each_window_bit_for_bit(name):
    c = case(name)
    g = R.Grid(c["fs"], shiftms=c["shiftms"], hop=c["hop"])
    T = g.frames(len(c["x"]))
    raw, want = c["got"]["raw"], c["want"]["raw"]
    assert raw.shape == want.shape == (T,)
    np.testing.assert_array_equal(raw, want)
    voiced = raw != 0
    assert voiced.sum() > 0.4 * T and (~voiced).sum() > 0.08 * T  # voiced - silence - voiced came through
    starts = np.flatnonzero(np.diff(voiced.astype(int)) == 1)
    assert len(starts) >= 1  # the contour is voiced again behind the silence


@pytest.mark.parametrize("name", list(CASES))
def test_conditioning_values_follow_float64_numpy(name):
    """uv exact; lcf0 within one fp32 ulp of continuous_f0 -> convert_f0 -> scaler in float64 (the float64 chain's own
    error, a few 1e-16 relative, is far below half an ulp: the single rounding differs by one unit at the most);
    cv_f0 = exp(cv_lcf0) uv within 1e-12 relative (float64, two library functions)."""
    c = case(name)
    got, want = c["got"], c["want"]
    np.testing.assert_array_equal(got["uv"], want["uv"])
    assert set(np.unique(got["uv"])) == {0.0, 1.0}
    d = np.abs(got["lcf0"].astype(np.float64) - want["lcf0"])
    print(name, "lcf0 max |diff| in ulp:", float((d / ulp32(want["lcf0"])).max()))
    assert (d <= ulp32(want["lcf0"])).all()
    np.testing.assert_allclose(got["cv_f0"], want["cv_f0"], rtol=1e-12, atol=0)
    assert sum(c["got"]["per"]) == len(want["uv"])


def test_without_low_cut_and_without_the_global_scaler():
    """The two switches off: the window is the raw signal, lcf0 is the converted value itself."""
    fs, org, cv = 16000, 2, 0
    x = voiced_silence_voiced(fs, (200, 120, 150), (164.0, 0, 98.0), 4)
    sf = make(fs, [(70, 400)], 2000, shiftms=5, scaler=None, low_cut=None)
    got = run(sf, [x], cut(len(x), [2000]), [org], [cv])[0]
    want = expect(x, fs, 70, 400, 5, None, org, cv, scaler=None, low_cut=None)
    np.testing.assert_array_equal(got["raw"], want["raw"])
    np.testing.assert_array_equal(got["uv"], want["uv"])
    assert (np.abs(got["lcf0"] - want["lcf0"]) <= ulp32(want["lcf0"])).all()
    np.testing.assert_allclose(got["cv_f0"], want["cv_f0"], rtol=1e-12, atol=0)


# -------------------------------------------------------------------------------------------- 2 cut invariance
def test_outputs_do_not_depend_on_the_cut():
    c = case("16k_shift5")
    x, fs, n = c["x"], c["fs"], len(c["x"])
    g = R.Grid(fs, shiftms=5)
    scheds = {"whole": [n], "block": R.cut(n, [g.Bs]), "primes": R.cut(n, [7, 0, 131, 1009, 2, 0, 3571, 13]),
              "edges": R.cut(n, [0, g.Bs + g.As - 1, 0, 1, 0, 3 * g.Bs + 5]), "late_end": R.cut(n, [3000]) + [0]}
    for name, counts in scheds.items():
        sf = make(fs, [(70, 400)], max(counts), shiftms=5)
        got = run(sf, [x], [(k,) for k in counts], [1], [2], late_end=name == "late_end")[0]
        for k in ("raw", "uv", "lcf0", "cv_f0"):
            np.testing.assert_array_equal(got[k], c["got"][k], err_msg=f"{name} {k}")
        assert max(got["per"]) <= sf.max_frames
        if name == "whole":  # everything in one push, in several rounds
            assert got["per"] == [len(c["got"]["uv"])] and sf.max_rounds > 5
    assert 0 in c["got"]["per"]  # a push with no ready block emits nothing


# -------------------------------------------------------------------------------------------- 3 ragged streams
@functools.lru_cache(maxsize=None)
def ragged():
    fs = 16000
    xs = [case("16k_shift5")["x"], voiced_silence_voiced(fs, (250, 120, 200), (96.4, 0, 230.0), 5),
          voiced_silence_voiced(fs, (420,), (310.0,), 6)]
    ranges, org, cv = [(70, 400), (40, 700), (70, 400)], [1, 0, 3], [2, 2, 0]
    alone = [run(make(fs, [ranges[s]], 4000, shiftms=5), [xs[s]], cut(len(xs[s]), [1600]), [org[s]], [cv[s]])[0] for s in range(3)]
    return dict(fs=fs, xs=xs, ranges=ranges, org=org, cv=cv, alone=alone)


def _ragged_plan(xs):
    pats = [(1600, 0, 3999, 16), (777, 2500, 0), (4000, 1, 1280, 0, 333)]
    plan, left, i = [], [len(x) for x in xs], 0
    while any(left):
        counts = tuple(min(p[i % len(p)], l) for p, l in zip(pats, left))
        left = [l - k for l, k in zip(left, counts)]
        plan.append(counts)
        i += 1
    return plan


def test_ragged_streams_equal_each_stream_alone_and_end_reuse_reset_behave():
    r = ragged()
    fs, xs = r["fs"], r["xs"]
    sf = make(fs, r["ranges"], 4000, shiftms=5)
    plan = _ragged_plan(xs)
    assert any(0 in p and max(p) > 0 for p in plan)
    together = run(sf, xs, plan, r["org"], r["cv"])
    for s in range(3):
        for k in ("raw", "uv", "lcf0", "cv_f0"):
            np.testing.assert_array_equal(together[s][k], r["alone"][s][k], err_msg=f"stream {s} {k}")
    assert np.array_equal(together[0]["raw"], case("16k_shift5")["got"]["raw"])
    # reuse: every stream ended, so the same object takes new utterances - here the signals in another order of rows
    # whose ranges agree (rows 0 and 2)
    swapped = [xs[2], xs[1], xs[0]]
    again = run(sf, swapped, _ragged_plan(swapped), [r["org"][2], r["org"][1], r["org"][0]], [r["cv"][2], r["cv"][1], r["cv"][0]])
    for a, s in ((0, 2), (1, 1), (2, 0)):
        for k in ("raw", "uv", "lcf0"):
            np.testing.assert_array_equal(again[a][k], r["alone"][s][k], err_msg=f"reuse row {a} {k}")
    # reset: streams 0 and 2 are abandoned mid-utterance and reset, stream 1 goes on; all three end as if alone
    o, c = spk(r["org"]), spk(r["cv"])
    half = torch.zeros(3, 4000, device="cuda")
    for s in range(3):
        half[s] = torch.from_numpy(xs[s][:4000]).cuda()
    sf.push(half, o, c)
    sf.reset([0, 2])
    rest = run(sf, [xs[0], xs[1][4000:], xs[2]], [(1600, 1600, 1600)] * 12, r["org"], r["cv"])
    np.testing.assert_array_equal(rest[0]["lcf0"], r["alone"][0]["lcf0"])
    np.testing.assert_array_equal(rest[2]["lcf0"], r["alone"][2]["lcf0"])
    n1 = len(r["alone"][1]["lcf0"])
    np.testing.assert_array_equal(rest[1]["lcf0"], r["alone"][1]["lcf0"][n1 - len(rest[1]["lcf0"]):])
    assert 0 < len(rest[1]["lcf0"]) < n1
    sf.reset()
    assert np.array_equal(run(sf, xs, plan, r["org"], r["cv"])[1]["raw"], r["alone"][1]["raw"])


def test_a_stream_shorter_than_harvests_minimum_emits_nothing():
    sf = make(16000, [(70, 400)], 4000, shiftms=5)
    x = case("16k_shift5")["x"]
    assert run(sf, [x[:63]], [(63,)], [0], [1])[0]["per"] == [0]
    got = run(sf, [x[:64]], [(64,)], [0], [1])[0]
    assert got["per"] == [1] and len(got["lcf0"]) == R.Grid(16000, shiftms=5).frames(64)


# -------------------------------------------------------------------------------------------- 5 carry
def test_silence_longer_than_a_window_emits_the_default_then_holds_the_last_cf0():
    from oracle.dataset import convert_f0

    fs, org, cv = 16000, 3, 1
    x = voiced_silence_voiced(fs, (600, 400, 700), (0, 143.9, 0), 9)
    sf = make(fs, [(70, 400)], 1600, shiftms=5)
    got = run(sf, [x], cut(len(x), [1600]), [org], [cv])[0]
    want = expect(x, fs, 70, 400, 5, None, org, cv)
    np.testing.assert_array_equal(got["raw"], want["raw"])
    np.testing.assert_array_equal(got["uv"], want["uv"])
    assert (np.abs(got["lcf0"] - want["lcf0"]) <= ulp32(want["lcf0"])).all()
    # block 0's window is the stream's first 180 ms, all silent: the default F0 of the source speaker, which convert_f0
    # maps onto the target speaker's mean
    first = np.float32((convert_f0(SPK_MEAN[org], SPK_MEAN[org], SPK_STD[org], SPK_MEAN[cv], SPK_STD[cv]) - SCALER[0]) / SCALER[1])
    assert (got["uv"][:16] == 0).all() and (np.abs(got["lcf0"][:16] - first) <= ulp32(first)).all()
    # the blocks from 1360 ms on see silence alone (their windows start 300 ms earlier, 60 ms behind the speech's end):
    # uv = 0 and the last cf0 emitted, unchanged to the end
    tail = got["lcf0"][1360 // 5:]
    assert len(tail) > 60 and (got["uv"][1360 // 5:] == 0).all() and (tail == tail[0]).all()
    assert tail[0] != first and (got["uv"] == 1).sum() > 60


# -------------------------------------------------------------------------------------------- 6 refusals
def test_refusals_leave_outputs_and_state_untouched():
    from crank_amd.world import StreamingF0

    c = case("16k_shift5")
    x, fs, n = c["x"], c["fs"], len(c["x"])
    for kw in (dict(shiftms=5, block_ms=30, fs=22050), dict(shiftms=5, hop_size=128), dict(), dict(shiftms=5, ahead_ms=0),
               dict(hop_size=8), dict(shiftms=5, back_ms=3), dict(shiftms=2.5)):
        with pytest.raises(ValueError):
            StreamingF0(kw.pop("fs", fs), [70], [400], SPK_MEAN, SPK_STD, 1600, **kw)
    for lo, hi in ((30, 400), (70, 900), (400, 70)):
        with pytest.raises(ValueError):
            StreamingF0(fs, [lo], [hi], SPK_MEAN, SPK_STD, 1600, shiftms=5)
    sf = make(fs, [(70, 400)], 1600, shiftms=5)
    o, cvs = spk([1]), spk([2])
    out = sf.empty_outputs(1, raw=True, cv_f0=True)
    for t in out.values():
        t.fill_(77)
    parts, at = [], 0
    bad = [lambda: sf.push(torch.zeros(1, 1600, dtype=torch.float64, device="cuda"), o, cvs, out=out),
           lambda: sf.push(torch.zeros(1, 1600), o, cvs, out=out),
           lambda: sf.push(torch.zeros(1600, device="cuda"), o, cvs, out=out),
           lambda: sf.push(torch.zeros(2, 1600, device="cuda"), o, cvs, out=out),
           lambda: sf.push(torch.zeros(1, 1601, device="cuda"), o, cvs, out=out),
           lambda: sf.push(torch.zeros(1, 1600, device="cuda"), o, cvs, n_valid=[1601], out=out),
           lambda: sf.push(torch.zeros(1, 1600, device="cuda"), o.long(), cvs, out=out),
           lambda: sf.push(torch.zeros(1, 1600, device="cuda"), o, cvs, out=dict(out, lcf0=out["lcf0"][:, :-1]))]
    i = 0
    while at < n:  # the refused pushes sit between the good ones of a whole utterance
        with pytest.raises((ValueError, RuntimeError)):
            bad[i % len(bad)]()
        i += 1
        assert all(bool((t == 77).all()) for t in out.values())
        k = min(1600, n - at)
        xx = torch.zeros(1, 1600, device="cuda")
        xx[0, :k] = torch.from_numpy(x[at:at + k]).cuda()
        at += k
        res = sf.push(xx, o, cvs, n_valid=[k], end=[int(at == n)])
        parts.append(res["lcf0"][0, :int(res["n_frames"][0]), 0].cpu().numpy())
    assert i >= len(bad)
    np.testing.assert_array_equal(np.concatenate(parts), c["got"]["lcf0"])
    sf.status()


# -------------------------------------------------------------------------------------------- 7 the chain
CHAIN_FS, CHAIN_HOP = 16000, 128


def _chain(dev, xs, sizes, org, cv):
    """wave -> (StreamingLogMel, StreamingF0) -> StreamingConverter in pushes of ``sizes`` samples (cycled).  The mel
    frames of a stream wait in a queue until their F0 frames arrive.  Returns per stream the decoded frames, indices,
    quantizer inputs and the lcf0 / uv / mel rows the converter was fed, and the longest wait in frames."""
    import types

    from crank_amd.net.module.mlfb import LogMelFilterBankLayer
    from crank_amd.stream import StreamingConverter

    S, nst = len(xs), dev.fx.nst
    layer = LogMelFilterBankLayer(fs=CHAIN_FS, hop_size=CHAIN_HOP, fft_size=1024, center=True, n_mels=80,
                                  scaler=types.SimpleNamespace(mean_=np.full(80, -4.0), var_=np.full(80, 4.0)))
    lm = layer.streaming(S, max(sizes))
    sf = make(CHAIN_FS, [(70, 400)] * S, max(sizes), hop=CHAIN_HOP)
    conv = StreamingConverter(dev.G, S, lm.max_frames + sf.max_frames)
    o, c = spk(org), spk(cv)
    at, done, i, waited = [0] * S, [False] * S, 0, 0
    mel_q = [torch.zeros(0, 80, device="cuda") for _ in xs]
    f0_q = [torch.zeros(0, 2, device="cuda") for _ in xs]
    got = [dict(decoded=[], mel=[], f0=[], qidx=[[] for _ in range(nst)], encoded=[[] for _ in range(nst)]) for _ in xs]
    while not all(done):
        C = sizes[i % len(sizes)]
        i += 1
        counts, end = [0] * S, [0] * S
        x = torch.zeros(S, C, device="cuda")
        for s in range(S):
            if done[s]:
                continue
            counts[s] = min(C, len(xs[s]) - at[s])
            x[s, :counts[s]] = torch.from_numpy(xs[s][at[s]:at[s] + counts[s]]).cuda()
            at[s] += counts[s]
            end[s] = int(at[s] == len(xs[s]))
            done[s] = bool(end[s])
        m = lm.push(x, n_valid=torch.tensor(counts, device="cuda"), end=torch.tensor(end, device="cuda"))
        f = sf.push(x, o, c, n_valid=counts, end=end)
        nm, nf = m["n_frames"].tolist(), f["n_frames"].tolist()
        take = [0] * S
        for s in range(S):
            mel_q[s] = torch.cat([mel_q[s], m["feats"][s, :nm[s]]])
            f0_q[s] = torch.cat([f0_q[s], torch.cat([f["lcf0"][s, :nf[s]], f["uv"][s, :nf[s]]], -1)])
            take[s] = min(len(mel_q[s]), len(f0_q[s]))
            waited = max(waited, len(mel_q[s]) - take[s])
            assert len(f0_q[s]) <= len(mel_q[s])  # the F0 frames never run ahead: they are the later ones
        K = max(take)
        if K == 0:
            continue
        feats, lcf0, uv = torch.zeros(S, K, 80, device="cuda"), torch.zeros(S, K, 1, device="cuda"), torch.zeros(S, K, 1, device="cuda")
        for s in range(S):
            feats[s, :take[s]], lcf0[s, :take[s]], uv[s, :take[s]] = mel_q[s][:take[s]], f0_q[s][:take[s], :1], f0_q[s][:take[s], 1:]
        out = conv.push(feats, lcf0, uv, c.long(), n_valid=torch.tensor(take, device="cuda"))
        for s in range(S):
            k = take[s]
            got[s]["decoded"].append(out["decoded"][s, :k].clone())
            got[s]["mel"].append(mel_q[s][:k])
            got[s]["f0"].append(f0_q[s][:k])
            for n in range(nst):
                got[s]["qidx"][n].append(out["qidx"][n][s, :k].clone())
                got[s]["encoded"][n].append(out["encoded"][n][s, :k].clone())
            mel_q[s], f0_q[s] = mel_q[s][k:], f0_q[s][k:]
    assert all(len(q) == 0 for q in mel_q + f0_q)
    sf.status()
    res = [dict(decoded=torch.cat(g["decoded"]), mel=torch.cat(g["mel"]), f0=torch.cat(g["f0"]),
                qidx=[torch.cat(q) for q in g["qidx"]], encoded=[torch.cat(e) for e in g["encoded"]]) for g in got]
    return res, waited


def test_chain_into_the_converter_is_cut_independent_and_equals_the_offline_forward():
    """A causal decoder_f0 generator (the streaming tests' fixture) fed by StreamingLogMel and StreamingF0.  Against the
    package's offline forward (bf16x3) on the same mel frames and the same streamed lcf0 / uv: test_gpu_stream.py's bound -
    identical indices on the frames the code margins keep, decoded within 1e-3 of the largest value."""
    from crank_amd import ops
    from tests import stream_inputs as SI
    from tests.test_gpu_stream import Dev, rel_err

    dev = Dev.of()
    assert dev.fx.conf["causal"] and dev.fx.conf["decoder_f0"]
    xs = [voiced_silence_voiced(CHAIN_FS, (420, 160, 500), (131.0, 0, 187.0), 11),
          voiced_silence_voiced(CHAIN_FS, (700,), (243.0,), 12)]
    org, cv = [0, 2], [1, 3]
    a, waited = _chain(dev, xs, [2048], org, cv)
    b, _ = _chain(dev, xs, [777, 4001, 1, 1280, 3000], org, cv)
    assert waited >= (100 + 0) * CHAIN_FS // 1000 // CHAIN_HOP  # mel frames were held for at least the look-ahead
    for s, x in enumerate(xs):
        T = 1 + len(x) // CHAIN_HOP
        assert a[s]["decoded"].shape == (T, dev.fx.conf["output_size"])
        for k in ("decoded", "mel", "f0"):
            assert torch.equal(a[s][k], b[s][k]), (s, k)
        assert all(torch.equal(p, q) for p, q in zip(a[s]["qidx"], b[s]["qidx"]))
        # the offline forward on this stream alone
        h = torch.full((1, T), cv[s], dtype=torch.long, device="cuda")
        ops.set_precision("bf16x3")
        try:
            with torch.no_grad():
                ref = dev.G(a[s]["mel"][None], None, a[s]["f0"][None], spkrvec=h, use_ema=False)
            torch.cuda.synchronize()
        finally:
            ops.set_precision("bf16")
        nst, above = dev.fx.nst, np.zeros((1, T), bool)
        left = 0
        for n in reversed(range(nst)):
            low = (SI.margins(a[s]["encoded"][n].cpu().numpy(), dev.fx.codebooks[n]) <= SI.MARGIN)[None]
            keep = ~(low | above)
            above = above | SI.downstream(low, dev.fx.reach)
            left += int((~keep).sum())
            differ = int((a[s]["qidx"][n].cpu() != ref["qidx"][n][0].cpu())[torch.as_tensor(keep[0])].sum())
            assert differ == 0, (s, n, differ)
        left += int(above.sum())
        assert left / ((nst + 1) * T) <= SI.MAX_LEFT_OUT, (s, left)
        err = rel_err(a[s]["decoded"][None].cpu(), ref["decoded"].cpu(), ~above)
        print(f"chain stream {s}: decoded max |diff| / max |ref| = {err:.3e} on {int((~above).sum())} of {T} frames")
        assert err <= 1e-3, (s, err)


def test_a_reset_with_an_id_out_of_range_is_the_librarys_error():
    sf = make(16000, [(70, 400)], 1600, shiftms=5)
    with pytest.raises(RuntimeError):
        sf.reset([1])
