"""crank_amd.live.LiveConverter(lookahead=True): the live loop on the recipe's default, non-causal generator - the fixture
generator of tests/stream_la_inputs.py with the layer, vocoder, scaler and signals of tests/test_gpu_live.py.  Cut
independence bit for bit, the generator's offline forward of the whole utterance on the rows the loop fed it, the offline
vocoder on the decoded utterance, utterances back to back, one shorter than the look-ahead, the reported latency.
Noise is zero throughout, so the waveform is a function of the decoded rows alone."""
import functools

import pytest
import torch

from tests.test_gpu_f0_stream import SPK_MEAN, SPK_STD, spk, voiced_silence_voiced
from tests.test_gpu_live import CV, CYCLE, FS, HOP, N_MELS, ORG, RANGE, drive, live, parts, same
from tests.test_gpu_stream_la import LaDev

pytestmark = pytest.mark.gpu

LA = 66


def la_live(S, max_samples):
    from crank_amd.live import LiveConverter

    p, dev = parts(), LaDev.of()
    assert not dev.fx.conf["causal"] and dev.fx.conf["decoder_f0"] and dev.fx.conf["input_size"] == N_MELS
    return LiveConverter(dev.G, p.layer, p.voc, S, max_samples, [RANGE[0]] * S, [RANGE[1]] * S, SPK_MEAN, SPK_STD, p.scaler,
                         lookahead=True)


def la_step(lc, org, cv, fed=None):
    """``drive``'s step on ``lc``: noise and sentinels over ``max_out`` frames; the decoded rows must be frame ``first + j``
    of the utterance.  fed: per stream a list that takes, per push, the rows the loop fed the generator (features,
    [lcf0, uv]) and the codes of the rows that left it."""
    S = lc.n_streams
    out = lc.empty_outputs(S, decoded=True)
    assert out["decoded"].shape[1] == lc.max_out == lc.max_chunk + LA and out["wave"].shape[1] == (lc.max_out + lc.sv.lookahead) * HOP
    noise = torch.zeros(S, lc.max_out * HOP, device="cuda")
    o, c = spk(org), spk(cv)
    emitted = [0] * S

    def step(x, counts, end):
        out["wave"].fill_(777.0)
        out["decoded"].fill_(777.0)
        res = lc.push(x, o, c, n_valid=counts, end=end, noise=noise, out=out)
        n, m, first = res["n_frames"].tolist(), res["n_out"].tolist(), res["first"].tolist()
        for s in range(S):
            assert bool((res["decoded"][s, n[s]:] == 777.0).all()) and bool((res["wave"][s, m[s]:] == 777.0).all())
            assert n[s] == 0 or first[s] == emitted[s], (s, first[s], emitted[s])
            emitted[s] = 0 if end[s] else emitted[s] + n[s]
            if fed is not None:
                k = int(lc._j["n_frames"][s])
                fed[s].append((lc._j["a"][s, :k].clone(), lc._j["b"][s, :k].clone(),
                               [q[s, :n[s]].clone() for q in lc._conv_out["qidx"]]))
        return [(res["decoded"][s, :n[s]].clone(), res["wave"][s, :m[s]].clone(), n[s]) for s in range(S)]

    return step


@functools.lru_cache(maxsize=None)
def base_run():
    """Both signals, one utterance per stream, pushes of 2048 samples; with what the generator was fed."""
    lc = la_live(2, 2048)
    fed = [[], []]
    res = drive(la_step(lc, ORG, CV, fed), [[x] for x in parts().xs], [2048])
    lc.status()
    return res, lc, fed


def test_cut_independence_the_offline_forward_and_the_offline_vocoder():
    from crank_amd import ops

    res, lc0, fed = base_run()
    p, dev = parts(), LaDev.of()
    lc = la_live(2, max(CYCLE))
    cyc = drive(la_step(lc, ORG, CV), [[x] for x in p.xs], CYCLE)
    lc.status()
    mean = torch.as_tensor(p.scaler["mlfb"].mean_, dtype=torch.float32, device="cuda")
    scale = torch.as_tensor(p.scaler["mlfb"].scale_, dtype=torch.float32, device="cuda")
    for s, x in enumerate(p.xs):
        a, b = res[s][0], cyc[s][0]
        assert a["n_frames"] != b["n_frames"] and same(a, b), s
        T = 1 + len(x) // HOP
        assert T > LA and a["decoded"].shape == (T, p.D) and a["wave"].shape == (T * HOP,)
        assert sum(a["n_frames"][:-1]) < T - LA + 1 and a["n_frames"][-1] >= LA  # the end push flushed the look-ahead
        off = p.voc.inference_batch([p.voc.normalize(a["decoded"] * scale + mean)], [torch.zeros(T * HOP, device="cuda")])[0]
        assert torch.equal(a["wave"], off), s
        # the generator's offline forward (bf16x3) of the whole utterance on the rows the loop fed it
        feats = torch.cat([f[0] for f in fed[s]])[None]
        cond = torch.cat([f[1] for f in fed[s]])[None]
        assert feats.shape[1] == T
        h = torch.full((1, T), CV[s], dtype=torch.int64, device="cuda")
        ops.set_precision("bf16x3")
        try:
            with torch.no_grad():
                ref = dev.G(feats, None, cond, spkrvec=h, use_ema=False)
            torch.cuda.synchronize()
        finally:
            ops.set_precision("bf16")
        for n in range(dev.fx.nst):
            assert torch.equal(torch.cat([f[2][n] for f in fed[s]]), ref["qidx"][n][0]), (s, n)
        err = float((a["decoded"] - ref["decoded"][0]).abs().max()) / float(ref["decoded"].abs().max())
        print(f"live look-ahead, stream {s}: decoded vs offline GPU bf16x3 max |diff| / max |ref| = {err:.3e} on {T} frames")
        assert err <= 1e-3


def test_two_utterances_back_to_back_and_one_shorter_than_the_lookahead():
    res, _, _ = base_run()
    xs = parts().xs
    short = voiced_silence_voiced(FS, (300,), (160.0,), 13)
    assert 0 < 1 + len(short) // HOP < LA
    lc = la_live(2, 2048)
    got = drive(la_step(lc, ORG, CV), [[xs[0], short, xs[0]], [xs[1]]], [2048], delays=[0, 6])
    lc.status()
    # stream 0 ends and starts over while stream 1 is in the middle of its utterance
    assert got[0][0]["end_push"] < got[1][0]["end_push"]
    assert same(got[0][0], res[0][0]) and same(got[1][0], res[1][0]) and same(got[0][2], res[0][0])
    alone = drive(la_step(la_live(1, 2048), ORG[:1], CV[:1]), [[short]], [2048])[0][0]
    n = 1 + len(short) // HOP
    assert same(got[0][1], alone) and alone["decoded"].shape[0] == n and len(alone["wave"]) == n * HOP
    assert sum(alone["n_frames"][:-1]) == 0 and alone["n_frames"][-1] == n  # nothing left before the end push


def test_latency_state_and_the_refusal_without_the_keyword():
    from crank_amd.live import LiveConverter
    from crank_amd.stream import LookaheadConverter

    _, lc, _ = base_run()
    causal = live(2, 2048)
    assert isinstance(lc.conv, LookaheadConverter) and lc.conv.lookahead == LA
    assert abs((lc.latency_ms - causal.latency_ms) - 1000.0 * LA * HOP / FS) < 1e-6
    assert lc.max_chunk == causal.max_chunk and lc.max_out == causal.max_chunk + LA and causal.max_out == causal.max_chunk
    assert lc.state_bytes > causal.state_bytes
    print(f"state bytes per stream: look-ahead loop {lc.state_bytes // 2} (converter {lc.conv.state_bytes // 2}, vocoder "
          f"{lc.sv.state_bytes // 2}), causal loop {causal.state_bytes // 2} (converter {causal.conv.state_bytes // 2}, "
          f"vocoder {causal.sv.state_bytes // 2})")
    p, dev = parts(), LaDev.of()
    with pytest.raises(NotImplementedError, match="causal") as err:
        LiveConverter(dev.G, p.layer, p.voc, 2, 2048, [RANGE[0]] * 2, [RANGE[1]] * 2, SPK_MEAN, SPK_STD, p.scaler)
    assert "66 frames after" in str(err.value)
    with pytest.raises(NotImplementedError, match="causal"):  # and the look-ahead loop is not for causal generators
        LiveConverter(p.dev.G, p.layer, p.voc, 2, 2048, [RANGE[0]] * 2, [RANGE[1]] * 2, SPK_MEAN, SPK_STD, p.scaler,
                      lookahead=True)
