"""crank_amd.live.LiveConverter - samples in, converted samples out - against the host loop it replaces (the four public
stages joined by Python queues and ``.tolist()`` read-backs, as INTEGRATION.md section O documented it), bit for bit: the
join only moves rows, ``crk_feat_renorm`` has torch's bits, and the converter and the vocoder do not depend on the cut.
Noise is zero throughout, so the waveform is a function of the decoded rows alone."""
import functools
import types

import numpy as np
import pytest
import torch

from tests.pwg_vocoder_ref import checkpoint_of, random_generator
from tests.test_gpu_f0_stream import SCALER, SPK_MEAN, SPK_STD, spk, voiced_silence_voiced

pytestmark = pytest.mark.gpu

FS, HOP, N_FFT, N_MELS = 16000, 128, 1024, 80
RANGE = (70, 400)
CYCLE = [777, 4001, 1, 1280, 3000]
ORG, CV = [0, 2], [1, 3]


@functools.lru_cache(maxsize=None)
def parts():
    """The causal decoder_f0 generator of the streaming tests, the chain test's log-mel layer, a small random vocoder on
    the generator's output width, crank's scaler and the chain test's two signals."""
    from crank_amd.net.module.mlfb import LogMelFilterBankLayer
    from crank_amd.vocoder import ParallelWaveGANVocoder
    from tests.test_gpu_stream import Dev

    dev = Dev.of()
    assert dev.fx.conf["causal"] and dev.fx.conf["decoder_f0"] and dev.fx.conf["input_size"] == N_MELS
    D = dev.fx.conf["output_size"]
    layer = LogMelFilterBankLayer(fs=FS, hop_size=HOP, fft_size=N_FFT, center=True, n_mels=N_MELS,
                                  scaler=types.SimpleNamespace(mean_=np.full(N_MELS, -4.0), var_=np.full(N_MELS, 4.0)))
    params = dict(layers=6, stacks=2, aux_channels=D, upsample_params={"upsample_scales": [2, 4, 4, 4]})
    rs = np.random.RandomState(3)
    stats = (rs.standard_normal(D).astype(np.float32), rs.uniform(0.5, 2.0, D).astype(np.float32))
    voc = ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(random_generator(6, **params)),
                                                 {"generator_params": params, "hop_size": HOP}, stats=stats, device="cuda")
    scaler = {"mlfb": types.SimpleNamespace(mean_=rs.standard_normal(D).astype(np.float32),
                                            scale_=rs.uniform(0.5, 2.0, D).astype(np.float32)),
              "lcf0": types.SimpleNamespace(mean_=np.array([SCALER[0]]), scale_=np.array([SCALER[1]]))}
    xs = [voiced_silence_voiced(FS, (420, 160, 500), (131.0, 0, 187.0), 11),
          voiced_silence_voiced(FS, (700,), (243.0,), 12)]
    return types.SimpleNamespace(dev=dev, layer=layer, voc=voc, scaler=scaler, xs=xs, D=D)


def live(S, max_samples):
    from crank_amd.live import LiveConverter

    p = parts()
    return LiveConverter(p.dev.G, p.layer, p.voc, S, max_samples, [RANGE[0]] * S, [RANGE[1]] * S, SPK_MEAN, SPK_STD, p.scaler)


def drive(step, utts, sizes, delays=None):
    """Feeds ``step(x, counts, end)`` pushes of ``sizes`` samples (cycled): stream s waits ``delays[s]`` pushes
    (n_valid = 0), then takes the signals of ``utts[s]`` one after the other, the end flag on the push with an utterance's
    last sample.  ``step`` returns per stream (decoded rows, samples, n_frames).  Returns per stream and utterance
    ``decoded``, ``wave``, the per-push ``n_frames`` and ``end_push``, the index of the push that carried its end flag."""
    S = len(utts)
    delays = [0] * S if delays is None else delays
    which, at, i = [0] * S, [0] * S, 0
    got = [[dict(decoded=[], wave=[], n_frames=[]) for _ in u] for u in utts]
    while any(which[s] < len(utts[s]) for s in range(S)):
        C = sizes[i % len(sizes)]
        counts, end, cur = [0] * S, [0] * S, list(which)
        x = torch.zeros(S, C, device="cuda")
        for s in range(S):
            if i < delays[s] or which[s] >= len(utts[s]):
                continue
            sig = utts[s][which[s]]
            counts[s] = min(C, len(sig) - at[s])
            x[s, :counts[s]] = torch.from_numpy(sig[at[s]:at[s] + counts[s]]).cuda()
            at[s] += counts[s]
            if at[s] == len(sig):
                end[s], at[s], which[s] = 1, 0, which[s] + 1
        res = step(x, counts, end)
        for s in range(S):
            dec, wav, n = res[s]
            if cur[s] < len(utts[s]) and i >= delays[s]:
                g = got[s][cur[s]]
                g["decoded"].append(dec)
                g["wave"].append(wav)
                g["n_frames"].append(n)
                if end[s]:
                    g["end_push"] = i
            else:
                assert n == 0 and len(wav) == 0, "an idle stream emitted something"
        i += 1
    return [[dict(decoded=torch.cat(g["decoded"]), wave=torch.cat(g["wave"]), n_frames=g["n_frames"], end_push=g["end_push"])
             for g in u] for u in got]


def live_step(lc, org, cv):
    S = lc.n_streams
    out = lc.empty_outputs(S, decoded=True)
    noise = torch.zeros(S, lc.max_chunk * HOP, device="cuda")
    o, c = spk(org), spk(cv)

    def step(x, counts, end):
        out["wave"].fill_(777.0)
        out["decoded"].fill_(777.0)
        res = lc.push(x, o, c, n_valid=counts, end=end, noise=noise, out=out)
        n, m = res["n_frames"].tolist(), res["n_out"].tolist()
        for s in range(S):
            assert bool((res["decoded"][s, n[s]:] == 777.0).all()) and bool((res["wave"][s, m[s]:] == 777.0).all())
        return [(res["decoded"][s, :n[s]].clone(), res["wave"][s, :m[s]].clone(), n[s]) for s in range(S)]

    return step


def host_step(S, max_samples, org, cv):
    """The loop of INTEGRATION.md section O as the parent commit documents it: Python queues per stream, ``.tolist()`` on
    both front ends' counts, ``torch.cat`` to grow and shrink the queues, padding into fresh tensors - completed with the
    de-scaling, the vocoder's normalisation and the vocoder's end flag."""
    from crank_amd.stream import StreamingConverter
    from crank_amd.world import StreamingF0

    p = parts()
    sl = p.layer.streaming(S, max_samples)
    sf = StreamingF0(FS, [RANGE[0]] * S, [RANGE[1]] * S, SPK_MEAN, SPK_STD, max_samples, hop_size=HOP, lcf0_scaler=SCALER)
    K_max = sl.max_frames + sf.max_frames
    conv, sv = StreamingConverter(p.dev.G, S, K_max), p.voc.streaming(S, K_max)
    mean = torch.as_tensor(p.scaler["mlfb"].mean_, dtype=torch.float32, device="cuda")
    scale = torch.as_tensor(p.scaler["mlfb"].scale_, dtype=torch.float32, device="cuda")
    mel_q = [torch.zeros(0, N_MELS, device="cuda") for _ in range(S)]
    f0_q = [torch.zeros(0, 2, device="cuda") for _ in range(S)]
    o, c = spk(org), spk(cv)

    def step(x, counts, end):
        nonlocal mel_q, f0_q
        ended = torch.tensor(end, device="cuda")
        fr = sl.push(x, n_valid=torch.tensor(counts, device="cuda"), end=ended)
        f0 = sf.push(x, o, c, n_valid=counts, end=end)
        nm, nf = fr["n_frames"].tolist(), f0["n_frames"].tolist()
        for s in range(S):
            mel_q[s] = torch.cat([mel_q[s], fr["feats"][s, :nm[s]]])
            f0_q[s] = torch.cat([f0_q[s], torch.cat([f0["lcf0"][s, :nf[s]], f0["uv"][s, :nf[s]]], -1)])
        take = [min(len(m), len(f)) for m, f in zip(mel_q, f0_q)]
        K = max(max(take), 1)
        feats, lcf0, uv = (torch.zeros(S, K, w, device="cuda") for w in (N_MELS, 1, 1))
        for s in range(S):
            k = take[s]
            feats[s, :k], lcf0[s, :k], uv[s, :k] = mel_q[s][:k], f0_q[s][:k, :1], f0_q[s][:k, 1:]
        dec = conv.push(feats, lcf0, uv, c.long(), n_valid=torch.tensor(take, device="cuda"))["decoded"]
        out = sv.push(p.voc.normalize(dec * scale + mean), torch.zeros(S, K * HOP, device="cuda"),
                      n_valid=torch.tensor(take, device="cuda"), end=ended)
        m = out["n_out"].tolist()
        res = [(dec[s, :take[s]].clone(), out["wave"][s, :m[s]].clone(), take[s]) for s in range(S)]
        for s in range(S):
            mel_q[s], f0_q[s] = mel_q[s][take[s]:], f0_q[s][take[s]:]
            if end[s]:  # what is left has no partner; every stage starts the next utterance from nothing
                mel_q[s], f0_q[s] = mel_q[s][:0], f0_q[s][:0]
                conv.reset([s])
        return res

    return step, sf


@functools.lru_cache(maxsize=None)
def base_run():
    """Both signals, one utterance per stream, pushes of 2048 samples through LiveConverter."""
    lc = live(2, 2048)
    res = drive(live_step(lc, ORG, CV), [[x] for x in parts().xs], [2048])
    lc.status()
    return res, lc


def same(a, b):
    return torch.equal(a["decoded"], b["decoded"]) and torch.equal(a["wave"], b["wave"])


def test_equals_the_host_loop_bit_for_bit():
    res, lc = base_run()
    step, sf = host_step(2, 2048, ORG, CV)
    ref = drive(step, [[x] for x in parts().xs], [2048])
    sf.status()
    for s in range(2):
        assert res[s][0]["n_frames"] == ref[s][0]["n_frames"], s
        assert max(res[s][0]["n_frames"]) > 0
        assert same(res[s][0], ref[s][0]), s
    assert lc.max_chunk < lc.sl.max_frames + lc.sf.max_frames  # the converter's grid is narrower than the host loop's
    assert lc.state_bytes > lc.sv.state_bytes and 180 < lc.latency_ms < 181 + 1000 * lc.sv.lookahead * HOP / FS


def test_cut_independence_length_and_the_offline_vocoder():
    res, _ = base_run()
    p = parts()
    lc = live(2, max(CYCLE))
    cyc = drive(live_step(lc, ORG, CV), [[x] for x in p.xs], CYCLE)
    lc.status()
    mean = torch.as_tensor(p.scaler["mlfb"].mean_, dtype=torch.float32, device="cuda")
    scale = torch.as_tensor(p.scaler["mlfb"].scale_, dtype=torch.float32, device="cuda")
    for s, x in enumerate(p.xs):
        a, b = res[s][0], cyc[s][0]
        assert a["n_frames"] != b["n_frames"] and same(a, b), s
        T = 1 + len(x) // HOP
        assert a["decoded"].shape == (T, p.D) and a["wave"].shape == (T * HOP,)
        off = p.voc.inference_batch([p.voc.normalize(a["decoded"] * scale + mean)], [torch.zeros(T * HOP, device="cuda")])[0]
        assert torch.equal(a["wave"], off), s


def test_staggered_streams_equal_their_runs_alone():
    res, _ = base_run()
    xs = parts().xs
    second = voiced_silence_voiced(FS, (350,), (160.0,), 13)
    lc = live(2, 2048)
    got = drive(live_step(lc, ORG, CV), [[xs[0], second], [xs[1]]], [2048], delays=[0, 6])
    lc.status()
    # stream 0 ends and starts over while stream 1 is in the middle of its utterance, and ends its second one beside it
    assert got[0][0]["end_push"] < got[1][0]["end_push"] - 1 and got[0][1]["end_push"] <= got[1][0]["end_push"]
    assert sum(got[1][0]["n_frames"][:got[0][0]["end_push"] - 6 + 1]) > 0  # stream 1 was emitting frames by then
    assert same(got[0][0], res[0][0]) and same(got[1][0], res[1][0])
    alone = drive(live_step(live(1, 2048), ORG[:1], CV[:1]), [[second]], [2048])
    assert same(got[0][1], alone[0][0]) and len(alone[0][0]["wave"]) == (1 + len(second) // HOP) * HOP


def test_an_utterance_below_half_a_window_emits_nothing_and_the_stream_goes_on():
    res, _ = base_run()
    xs = parts().xs
    short = voiced_silence_voiced(FS, (10,), (150.0,), 14)[:200]
    assert 64 <= len(short) <= N_FFT // 2
    lc = live(1, 2048)
    got = drive(live_step(lc, ORG[1:], CV[1:]), [[short, xs[1]]], [2048])
    lc.status()  # no flag: the F0 rows without a mel frame were dropped by the join, which is no error
    assert len(got[0][0]["wave"]) == 0 and len(got[0][0]["decoded"]) == 0
    assert same(got[0][1], res[1][0])
    lc.reset([0])
    assert same(drive(live_step(lc, ORG[1:], CV[1:]), [[xs[1]]], [1000, 2048, 1])[0][0], res[1][0])


def test_constructor_refusals_name_their_key():
    from crank_amd.live import LiveConverter
    from crank_amd.net.module.mlfb import LogMelFilterBankLayer

    p = parts()
    G = p.dev.G
    args = (1, 2048, [70], [400], SPK_MEAN, SPK_STD, p.scaler)
    fake = lambda **kw: types.SimpleNamespace(conf=dict(G.conf, **kw), spkr_size=G.spkr_size)  # noqa: E731
    with pytest.raises(NotImplementedError, match="causal"):
        LiveConverter(fake(causal=False), p.layer, p.voc, *args)
    with pytest.raises(NotImplementedError, match="use_raw"):
        LiveConverter(fake(use_raw=True), p.layer, p.voc, *args)
    with pytest.raises(NotImplementedError, match="encoder_f0"):
        LiveConverter(fake(encoder_f0=True), p.layer, p.voc, *args)
    with pytest.raises(NotImplementedError, match="input_size"):
        LiveConverter(G, LogMelFilterBankLayer(fs=FS, hop_size=HOP, fft_size=N_FFT, n_mels=40), p.voc, *args)
    with pytest.raises(NotImplementedError, match="output_size"):
        LiveConverter(G, p.layer, types.SimpleNamespace(aux_channels=p.D + 1), *args)
    with pytest.raises(ValueError, match="one search range per stream"):
        LiveConverter(G, p.layer, p.voc, 2, 2048, [70], [400], SPK_MEAN, SPK_STD, p.scaler)
    lc = live(1, 1024)
    for bad in (lambda: lc.push(torch.zeros(1, 1025, device="cuda"), spk([0]), spk([1])),
                lambda: lc.push(torch.zeros(2, 1024, device="cuda"), spk([0]), spk([1])),
                lambda: lc.push(torch.zeros(1, 1024), spk([0]), spk([1])),
                lambda: lc.push(torch.zeros(1, 1024, device="cuda"), spk([0]).long(), spk([1])),
                lambda: lc.push(torch.zeros(1, 1024, device="cuda"), spk([0]), spk([1]), n_valid=[1025]),
                lambda: lc.push(torch.zeros(1, 1024, device="cuda"), spk([0]), spk([1]), n_valid=spk([1024])),
                lambda: lc.push(torch.zeros(1, 1024, device="cuda"), spk([0]), spk([1]), end=spk([1])),
                lambda: lc.push(torch.zeros(1, 1024, device="cuda"), spk([0]), spk([1]), noise=torch.zeros(1, 3, device="cuda"))):
        with pytest.raises(ValueError):
            bad()


def test_packed_lcf0_uv_equals_the_two_tensor_form():
    dev = parts().dev
    C = 40
    x, lcf0, uv = (t[:, :C].contiguous() for t in (dev.x, dev.lcf0, dev.uv))
    S = x.shape[0]
    a = dev.converter(S, C).push(x, lcf0, uv, dev.spk)
    b = dev.converter(S, C).push(x, None, None, dev.spk, lcf0_uv=torch.cat([lcf0, uv], -1))
    assert torch.equal(a["decoded"], b["decoded"])
    assert all(torch.equal(p, q) for p, q in zip(a["qidx"] + a["encoded"], b["qidx"] + b["encoded"]))
    with pytest.raises(ValueError, match="one form"):
        dev.converter(S, C).push(x, lcf0, uv, dev.spk, lcf0_uv=torch.cat([lcf0, uv], -1))


def test_without_decoder_f0_there_is_no_f0_stage_and_no_join():
    """The three-stage chain of INTEGRATION.md section N through LiveConverter: two utterances on one stream, equal to the
    public stages called one by one, with ``first`` counting the utterance's frames."""
    from crank_amd.live import LiveConverter
    from crank_amd.stream import StreamingConverter
    from tests.test_gpu_stream import Dev

    p = parts()
    dev = Dev.of(decoder_f0=False)
    lc = LiveConverter(dev.G, p.layer, p.voc, 1, 2048, scaler=p.scaler)
    assert lc.join is None and lc.sf is None and lc.max_chunk == lc.sl.max_frames
    assert abs(lc.latency_ms - 1000 * (N_FFT // 2 + lc.sv.lookahead * HOP) / FS) < 1e-9
    utts = [[p.xs[1], p.xs[0][:5000]]]
    firsts = []
    inner = live_step(lc, [0], [1])

    def step(x, counts, end):
        res = inner(x, counts, [2 * e for e in end])  # (any non-zero value is an end flag)
        firsts.append((int(lc._first[0]), res[0][2], end[0]))
        return res

    got = drive(step, utts, [2048, 700])
    at = 0
    for after, n, end in firsts:  # the count behind a push: the frames so far, 0 again behind an end
        at = 0 if end else at + n
        assert after == at
    sl, conv, sv = p.layer.streaming(1, 2048), StreamingConverter(dev.G, 1, lc.max_chunk), p.voc.streaming(1, lc.max_chunk)
    mean = torch.as_tensor(p.scaler["mlfb"].mean_, dtype=torch.float32, device="cuda")
    scale = torch.as_tensor(p.scaler["mlfb"].scale_, dtype=torch.float32, device="cuda")

    def ref_step(x, counts, end):
        ended = torch.tensor(end, device="cuda")
        fr = sl.push(x, n_valid=torch.tensor(counts, device="cuda"), end=ended)
        dec = conv.push(fr["feats"], None, None, spk([1]).long(), n_valid=fr["n_frames"])["decoded"]
        out = sv.push(p.voc.normalize(dec * scale + mean), torch.zeros(1, lc.max_chunk * HOP, device="cuda"),
                      n_valid=fr["n_frames"], end=ended)
        n, m = int(fr["n_frames"][0]), int(out["n_out"][0])
        if end[0]:
            conv.reset([0])
        return [(dec[0, :n].clone(), out["wave"][0, :m].clone(), n)]

    ref = drive(ref_step, utts, [2048, 700])
    for u in range(2):
        assert same(got[0][u], ref[0][u]) and got[0][u]["n_frames"] == ref[0][u]["n_frames"], u
        assert len(got[0][u]["wave"]) == (1 + len(utts[0][u]) // HOP) * HOP
    with pytest.raises(ValueError, match="decoder_f0 = false"):
        conv.push(torch.zeros(1, 4, N_MELS, device="cuda"), None, None, spk([1]).long(), lcf0_uv=torch.zeros(1, 4, 2, device="cuda"))
