"""WORLD synthesis (crk_world_*, csrc/world_kernels.hip) against the CPU restatement tests/world_synth_ref.py beyond the
configuration of tests/test_gpu_world.py: other sampling rates (1 and 5 aperiodicity bands, the 15 kHz cap), F0
contours that reach the unvoiced cutoff, the long-interval pulse branch, several pulses per frame and flipping voicing,
mcep orders 1 / 60 / 128 and alpha 0, utterance lengths on the 2048-sample chunks of the time base, and a response
buffer smaller than one utterance's pulses.  Every case first asserts, on the host, that its inputs (or the
restatement's pulses) reach the edge the case is named after."""
import functools

import numpy as np
import pytest
import torch

from tests import world_synth_ref as R
from tests.world_inputs import contour, utterance, with_f0

gpu = pytest.mark.gpu

CHUNK = 2048  # samples per chunk of world_timebase_kernel


def lowest(fs):
    """The lowest voiced F0 of the time base (WORLD divides the integers)."""
    return fs // R.FFTL + 1


def _f0_set(fs, seed):
    """Named F0 contours of one ragged batch at fs (the cepstra and coded aperiodicity are seeded per utterance)."""
    rng = np.random.default_rng(seed)
    lo = lowest(fs)
    near = lo + rng.uniform(0, 1.5, 12)  # near the cutoff, next to unvoiced frames: at 30 ms, seed 0 gives a pulse
    near[rng.random(12) < 0.35] = 0.0    # interval longer than 1024 samples at 22050 and 44100 (asserted below)
    f0s = {
        "cutoff": np.array([150.0, 140.0, lo - 0.5, lo - 1.0, lo - 0.01, lo + 0.0, lo + 0.5, lo + 0.99, 120.0, 0.0,
                            lo - 0.3, 130.0]),
        "long_interval": near,
        "high_f0": contour(rng, 10, 800.0, 1000.0),
        "all_unvoiced": np.zeros(9),
        "all_voiced": contour(rng, 11, 90.0, 300.0),
        "flip": np.where(np.arange(13) % 2 == 0, contour(rng, 13, 100.0, 250.0), 0.0),
        "two_frames": np.array([180.0, 0.0]),
    }
    return f0s


def _utts(fs, order1, f0s, seed):
    rng = np.random.default_rng(seed + 100)
    return [with_f0(rng, f, order1, R.n_bands(fs)) for f in f0s.values()]


def _plain(fs, order1, lens, seed):
    rng = np.random.default_rng(seed)
    return [utterance(rng, T, order1, R.n_bands(fs)) for T in lens]


# name -> (fs, shiftms, alpha, order1, utterance names, utterances)
@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, rest = name.partition("-")
    if kind == "rate":  # rate-<fs>-<shiftms>
        fs, shiftms = rest.split("-")
        fs, shiftms = int(fs), float(shiftms)
        order1, alpha = {16000: (25, 0.41), 24000: (40, 0.466), 44100: (40, 0.544), 48000: (50, 0.554)}[fs]
        lens = [2, 3, 57, 150]
        return fs, shiftms, alpha, order1, [f"T{T}" for T in lens], _plain(fs, order1, lens, fs + int(shiftms))
    if kind == "f0":  # f0-<fs>: the named contours at 30 ms
        fs = int(rest)
        f0s = _f0_set(fs, 0)
        return fs, 30.0, 0.466, 35, list(f0s), _utts(fs, 35, f0s, fs)
    if kind == "order":  # order-<order + 1>-<alpha>
        order1, alpha = rest.split("-")
        order1, alpha = int(order1), float(alpha)
        lens = [2, 3, 40]
        return 22050, 10.0, alpha, order1, [f"T{T}" for T in lens], _plain(22050, order1, lens, order1)
    if kind == "chunk":  # chunk-<fs>-<shiftms>: lengths on and around multiples of 2048 samples
        fs, shiftms = rest.split("-")
        fs, shiftms = int(fs), float(shiftms)
        lens = [16, 2, 32, 17, 33] if fs == 16000 else [16, 2, 32]
        return fs, shiftms, 0.466, 35, [f"T{T}" for T in lens], _plain(fs, 35, lens, 7)
    raise KeyError(name)


RATES = ["rate-16000-10", "rate-16000-5.80499", "rate-44100-10", "rate-44100-5.80499", "rate-48000-10",
         "rate-48000-5.80499", "rate-24000-5.333333"]
F0S = ["f0-22050", "f0-44100"]
ORDERS = ["order-1-0.466", "order-60-0.466", "order-128-0.466", "order-35-0.0"]
CHUNKS = ["chunk-16000-8", "chunk-24000-5.333333"]
CASES = RATES + F0S + ORDERS + CHUNKS


@functools.lru_cache(maxsize=None)
def _synth(fs, shiftms, alpha, pulse_capacity=None):
    from crank_amd.world import WorldSynthesizer

    kw = {} if pulse_capacity is None else {"pulse_capacity": pulse_capacity}
    return WorldSynthesizer(fs, 1024, shiftms, alpha, **kw)


@functools.lru_cache(maxsize=None)
def _ref(name, with_r):
    fs, shiftms, alpha, _, _, utts = case(name)
    out = []
    for f0, mc, cap, rm in utts:
        sp, ap = R.frame_tables(mc, cap, rm if with_r else None, fs, 1024, alpha)
        out.append((sp, ap, R.pulses(f0, fs, 1024, shiftms), R.synthesize(f0, sp, ap, fs, shiftms)))
    return out


def _run(name, with_r, idx=None, pulse_capacity=None):
    fs, shiftms, alpha, _, _, utts = case(name)
    syn = _synth(fs, shiftms, alpha, pulse_capacity)
    ins = utts if idx is None else [utts[i] for i in idx]
    f0s, mcs, caps, rms = zip(*ins)
    ys = syn.synthesis_batch(list(f0s), list(mcs), list(caps), list(rms) if with_r else None)
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in ys], syn.last_pulse_count


def _rel_l2(y, ry):
    den = np.linalg.norm(ry)
    if den == 0:  # a single pulse (the last one of its utterance) responds with zeros
        return 0.0 if np.array_equal(y, ry) else np.inf
    return float(np.linalg.norm(y - ry) / den)


# ---- what each case reaches (host side, from the inputs or the restatement)
def test_sampling_rates_reach_one_and_five_bands():
    from crank_amd.world import n_bands

    for name in RATES:
        fs, shiftms, _, _, _, utts = case(name)
        bands = utts[0][2].shape[1]
        assert bands == n_bands(fs) == R.n_bands(fs)
        if fs == 16000:
            assert bands == 1
        elif fs in (44100, 48000):  # the 15 kHz cap binds: the top knot is fs / 2, above 3000 * bands + 3000
            assert bands == 5 and fs / 2.0 - 3000.0 > 15000.0
        else:
            assert shiftms == 5.333333
            assert [R.y_length(T, fs, shiftms) for T in (57, 150)] == [128 * 57 - 1, 128 * 150 - 1]


@pytest.mark.parametrize("name", F0S)
def test_f0_contours_reach_their_edges(name):
    fs, shiftms, _, _, names, utts = case(name)
    lo = lowest(fs)
    by = dict(zip(names, utts))
    f0 = by["cutoff"][0]
    voiced = f0[f0 > 0]
    dropped, kept = voiced[(voiced >= lo - 1) & (voiced < lo)], voiced[(voiced >= lo) & (voiced < lo + 1)]
    assert len(dropped) >= 2 and len(kept) >= 2, (lo, f0)
    assert lo + 0.0 in kept and lo - 0.01 in dropped
    # the time base drops the first set (zeroing them changes no pulse) and keeps the second (zeroing them does)
    same = R.pulses(np.where(f0 < lo, 0.0, f0), fs, 1024, shiftms)[0]
    moved = R.pulses(np.where(f0 < lo + 1, 0.0, f0), fs, 1024, shiftms)[0]
    pos = R.pulses(f0, fs, 1024, shiftms)[0]
    assert np.array_equal(pos, same) and not np.array_equal(pos, moved)
    _, ns, _, _, _ = R.pulses(by["long_interval"][0], fs, 1024, shiftms)
    assert ns.max() > R.FFTL, ns.max()  # the min(ns, fftl) branch of the noise segment
    pos, _, _, pvuv, _ = R.pulses(by["high_f0"][0], fs, 1024, shiftms)
    per_frame = np.bincount((pos / (fs * shiftms / 1000.0)).astype(int))
    assert per_frame.max() >= 20 and (pvuv == 1).all()  # several pulses per frame
    assert (by["all_unvoiced"][0] == 0).all() and (by["all_voiced"][0] >= lo).all()
    v = by["flip"][0] > 0
    assert (v[1:] != v[:-1]).all()
    assert len(by["two_frames"][0]) == 2


def test_orders_reach_1_60_128_and_alpha_0():
    from crank_amd.world import MAX_ORDER1

    got = {(case(n)[3], case(n)[2]) for n in ORDERS}
    assert {(1, 0.466), (60, 0.466), (MAX_ORDER1, 0.466), (35, 0.0)} == got and MAX_ORDER1 == 128
    for n in ORDERS:
        assert all(u[1].shape[1] == case(n)[3] for u in case(n)[5])


def test_chunk_lengths_reach_2048_sample_boundaries():
    fs, shiftms, _, _, _, utts = case("chunk-16000-8")
    ylen = [R.y_length(len(u[0]), fs, shiftms) for u in utts]
    assert ylen == [2048, 256, 4096, 2048 + 128, 4096 + 128]  # on a multiple, a 2-frame utterance, past a multiple
    assert ylen[0] % CHUNK == ylen[2] % CHUNK == 0 and 0 < ylen[3] % CHUNK < ylen[1] and 0 < ylen[4] % CHUNK < ylen[1]
    fs, shiftms, _, _, _, utts = case("chunk-24000-5.333333")
    ylen = [R.y_length(len(u[0]), fs, shiftms) for u in utts]
    assert ylen == [2047, 255, 4095]  # one sample below a multiple: int(T * 5.333333 * 24) = 128 T - 1
    assert (ylen[0] + 1) % CHUNK == (ylen[2] + 1) % CHUNK == 0


@gpu
# ---- the kernels against the restatement
@pytest.mark.parametrize("name,with_r", [(n, r) for n in CASES for r in (False, True)])
def test_frame_tables_match_restatement(name, with_r):
    fs, shiftms, alpha, _, _, utts = case(name)
    syn = _synth(fs, shiftms, alpha)
    got = syn.frame_tables_batch([u[1] for u in utts], [u[2] for u in utts], [u[3] for u in utts] if with_r else None)
    for (sp, ap), (rsp, rap, _, _) in zip(got, _ref(name, with_r)):
        sp, ap = sp.cpu().numpy(), ap.cpu().numpy()
        assert np.abs(sp / rsp - 1).max() < 1e-12
        assert np.abs(ap / rap - 1).max() < 1e-12


@gpu
@pytest.mark.parametrize("name", CASES)
def test_pulse_positions_identical(name):
    fs, shiftms, alpha, _, names, utts = case(name)
    got = _synth(fs, shiftms, alpha).pulses_batch([u[0] for u in utts])
    for n, (pos, ns, shift, vuv), (_, _, (rpos, rns, rshift, rvuv, _), _) in zip(names, got, _ref(name, False)):
        assert np.array_equal(pos, rpos), n
        assert np.array_equal(ns, rns), n
        assert np.array_equal(vuv, rvuv), n
        assert np.array_equal(shift, rshift), n


@gpu
@pytest.mark.parametrize("name,with_r", [(n, r) for n in CASES for r in (False, True)])
def test_waveforms_match_restatement(name, with_r):
    fs, shiftms, _, _, names, utts = case(name)
    ys, _ = _run(name, with_r)
    for n, u, y, (_, _, _, ry) in zip(names, utts, ys, _ref(name, with_r)):
        assert y.shape == (R.y_length(len(u[0]), fs, shiftms),) == ry.shape, n
        assert np.isfinite(y).all(), n
        assert _rel_l2(y, ry) < 1e-9, (n, _rel_l2(y, ry))


@gpu
@pytest.mark.parametrize("name", CASES)
def test_ragged_batch_bit_identical_to_single_calls(name):
    with_r = name.startswith(("rate", "f0"))
    batch, _ = _run(name, with_r)
    for i, y in enumerate(batch):
        assert np.array_equal(_run(name, with_r, [i])[0][0], y), i


@gpu
@pytest.mark.parametrize("name", ["f0-22050", "chunk-16000-8"])
def test_pulse_capacity_below_one_utterance_gives_the_same_bits(name):
    """A response buffer smaller than one utterance's pulses: that utterance's overlap-add spans several rounds."""
    fs, shiftms, _, _, _, utts = case(name)
    per_utt = [len(R.pulses(u[0], fs, 1024, shiftms)[0]) for u in utts]
    cap = max(per_utt) // 3
    assert 1 <= cap < max(per_utt)
    full, P = _run(name, True)
    assert P == sum(per_utt)
    small, P2 = _run(name, True, pulse_capacity=cap)
    assert P2 == P
    for a, b in zip(small, full):
        assert np.array_equal(a, b)
