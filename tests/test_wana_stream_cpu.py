"""Streaming CheapTrick / mel-cepstrum analysis without a GPU: the definition in sets (tests/wana_stream_ref.py) streamed
under every schedule is the offline restatement (tests/world_analysis_ref.py) of the whole utterance, value for value;
``analysis_capacities`` is exact at toy sizes; the new C symbols are declared, bound and exported."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import wana_stream_ref as W
from tests import world_analysis_cases as C
from tests import world_analysis_ref as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, SHIFT, DIM, ALPHA = 16000, 5.0, 24, 0.41


@functools.lru_cache(maxsize=None)
def _utterance():
    """2000 samples, 26 rows (the last frame is centred at the signal's end): voiced runs, zeros, the longest window (an F0
    just above the floor), fs / 4, the floor."""
    rng = np.random.default_rng(5)
    x = C._harmonic(rng, 2000, FS, 150.0).astype(np.float32)
    f0 = 150.0 + 30.0 * np.sin(np.arange(26) / 3.0)
    f0[4:7] = 0.0
    f0[9] = np.nextafter(A.f0_floor(FS), 1e9)
    f0[12] = FS / 4.0
    f0[15] = A.f0_floor(FS)
    return x, f0


@functools.lru_cache(maxsize=None)
def _offline(low_cut):
    x, f0 = _utterance()
    y = W.low_cut(x, FS, low_cut) if low_cut is not None else x.astype(np.float64)
    sp = A.cheaptrick(y, f0, FS, SHIFT)
    return y, sp, A.sp2mc(sp, DIM, ALPHA), A.frame_shapes(f0, FS, SHIFT)


def _schedules():
    x, f0 = _utterance()
    late = [(37, 0), (1, 0), (500, 0), (3, 0), (800, 0), (160, 16), (160, 0), (0, 0), (1, 0)]  # rows 180 ms and more late
    return {"single": [(len(x), len(f0))],
            "pushes_of_160": [(160, 2)] * 13,
            "irregular_late_f0": late,
            "f0_first": [(0, len(f0))] + [(333, 0)] * 7,
            "one_sample_pushes_at_the_end": [(1990, 26)] + [(1, 0)] * 10}


@pytest.mark.parametrize("low_cut", [70, None])
@pytest.mark.parametrize("name", list(_schedules()))
def test_the_streamed_definition_is_the_offline_analysis_value_for_value(name, low_cut):
    x, f0 = _utterance()
    y, sp, mc, sh = _offline(low_cut)
    ref = W.McepStreamRef(FS, SHIFT, DIM, ALPHA, low_cut, f0_capacity=len(f0), ring_capacity=len(x) + 1024,
                          max_utt_frames=len(f0))
    got = W.stream_utterance(ref, x, f0, _schedules()[name])
    assert ref.flags == 0 and got["n_dropped"] == 0
    assert got["index"] == list(range(len(f0)))
    assert got["offset"] == sh["offset"].tolist()
    assert np.array_equal(got["sp"], sp)
    assert np.array_equal(got["mcep"], mc)
    assert np.array_equal(got["feats"], mc[:, 1:].astype(np.float32))
    assert (ref.n, ref.rows, ref.emitted, ref.doff) == (0, 0, 0, 0)


def test_frames_leave_as_soon_as_their_window_is_complete_and_not_before():
    x, f0 = _utterance()
    ref = W.McepStreamRef(FS, SHIFT, DIM, ALPHA, 70, len(f0), len(x) + 1024, len(f0))
    out = ref.push(x[:591], f0)  # frame 1 is centred at sample 80: it needs 80 + 512 samples
    assert out["index"] == [0]
    assert ref.push(x[591:592], f0[:0])["index"] == [1]
    assert ref.push(x[592:], f0[:0], end=True)["index"] == list(range(2, len(f0)))


def test_the_tap_order_chain_is_the_reference_low_cut_up_to_the_order_of_its_sums():
    x, _ = _utterance()
    taps = A.low_cut_taps(FS, 70)
    # 255 products of relative error 2^-53 each and 254 sums: 255 * 2^-52 * sum |h| max |x| bounds either evaluation
    bound = 2 * 255 * 2.0 ** -52 * np.abs(taps).sum() * np.abs(x).max()
    assert np.abs(W.low_cut(x, FS, 70) - A.low_cut_filter(x, FS, 70)).max() <= bound
    # and it does not depend on the cut
    whole = W.low_cut(x, FS, 70)
    parts, at = [], 0
    for c in (1, 100, 253, 254, 255, 700, len(x)):
        c = min(c, len(x) - at)
        parts.append(W.low_cut_chain(taps, x[max(0, at - 254):at], x[at:at + c], at))
        at += c
    assert at == len(x) and np.array_equal(np.concatenate(parts), whole)


def test_shape_of_is_frame_shapes_row_by_row():
    f0 = np.concatenate([C.floor_f0s(FS), [0.0, 70.0, FS / 4.0]])
    for shiftms in (5.0, 5.333333, 10.0):
        sh = A.frame_shapes(f0, FS, shiftms)
        for k, f in enumerate(f0):
            assert W.shape_of(f, k, FS, shiftms) == (sh["f0"][k], sh["origin"][k], sh["half"][k], sh["dc_limit"][k],
                                                     sh["boundary"][k])


def test_flags_of_the_definition():
    x, f0 = _utterance()
    mk = lambda **kw: W.McepStreamRef(FS, SHIFT, DIM, ALPHA, 70, **{**dict(f0_capacity=len(f0), ring_capacity=4096,  # noqa: E731
                                                                             max_utt_frames=len(f0)), **kw})
    _, sp, mc, sh = _offline(70)
    # 2: a queue one row short drops the newest row
    ref = mk(f0_capacity=len(f0) - 1)
    got = W.stream_utterance(ref, x, f0, [(len(x), len(f0))])
    assert ref.flags == W.FLAG_QUEUE and got["n_dropped"] == 1 and np.array_equal(got["mcep"], mc[:-1])
    # 4: the table of one frame's 1536 draws ends inside frame 1 (834 draws each); the frames still leave
    ref = mk(max_utt_frames=1)
    got = W.stream_utterance(ref, x, f0, [(len(x), len(f0))])
    assert ref.flags == W.FLAG_DRAWS and len(got["index"]) == len(f0) and np.array_equal(got["mcep"][:1], mc[:1])
    # 8: a row two shifts past the end
    ref = mk(f0_capacity=len(f0) + 2)
    got = W.stream_utterance(ref, x, np.concatenate([f0, [100.0, 100.0]]), [(len(x), len(f0) + 2)])
    assert ref.flags == W.FLAG_PAST_END and got["n_dropped"] == 1 and np.array_equal(got["mcep"][:len(f0)], mc)
    # 16: a NaN row is analysed as unvoiced
    bad = f0.copy()
    bad[4] = np.nan
    ref = mk()
    got = W.stream_utterance(ref, x, bad, [(len(x), len(f0))])
    assert ref.flags == W.FLAG_F0 and np.array_equal(got["mcep"], mc)  # (row 4 is 0 in the utterance)
    # 1: rows that come after their window left a small ring; later frames keep the offline bits
    ref = mk(ring_capacity=1200)
    got = W.stream_utterance(ref, x, f0, [(1800, 0), (100, len(f0))])
    assert ref.flags == W.FLAG_RING and got["n_dropped"] > 0
    assert got["index"] == list(range(got["n_dropped"], len(f0)))
    assert np.array_equal(got["mcep"], mc[got["n_dropped"]:]) and got["offset"] == sh["offset"][got["n_dropped"]:].tolist()


# ------------------------------------------------------------------------------------------------ capacities
def _histories_flags(fs, shiftms, lag_ms, C_max, R_max, reach, ring, queue, n_stop):
    """The union of the flags any history within the lag raises, by trying every history: pushes of 0 .. C_max samples and
    0 .. R_max rows, ended or not, from the start state until n passes n_stop.  Within the lag: after a push every frame
    with origin + L <= n has its row and no row has origin > n; an end push has n >= 1 and at most the rows the offline
    call takes."""
    shift = shiftms / 1000.0 * fs
    L = int(np.ceil(lag_ms * fs / 1000.0))
    origins = [W.origin_of(k, fs, shiftms) for k in range(n_stop + 8)]
    ns = range(n_stop + C_max + 1)
    lo = [sum(1 for o in origins if o + L <= n) for n in ns]
    hi = [sum(1 for o in origins if o <= n) for n in ns]
    t_end = [sum(1 for k in range(len(origins)) if not k * shift > n + shift) for n in ns]
    seen, todo, flags = set(), [(0, 0, 0)], 0
    while todo:
        st = todo.pop()
        if st in seen:
            continue
        seen.add(st)
        n0, rows0, em0 = st
        for c in range(C_max + 1):
            for r in range(R_max + 1):
                n1, rows1 = n0 + c, rows0 + r
                for end in (False, True):
                    if end:
                        if n1 < 1 or rows1 > t_end[n1] or rows1 < lo[n1]:
                            continue
                    elif n1 > n_stop or not lo[n1] <= rows1 <= hi[n1]:
                        continue
                    (n, rows, em), keep, leaving, refused, f = W.plan_push(n0, rows0, em0, c, r, end, fs, shiftms, ring,
                                                                          queue, lambda k: reach, reach)
                    flags |= f
                    if not end and not f:
                        todo.append((n, rows, em))
    return flags


@pytest.mark.parametrize("lag_ms", [0.0, 5.0, 9.0, 14.0])
@pytest.mark.parametrize("shiftms,C_max", [(4.0, 3), (3.0, 5), (5.0, 2)])
def test_analysis_capacities_are_exact_at_toy_sizes(lag_ms, shiftms, C_max):
    fs, reach, R_max = 1000, 3, 8  # (8 rows: the largest toy queue, so one push can fill it)
    ring, queue = W.analysis_capacities(fs, shiftms, lag_ms, C_max, R_max, reach)
    args = (fs, shiftms, lag_ms, C_max, R_max, reach)
    assert _histories_flags(*args, ring, queue, 40) == 0
    assert _histories_flags(*args, ring - 1, queue, 40) & W.FLAG_RING
    assert _histories_flags(*args, ring, queue - 1, 40) & W.FLAG_QUEUE


def test_the_package_helper_is_the_restated_closed_form():
    from crank_amd.world import analysis_capacities

    for fs, shiftms, lag, cs, rs in [(16000, 5.0, 260.0, 1280, 52), (22050, 5.0, 0.0, 160, 4), (24000, 10.0, 100.0, 4000, 30),
                                     (16000, 5.333333, 31.0, 37, 3), (1000, 4.0, 9.0, 3, 6)]:
        assert analysis_capacities(fs, shiftms, lag, cs, rs) == W.analysis_capacities(fs, shiftms, lag, cs, rs)
    assert analysis_capacities(1000, 4.0, 9.0, 3, 6, reach=3) == W.analysis_capacities(1000, 4.0, 9.0, 3, 6, 3)
    assert analysis_capacities(16000, 5.0, 260.0, 1280, 52) == (4160 - 1 + 1280 + 511, (1280 + 4160) // 80 + 1)
    with pytest.raises(ValueError):
        analysis_capacities(16000, 0.0, 10.0, 160, 2)


# ------------------------------------------------------------------------------------------------ symbols
def test_wana_stream_symbols_are_declared_bound_and_exported():
    from crank_amd import _lib

    names = ["crk_wana_stream_create", "crk_wana_stream_destroy", "crk_wana_stream_state_bytes",
             "crk_wana_stream_max_frames", "crk_wana_stream_reset", "crk_wana_stream_push", "crk_wana_stream_status"]
    lib_path = os.path.join(REPO, "crank_amd", "libcrank_hip.so")
    assert os.path.exists(lib_path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(lib_path)
    assert not [s for s in names if not hasattr(lib, s)]
    assert not [s for s in names if s not in _lib.SIGNATURES]
    header = open(os.path.join(REPO, "include", "crank_hip.h")).read()
    assert all(f"{s}(" in header for s in names)
    assert {s for s in _lib.SIGNATURES if s.startswith("crk_wana_stream_")} == set(names)


def test_streaming_mcep_refuses_bad_sizes_before_touching_the_library(monkeypatch):
    from crank_amd import _lib
    from crank_amd.world import StreamingMcep

    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "lib", no_lib)
    good = dict(fs=16000, shiftms=5.0, n_streams=2, max_samples=160, max_f0_in=4, f0_capacity=16, ring_capacity=2048)
    for bad in (dict(shiftms=0.0), dict(n_streams=0), dict(max_samples=0), dict(max_f0_in=0), dict(f0_capacity=0),
                dict(ring_capacity=100), dict(dim=128), dict(alpha=1.0), dict(max_utt_frames=0), dict(fs=4000),
                dict(dim=0, use_mcep_0th=False)):
        with pytest.raises(ValueError):
            StreamingMcep(**{**good, **bad})
