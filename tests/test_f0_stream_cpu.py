"""The streaming F0 front end's state machine and grid against its definition, on the host (tests/f0_stream_ref.py), and
the one real case: the blockwise Harvest contour against the whole-signal contour (tests/harvest_ref.py).

RECORDED holds what

    python -m tests.test_f0_stream_cpu

printed for the real case: the share of 1 ms frames whose voicing differs between the streamed and the whole-signal
contour, and the largest relative F0 difference over frames both voice.  The test recomputes them; its bounds are the
issue's 1 % of frames and 10 x the recorded difference."""
import functools

import numpy as np
import pytest

from tests import f0_stream_ref as R

# name -> dict(flips, frames, rel)
RECORDED = {
    "gap_8k": dict(flips=3, frames=501, rel=4.537e-02),  # all within 35 ms of the silence's edges; median 6.8e-09
}


def stand_in(fs):
    """A deterministic 1 ms 'estimator' of the window's samples and length; unvoiced where the signal is (near) silent."""
    def est(w):
        T1 = (1000 * len(w)) // fs + 1
        pos = np.minimum(np.arange(T1) * fs // 1000, len(w) - 1)
        v = 100.0 + 40.0 * np.abs(np.sin(3.0 * w[pos] + 0.01 * len(w))) + 1e-3 * float(np.sum(w)) + 0.25 * w[0]
        return np.where(np.abs(w[pos]) < 1e-6, 0.0, v)
    return est


def signal(n, fs, seed=3):
    """Noise with silences: a short one inside a window, one longer than a window (the carry path), and one at the start."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    for a, b in ((0, 30), (200, 230), (420, 1000)):
        x[a * fs // 1000:b * fs // 1000] = 0.0
    return x


def taps_of(fs):
    from scipy.signal import firwin

    return firwin(255, 70 / (fs // 2), pass_zero=False)


def schedules(n, grid):
    Bs, As = grid.Bs, grid.As
    return {"whole": [n], "block": R.cut(n, [Bs]), "primes": R.cut(n, [7, 0, 131, 1009, 2, 0, 3571, 13]),
            "zeros": R.cut(n, [0, Bs + As - 1, 0, 1, 0, 3 * Bs + 5])}


CONFIGS = {
    "shift5": dict(fs=8000, shiftms=5),
    "shift1": dict(fs=8000, shiftms=1),
    "hop100": dict(fs=8000, hop=100),
    "hop37": dict(fs=8000, hop=37),
    "small_shift3": dict(fs=8000, shiftms=3, back=50, ahead=10, block=20),
    "small_hop9": dict(fs=8000, hop=9, back=30, ahead=1, block=8),
}


@pytest.mark.parametrize("low_cut", [False, True])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_machine_equals_definition_over_schedules(name, low_cut):
    cfg = CONFIGS[name]
    grid = R.Grid(**cfg)
    fs = grid.fs
    est, taps = stand_in(fs), taps_of(fs) if low_cut else None
    n = 10400 + 37 if "small" not in name else 3211
    x = signal(n, fs)
    want = R.define(x, grid, est, taps)
    assert len(want[0]) == grid.frames(n) and (want[1] == 0).any() and (want[1] == 1).any()
    scheds = schedules(n, grid)
    if low_cut:  # the filter is the slow part on the host: two schedules suffice for the ring's extra reach
        scheds = {k: scheds[k] for k in ("primes", "zeros")}
    for sname, counts in scheds.items():
        m = R.Machine(grid, est, max(counts) if max(counts) else 1, taps)
        got, per = m.run(x, counts)
        for g, w, what in zip(got, want, ("raw", "uv", "cf0")):
            np.testing.assert_array_equal(g, w, err_msg=f"{name} {sname} {what}")
        assert max(per) <= R.max_frames(grid, max(max(counts), 1)), (name, sname)
        assert m.reads_ring > 0 or len(counts) == 1
        assert (m.n, m.b, m.carry) == (0, 0, m.carry0)  # the end returned the stream to its start state


@pytest.mark.parametrize("name", ["shift5", "hop37", "small_hop9"])
def test_end_lengths_around_the_minimum_and_a_readiness_boundary(name):
    grid = R.Grid(**CONFIGS[name])
    est = stand_in(grid.fs)
    edge = [grid.Bs + grid.As, 2 * grid.Bs + grid.As, 5 * grid.Bs + grid.As]
    lengths = [0, 1, 63, 64, 65] + [e + d for e in edge for d in (-1, 0, 1)]
    for n in lengths:
        x = signal(max(n, 1), grid.fs, seed=n)[:n]
        want = R.define(x, grid, est)
        assert len(want[0]) == (grid.frames(n) if n >= 64 else 0)
        for counts in ([n], R.cut(n, [grid.Bs]), R.cut(n, [grid.Bs + grid.As, 0]), R.cut(n, [n, 0]) + [0]):
            m = R.Machine(grid, est, max(max(counts), 1))
            got, _ = m.run(x, counts)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w, err_msg=f"{name} n={n} {counts[:4]}")


def test_an_ended_stream_starts_again_and_reuse_equals_a_fresh_machine():
    grid = R.Grid(**CONFIGS["small_shift3"])
    est = stand_in(grid.fs)
    x, y = signal(2000, grid.fs, 1), signal(1777, grid.fs, 2)
    m = R.Machine(grid, est, 500)
    m.run(x, R.cut(len(x), [333]))
    got, _ = m.run(y, R.cut(len(y), [500]))
    for g, w in zip(got, R.define(y, grid, est)):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("cfg", [dict(fs=2000, shiftms=3, back=5, ahead=2, block=4), dict(fs=2000, hop=3, back=5, ahead=2, block=4),
                                 dict(fs=4000, hop=5, back=3, ahead=1, block=3), dict(fs=4000, hop=4, back=3, ahead=2, block=2),
                                 dict(fs=4000, shiftms=2, back=3, ahead=1, block=3), dict(fs=1000, shiftms=1, back=4, ahead=1, block=4)])
def test_max_frames_is_exact_over_all_histories(cfg):
    """The closed form against every history, push size and end flag at a toy size (several periods of the counts)."""
    grid = R.Grid(min_samples=4, **cfg)
    step = grid.hop if grid.hop else max(grid.shiftms * grid.fs // 1000, 1)
    n0_max = grid.As + 3 * grid.Bs * step + 2
    for max_samples in (1, 2, 5, 9, 17, 40):
        assert R.max_frames(grid, max_samples) == R.max_frames_brute(grid, max_samples, n0_max), (cfg, max_samples)


def test_the_hop_grid_is_the_shiftms_grid_wherever_both_exist():
    t = np.arange(5000)
    for fs, shiftms in ((16000, 5), (8000, 1), (24000, 10), (48000, 5), (22050, 20), (44100, 20), (16000, 3)):
        hop = shiftms * fs // 1000
        assert hop * 1000 == shiftms * fs
        a, b = R.Grid(fs, shiftms=shiftms, back=300, ahead=100, block=80), R.Grid(fs, hop=hop, back=300, ahead=100, block=80)
        np.testing.assert_array_equal(a.idx(t), b.idx(t))
        for n in (0, 63, 64, 1000, 12345, fs):
            assert a.frames(n) == b.frames(n)
        for m in range(0, 2000, 7):
            assert R.first_frame(a, m) == R.first_frame(b, m)
    # the recipe's grid, which no integer shiftms serves: frame t sits at the 1 ms frame nearest t * 128 samples
    g = R.Grid(22050, hop=128, back=300, ahead=100, block=80)
    np.testing.assert_array_equal(g.idx(t), np.floor(t * 128 * 1000.0 / 22050 + 0.5).astype(np.int64))


def test_grid_refuses_boundaries_off_a_whole_sample():
    for fs, ms in ((22050, 30), (44100, 5), (22050, 1)):
        with pytest.raises(AssertionError):
            R.Grid(fs, shiftms=5, back=300, ahead=100, block=ms)
    R.Grid(22050, hop=128, back=300, ahead=100, block=80)
    R.Grid(44100, hop=256, back=300, ahead=100, block=80)


# ------------------------------------------------------------------------------------------------------ the real case
@functools.lru_cache(maxsize=None)
def measure(name="gap_8k"):
    """Streamed (blockwise, at the defaults 300 / 100 / 80 ms) against whole-signal Harvest on the 1 ms grid."""
    from tests import harvest_cases as HC
    from tests import harvest_ref as H

    c = HC.cases()[name]
    w, fs = c["utts"][0], c["fs"]
    est = lambda s: H.harvest(s, fs, w["minf0"], w["maxf0"], shiftms=1)  # noqa: E731
    whole = est(w["x"])
    streamed = R.define(w["x"], R.Grid(fs, shiftms=1), est)[0]
    assert len(whole) == len(streamed)
    d, flips = HC.rel(streamed, whole)
    return dict(flips=flips, frames=len(whole), rel=d, unvoiced=int(np.sum(whole == 0)), voiced=int(np.sum(whole != 0)))


def test_streamed_harvest_follows_the_whole_signal_contour_across_a_silence():
    """gap_8k: voiced - 50 ms of digital silence (longer than Harvest bridges) - voiced, 0.5 s at 8 kHz; no low cut, so the
    silence stays exactly zero."""
    m, rec = measure(), RECORDED["gap_8k"]
    print("gap_8k", m)
    assert m["unvoiced"] >= 25 and m["voiced"] >= 300  # the whole-signal contour leaves most of the 50 ms gap unvoiced
    assert m["frames"] == rec["frames"]
    assert m["flips"] <= 0.01 * m["frames"]
    assert m["rel"] <= 10.0 * rec["rel"]


if __name__ == "__main__":
    print(measure())
