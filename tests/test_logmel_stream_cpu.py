"""The streaming log-mel front end's state machine on the host (tests/logmel_stream_ref.py restates the ring, the counts
and the read rule of crank_amd/csrc/logmel_stream_kernels.hip in float64): for every case and schedule the frames it
gathers are the rows tests/logmel_cases.mel_energies gathers from the whole signal, every read lies in the ring's last
n_fft positions or in the push (asserted inside the machine), the counts are the offline counts, max_frames is exact,
and a stream reused after its end repeats itself.  Nothing here imports crank_amd."""
import numpy as np
import pytest

from tests import logmel_cases as C
from tests import logmel_stream_ref as R

BY = {c["name"]: c for c in C.cases()}


def _schedules(case, n):
    return R.schedules(n, case["n_fft"], case["hop"], ones=case["name"] in R.ONES)


@pytest.mark.parametrize("name", R.NAMES + ["T1"])
def test_frames_are_the_whole_signal_frames_for_every_schedule(name):
    case = BY[name]
    x = C.signal(case)
    row = x[-1]  # (the last row: rows differ)
    want = R.whole_frames(case, row)
    assert want.shape == (C.n_frames(case), case["n_fft"])
    ref_e = C.mel_energies(case, x[-1:])[0]
    assert np.array_equal(R.energies_of(case, want), ref_e)  # whole_frames restates mel_energies' gather
    from_ring = 0
    for tag, counts in _schedules(case, len(row)).items():
        m = R.Machine(case["n_fft"], case["hop"], case["center"])
        got, per = m.run(row, counts)
        assert got.shape == want.shape and np.array_equal(got, want), (name, tag)
        assert np.array_equal(R.energies_of(case, got), ref_e), (name, tag)
        # nothing is emitted before it is computable, everything once it is
        done = np.cumsum(counts)
        for i, n in enumerate(done):
            last = i + 1 == len(done)
            assert sum(per[:i + 1]) == R.frames_ready(int(n), case["n_fft"], case["hop"], case["center"], end=last)
        assert (m.n, m.f) == (0, 0)
        from_ring += m.reads_ring
    assert from_ring > 0 or len(row) <= case["n_fft"]  # (the schedules do exercise the ring)


def test_frame_counts_are_the_offline_counts_at_every_end():
    for n_fft, hop in ((8, 1), (8, 3), (8, 4), (8, 8), (8, 9), (16, 5), (1024, 128), (512, 100), (2048, 300)):
        for center in (False, True):
            case = dict(n_fft=n_fft, hop=hop, center=center)
            lo = n_fft // 2 + 1 if center else n_fft
            for n in list(range(lo, lo + 4 * max(hop, n_fft) + 3)) + [99999]:
                assert R.frames_ready(n, n_fft, hop, center, end=True) == C.n_frames(case, n), (n_fft, hop, center, n)
                assert R.frames_ready(n, n_fft, hop, center) <= C.n_frames(case, n)
            for n in range(0, lo):  # what the offline call refuses (centred) or has no frame for (uncentred)
                assert R.frames_ready(n, n_fft, hop, center, end=True) == 0


def test_ready_never_runs_ahead_of_the_samples():
    """A frame counted ready at n reads no sample at or past n (centred: none that the right mirror would supply)."""
    for n_fft, hop in ((8, 1), (8, 3), (8, 9), (1024, 128)):
        h = n_fft // 2
        for n in range(0, 6 * n_fft):
            f = R.frames_ready(n, n_fft, hop, True)
            assert f == 0 or (f - 1) * hop + h <= n < f * hop + h or n <= h
            f = R.frames_ready(n, n_fft, hop, False)
            assert f == 0 or (f - 1) * hop + n_fft <= n < f * hop + n_fft


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("hop", [1, 3, 4, 8, 9])
def test_max_frames_is_never_exceeded_and_is_attained(hop, center):
    for M in (1, 2, 3, 4, 5, 8, 9, 17, 31):
        assert R.max_frames(8, hop, center, M) == R.max_frames_brute(8, hop, center, M), (hop, center, M)


def test_max_frames_at_other_small_sizes():
    for n_fft, hop, M in ((4, 1, 3), (4, 2, 7), (16, 5, 11), (16, 17, 40), (16, 8, 1), (32, 7, 64)):
        for center in (False, True):
            assert R.max_frames(n_fft, hop, center, M) == R.max_frames_brute(n_fft, hop, center, M), (n_fft, hop, center, M)


@pytest.mark.parametrize("name", ["centred_600", "r512_centred_B3", "hop1500", "fs22050_hop128"])
def test_a_stream_reused_after_end_repeats_its_first_run(name):
    case = BY[name]
    row, other = C.signal(case)[0], C.signal(case)[-1][::-1]
    counts = R.cut(len(row), R.mixed_sizes(case["n_fft"], case["hop"]))
    m = R.Machine(case["n_fft"], case["hop"], case["center"])
    first, _ = m.run(row, counts)
    m.run(other, R.cut(len(other), [37]))
    h = case["n_fft"] // 2
    assert len(m.push(other[:h], end=True)) == 0  # an utterance ended at n <= h emits nothing and resets
    again, _ = m.run(row, R.cut(len(row), [case["hop"] + 1]))
    assert np.array_equal(first, again) and np.array_equal(first, R.whole_frames(case, row))


def test_the_named_cases_exist_and_the_mixed_schedule_has_its_edges():
    assert all(n in BY for n in R.NAMES) and len(set(R.NAMES)) == len(R.NAMES) == 21
    for name in R.NAMES:
        case = BY[name]
        assert case["center"] == (name in R.CENTRED), name
        sizes = R.mixed_sizes(case["n_fft"], case["hop"])
        assert 0 in sizes and max(sizes) > 2 * case["n_fft"]
    long_ = R.cut(9999, R.mixed_sizes(1024, 128))
    assert 0 in long_ and max(long_) > 2048 and sum(long_) == 9999
    assert {BY[n]["n_fft"] for n in R.NAMES} == {512, 1024, 2048}
