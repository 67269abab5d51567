"""The frame join's state machine (tests/join_ref.py, restating csrc/join_kernels.h) against the obvious definition, and
``crank_amd.live.join_capacities`` against brute force over the two front ends' own counting rules.  No GPU."""
import numpy as np
import pytest

from tests import f0_stream_ref as FR
from tests import join_ref as JR
from tests import logmel_stream_ref as LR


def _run(seed, S, wa, wb, ma, mb, ca, cb, n_push, **kw):
    m, ref = JR.Join(S, wa, wb, ma, mb, ca, cb), JR.Lists(S, ca, cb)
    seen = dict(a_leads=0, b_leads=0, zero=0, end_surplus_a=0, end_surplus_b=0, end_empty=0, reuse=0, over_a=0, over_b=0)
    ended = [False] * S
    for i, (n_a, n_b, end) in enumerate(JR.schedule(seed, S, ma, mb, n_push, **kw)):
        a, b = JR.rows_for(1000 * seed + 2 * i, S, ma, wa), JR.rows_for(1000 * seed + 2 * i + 1, S, mb, wb)
        out_a = np.full((S, m.max_frames + 1, wa), np.float32(777))
        out_b = np.full((S, m.max_frames + 1, wb), np.float32(777))
        wa0, wb0 = m.A.wait.copy(), m.B.wait.copy()
        n, first, dropped = m.push(a, n_a, b, n_b, end, out_a, out_b)
        for s in range(S):
            pairs, f, d = ref.push(s, a[s, :n_a[s]], b[s, :n_b[s]], end[s])
            assert (n[s], first[s], dropped[s]) == (len(pairs), f, d), (i, s)
            for j, (ra, rb) in enumerate(pairs):
                assert np.array_equal(out_a[s, j], ra) and np.array_equal(out_b[s, j], rb), (i, s, j)
            assert (out_a[s, n[s]:] == 777).all() and (out_b[s, n[s]:] == 777).all()
            assert m.overflow[s] == ref.overflow[s]
            assert (m.A.wait[s], m.B.wait[s]) == (len(ref.qa[s]), len(ref.qb[s]))
            seen["a_leads"] += m.A.wait[s] > 0
            seen["b_leads"] += m.B.wait[s] > 0
            seen["zero"] += n_a[s] == 0 and n_b[s] == 0
            if end[s]:
                ta, tb = wa0[s] + n_a[s], wb0[s] + n_b[s]
                seen["end_surplus_a"] += ta > tb
                seen["end_surplus_b"] += tb > ta
                seen["end_empty"] += ta == 0 and tb == 0
            elif ended[s] and n[s]:
                seen["reuse"] += 1
            ended[s] = ended[s] or bool(end[s])
        seen["over_a"] = int((m.overflow & 1).sum())
        seen["over_b"] = int((m.overflow & 2).sum())
    return seen


def test_state_machine_equals_two_lists_with_each_side_leading():
    a = _run(1, 4, 5, 2, 3, 4, 1500, 1500, 300, lead="a")
    b = _run(2, 4, 5, 2, 3, 4, 1500, 1500, 300, lead="b")
    assert a["a_leads"] > 50 and b["b_leads"] > 50
    for seen in (a, b):
        assert seen["zero"] and seen["end_empty"] and seen["reuse"]
        assert seen["over_a"] == 0 and seen["over_b"] == 0
    assert a["end_surplus_a"] and b["end_surplus_b"]


@pytest.mark.parametrize("ca,cb", [(7, 7), (1, 1), (0, 3), (3, 0), (0, 0)])
def test_small_rings_wrap_and_overflow_keeps_the_oldest_rows(ca, cb):
    a = _run(3, 3, 3, 1, 4, 4, ca, cb, 400, lead="a", burst=0.2, p_end=0.03)
    b = _run(4, 3, 3, 1, 4, 4, ca, cb, 400, lead="b", burst=0.2, p_end=0.03)
    assert a["over_a"] and b["over_b"]  # every capacity here is overrun by a burst, cap = 0 by any lone row


def test_reset_restarts_one_stream():
    m = JR.Join(2, 2, 2, 2, 2, 3, 3)
    a, b = JR.rows_for(1, 2, 2, 2), JR.rows_for(2, 2, 2, 2)
    out_a, out_b = np.zeros((2, m.max_frames, 2), np.float32), np.zeros((2, m.max_frames, 2), np.float32)
    m.push(a, [2, 2], b, [1, 1], None, out_a, out_b)
    m.reset([1])
    assert (m.A.wait.tolist(), m.first.tolist()) == ([1, 0], [1, 0])
    n, first, _ = m.push(a, [0, 0], b, [2, 2], None, out_a, out_b)
    assert (n.tolist(), first.tolist()) == ([1, 0], [1, 0]) and np.array_equal(out_a[0, 0], a[0, 1])
    assert m.B.wait.tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------- the capacities
GRIDS = [  # fs, n_fft, hop, center, back, ahead, block
    (16000, 1024, 128, True, 300, 100, 80),    # the recipe's grid
    (22050, 1024, 128, True, 300, 100, 80),    # (block_ms and ahead_ms are multiples of 20: whole samples at 22 050 Hz)
    (16000, 2048, 128, True, 300, 1, 4),       # F0 leads: 16 samples of look-ahead, blocks of Harvest's 64 samples
    (16000, 1024, 128, False, 300, 100, 80),
    (16000, 2048, 256, False, 300, 1, 8),
]


def _counts(fs, n_fft, hop, center, back, ahead, block, n_max):
    """Frames each front end has emitted at every sample count below n_max (no end flag)."""
    grid = FR.Grid(fs, hop=hop, back=back, ahead=ahead, block=block)
    mel = np.array([LR.frames_ready(n, n_fft, hop, center) for n in range(n_max)])
    per_blocks = {}
    f0 = np.zeros(n_max, np.int64)
    for n in range(n_max):
        J = grid.blocks(n)
        if J not in per_blocks:
            per_blocks[J] = FR.first_frame(grid, J * block)
        f0[n] = per_blocks[J]
    return grid, mel, f0


@pytest.mark.parametrize("g", GRIDS)
def test_capacities_are_never_exceeded_and_attained_within_one_row(g):
    from crank_amd.live import join_capacities, join_max_frames

    fs, n_fft, hop, center, back, ahead, block = g
    n_max = fs + 2 * n_fft + 2  # more than one second, sample by sample
    grid, mel, f0 = _counts(*g, n_max)
    lead_a, lead_b = int((mel - f0).max()), int((f0 - mel).max())
    cap_a, cap_b = join_capacities(fs, n_fft, hop, center, back, ahead, block, 1024)
    print(f"{g}: mel leads by {lead_a} (cap_a {cap_a}), F0 leads by {lead_b} (cap_b {cap_b})")
    assert max(lead_a, 0) <= cap_a <= max(lead_a, 0) + 1
    assert max(lead_b, 0) <= cap_b <= max(lead_b, 0) + 1
    if (n_fft, ahead) == (2048, 1):
        assert lead_b > 0 and cap_b > 0  # the grid on which F0 leads
    if (n_fft, ahead, center) == (1024, 100, True):
        assert lead_b <= 0 and cap_b == 0 and lead_a >= 100 * fs // 1000 // hop  # the recipe's: F0 is the later side
    # max_frames bounds every push: what one push emits is what both sides have, waiting plus new, the end flush included
    for max_samples in (1, 1024):
        max_a = LR.max_frames(n_fft, hop, center, max_samples)
        max_b = FR.max_frames(grid, max_samples)
        bound = join_max_frames(cap_a, cap_b, max_a, max_b)
        step = 1 if max_samples == 1 else 37
        for n0 in range(0, n_max - max_samples, step):
            n1 = n0 + max_samples
            done = min(mel[n0], f0[n0])
            assert min(mel[n1], f0[n1]) - done <= bound
            if n1 >= grid.min_samples:  # the end push: both flush to the offline count (mel: none at or below the half window)
                ma = LR.frames_ready(n1, n_fft, hop, center, end=True)
                assert ma - mel[n0] <= max_a and grid.frames(n1) - f0[n0] <= max_b
                assert min(ma, grid.frames(n1)) - done <= bound
