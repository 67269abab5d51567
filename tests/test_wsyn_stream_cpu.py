"""Streaming WORLD synthesis without a GPU: the definition in sets (tests/wsyn_stream_ref.py)
equals the offline restatement under every cut; ``synthesis_capacities`` holds on walks of row histories at toy sizes and
is tight (one unit less overflows on some history); the module's refusals; the C-ABI names."""
import itertools
import os

import numpy as np
import pytest

from crank_amd import _lib
from crank_amd.world import StreamingWorldSynthesizer, longest_pulse_interval, synthesis_capacities
from tests import world_synth_ref as R
from tests import wsyn_stream_ref as W
from tests.world_inputs import with_f0
from tests.wsyn_inputs import ALPHA, FS, SHIFTMS, short

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["crk_wsyn_stream_create", "crk_wsyn_stream_destroy", "crk_wsyn_stream_state_bytes", "crk_wsyn_stream_max_out",
         "crk_wsyn_stream_reset", "crk_wsyn_stream_push", "crk_wsyn_stream_status"]


# ---------------------------------------------------------------------------------------------- definition == offline
@pytest.mark.parametrize("T", range(2, 13))
def test_every_cut_equals_the_offline_restatement(T):
    """Every cut of T rows into pushes of at most 3 rows, the end flag on the last rows and on a push of its own: the
    samples that leave, joined, are world_synth_ref.synthesis value for value, and their counts sum to y_length(T).  One
    memo of frame tables and responses per utterance, keyed by every input of each, keeps the FFT work to one per pulse."""
    rng = np.random.default_rng(T)
    f0, mc, cap, rmc = with_f0(rng, short(T, T), 8, 1)
    rmc = rmc if T % 3 else None
    ref = R.synthesis(f0, mc, cap, rmc, fs=FS, shiftms=SHIFTMS, alpha=ALPHA)
    assert len(ref) == R.y_length(T, FS, SHIFTMS)
    pos, ns, shift, pvuv, _ = R.pulses(f0, FS, R.FFTL, SHIFTMS)
    memo = {}
    for cut in W.cuts(T, 3):
        for end_alone in (False, True):
            st = W.Stream(FS, SHIFTMS, ALPHA, rmc is not None, memo=memo)
            y, counts = W.run(st, f0, mc, cap, rmc, cut, end_alone)
            assert sum(counts) == len(ref)
            assert np.array_equal(y, ref), (cut, end_alone)
            assert st.flags == 0
            added = np.array(st.added, np.float64).reshape(-1, 5)
            assert np.array_equal(added[:, 0], pos) and np.array_equal(added[:, 1], ns)
            assert np.array_equal(added[:, 2], shift) and np.array_equal(added[:, 3], pvuv)
            assert np.array_equal(added[:, 4], pos - pos[0] if len(pos) else pos)
            assert st.n == 0 and st.pend is None and not st.f0  # back at the start state


def test_short_end_and_empty_end():
    st = W.Stream(FS, SHIFTMS, ALPHA, responses=False)
    assert len(st.push([], end=True)) == 0 and st.flags == 0  # a no-op reset
    assert len(st.push([150.0], end=True)) == 0 and st.flags == W.FLAG_SHORT and st.dropped == 1
    st.reset()
    st.push([np.nan, -1.0, 1000.5, 150.0])
    assert st.flags == W.FLAG_F0 and st.f0 == [0.0, 0.0, 0.0, 150.0]


# ---------------------------------------------------------------------------------------------- capacities
# The toys: 16-point responses (a pulse at s covers s - 7 .. s + 8, the floor is fs // 16 + 1 Hz) at 3 and 2 samples a
# frame, where the ramps next to unvoiced rows are one sample long and the closed forms can be met exactly, and at 10
# samples a frame, where they cannot (the no-flag walk only).
TOYS = [(2000, 1.5, 16, 400.0), (2000, 1.0, 16, 400.0), (2000, 5.0, 16, 400.0)]


def _alphabet(fs, fftl, ceil):
    low = fs // fftl + 1
    return np.array([0.0, low, low + 1.0, low + 5.0, low * 1.2, low * 1.5, 2.0 * low - 1.0, 333.0, ceil])


def _histories(toy, trials, seed):
    """Row histories within f0_ceil.  Structured: a steady stretch at the floor, up to two free rows (they set the
    phase), one unvoiced row, the floor again - the ramp into a slowest contour, where the closed forms are met.  Then
    `trials` seeded ones: free rows, or a free prefix before a steady stretch at the floor or the ceiling."""
    fs, _, fftl, ceil = toy
    al = _alphabet(fs, fftl, ceil)
    for k in range(3):
        for pre in itertools.product(al, repeat=k):
            for lead in range(0, 24, 1 if k < 2 else 5):
                yield np.array([al[1]] * lead + list(pre) + [0.0] + [al[1]] * 14)
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        T = int(rng.integers(2, 41))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            yield rng.choice(al, T)
            continue
        k = int(rng.integers(0, min(T, 6)))
        f0 = np.concatenate([rng.choice(al, k), np.full(T - k, al[1] if kind == 1 else ceil)])
        if rng.random() < 0.5:
            f0[-1] = rng.choice(al)
        yield f0


def _walk(toy, r, caps, trials, seed, want=0):
    """Every history cut into pushes of r rows and into seeded pushes of 1 .. r; before every push the stream is also
    ended there, with 0 .. r rows.  Returns the union of the capacity flags seen (at once when `want` is among them)."""
    fs, shiftms, fftl, ceil = toy
    rng = np.random.default_rng(seed + 1)
    seen = 0
    for f0 in _histories(toy, trials, seed):
        for full in (True, False) if r > 1 else (True,):
            st = W.Stream(fs, shiftms, f0_ceil=ceil, fftl=fftl, caps=caps, responses=False)
            k, T = 0, len(f0)
            while k < T:
                c = min(T - k, r if full else int(rng.integers(1, r + 1)))
                for ce in {0, c, min(T - k, r)}:
                    fork = st.clone()
                    fork.push(f0[k:k + ce], end=True)
                    seen |= fork.flags
                st.push(f0[k:k + c])
                k += c
            seen |= st.flags
            if seen & want:
                return seen
    return seen & (W.FLAG_RING | W.FLAG_QUEUE | W.FLAG_PULSES | W.FLAG_OUT)


@pytest.mark.parametrize("toy", TOYS)
@pytest.mark.parametrize("r", [1, 2, 3])
def test_capacities_never_flag_within_f0_ceil(toy, r):
    caps = synthesis_capacities(toy[0], toy[1], r, toy[3], fftl=toy[2])
    assert _walk(toy, r, caps, 150, r) == 0


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("name,flag", [("rows", W.FLAG_QUEUE), ("ring", W.FLAG_RING), ("pulses", W.FLAG_PULSES),
                                       ("out", W.FLAG_OUT)])
def test_each_capacity_is_tight(name, flag, r):
    """One unit less of each capacity has a history within f0_ceil that sets its flag, at the toy where the closed
    forms can be met (3 samples a frame), for pushes of one row and of two."""
    toy = TOYS[0]
    caps = synthesis_capacities(toy[0], toy[1], r, toy[3], fftl=toy[2])
    caps[name] -= 1
    assert _walk(toy, r, caps, 3000, 7, want=flag) & flag, f"no history overflows {name} - 1 = {caps[name]}"


def test_capacities_at_the_recipe_sizes():
    caps = synthesis_capacities(16000, 5, 16, 1000.0)
    assert longest_pulse_interval(16000, 5) == 1021  # 1000 samples at 16 Hz and two 40-sample ramps' 20.5
    assert caps == {"rows": 2 + 13 + 16, "ring": 1021 + 511 + 1281 + 512, "pulses": 89, "out": 1021 + 1 + 511 + 1360}
    for bad in (dict(fs=16000, shiftms=0.1, max_rows_in=4), dict(fs=16000, shiftms=5, max_rows_in=0),
                dict(fs=16000, shiftms=5, max_rows_in=4, f0_ceil=4000.5), dict(fs=16000, shiftms=5, max_rows_in=4, f0_ceil=0)):
        with pytest.raises(ValueError):
            synthesis_capacities(**bad)


# ---------------------------------------------------------------------------------------------- refusals, names
@pytest.mark.parametrize("kw", [dict(fs=8000), dict(shiftms=0.1), dict(order1=0), dict(order1=129), dict(alpha=1.0),
                                dict(f0_ceil=4000.5), dict(n_streams=0), dict(max_rows_in=0), dict(max_utt_samples=0),
                                dict(capacities={"rows": 1, "ring": 4096, "pulses": 8, "out": 64}),
                                dict(capacities={"rows": 8, "ring": 512, "pulses": 8, "out": 64}),
                                dict(capacities={"rows": 8, "ring": 4096, "pulses": 0, "out": 64})])
def test_constructor_refuses_before_touching_the_device(kw):
    args = dict(fs=16000, shiftms=5.0, n_streams=2, max_rows_in=4, order1=25, alpha=0.41)
    args.update(kw)
    with pytest.raises(ValueError):
        StreamingWorldSynthesizer(**args)


def test_abi_names():
    header = open(os.path.join(REPO, "include", "crank_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
