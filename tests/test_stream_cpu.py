"""Streaming conversion (crank_amd.stream, csrc/stream_kernels.hip), the part that needs no GPU: the state definition the
kernel implements (tests/stream_ref.py against the oracle's offline causal forward, float64), the fixture's code margins,
the exported symbols and the constructor's refusals."""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import stream_inputs as SI
from tests.helpers import REPO, load_yaml
from tests.stream_ref import StreamRef, oracle_in_float64


@pytest.fixture(scope="module")
def offline64():
    """The oracle's offline causal forward on the default fixture, in float64."""
    fx = SI.fixture()
    orac = copy.deepcopy(fx.orac).double()
    with oracle_in_float64():
        return fx.offline(orac, torch.float64)


@pytest.mark.parametrize("schedule", sorted(SI.SCHEDULES))
def test_chunked_stateful_restatement_equals_the_offline_causal_forward(schedule, offline64):
    """Stream 0 of the default fixture pushed through StreamRef in every chunk schedule of the GPU tests: decoded and the
    quantizers' inputs within 1e-12 of the offline forward (relative to the largest value), identical indices.  The last of
    the 150 frames lie behind the whole 132-frame receptive chain: they depend on every layer's carried state."""
    fx = SI.fixture()
    assert fx.reach == 132 and SI.T > fx.reach
    dec_h, h = fx.dec_cond()
    emb = fx.orac.spkr_embedding(h[0]).detach()
    cond = torch.cat([dec_h[0], emb], -1)
    ref = StreamRef(fx.orac)
    dec, qidx, enc, t = [], [[] for _ in range(fx.nst)], [[] for _ in range(fx.nst)], 0
    for c in SI.SCHEDULES[schedule]:
        d, q, e = ref.push(fx.x[0, t: t + c], cond[t: t + c])
        dec.append(d)
        for n in range(fx.nst):
            qidx[n].append(q[n])
            enc[n].append(e[n])
        t += c
    assert t == SI.T
    want = offline64["decoded"][0]
    assert float((torch.cat(dec) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for n in range(fx.nst):
        assert torch.equal(torch.cat(qidx[n]), offline64["qidx"][n][0])
        want = offline64["encoded"][n][0]
        assert float((torch.cat(enc[n]) - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name", ["default"] + sorted(SI.VARIANTS))
def test_fixture_margins_leave_out_at_most_two_percent(name):
    """The oracle alone: frames whose best two codes lie within MARGIN of each other, with everything behind them in the
    receptive chain, are at most 2 % of the frames the GPU tests compare; and the codes are spread, not collapsed."""
    fx = SI.fixture(**SI.VARIANTS.get(name, {}))
    print(f"{name}: left out {fx.left_out:.4f} of the compared frames, reach {fx.reach}")
    assert fx.left_out <= SI.MAX_LEFT_OUT
    for n in range(fx.nst):
        assert len(np.unique(fx.ref["qidx"][n].numpy())) >= 8


def test_stream_symbols_are_exported_and_bound():
    from crank_amd import _lib

    names = ["crk_stream_create", "crk_stream_destroy", "crk_stream_reserve", "crk_stream_state_bytes",
             "crk_stream_prepare", "crk_stream_reset", "crk_stream_push"]
    lib_path = os.path.join(REPO, "crank_amd", "libcrank_hip.so")
    assert os.path.exists(lib_path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(lib_path)
    assert not [s for s in names if not hasattr(lib, s)]
    assert not [s for s in names if s not in _lib.SIGNATURES]
    header = open(os.path.join(REPO, "include", "crank_hip.h")).read()
    assert all(f"{s}(" in header for s in names)
    # the header's struct under the C ABI's natural alignment: 9 ints (+ 4 bytes of padding), 9 long long, 6 ints, 1 long long
    assert ctypes.sizeof(_lib.StreamDesc) == 40 + 72 + 24 + 8


def _stub(**over):
    """What the constructor's checks read of a generator (a real one needs the GPU)."""
    return types.SimpleNamespace(conf=load_yaml(None, **over), spkr_size=4)


@pytest.mark.parametrize("over,key", [
    (dict(causal=False), "causal"),
    (dict(causal=True, use_raw=True), "use_raw"),
    (dict(causal=True, emb_dim=[48, 64, 64]), r"emb_dim\[0\]"),
    (dict(causal=True, kernel_size=[7, 3, 3]), r"kernel_size\[0\]"),
    (dict(causal=True, input_size=200), "input_size"),
    (dict(causal=True, n_layers=[8, 2, 2]), r"n_layers\[0\]"),
])
def test_constructor_refuses_by_key_before_touching_the_library(over, key, monkeypatch):
    from crank_amd import _lib, stream

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(NotImplementedError, match=key) as err:
        stream.StreamingConverter(_stub(**over), 2, 64)
    if key == "causal":  # the look-ahead a non-causal model needs: half of its 132-frame receptive chain
        assert "66 frames after" in str(err.value)
