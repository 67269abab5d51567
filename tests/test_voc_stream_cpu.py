"""Streaming vocoding (crank_amd.vocoder.StreamingVocoder, csrc/voc_stream_kernels.hip), the part that needs no GPU: the
look-ahead rule, its safety on the offline restatement alone, the frontier scheme the kernels implement
(tests/voc_stream_ref.py against tests/pwg_vocoder_ref.py in float64) and the exported symbols."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import REPO
from tests.pwg_vocoder_ref import random_generator
from tests.voc_stream_ref import ChunkedVocoderRef

AUX = 8
# name -> (generator parameters, look-ahead in frames)
CONFIGS = {
    "10/1 [2,2] win 2": (dict(layers=10, stacks=1, aux_context_window=2, upsample_params={"upsample_scales": [2, 2]}), 260),
    "6/2 [5,6] win 0": (dict(layers=6, stacks=2, aux_context_window=0, upsample_params={"upsample_scales": [5, 6]}), 2),
    "30/3 [4,4,4,4] win 2": (dict(layers=30, stacks=3, aux_context_window=2, upsample_params={"upsample_scales": [4, 4, 4, 4]}), 16),
    "4/2 [2,3] win 1": (dict(layers=4, stacks=2, aux_context_window=1, upsample_params={"upsample_scales": [2, 3]}), 4),
}


def _hop(params):
    return int(np.prod(params["upsample_params"]["upsample_scales"]))


@functools.lru_cache(maxsize=None)
def _generator(name):
    g = random_generator(21, aux_channels=AUX, **CONFIGS[name][0])
    g.remove_weight_norm()
    return g


def test_lookahead_of_the_default_and_of_the_three_other_configurations():
    from crank_amd.vocoder import GENERATOR_DEFAULTS, generator_params, lookahead_frames

    assert lookahead_frames(GENERATOR_DEFAULTS) == 16
    assert lookahead_frames(generator_params({})) == 16
    for name, (params, la) in CONFIGS.items():
        assert lookahead_frames(generator_params({"generator_params": params})) == la, name


@pytest.mark.parametrize("name", list(CONFIGS))
def test_offline_samples_la_frames_back_do_not_depend_on_later_frames_or_their_noise(name):
    """PWGVocoderRef alone: with frames >= F and their noise replaced, every sample of frames < F - LA is identical."""
    params, la = CONFIGS[name]
    g, H = _generator(name), _hop(params)
    T = la + 24
    F = la + 14
    gen = torch.Generator().manual_seed(3)
    c, x = torch.randn(T, AUX, generator=gen), torch.randn(T * H, generator=gen)
    c2, x2 = c.clone(), x.clone()
    c2[F:] = torch.randn(T - F, AUX, generator=gen) * 3
    x2[F * H:] = torch.randn((T - F) * H, generator=gen) * 3
    with torch.no_grad():
        y, y2 = g.inference(c, x), g.inference(c2, x2)
    n = (F - la) * H
    assert n > 0 and torch.equal(y[:n], y2[:n])
    assert not torch.equal(y, y2)


def _chunks(kind, T):
    if kind == "ones":
        return [1] * T
    if kind == "whole":
        return [T]
    rs, out = np.random.RandomState(T), []
    while sum(out) < T:
        out.append(min(int(rs.randint(1, 8)), T - sum(out)))
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """(chunked restatement, [(c, x, float64 offline waveform)] for utterances longer than, shorter than and around LA)."""
    import copy

    params, la = CONFIGS[name]
    g, H = _generator(name), _hop(params)
    g64 = copy.deepcopy(g).double()
    gen = torch.Generator().manual_seed(8)
    utts = []
    for T in (la + 13, max(1, la - 1), 1):
        c = torch.randn(T, AUX, generator=gen, dtype=torch.float64)
        x = torch.randn(T * H, generator=gen, dtype=torch.float64)
        with torch.no_grad():
            utts.append((c.numpy(), x.numpy(), g64.inference(c, x).numpy()))
    return ChunkedVocoderRef(g, la + 13), utts


def _run(ref, c, x, chunks, H):
    """Push an utterance in `chunks`, the end flag on the last; (emitted per push, frames before each push)."""
    outs, t = [], 0
    for i, n in enumerate(chunks):
        outs.append(ref.push(c[t:t + n], x[t * H:(t + n) * H], end=i + 1 == len(chunks)))
        t += n
    return outs


@pytest.mark.parametrize("kind", ["ones", "random", "whole"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_chunked_frontier_restatement_equals_the_offline_restatement(name, kind):
    """Float64 on both sides: within 1e-12 of the peak (rounding of <= 272-term sums with headroom; a position error is
    O(1), and reading a position no stage has computed yet is NaN).  The first utterance is longer than LA, the second
    shorter, the third one frame: all three back to back through `end` on one state.  What each push emits follows the
    rule max(0, T - LA) frames, everything at the end."""
    params, la = CONFIGS[name]
    ref, utts = _case(name)
    H = _hop(params)
    assert ref.LA == la and ref.H == H
    ref.reset()
    for c, x, want in utts:
        chunks = _chunks(kind, len(c))
        outs = _run(ref, c, x, chunks, H)
        t = 0
        for i, (n, o) in enumerate(zip(chunks, outs)):
            end = i + 1 == len(chunks)
            emitted = ((t + n) if end else max(0, t + n - la)) - max(0, t - la)
            assert len(o) == emitted * H, (i, len(o), emitted)
            t += n
        got = np.concatenate(outs)
        assert got.shape == want.shape
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert ref.T == 0


def test_voc_stream_symbols_are_declared_bound_and_exported():
    from crank_amd import _lib

    names = ["crk_voc_stream_create", "crk_voc_stream_destroy", "crk_voc_stream_state_bytes", "crk_voc_stream_lookahead",
             "crk_voc_stream_reset", "crk_voc_stream_push"]
    lib_path = os.path.join(REPO, "crank_amd", "libcrank_hip.so")
    assert os.path.exists(lib_path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(lib_path)
    assert not [s for s in names if not hasattr(lib, s)]
    assert not [s for s in names if s not in _lib.SIGNATURES]
    header = open(os.path.join(REPO, "include", "crank_hip.h")).read()
    assert all(f"{s}(" in header for s in names)
    assert {s for s in _lib.SIGNATURES if s.startswith("crk_voc_stream_")} == set(names)


@pytest.mark.parametrize("n_streams,max_chunk", [(0, 4), (2, 0), (-1, 1)])
def test_streaming_refuses_sizes_below_one_before_touching_the_library(n_streams, max_chunk, monkeypatch):
    import types

    from crank_amd import _lib, vocoder

    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "lib", no_lib)
    stub = types.SimpleNamespace(device=torch.device("cuda"))
    with pytest.raises(ValueError, match="both must be at least 1"):
        vocoder.StreamingVocoder(stub, n_streams, max_chunk)
