"""Look-ahead streaming conversion (crank_amd.stream.LookaheadConverter, csrc/stream_la_kernels.hip), the part that needs no
GPU: the scheme the kernel implements (tests/stream_la_ref.py against the oracle's offline non-causal forward, float64),
the one-sided look-ahead property on the oracle alone, the fixtures' code margins, the exported symbols and the refusals."""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import stream_la_inputs as LI
from tests.helpers import REPO, load_yaml
from tests.stream_la_ref import LookaheadRef
from tests.stream_ref import oracle_in_float64

CONFS = {"default": {}, "small": LI.SMALL}
CHUNKINGS = {"c1": lambda n: [1] * n, "mixed": lambda n: LI.SCHEDULES["mixed"] if n == LI.T else _cut((1, 7, 16, 2, 33, 1), n),
             "whole": lambda n: [n]}


def _cut(sizes, total):
    out, done, i = [], 0, 0
    while done < total:
        out.append(min(sizes[i % len(sizes)], total - done))
        done += out[-1]
        i += 1
    return out


@pytest.fixture(scope="module")
def orac64():
    made = {}

    def get(name):
        if name not in made:
            made[name] = copy.deepcopy(LI.fixture(**CONFS[name]).orac).double()
        return made[name]
    return get


def _cond(fx, s):
    dec_h, h = fx.dec_cond()
    return torch.cat([dec_h[s], fx.orac.spkr_embedding(h[s]).detach()], -1)


def _stream(ref, fx, s, lo, hi, sizes, end_alone):
    """Frames [lo, hi) of fixture stream s through ``ref`` as one utterance cut into `sizes`; the end flag on the push with
    the last frames, or (end_alone) on a later push without frames.  Returns decoded, qidx, encoded of the whole utterance
    after checking that every push emitted frames [max(0, T - LA), max(0, T' - LA)) and the end push the rest."""
    cond = _cond(fx, s)
    dec, qidx, enc, t, emitted = [], [[] for _ in range(fx.nst)], [[] for _ in range(fx.nst)], lo, 0
    pushes = [(c, False) for c in sizes]
    pushes = pushes + [(0, True)] if end_alone else pushes[:-1] + [(pushes[-1][0], True)]
    for c, end in pushes:
        first, d, q, e = ref.push(fx.x[s, t: t + c], cond[t: t + c], end=end)
        t += c
        want = (hi - lo) if end else max(0, t - lo - ref.la)
        assert first == emitted and d.shape[0] == want - emitted, (first, emitted, d.shape, want)
        emitted = want
        dec.append(d)
        for n in range(fx.nst):
            qidx[n].append(q[n])
            enc[n].append(e[n])
    assert t == hi
    return torch.cat(dec), [torch.cat(q) for q in qidx], [torch.cat(e) for e in enc]


def _check(got, want):
    dec, qidx, enc = got
    assert not bool(torch.isnan(dec).any()), "a frame nobody computed was read"
    ref = want["decoded"][0]
    assert float((dec - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    for n in range(len(qidx)):
        assert torch.equal(qidx[n], want["qidx"][n][0])
        ref = want["encoded"][n][0]
        assert float((enc[n] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("name", sorted(CONFS))
def test_chunked_restatement_equals_the_offline_non_causal_forward(name, chunking, orac64):
    """All S = 3 streams of T = 150 frames, each an utterance of its own, through LookaheadRef frame by frame, in the mixed
    schedule and at once: decoded and the quantizers' inputs within 1e-12 of the oracle's offline forward of the whole
    utterance in float64, identical indices; the end flag alternately with the last frames and alone."""
    fx = LI.fixture(**CONFS[name])
    assert fx.la == (66 if name == "default" else 12) and LI.T > 2 * fx.la
    ref = LookaheadRef(fx.orac)
    assert ref.la == fx.la
    for s in range(LI.S):
        with oracle_in_float64():
            want = fx.offline_part(orac64(name), s, 0, LI.T, torch.float64)
        _check(_stream(ref, fx, s, 0, LI.T, CHUNKINGS[chunking](LI.T), end_alone=bool(s % 2)), want)


@pytest.mark.parametrize("end_alone", [False, True])
@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
def test_three_utterances_back_to_back_on_one_stream(chunking, end_alone, orac64):
    """Small configuration, one LookaheadRef: utterances of 40 frames, 5 (shorter than the look-ahead of 12) and 1."""
    fx = LI.fixture(**LI.SMALL)
    ref = LookaheadRef(fx.orac)
    for s, (lo, n) in enumerate(((0, 40), (50, 5), (70, 1))):
        with oracle_in_float64():
            want = fx.offline_part(orac64("small"), s, lo, lo + n, torch.float64)
        _check(_stream(ref, fx, s, lo, lo + n, CHUNKINGS[chunking](n), end_alone), want)


@pytest.mark.parametrize("name", sorted(CONFS))
def test_frames_more_than_the_lookahead_before_a_change_do_not_change(name):
    """The oracle alone: with frames >= F and their conditioning replaced, frames < F - LA of decoded, encoded and qidx are
    the same, bit for bit (one-sided: LA is an upper bound, a quantizer swallows differences that flip no code - the first
    frame that does change is printed)."""
    fx = LI.fixture(**CONFS[name])
    F, s = 100, 0
    g = torch.Generator().manual_seed(5)
    x, lcf0, uv = fx.x[s].clone(), fx.lcf0[s].clone(), fx.uv[s].clone()
    x[F:] = torch.randn(LI.T - F, x.shape[1], generator=g)
    lcf0[F:] = torch.randn(LI.T - F, 1, generator=g)
    uv[F:] = 1.0 - uv[F:]
    a = fx.offline_part(fx.orac, s, 0, LI.T)
    b = fx.offline_part(fx.orac, s, 0, LI.T, x=x, lcf0=lcf0, uv=uv)
    keep = F - fx.la
    assert keep > 0
    assert torch.equal(a["decoded"][0, :keep], b["decoded"][0, :keep])
    assert not torch.equal(a["decoded"][0, F:], b["decoded"][0, F:])
    for n in range(fx.nst):
        assert torch.equal(a["qidx"][n][0, :keep], b["qidx"][n][0, :keep])
        assert torch.equal(a["encoded"][n][0, :keep], b["encoded"][n][0, :keep])
    changed = np.nonzero((a["decoded"][0] != b["decoded"][0]).any(-1).numpy())[0]
    print(f"{name}: look-ahead {fx.la}, frames >= {F} replaced, first changed frame {int(changed[0])}")


@pytest.mark.parametrize("name", ["default", "small"] + sorted(LI.VARIANTS))
def test_fixture_margins_leave_out_nothing(name):
    """The non-causal fixtures with the draw of tests/stream_inputs.py: the share of frames whose best two codes lie within
    MARGIN of each other, with everything within the look-ahead on either side, is 0.0 - under the cap of 2 %."""
    fx = LI.fixture(**(LI.SMALL if name == "small" else LI.VARIANTS.get(name, {})))
    print(f"{name}: left out {fx.left_out:.4f} of the compared frames, look-ahead {fx.la}")
    assert not fx.conf["causal"]
    assert fx.left_out <= LI.MAX_LEFT_OUT
    assert fx.left_out == 0.0
    for n in range(fx.nst):
        assert len(np.unique(fx.ref["qidx"][n].numpy())) >= 8


def test_lookahead_frames():
    from crank_amd.stream import lookahead_frames, receptive_chain

    conf = load_yaml(None)
    assert not conf["causal"]  # the recipe's default
    assert lookahead_frames(conf) == 66 == receptive_chain(conf) // 2
    assert lookahead_frames(load_yaml(None, **LI.SMALL)) == 12


def test_lookahead_symbols_are_declared_bound_and_exported():
    from crank_amd import _lib, stream

    names = ["crk_lstream_create", "crk_lstream_destroy", "crk_lstream_lookahead", "crk_lstream_reserve",
             "crk_lstream_state_bytes", "crk_lstream_prepare", "crk_lstream_reset", "crk_lstream_push"]
    lib_path = os.path.join(REPO, "crank_amd", "libcrank_hip.so")
    assert os.path.exists(lib_path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(lib_path)
    assert not [s for s in names if not hasattr(lib, s)]
    assert not [s for s in names if s not in _lib.SIGNATURES]
    header = open(os.path.join(REPO, "include", "crank_hip.h")).read()
    assert all(f"{s}(" in header for s in names)
    for sym in ("LookaheadConverter", "check_lookahead_conf", "lookahead_frames"):
        assert hasattr(stream, sym), sym


def _stub(**over):
    """What the constructor's checks read of a generator (a real one needs the GPU)."""
    return types.SimpleNamespace(conf=load_yaml(None, **over), spkr_size=4)


@pytest.mark.parametrize("over,key", [
    (dict(causal=True), "causal"),
    (dict(use_raw=True), "use_raw"),
    (dict(emb_dim=[48, 64, 64]), r"emb_dim\[0\]"),
    (dict(kernel_size=[7, 3, 3]), r"kernel_size\[0\]"),
    (dict(kernel_size=[4, 3, 3]), r"kernel_size\[0\] = 4.*odd"),
    (dict(input_size=200), "input_size"),
    (dict(n_layers=[8, 2, 2]), r"n_layers\[0\]"),
])
def test_constructor_refuses_by_key_before_touching_the_library(over, key, monkeypatch):
    from crank_amd import _lib, stream

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(NotImplementedError, match=key):
        stream.LookaheadConverter(_stub(**over), 2, 64)
    with pytest.raises(NotImplementedError, match=key):
        stream.check_lookahead_conf(load_yaml(None, **over), 4)


def test_the_causal_converter_still_refuses_and_names_the_new_class():
    from crank_amd import stream

    with pytest.raises(NotImplementedError, match="66 frames after") as err:
        stream.check_stream_conf(load_yaml(None), 4)
    assert "causal" in str(err.value) and "LookaheadConverter" in str(err.value)
    stream.check_lookahead_conf(load_yaml(None), 4)
    stream.check_stream_conf(load_yaml(None, causal=True, kernel_size=[4, 3, 3]), 4)  # (even sizes stay with the causal path)
