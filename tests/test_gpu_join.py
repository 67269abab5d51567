"""The device frame join (crank_amd.live.FrameJoin, csrc/join_kernels.hip) against tests/join_ref.py bit for bit - rows,
``n_frames``, ``first``, ``n_dropped``, the overflow flags and a sentinel in every output row at and past ``n_frames`` - and
``crk_feat_renorm`` against the torch expression it replaces."""
import ctypes

import numpy as np
import pytest
import torch

from tests import join_ref as JR

pytestmark = pytest.mark.gpu

SENT = 12345.0


def flags_of(fj):
    from crank_amd import _lib

    flags = (ctypes.c_int * fj.n_streams)()
    _lib.check(_lib.lib().crk_join_status(fj._handle, flags, _lib.stream_ptr()), "crk_join_status")
    return list(flags)


class Pair:
    """A device join and the reference machine, fed the same pushes."""

    def __init__(self, S, wa, wb, ma, mb, ca, cb, pad_a=0, pad_b=0):
        from crank_amd.live import FrameJoin

        self.fj, self.ref = FrameJoin(S, wa, wb, ma, mb, ca, cb), JR.Join(S, wa, wb, ma, mb, ca, cb)
        assert self.fj.max_frames == self.ref.max_frames and self.fj.state_bytes > 0
        self.S, self.shape_a, self.shape_b, self.pad_a, self.pad_b = S, (S, ma, wa), (S, mb, wb), pad_a, pad_b
        self.out = self.fj.empty_outputs(S)

    def _dev(self, rows, pad):
        """The rows on the device, in a buffer whose row stride is the width plus `pad`."""
        S, m, w = rows.shape
        buf = torch.full((S, m, w + pad), float("nan"), device="cuda")
        buf[:, :, :w] = torch.from_numpy(rows).cuda()
        return buf[:, :, :w]

    def push(self, seed, n_a, n_b, end):
        a, b = JR.rows_for(seed, *self.shape_a), JR.rows_for(seed + 1, *self.shape_b)
        for k in ("a", "b"):
            self.out[k].fill_(SENT)
        i32 = lambda v: torch.as_tensor(np.asarray(v, np.int32), device="cuda")  # noqa: E731
        got = self.fj.push(self._dev(a, self.pad_a), i32(n_a), self._dev(b, self.pad_b), i32(n_b),
                           None if end is None else i32(end), out=self.out)
        assert got is self.out
        want_a = np.full(tuple(self.out["a"].shape), np.float32(SENT))
        want_b = np.full(tuple(self.out["b"].shape), np.float32(SENT))
        n, first, dropped = self.ref.push(a, n_a, b, n_b, end, want_a, want_b)
        assert got["n_frames"].tolist() == n.tolist() and got["first"].tolist() == first.tolist()
        assert got["n_dropped"].tolist() == dropped.tolist()
        assert np.array_equal(got["a"].cpu().numpy(), want_a) and np.array_equal(got["b"].cpu().numpy(), want_b)
        return n

    def run(self, seed, n_push, **kw):
        S = self.S
        self.push(seed, [0] * S, [0] * S, [0] * S)  # a push with nothing anywhere
        emitted = 0
        for i, (n_a, n_b, end) in enumerate(JR.schedule(seed, S, self.shape_a[1], self.shape_b[1], n_push, **kw)):
            emitted += int(self.push(1000 * seed + 2 * i, n_a, n_b, end).sum())
        assert flags_of(self.fj) == self.ref.overflow.tolist()
        return emitted


CASES = [  # S, width_a, width_b, max_in_a, max_in_b, cap_a, cap_b, pad_a, pad_b, lead
    (5, 80, 2, 9, 11, 19, 0, 0, 0, "a"),     # the live loop's shape: 16-byte vectors for the mel rows
    (5, 80, 2, 9, 11, 7, 7, 4, 2, "b"),      # lda = 84 (still vectors), ldb = 4
    (1, 80, 2, 3, 3, 1, 1, 3, 0, "a"),       # lda = 83: the scalar path on wide rows
    (5, 3, 5, 4, 4, 7, 7, 4, 2, "a"),        # odd widths and strides
    (5, 3, 5, 4, 4, 0, 7, 0, 0, "b"),
    (1, 1, 1, 2, 3, 7, 1, 0, 0, "a"),
    (5, 1, 1, 5, 5, 1, 0, 1, 1, "a"),
    (5, 1, 1, 5, 5, 0, 0, 0, 0, "b"),
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_join_equals_the_reference_machine_bit_for_bit(case):
    S, wa, wb, ma, mb, ca, cb, pa, pb, lead = case
    p = Pair(S, wa, wb, ma, mb, ca, cb, pa, pb)
    emitted = p.run(11, 70 if S > 1 else 300, lead=lead, burst=0.15, p_end=0.05)
    assert emitted > 10 * max(ca + ma, cb + mb)  # the heads went round their rings several times
    assert any(p.ref.overflow)  # every capacity here is overrun by the bursts


def test_end_with_rows_on_one_side_only_then_a_normal_utterance():
    """An utterance of 64 .. n_fft / 2 samples: F0 rows (B) and no mel frame (A)."""
    p = Pair(2, 80, 2, 13, 12, 19, 0)
    assert p.push(1, [0, 3], [2, 3], [1, 0]).tolist() == [0, 3]
    assert p.out["n_dropped"].tolist() == [2, 0]
    assert p.push(3, [4, 4], [1, 2], [0, 0]).tolist() == [1, 2]
    assert p.out["first"].tolist() == [0, 3]
    assert p.push(5, [0, 0], [5, 5], [1, 1]).tolist() == [3, 2]  # A's waiting rows leave, B's surplus is dropped
    assert p.out["n_dropped"].tolist() == [2, 3] and flags_of(p.fj) == [0, 0]


def test_reset_of_one_stream_leaves_the_others_alone():
    p = Pair(3, 3, 5, 4, 4, 7, 7)
    p.push(1, [4, 4, 4], [0, 0, 2], None)
    p.push(3, [4, 4, 4], [0, 0, 0], None)  # streams 0 and 1 overflow ring A: 8 rows for 7 slots
    assert flags_of(p.fj) == [1, 1, 0]
    p.fj.reset([1])
    p.ref.reset([1])
    assert flags_of(p.fj) == [1, 0, 0]
    assert p.push(5, [1, 1, 1], [4, 4, 4], None).tolist() == [4, 1, 4]
    assert p.out["first"].tolist() == [0, 0, 2]
    with pytest.raises(RuntimeError, match="rows were lost"):
        p.fj.status()
    p.fj.reset()
    p.ref.reset()
    p.fj.status()
    p.run(7, 10)


def test_refused_calls_leave_state_and_outputs_untouched():
    from crank_amd import _lib
    from crank_amd.live import FrameJoin

    p = Pair(2, 80, 2, 4, 4, 7, 7)
    p.push(1, [4, 3], [1, 1], None)
    fj, L = p.fj, _lib.lib()
    a, b = torch.zeros(3, 4, 80, device="cuda"), torch.zeros(3, 4, 2, device="cuda")
    n = torch.full((3,), 4, dtype=torch.int32, device="cuda")
    out = {k: torch.full_like(v, 77) for k, v in FrameJoin(3, 80, 2, 4, 4, 7, 7).empty_outputs(3).items()}

    def raw(a_ptr, S, C_out):
        return L.crk_join_push(fj._handle, a_ptr, 80, n.data_ptr(), b.data_ptr(), 2, n.data_ptr(), None, S,
                               out["a"].data_ptr(), 80, out["b"].data_ptr(), 2, C_out, out["n_frames"].data_ptr(),
                               out["first"].data_ptr(), out["n_dropped"].data_ptr(), _lib.stream_ptr())

    assert raw(None, 2, fj.max_frames) == 1          # a null pointer
    assert raw(a.data_ptr(), 2, fj.max_frames - 1) == 1  # C_out < max_frames
    assert raw(a.data_ptr(), 3, fj.max_frames) == 3  # more rows than streams
    assert raw(a.data_ptr(), 0, fj.max_frames) == 1
    bad = [lambda: fj.push(a[:2].double(), n[:2], b[:2], n[:2], out=p.out),
           lambda: fj.push(a[:2].cpu(), n[:2], b[:2], n[:2], out=p.out),
           lambda: fj.push(a[:2, :3], n[:2], b[:2], n[:2], out=p.out),
           lambda: fj.push(a[:2], n[:2].long(), b[:2], n[:2], out=p.out),
           lambda: fj.push(a[:2], n[:2], b[:2, :, :1], n[:2], out=p.out),
           lambda: fj.push(a[:2], n[:2], b[:2], n[:2], end=torch.zeros(2, dtype=torch.int32), out=p.out),
           lambda: fj.push(a[:2], n[:2], b[:2], n[:2], out=dict(p.out, a=p.out["a"][:, :-1])),
           lambda: fj.reset([2])]
    for k in ("a", "b"):
        p.out[k].fill_(SENT)
    for f in bad:
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out.values())
    assert bool((p.out["a"] == SENT).all()) and bool((p.out["b"] == SENT).all())
    for kw in (dict(n_streams=0), dict(width_a=0), dict(max_in_b=0), dict(cap_a=-1)):
        args = dict(n_streams=2, width_a=80, width_b=2, max_in_a=4, max_in_b=4, cap_a=7, cap_b=7)
        with pytest.raises(ValueError):
            FrameJoin(**dict(args, **kw))
    p.run(9, 12)  # the state is where the reference machine's is


def test_captured_push_follows_the_counts_equals_eager_and_allocates_nothing():
    from crank_amd import _lib
    from crank_amd.live import FrameJoin

    S, wa, wb, ma, mb, ca, cb = 3, 80, 2, 5, 6, 7, 3
    sched = JR.schedule(21, S, ma, mb, 30, lead="a", p_end=0.1)
    eager = Pair(S, wa, wb, ma, mb, ca, cb)
    fj = FrameJoin(S, wa, wb, ma, mb, ca, cb)
    st = dict(a=torch.zeros(S, ma, wa, device="cuda"), b=torch.zeros(S, mb, wb, device="cuda"),
              n_a=torch.zeros(S, dtype=torch.int32, device="cuda"), n_b=torch.zeros(S, dtype=torch.int32, device="cuda"),
              end=torch.zeros(S, dtype=torch.int32, device="cuda"), out=fj.empty_outputs(S))
    fj.push(st["a"], st["n_a"], st["b"], st["n_b"], st["end"], out=st["out"])  # warm: both kernels have launched once
    fj.reset()
    torch.cuda.synchronize()
    allocs0 = _lib.lib().crk_debug_alloc_count()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fj.push(st["a"], st["n_a"], st["b"], st["n_b"], st["end"], out=st["out"])
    fj.reset()
    counts = set()
    for i, (n_a, n_b, end) in enumerate(sched):
        seed = 1000 * 21 + 2 * i
        eager.push(seed, n_a, n_b, end)
        st["a"].copy_(torch.from_numpy(JR.rows_for(seed, S, ma, wa)))
        st["b"].copy_(torch.from_numpy(JR.rows_for(seed + 1, S, mb, wb)))
        for k, v in (("n_a", n_a), ("n_b", n_b), ("end", end)):
            st[k].copy_(torch.from_numpy(v))
        for k in ("a", "b"):
            st["out"][k].fill_(SENT)
        graph.replay()
        for k in ("a", "b", "n_frames", "first", "n_dropped"):
            assert torch.equal(st["out"][k], eager.out[k]), (i, k)
        counts.add(tuple(st["out"]["n_frames"].tolist()))
    torch.cuda.synchronize()
    assert len(counts) > 5  # the counts changed between replays
    assert _lib.lib().crk_debug_alloc_count() == allocs0
    assert flags_of(fj) == flags_of(eager.fj)


@pytest.mark.parametrize("S,C,D", [(1, 1, 1), (3, 13, 80), (2, 40, 7)])
def test_feat_renorm_has_the_bits_of_the_torch_expression(S, C, D):
    from crank_amd.live import feat_renorm

    g = torch.Generator().manual_seed(S * 100 + D)
    x = (torch.randn(S, C, D, generator=g) * 3).cuda()
    scale, vscale = (torch.rand(D, generator=g) * 2 + 0.3).cuda(), (torch.rand(D, generator=g) * 2 + 0.3).cuda()
    mean, vmean = torch.randn(D, generator=g).cuda() * 5, torch.randn(D, generator=g).cuda() * 5
    n = torch.as_tensor([(7 * s + C - 1) % (C + 1) for s in range(S)], dtype=torch.int32, device="cuda")
    n[0] = C
    out = torch.full((S, C, D), SENT, device="cuda")
    feat_renorm(x, scale, mean, vmean, vscale, n, out)
    ref = ((x * scale + mean) - vmean) / vscale
    for s in range(S):
        k = int(n[s])
        assert torch.equal(out[s, :k], ref[s, :k]), s
        assert bool((out[s, k:] == SENT).all())
    with pytest.raises(ValueError):
        feat_renorm(x, scale[:-1] if D > 1 else scale.double(), mean, vmean, vscale, n, out)
    with pytest.raises(ValueError):
        feat_renorm(x, scale, mean, vmean, vscale, n.long(), out)
