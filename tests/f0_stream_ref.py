"""Restatement of the streaming F0 front end (crank_amd/csrc/f0_stream_kernels.hip): the block grid in sets, the
definition computed by slicing the whole signal, and the state machine - a ring of raw samples with an assert on every
read, and two counts - that the kernels implement.  Host only: numpy; nothing here imports crank_amd.

The 1 ms estimator is a callable ``est(window float64) -> contour of int(1000 len / fs) + 1 frames``: Harvest
(tests/harvest_ref.harvest at a frame period of 1 ms) in the one real case, a cheap stand-in everywhere else.

All grid arithmetic is in whole milliseconds and integers.  Block j = the 1 ms frames [j block, (j + 1) block), ready once
the stream holds ((j + 1) block + ahead) ms; its window = the (low-cut) signal over [max(j block - back, 0) ms,
((j + 1) block + ahead) ms), truncated at the stream's start and, at the end, at the last sample."""
import numpy as np

MIN_SAMPLES = 64  # Harvest's shortest signal


class Grid:
    def __init__(self, fs, shiftms=None, hop=None, back=300, ahead=100, block=80, min_samples=MIN_SAMPLES):
        assert (shiftms is None) != (hop is None)
        for ms in (back, ahead, block):
            assert ms >= 1 and (ms * fs) % 1000 == 0, "every grid boundary falls on a whole sample"
        assert hop is None or 1000 * hop >= fs
        self.fs, self.shiftms, self.hop, self.back, self.ahead, self.block = fs, shiftms, hop, back, ahead, block
        self.Bs, self.As, self.Ks = block * fs // 1000, ahead * fs // 1000, back * fs // 1000
        self.min_samples = min_samples
        assert min(self.Bs, self.Ks) >= min_samples, "every window holds the estimator's minimum"

    def idx(self, t):
        """The 1 ms frame of output frame t."""
        t = np.asarray(t, np.int64)
        return t * self.shiftms if self.hop is None else (2000 * t * self.hop + self.fs) // (2 * self.fs)

    def frames(self, n):
        """The offline frame count of n samples."""
        return (1000 * n) // (self.fs * self.shiftms) + 1 if self.hop is None else 1 + n // self.hop

    def frames_1ms(self, n):
        return (1000 * n) // self.fs + 1

    def blocks(self, n, end=False):
        """Blocks that exist once n samples have arrived."""
        if end:
            return 0 if n < self.min_samples else (self.frames_1ms(n) - 1) // self.block + 1
        return sum(1 for j in range(n // self.Bs + 1) if (j + 1) * self.Bs + self.As <= n)

    def window(self, j, n, end):
        """Block j's window once n samples have arrived: (first 1 ms frame, first sample, one past the last sample)."""
        a_ms = max(j * self.block - self.back, 0)
        hi = ((j + 1) * self.block + self.ahead) * self.fs // 1000
        if end:
            hi = min(hi, n)
        assert hi <= n
        return a_ms, a_ms * self.fs // 1000, hi

    def _frames_in(self, lo_ms, hi_ms, n, end):
        """Output frames whose 1 ms frame lies in [lo_ms, hi_ms): at the end those below the offline count, their index
        clamped to the last 1 ms frame, as harvest_ref.subsample clamps it."""
        if end:
            t = np.arange(self.frames(n))
            i = np.minimum(self.idx(t), self.frames_1ms(n) - 1)
        else:
            t = np.arange(self.frames(hi_ms * self.fs // 1000 + self.fs) + 2)  # past every frame below hi_ms
            i = self.idx(t)
            assert i[-1] >= hi_ms
        return t[(i >= lo_ms) & (i < hi_ms)]

    def held(self, a_ms, T1, n, end):
        """Output frames a window of T1 1 ms frames from a_ms holds."""
        return self._frames_in(a_ms, a_ms + T1, n, end)

    def emitted(self, j, n, end):
        """Output frames block j emits."""
        return self._frames_in(j * self.block, (j + 1) * self.block, n, end)


def low_cut(taps, sample, pos):
    """The causal FIR at the positions ``pos`` of a signal read through ``sample(positions)``: the taps in order, zero
    history below position 0."""
    pos = np.asarray(pos, np.int64)
    acc = np.zeros(len(pos))
    for k, h in enumerate(taps):
        ok = pos - k >= 0
        if not ok.any():
            break
        v = np.zeros(len(pos))
        v[ok] = sample(pos[ok] - k)
        acc = acc + h * v
    return acc


def finish(g, emit, carry):
    """From a window's contour g at the output frames it holds to (raw, uv, cf0) at its block's frames ``emit`` (indices
    into g), and the new carry.  convert_continuos_f0 with its end-fill quirk (tests/harvest_ref.continuous_f0), or
    uv = 0 and cf0 = the carry where g has no voiced frame."""
    from tests.harvest_ref import continuous_f0

    g = np.asarray(g, np.float64)
    if (g != 0).any():
        uv, cf0 = continuous_f0(g)[:2]
        uv = uv.astype(np.float64)
    else:
        uv, cf0 = np.zeros(len(g)), np.full(len(g), float(carry))
    if len(emit):
        carry = cf0[emit[-1]]
    return g[emit], uv[emit], cf0[emit], carry


def block_outputs(grid, est, window, j, n, end, carry):
    """One block from its window's samples: the estimator, the frames held, the finish."""
    a_ms, a, hi = grid.window(j, n, end)
    f1 = np.asarray(est(window), np.float64)
    T1 = (1000 * (hi - a)) // grid.fs + 1
    assert len(f1) == T1 and len(window) == hi - a >= grid.min_samples
    # a window the end did not truncate holds what it would have held had the stream gone on: the cut cannot matter
    truncated = end and ((j + 1) * grid.block + grid.ahead) * grid.fs // 1000 > n
    held, emit = grid.held(a_ms, T1, n, truncated), grid.emitted(j, n, end)
    assert len(emit) == 0 or (emit[0] >= held[0] and emit[-1] <= held[-1])
    local = np.minimum(grid.idx(held) - a_ms, T1 - 1)
    return finish(f1[local], emit - held[0] if len(emit) else emit, carry)


def define(x, grid, est, taps=None, carry0=100.0):
    """The definition: every block of the whole signal x (ended at len(x)) by slicing.  Returns (raw, uv, cf0), each
    the offline frame count long (empty below the minimum length)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    y = x if taps is None else low_cut(taps, lambda p: x[p], np.arange(n))
    outs, carry = [], carry0
    for j in range(grid.blocks(n, True)):
        a_ms, a, hi = grid.window(j, n, True)
        r = block_outputs(grid, est, y[a:hi], j, n, True, carry)
        outs.append(r[:3])
        carry = r[3]
    cat = [np.concatenate([o[i] for o in outs]) if outs else np.zeros(0) for i in range(3)]
    assert len(cat[0]) == (grid.frames(n) if n >= grid.min_samples else 0), (len(cat[0]), grid.frames(n))
    return cat


class Machine:
    """One stream as the kernels keep it: a power-of-two ring of raw samples addressed by absolute position, the samples
    received and the blocks emitted.  Reads below the old count come from the ring, the rest from the push."""

    def __init__(self, grid, est, max_samples, taps=None, carry0=100.0):
        self.grid, self.est, self.taps, self.carry0 = grid, est, taps, carry0
        self.reach = 0 if taps is None else len(taps) - 1
        need = grid.Ks + grid.Bs + grid.As + self.reach + max_samples
        self.ring_n = 1 << int(np.ceil(np.log2(need)))
        self.max_samples = max_samples
        self.ring = np.zeros(self.ring_n)
        self.n = self.b = 0
        self.carry = carry0
        self.reads_ring = self.reads_push = 0

    def _sample(self, x, n0):
        def get(pos):
            old = pos < n0
            # the ring bound: what is read below the old count is among the last ring_n samples received
            assert (pos >= 0).all() and (pos[old] >= n0 - self.ring_n).all() and (pos[~old] - n0 < len(x)).all()
            # and needs no more than the window's span and the filter's reach
            assert (pos[old] > n0 - (self.grid.Ks + self.grid.Bs + self.grid.As + self.reach)).all()
            out = np.empty(len(pos))
            out[old] = self.ring[pos[old] & (self.ring_n - 1)]
            out[~old] = x[pos[~old] - n0]
            self.reads_ring += int(old.sum())
            self.reads_push += int((~old).sum())
            return out
        return get

    def push(self, x, end=False):
        """x: the push's samples (any count up to max_samples, 0 included).  Returns (raw, uv, cf0) of the frames
        emitted."""
        x = np.asarray(x, np.float64)
        assert len(x) <= self.max_samples
        g, n0, b0 = self.grid, self.n, self.b
        n1 = n0 + len(x)
        b1 = max(b0, g.blocks(n1, end))
        get = self._sample(x, n0)
        outs = []
        for j in range(b0, b1):  # one round each
            a_ms, a, hi = g.window(j, n1, end)
            pos = np.arange(a, hi)
            w = get(pos) if self.taps is None else low_cut(self.taps, get, pos)
            r = block_outputs(g, self.est, w, j, n1, end, self.carry)
            outs.append(r[:3])
            self.carry = r[3]
        keep = min(len(x), self.ring_n)
        at = n0 + np.arange(len(x) - keep, len(x))
        self.ring[at & (self.ring_n - 1)] = x[len(x) - keep:]
        self.n, self.b = (0, 0) if end else (n1, b1)
        if end:
            self.carry = self.carry0
        return [np.concatenate([o[i] for o in outs]) if outs else np.zeros(0) for i in range(3)]

    def run(self, x, counts):
        """The whole of x in pushes of ``counts`` samples, the end flag on the last: (raw, uv, cf0), frames per push."""
        assert sum(counts) == len(x)
        got, per, at = [], [], 0
        for i, c in enumerate(counts):
            got.append(self.push(x[at:at + c], end=i + 1 == len(counts)))
            per.append(len(got[-1][0]))
            at += c
        return [np.concatenate([o[i] for o in got]) for i in range(3)], per


def max_frames(grid, max_samples):
    """The most frames one push of at most max_samples emits over all histories, the end flush included (the closed form
    of fs_max_frames)."""
    K = grid.As + grid.Bs - 1 + max_samples
    if grid.hop is None:
        return (1000 * K) // (grid.fs * grid.shiftms) + 1
    d = int(np.gcd(grid.Bs, grid.hop))
    return 1 + (K + (grid.fs // 2000) // d * d) // grid.hop


def first_frame(grid, m):
    """The first output frame at or after 1 ms frame m."""
    t = 0
    while grid.idx(t) < m:
        t += 1
    return t


def max_frames_brute(grid, max_samples, n0_max):
    """The same by trying every history below n0_max, every push size and both end flags."""
    best = 0
    for n0 in range(n0_max):
        f0 = first_frame(grid, grid.blocks(n0) * grid.block)
        for c in range(max_samples + 1):
            n1 = n0 + c
            best = max(best, first_frame(grid, grid.blocks(n1) * grid.block) - f0)
            if n1 >= grid.min_samples:
                best = max(best, grid.frames(n1) - min(f0, grid.frames(n1)))
    return best


def cut(n, sizes):
    """``sizes`` cycled until n samples are taken (the last push clipped); zeros are kept."""
    out, done, i = [], 0, 0
    while done < n:
        c = min(sizes[i % len(sizes)], n - done)
        out.append(c)
        done += c
        i += 1
    return out or [0]
