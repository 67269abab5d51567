"""Test-side definition of streaming WORLD synthesis (crank_amd.world.StreamingWorldSynthesizer, csrc/
world_stream_kernels.hip), in sets, on top of tests/world_synth_ref.py, whose arithmetic it calls
value for value: under every cut of an utterance's rows into pushes the samples that leave, joined, are
``world_synth_ref.synthesis`` of the whole utterance (tests/test_wsyn_stream_cpu.py asserts it with array_equal).

Row k of an utterance is frame k: an F0 value, an mcep row, a codeap row, an rmcep row with power modification.  A
stream keeps
  * the rows still open to the time base or to a pulse (``row_lo`` .. R - 1);
  * the time front: n samples have their phase; the running total, the last wrapped phase and vuv;
  * the utterance's first pulse (the origin of the noise offsets) and the pending pulse - found, not yet added;
  * the sums of the samples a pulse can still reach (the ring), emitted samples gone.
``push(rows, end)``:
  1. commit: sanitise (an F0 not finite, negative or above f0_ceil is 0, flag 16) and append the rows the queue has room
     for (flag 2, the newest dropped and counted); their sp / ap rows;
  2. front: with R rows so far the time base runs over every sample i whose frame (the last j with j fp <= i / fs) is at
     most R - 2; at an end T = R and it runs to y_length(T) with the clamp to T - 1 and the extrapolated knot;
  3. pulses: a pulse at i is found when sample i + 1 has its wrapped phase; it is added when its successor is found
     (noise size = the distance), at an end the last one with noise size 0;
  4. out: sample i leaves once i + 511 < B, B the pending pulse if there is one, else n - 1; at an end every sample below
     y_length(T) leaves and the stream returns to its start state.
An end push with one row drops it (flag 8); an end push on an empty stream is a no-op.  The capacities (``caps``: rows,
ring, pulses, out) only set flags here (1 ring, 32 pulses, 64 out; the row queue also drops): the restatement itself
keeps everything.  ``fftl`` other than 1024 is the toy of the capacity tests (``responses=False``: positions and counts
only)."""
import copy
import math

import numpy as np

from tests import world_synth_ref as R

FLAG_RING, FLAG_QUEUE, FLAG_NOISE, FLAG_SHORT, FLAG_F0, FLAG_PULSES, FLAG_OUT = 1, 2, 4, 8, 16, 32, 64


class Stream:
    def __init__(self, fs, shiftms, alpha=0.42, power_mod=False, f0_ceil=1000.0, caps=None, fftl=R.FFTL,
                 max_utt_samples=None, responses=True, memo=None):
        self.fs, self.shiftms, self.alpha, self.power_mod = int(fs), float(shiftms), float(alpha), bool(power_mod)
        self.f0_ceil, self.caps, self.N = float(f0_ceil), caps, int(fftl)
        self.lo, self.hi = self.N // 2 - 1, self.N // 2  # a pulse at s covers s - lo .. s + hi
        self.max_utt_samples = max_utt_samples
        self.responses = responses
        self.memo = {} if memo is None else memo  # frame tables and responses by their inputs (the cuts of one utterance)
        self.fp = self.shiftms / 1000.0
        self.flags = 0
        self.added = []  # (pos, ns, shift, vuv, noise offset) of every pulse added, all utterances
        self._start()

    def _start(self):
        self.f0, self.sp, self.ap = [], [], []
        self.row_lo = 0
        self.n = self.emitted = 0
        self.j = 0
        self.total, self.wprev, self.vprev = 0.0, 0.0, 0.0
        self.pend = None
        self.pos0 = None
        self.acc = np.zeros(0)

    def reset(self):
        self.flags = 0
        self._start()

    def clone(self):
        """An independent copy of the stream as it stands (``added`` starts empty)."""
        c = copy.copy(self)
        c.f0, c.sp, c.ap, c.added, c.acc = list(self.f0), list(self.sp), list(self.ap), [], self.acc.copy()
        return c

    # ---- rows
    def _tables(self, mc, cap, rmc):
        key = ("row", mc.tobytes(), cap.tobytes(), None if rmc is None else rmc.tobytes())
        if key not in self.memo:
            sp, ap = R.frame_tables(mc[None], cap[None], None if rmc is None else rmc[None], self.fs, R.FFTL, self.alpha)
            self.memo[key] = (sp[0], ap[0])
        return self.memo[key]

    def _response(self, pos, ns, shift, vuv, off, T):
        q = pos / self.fs / self.fp
        lo, hi = min(T - 1, int(math.floor(q))), min(T - 1, int(math.ceil(q)))
        assert self.row_lo <= lo <= hi < T
        key = ("pulse", pos, ns, shift, vuv, off, lo, hi)
        if key not in self.memo:
            asafe = [np.clip(self.ap[k], 0.001, 0.999999999999) for k in (lo, hi)]
            if lo == hi:
                env, ratio = np.abs(self.sp[lo]), asafe[0] ** 2
            else:
                a = q - lo
                env = (1.0 - a) * np.abs(self.sp[lo]) + a * np.abs(self.sp[hi])
                ratio = ((1.0 - a) * asafe[0] + a * asafe[1]) ** 2
            seg = R.noise(off + min(ns, self.N))[off:]
            self.memo[key] = R.pulse_response(env, ratio, vuv, ns, shift, self.fs, seg)
        return self.memo[key]

    # ---- a push
    def push(self, f0, mcep=None, codeap=None, rmcep=None, end=False):
        """The samples that leave (float64 array); ``self.dropped`` the rows dropped."""
        fs, fp, N = self.fs, self.fp, self.N
        f0 = np.asarray(f0, np.float64).reshape(-1)
        if (rmcep is not None) != self.power_mod and len(f0) and self.responses:
            raise ValueError("rmcep goes with power modification")
        # 1. commit
        keep = len(f0)
        if self.caps is not None:
            keep = max(0, min(keep, self.caps["rows"] - (len(self.f0) - self.row_lo)))
            if keep < len(f0):
                self.flags |= FLAG_QUEUE
        self.dropped = len(f0) - keep
        for r in range(keep):
            v = float(f0[r])
            if not v >= 0.0 or not v <= self.f0_ceil:
                v = 0.0
                self.flags |= FLAG_F0
            self.f0.append(v)
            if self.responses:
                sp, ap = self._tables(np.asarray(mcep[r], np.float64), np.asarray(codeap[r], np.float64),
                                      None if rmcep is None else np.asarray(rmcep[r], np.float64))
                self.sp.append(sp)
                self.ap.append(ap)
        T = len(self.f0)
        if end and T < 2:
            if T:
                self.flags |= FLAG_SHORT
                self.dropped += T
            self._start()
            return np.zeros(0)
        # 2. front, 3. the pulses found
        lowest = fs // N + 1.0
        cf = [0.0 if v < lowest else v for v in self.f0]
        cv = [0.0 if v == 0.0 else 1.0 for v in cf]
        n1 = None
        if end:
            cf.append(cf[T - 1] * 2 - cf[T - 2])
            cv.append(cv[T - 1] * 2 - cv[T - 2])
            n1 = R.y_length(T, fs, self.shiftms)
        two_pi = 2.0 * math.pi
        found = []
        i, j = self.n, self.j
        while n1 is None or i < n1:
            xi = i / fs
            while j + 1 < T and (j + 1) * fp <= xi:
                j += 1
            if not end and j > T - 2:
                break
            s = (xi - j * fp) / ((j + 1) * fp - j * fp)
            v = 1.0 if cv[j] + s * (cv[j + 1] - cv[j]) > 0.5 else 0.0
            f = cf[j] + s * (cf[j + 1] - cf[j]) if v != 0.0 else R.DEFAULT_F0
            self.total = self.total + two_pi * f / fs
            w = math.fmod(self.total, two_pi)
            if i >= 1 and abs(w - self.wprev) > math.pi:
                y1, y2 = self.wprev - two_pi, w
                found.append((i - 1, -y1 / (y2 - y1) / fs, self.vprev))
            self.wprev, self.vprev = w, v
            i += 1
        n0, self.n, self.j = self.n, i, j
        n = self.n
        lst = ([self.pend] if self.pend is not None else []) + found
        n_add = len(lst) if end else max(len(lst) - 1, 0)
        caps = self.caps
        if caps is not None and (len(lst) > caps["pulses"] + 1 or n_add > caps["pulses"]):
            self.flags |= FLAG_PULSES
        if self.pos0 is None and lst:
            self.pos0 = lst[0][0]
        # 4. add, emit
        E0 = self.emitted
        top = n if end else n + self.hi - 1  # one past the last sample a pulse found so far can reach
        if caps is not None and top - E0 > caps["ring"]:
            self.flags |= FLAG_RING
        if self.responses and len(self.acc) < top:
            self.acc = np.concatenate([self.acc, np.zeros(top - len(self.acc) + 4096)])
        for k in range(n_add):
            pos, shift, vuv = lst[k]
            ns = lst[k + 1][0] - pos if k + 1 < len(lst) else 0
            off = pos - self.pos0
            if ns > 0 and self.max_utt_samples is not None and off + min(ns, N) > self.max_utt_samples:
                self.flags |= FLAG_NOISE
            self.added.append((pos, ns, shift, vuv, off))
            if self.responses:
                r = self._response(pos, ns, shift, vuv, off, T)
                o = pos - self.lo
                a0, a1 = max(0, -o), min(N, top - o)
                assert a0 + o >= E0
                self.acc[a0 + o:a1 + o] += r[a0:a1]  # overlap-add, pulse after pulse
        self.pend = None if end or not lst else lst[-1]
        B = self.pend[0] if self.pend is not None else n - 1
        E1 = n if end else max(E0, min(n, B - self.lo))
        if caps is not None and E1 - E0 > caps["out"]:
            self.flags |= FLAG_OUT
        y = self.acc[E0:E1].copy() if self.responses else np.zeros(E1 - E0)
        self.emitted = E1
        self.row_lo = max(0, min(T - 2, int(math.floor(max(B, 0) / fs / fp))))
        self.rows_held = T - self.row_lo
        if end:
            self._start()
        return y


def cuts(T, most):
    """Every way to cut T rows into pushes of 1 .. most rows."""
    if T == 0:
        yield []
        return
    for c in range(1, min(most, T) + 1):
        for rest in cuts(T - c, most):
            yield [c] + rest


def run(stream, f0, mcep, codeap, rmcep, cut, end_alone=False):
    """Pushes one utterance through ``stream`` under ``cut``; (samples, emitted counts per push).  ``end_alone``: the end
    flag comes on a further push that brings no rows."""
    out, counts, k = [], [], 0
    for idx, c in enumerate(cut):
        last = idx == len(cut) - 1 and not end_alone
        sl = slice(k, k + c)
        y = stream.push(f0[sl], None if mcep is None else mcep[sl], None if codeap is None else codeap[sl],
                        None if rmcep is None else rmcep[sl], end=last)
        out.append(y)
        counts.append(len(y))
        k += c
    if end_alone:
        y = stream.push(np.zeros(0), None if mcep is None else mcep[:0], None if codeap is None else codeap[:0],
                        None if rmcep is None else rmcep[:0], end=True)
        out.append(y)
        counts.append(len(y))
    return np.concatenate(out) if out else np.zeros(0), counts
