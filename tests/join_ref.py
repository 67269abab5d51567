"""The frame join (csrc/join_kernels.hip, crank_amd.live.FrameJoin) as a numpy state machine: per stream a ring per side
with cap + max_in slots, the waiting counts, the heads, ``first`` and the sticky overflow flags - and an assert on every
read of a slot that nobody wrote, on every write into a slot that is read in the same push, and on the counts."""
import numpy as np


class Side:
    def __init__(self, S, width, max_in, cap):
        self.width, self.max_in, self.cap = width, max_in, cap
        self.slots = cap + max_in if cap else 0
        self.ring = np.zeros((S, max(self.slots, 1), width), np.float32)
        self.written = np.zeros((S, max(self.slots, 1)), bool)  # a slot holds a row of the current utterance
        self.wait = np.zeros(S, np.int64)
        self.head = np.zeros(S, np.int64)


class Join:
    def __init__(self, S, width_a, width_b, max_in_a, max_in_b, cap_a, cap_b):
        self.S = S
        self.A, self.B = Side(S, width_a, max_in_a, cap_a), Side(S, width_b, max_in_b, cap_b)
        self.first = np.zeros(S, np.int64)
        self.overflow = np.zeros(S, np.int64)
        self.max_frames = min(cap_a + max_in_a, cap_b + max_in_b)

    def reset(self, streams=None):
        for s in range(self.S) if streams is None else streams:
            for sd in (self.A, self.B):
                sd.wait[s] = sd.head[s] = 0
                sd.written[s] = False
            self.first[s] = self.overflow[s] = 0

    def _side(self, sd, s, rows, n, take, end, out):
        """Emits this side's rows of the push's pairs into out[:take]; returns the rows lost."""
        w0, head = int(sd.wait[s]), int(sd.head[s])
        assert 0 <= w0 <= sd.cap
        read = set()
        for j in range(take):
            if j < w0:
                slot = (head + j) % sd.slots
                assert sd.written[s, slot], "a read of a slot nobody wrote"
                read.add(slot)
                out[j] = sd.ring[s, slot]
            else:
                assert j - w0 < n
                out[j] = rows[j - w0]
        skip = max(take - w0, 0)
        old_left = max(w0 - take, 0)
        surplus = n - skip
        keep = 0 if end else min(surplus, sd.cap - old_left)
        lost = 0 if end else surplus - keep
        kept_slots = {(head + i) % sd.slots for i in range(take, w0)}
        assert len(kept_slots) == old_left
        for r in range(keep):
            slot = (head + w0 + skip + r) % sd.slots
            assert slot not in read, "a slot read and written in one push"
            assert slot not in kept_slots, "a waiting row overwritten"
            kept_slots.add(slot)
            sd.ring[s, slot] = rows[skip + r]
            sd.written[s, slot] = True
        if end:
            sd.wait[s] = sd.head[s] = 0
            sd.written[s] = False
        else:
            sd.wait[s] = old_left + keep
            sd.head[s] = (head + take) % sd.slots if sd.slots else 0
            assert sd.wait[s] <= sd.cap
        return lost

    def push(self, a, n_a, b, n_b, end, out_a, out_b):
        """a (S, max_in_a, width_a), b likewise, n_a / n_b / end (S,) integers; out_a / out_b (S, >= max_frames, width) are
        written below the returned counts only.  Returns n_frames, first, n_dropped (S,) int32."""
        S = self.S
        n_frames, first, dropped = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            na = min(max(int(n_a[s]), 0), self.A.max_in)
            nb = min(max(int(n_b[s]), 0), self.B.max_in)
            e = bool(end[s]) if end is not None else False
            ta, tb = int(self.A.wait[s]) + na, int(self.B.wait[s]) + nb
            take = min(ta, tb)
            assert take <= self.max_frames
            la = self._side(self.A, s, a[s], na, take, e, out_a[s])
            lb = self._side(self.B, s, b[s], nb, take, e, out_b[s])
            n_frames[s], first[s] = take, self.first[s]
            if e:
                dropped[s] = (ta - take) + (tb - take)
                self.first[s] = 0
            else:
                self.first[s] += take
                self.overflow[s] |= (1 if la else 0) | (2 if lb else 0)
        return n_frames, first, dropped


class Lists:
    """The obvious definition: two Python lists per stream."""

    def __init__(self, S, cap_a, cap_b):
        self.qa, self.qb = [[] for _ in range(S)], [[] for _ in range(S)]
        self.cap_a, self.cap_b = cap_a, cap_b
        self.first, self.overflow = [0] * S, [0] * S

    def push(self, s, rows_a, rows_b, end):
        self.qa[s] += list(rows_a)
        self.qb[s] += list(rows_b)
        take = min(len(self.qa[s]), len(self.qb[s]))
        pairs = list(zip(self.qa[s][:take], self.qb[s][:take]))
        self.qa[s], self.qb[s] = self.qa[s][take:], self.qb[s][take:]
        first, dropped = self.first[s], 0
        if end:
            dropped = len(self.qa[s]) + len(self.qb[s])
            self.qa[s], self.qb[s], self.first[s] = [], [], 0
        else:
            self.first[s] += take
            if len(self.qa[s]) > self.cap_a:
                self.qa[s], self.overflow[s] = self.qa[s][:self.cap_a], self.overflow[s] | 1
            if len(self.qb[s]) > self.cap_b:
                self.qb[s], self.overflow[s] = self.qb[s][:self.cap_b], self.overflow[s] | 2
        return pairs, first, dropped


def schedule(seed, S, max_in_a, max_in_b, n_push, lead="a", p_end=0.08, p_zero=0.15, burst=0.0):
    """Per push (n_a, n_b, end), each (S,): side `lead` tends to run ahead, pushes with n = 0 on either or both sides, end
    flags with and without a surplus, streams on different schedules; `burst`: the chance of a full-width push of the
    leading side alone (what overflows a ring)."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n_push):
        n_a, n_b = rs.randint(0, max_in_a + 1, S), rs.randint(0, max_in_b + 1, S)
        hold = rs.rand(S) < 0.5
        if lead == "a":
            n_b = np.where(hold, 0, n_b)
        elif lead == "b":
            n_a = np.where(hold, 0, n_a)
        z = rs.rand(S) < p_zero
        n_a, n_b = np.where(z, 0, n_a), np.where(z, 0, n_b)
        b = rs.rand(S) < burst
        if lead == "b":
            n_b, n_a = np.where(b, max_in_b, n_b), np.where(b, 0, n_a)
        else:
            n_a, n_b = np.where(b, max_in_a, n_a), np.where(b, 0, n_b)
        out.append((n_a.astype(np.int32), n_b.astype(np.int32), (rs.rand(S) < p_end).astype(np.int32)))
    return out


def rows_for(seed, S, max_in, width):
    """(S, max_in, width) float32 rows that are all different."""
    return np.random.RandomState(seed).standard_normal((S, max_in, width)).astype(np.float32)
