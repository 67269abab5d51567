"""Test-side restatement, in sets, of streaming CheapTrick / mel-cepstrum analysis (crank_amd/world.py ``StreamingMcep``,
csrc/wana_stream_kernels.hip), on top of tests/world_analysis_ref.py.

The offline analysis touches an utterance, per frame, through four things only: the samples within ``half <= 511`` of the
frame's origin (clamped to the signal), the frame's F0, its index, and its offset into the utterance's randn stream - the
sum of the earlier frames' draw counts ``2 half + 1 + 513``.  A stream carries each of them:

  * y, the signal the analysis sees: the causal 255-tap low cut of the stream with zero history at the utterance's start,
    each sample once, in the push that brings it, as the chain ``acc += h[k] * x[p - k]`` in tap order (the kernels fuse
    each step; numpy rounds the product first - the only arithmetic difference between this file and the device), or
    ``float64(x)`` without a low cut.  Only positions ``>= n - ring_capacity`` can still be read;
  * the F0 rows that have arrived and whose frames have not left (at most ``f0_capacity``); row k of an utterance is
    frame k;
  * the counts n (samples), rows, emitted (frames that left) and the draw offset of the next frame.

``plan_push`` is the whole of the bookkeeping, on integers alone; ``McepStreamRef`` adds the arithmetic of
world_analysis_ref frame by frame.  Frame i leaves in the first push after which its row has arrived and
``n >= origin_i + reach + 1`` (reach = 511, the clamp of ``half``: readiness never depends on the F0), in order; a push
with the end flag lets every waiting frame leave, windows clamped at n, and returns the stream to its start state.

Flags (sticky on the device): 1 a leaving frame's window start ``max(0, origin - half)`` is below ``n - ring_capacity``:
dropped and counted, its draws still consumed; 2 the rows of a push that the queue has no room for: dropped (the newest)
and counted; 4 a frame's draws pass ``max_utt_frames * 1536``: the table index is clamped to its last value, the frame is
emitted; 8 at an end push the rows k with ``k shift > n + shift`` (what ``WorldAnalyzer._batch`` refuses), or any row
when n == 0: dropped and counted; 16 a row that is not finite, negative or above fs / 4: analysed as 0.
"""
import numpy as np

from tests import world_analysis_ref as war

FFTL = war.FFTL
K = FFTL // 2 + 1
REACH = FFTL // 2 - 1
DRAWS_PER_FRAME = 2 * REACH + 1 + K
FLAG_RING, FLAG_QUEUE, FLAG_DRAWS, FLAG_PAST_END, FLAG_F0 = 1, 2, 4, 8, 16


def origin_of(k, fs, shiftms):
    """frame_shapes' origin of frame k."""
    t = k * float(shiftms) / 1000.0
    return war.matlab_round(t * fs + 0.001)


def shape_of(f0, k, fs, shiftms, fftl=FFTL):
    """frame_shapes' row for one frame: (F0 used, origin, half, dc_limit, boundary)."""
    cur = war.DEFAULT_F0 if f0 <= war.f0_floor(fs, fftl) else float(f0)
    width = cur * 2.0 / 3.0
    return (cur, origin_of(k, fs, shiftms), war.matlab_round(1.5 * fs / cur), 2 + int(cur * fftl / fs),
            int(width * fftl / fs) + 1)


def analysis_capacities(fs, shiftms, f0_lag_ms, max_samples, max_f0_in, reach=REACH):
    """The closed form of crank_amd.world.analysis_capacities, restated (the CPU test compares the two and brute-forces
    this one)."""
    shift = float(shiftms) / 1000.0 * fs
    lag = int(np.ceil(float(f0_lag_ms) * fs / 1000.0))
    m = max(lag, reach + 1)
    return m - 1 + max_samples + reach, int(np.floor((max_samples + m - 0.499) / shift)) + 2


def plan_push(n, rows, emitted, c, r, end, fs, shiftms, ring_capacity, f0_capacity, half_of, reach=REACH):
    """The bookkeeping of one push of c samples and r rows on a stream at (n, rows, emitted).  half_of(k): the half window
    of waiting frame k (its row is among the rows kept).  Returns (n, rows, emitted) after the commit - before the reset
    an end push makes -, the kept rows, the frames that leave as (k, dropped), the rows refused at the end, and the flags
    1, 2, 8 raised."""
    shift = float(shiftms) / 1000.0 * fs
    keep = max(0, min(r, f0_capacity - (rows - emitted)))
    flags = FLAG_QUEUE if keep < r else 0
    n, rows = n + c, rows + keep
    leaving = []
    k = emitted
    while k < rows:
        if end:
            ok = n > 0 and not k * shift > n + shift
        else:
            ok = n >= origin_of(k, fs, shiftms) + reach + 1
        if not ok:
            break
        drop = max(0, origin_of(k, fs, shiftms) - half_of(k)) < n - ring_capacity
        if drop:
            flags |= FLAG_RING
        leaving.append((k, drop))
        k += 1
    refused = rows - k if end else 0
    if refused:
        flags |= FLAG_PAST_END
    return (n, rows, k), keep, leaving, refused, flags


def low_cut_chain(taps, tail, x_new, p0):
    """Samples p0 .. p0 + len(x_new) of the causal FIR with zero history before sample 0, each as the chain over the taps
    in order; tail: the min(len(taps) - 1, p0) raw samples before p0."""
    taps = np.asarray(taps, np.float64)
    tail, x_new = np.asarray(tail, np.float64), np.asarray(x_new, np.float64)
    t = len(tail)
    assert t == min(len(taps) - 1, p0)
    buf = np.concatenate([tail, x_new])
    m = len(x_new)
    acc = np.zeros(m)
    for k in range(len(taps)):
        i0 = max(0, k - p0)  # sample p0 + i reaches back to p0 + i - k >= 0
        if i0 >= m:
            break
        acc[i0:] = acc[i0:] + taps[k] * buf[t + i0 - k:t + m - k]
    return acc


def low_cut(x, fs, cutoff=70):
    """The whole signal through low_cut_chain: the reference's low_cut_filter up to the order of its sums."""
    x = np.asarray(x, np.float32)
    return low_cut_chain(war.low_cut_taps(fs, cutoff), np.zeros(0), x, 0)


def frame_features(y, n, f0, k, off, table, fs, shiftms, dim, alpha, fft=None):
    """(sp row, mcep row) of frame k of a signal y[:n] at draw offset off: world_analysis_ref's cheaptrick and sp2mc for
    one frame.  table: the randn table; an index past it reads its last value."""
    cur, origin, half, dc, bound = shape_of(f0, k, fs, shiftms)
    nw = 2 * half + 1
    idx = np.minimum(off + np.arange(nw + K), len(table) - 1)
    nz = table[idx]
    p = war.frame_power(y[:n], cur, origin, half, dc, fs, FFTL, nz[:nw], fft)
    p = war.linear_smoothing(p, cur * 2.0 / 3.0, bound, fs, FFTL)
    p = p + np.abs(nz[nw:]) * war.EPS
    c = war._even_fft(np.log(p), fft)
    sm, cp = war.lifters(cur, fs, FFTL)
    sp = np.exp(war._even_fft(c * sm * cp / FFTL, fft))
    return sp, war.sp2mc(sp[None], dim, alpha, fft=fft)[0]


def feats_of(mcep, first, scaler=None):
    """The rows a generator takes: float64 throughout, one rounding to float32."""
    m = np.asarray(mcep, np.float64)
    if scaler is not None:
        m = (m - np.asarray(scaler[0], np.float64)) / np.asarray(scaler[1], np.float64)
    return m[..., first:].astype(np.float32)


class McepStreamRef:
    """One stream.  ``push(x, f0_rows, end)`` returns the frames that leave: dict of index, offset (draw offsets), sp,
    mcep, feats, n_dropped; ``flags`` is sticky until ``reset``."""

    def __init__(self, fs, shiftms, dim, alpha, low_cut, f0_capacity, ring_capacity, max_utt_frames, use_mcep_0th=False,
                 scaler=None, fft=None):
        self.fs, self.shiftms, self.dim, self.alpha = int(fs), float(shiftms), int(dim), float(alpha)
        self.taps = None if low_cut is None else war.low_cut_taps(self.fs, low_cut)
        self.f0_capacity, self.ring_capacity = int(f0_capacity), int(ring_capacity)
        self.table = war.noise(int(max_utt_frames) * DRAWS_PER_FRAME)
        self.first, self.scaler, self.fft = 0 if use_mcep_0th else 1, scaler, fft
        self.flags = 0
        self.reset()

    def reset(self):
        self.n = self.rows = self.emitted = self.doff = 0
        self.raw = np.zeros(0, np.float32)  # the utterance's raw samples (the filter reads the last 254)
        self.y = np.zeros(0)                # y by absolute position (only the last ring_capacity may be read)
        self.f0 = {}                        # waiting rows by frame index
        self.flags = 0

    def push(self, x, f0_rows, end=False):
        x = np.asarray(x, np.float32).reshape(-1)
        f0_rows = np.asarray(f0_rows, np.float64).reshape(-1)
        half_of = lambda k: shape_of(self.f0[k], k, self.fs, self.shiftms)[2]  # noqa: E731
        # the rows that fit wait under their frame index before the plan looks at them
        keep = max(0, min(len(f0_rows), self.f0_capacity - (self.rows - self.emitted)))
        for j in range(keep):
            v = f0_rows[j]
            if not np.isfinite(v) or v < 0 or v > self.fs / 4.0:
                v = 0.0
                self.flags |= FLAG_F0
            self.f0[self.rows + j] = float(v)
        (n, rows, emitted), kept, leaving, refused, flags = plan_push(
            self.n, self.rows, self.emitted, len(x), len(f0_rows), end, self.fs, self.shiftms, self.ring_capacity,
            self.f0_capacity, half_of)
        assert kept == keep
        self.flags |= flags
        if self.taps is None:
            y_new = x.astype(np.float64)
        else:
            t = min(len(self.taps) - 1, self.n)
            y_new = low_cut_chain(self.taps, self.raw[len(self.raw) - t:], x, self.n)
        self.raw, self.y = np.concatenate([self.raw, x]), np.concatenate([self.y, y_new])
        out = dict(index=[], offset=[], sp=[], mcep=[], n_dropped=(len(f0_rows) - keep) + refused)
        for k, drop in leaving:
            half = half_of(k)
            count = 2 * half + 1 + K
            if self.doff + count > len(self.table):
                self.flags |= FLAG_DRAWS
            if drop:
                out["n_dropped"] += 1
            else:
                assert max(0, origin_of(k, self.fs, self.shiftms) - half) >= n - self.ring_capacity
                sp, mc = frame_features(self.y, n, self.f0[k], k, self.doff, self.table, self.fs, self.shiftms, self.dim,
                                        self.alpha, self.fft)
                out["index"].append(k)
                out["offset"].append(self.doff)
                out["sp"].append(sp)
                out["mcep"].append(mc)
            self.doff += count
            del self.f0[k]
        out["sp"] = np.array(out["sp"]).reshape(-1, K)
        out["mcep"] = np.array(out["mcep"]).reshape(-1, self.dim + 1)
        out["feats"] = feats_of(out["mcep"], self.first, self.scaler)
        self.n, self.rows, self.emitted = n, rows, emitted
        if end:
            flags = self.flags
            self.reset()
            self.flags = flags
        return out


def stream_utterance(ref, x, f0, schedule):
    """Runs one utterance through ``ref`` under ``schedule`` - a list of (samples, rows) per push, the last push carrying
    the end flag and whatever is left - and returns the concatenated outputs."""
    x, f0 = np.asarray(x, np.float32), np.asarray(f0, np.float64)
    outs, a, b = [], 0, 0
    for i, (c, r) in enumerate(schedule):
        last = i + 1 == len(schedule)
        c1, r1 = (len(x), len(f0)) if last else (min(a + c, len(x)), min(b + r, len(f0)))
        outs.append(ref.push(x[a:c1], f0[b:r1], end=last))
        a, b = c1, r1
    return dict(index=sum((o["index"] for o in outs), []), offset=sum((o["offset"] for o in outs), []),
                sp=np.concatenate([o["sp"] for o in outs]), mcep=np.concatenate([o["mcep"] for o in outs]),
                feats=np.concatenate([o["feats"] for o in outs]), n_dropped=sum(o["n_dropped"] for o in outs))
