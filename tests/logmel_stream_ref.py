"""Float64 restatement of the streaming log-mel front end's state machine (crank_amd/csrc/logmel_stream_kernels.hip) and
the sample-count schedules of its tests.  Host only: numpy and tests/logmel_cases.py; nothing here imports crank_amd.

Per stream the machine keeps what the kernel keeps - a ring of the last n_fft samples addressed by absolute sample index
(pos & (n_fft - 1)), the samples received and the frames emitted - and reads by the kernel's rule: positions below the
old count from the ring, positions at or above it from the push's own input.  Every read is asserted to lie in the
ring's last n_fft positions or inside the push.  It gathers the SAMPLES of each frame (before the window); the energies
follow from them as tests/logmel_cases.mel_energies computes them."""
import numpy as np

from tests import logmel_cases as C


def frames_ready(n_total, n_fft, hop, center, end=False):
    """Frames of an utterance that exist once n_total samples have arrived (section 1 of the feature's contract)."""
    h = n_fft // 2
    if center:
        if n_total <= h:
            return 0
        return 1 + n_total // hop if end else (n_total - h) // hop + 1
    return 0 if n_total < n_fft else (n_total - n_fft) // hop + 1


def max_frames(n_fft, hop, center, max_samples):
    """The largest count one push of at most max_samples samples can emit over all histories, the end flush included."""
    if center:
        return 1 + (n_fft // 2 + max_samples) // hop
    return (max_samples + hop - 1) // hop


def max_frames_brute(n_fft, hop, center, max_samples):
    """The same by trying every history up to two hops past the point where the counts become periodic in hop."""
    best = 0
    for n0 in range(0, 2 * n_fft + 3 * hop + 2):
        f0 = frames_ready(n0, n_fft, hop, center)
        for c in range(0, max_samples + 1):
            for end in (False, True):
                best = max(best, frames_ready(n0 + c, n_fft, hop, center, end) - f0)
    return best


class Machine:
    """One stream."""

    def __init__(self, n_fft, hop, center):
        assert n_fft & (n_fft - 1) == 0
        self.n_fft, self.hop, self.center = n_fft, hop, bool(center)
        self.ring = np.zeros(n_fft)
        self.n = self.f = 0
        self.reads_ring = self.reads_push = 0

    def push(self, x, end=False):
        """x: the push's new samples (float32 or float64, any count including 0).  Returns (k, n_fft) float64: the samples
        of the frames that became computable."""
        x = np.asarray(x, np.float64)
        n_fft, hop, h = self.n_fft, self.hop, self.n_fft // 2
        n0, f0 = self.n, self.f
        n1 = n0 + len(x)
        f1 = frames_ready(n1, n_fft, hop, self.center, end)
        assert f1 >= f0 == frames_ready(n0, n_fft, hop, self.center)
        frames = np.empty((f1 - f0, n_fft))
        for i, t in enumerate(range(f0, f1)):
            pos = t * hop + np.arange(n_fft)
            if self.center:
                pos = pos - h
                pos = np.where(pos < 0, -pos, pos)
                pos = np.where(pos >= n1, 2 * (n1 - 1) - pos, pos)
            old = pos < n0
            # the ring bound: what is read below the old count is among the last n_fft samples received before this push
            assert (pos[old] >= max(0, n0 - n_fft)).all(), (t, n0, int(pos[old].min()))
            assert (pos[~old] - n0 < len(x)).all() and (pos >= 0).all(), (t, n0, n1)
            frames[i, old] = self.ring[pos[old] & (n_fft - 1)]
            frames[i, ~old] = x[pos[~old] - n0]
            self.reads_ring += int(old.sum())
            self.reads_push += int((~old).sum())
        keep = min(len(x), n_fft)
        at = n0 + np.arange(len(x) - keep, len(x))
        self.ring[at & (n_fft - 1)] = x[len(x) - keep:]
        self.n, self.f = (0, 0) if end else (n1, f1)
        return frames

    def run(self, x, counts):
        """The whole of x in pushes of `counts` samples, the end flag on the last.  Returns (frames, frames per push)."""
        assert sum(counts) == len(x)
        got, per, at = [], [], 0
        for i, c in enumerate(counts):
            got.append(self.push(x[at:at + c], end=i + 1 == len(counts)))
            per.append(len(got[-1]))
            at += c
        return np.concatenate(got), per


def whole_frames(case, row):
    """(T, n_fft) float64: the samples of every frame as tests/logmel_cases.mel_energies gathers them from the whole signal."""
    n_fft, hop = case["n_fft"], case["hop"]
    T = C.n_frames(case, len(row))
    r = np.asarray(row).astype(np.float64)
    if case["center"]:
        r = np.pad(r, n_fft // 2, mode="reflect")
    return r[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]]


def energies_of(case, frames):
    """float64 (T, n_mels) mel energies of gathered frames, by the expression of mel_energies."""
    return np.abs(np.fft.rfft(frames * C.window64(case), axis=-1)) @ C.basis_of(case).astype(np.float64)


# -------------------------------------------------------------------------------------------------------- schedules
def cut(n, sizes):
    """`sizes` cycled until n samples are taken (the last push clipped); zeros are kept."""
    out, done, i = [], 0, 0
    while done < n:
        c = min(sizes[i % len(sizes)], n - done)
        out.append(c)
        done += c
        i += 1
    return out


def mixed_sizes(n_fft, hop):
    """Contains 0 and a push larger than 2 n_fft; the rest straddles hop and n_fft / 2."""
    return [5, 0, 2 * n_fft + 11, 1, 0, hop, n_fft // 2 + 3, 333]


def schedules(n, n_fft, hop, ones=False):
    """name -> sample counts per push, each summing to n."""
    out = {"hop": cut(n, [hop]), "hop+1": cut(n, [hop + 1]), "c37": cut(n, [37]), "n_fft": cut(n, [n_fft]),
           "mixed": cut(n, mixed_sizes(n_fft, hop)), "whole": [n]}
    if hop > 1:
        out["hop-1"] = cut(n, [hop - 1])
    if ones:
        out["c1"] = [1] * n
    return out


UNCENTRED = ["fs22050_hop128", "hop1024", "hop1500", "win2", "r512_win400", "r2048_hop300_win1200"]
CENTRED = ["centred_513", "centred_600", "centred_1500", "centred_9999", "centred_B4", "scaler_centred", "r512_centred_B3",
           "fixture_centred_9999"]
SILENCE = ["silence", "scaler_silence", "broad_clamp"]
BASIS = ["mel256", "basis_run64_65", "basis_empty", "basis_fill40"]
NAMES = UNCENTRED + CENTRED + SILENCE + BASIS
ONES = ("centred_600", "T1")  # the cases short enough for one sample per push
