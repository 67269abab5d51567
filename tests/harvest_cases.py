"""Inputs of the Harvest tests and what the restatement (tests/harvest_ref.py) alone says about them.

``cases()`` gives ragged batches of waveforms with a search range each: harmonic sums whose F0 is known (constant, glide,
voiced - digital silence - voiced), a WORLD-synthesised vowel (tests/world_synth_ref.synthesis), a ragged batch with two
ranges and an utterance shorter than the longest band-pass filter.  ``contour_tables()`` and ``raw_table()`` are hand-built
tables that put the contour and run-detection rules on their edges.  ``edges_reached()`` asserts on the host that each
does.

RECORDED holds, per case, what

    python -m tests.harvest_cases

printed: the relative F0 error of the restatement on interior voiced frames (``err``), and the spread between its two
evaluation orders (direct / FFT band-pass, direct bins / numpy.fft, float64 / longdouble recurrence): ``s_dec`` relative
to the decimated signal's peak, ``s_raw``, ``s_ref``, ``s_score`` the largest relative differences of cells both orders
fill, and the flip counts.  tests/test_harvest_cpu.py recomputes them.  The GPU tests' bounds are 10 x the recorded
spread plus the floor the issue set.
"""
import functools

import numpy as np

from tests import harvest_ref as H
from tests import world_synth_ref as R

NOISE = 1e-3  # white noise under every voiced stretch: no harmonic bin of a refinement window is empty

# name -> dict(err, s_dec, s_raw, s_ref, s_score)
RECORDED = {
    "const_16k": dict(err=6.482e-04, s_dec=4.890e-16, s_raw=2.238e-12, s_ref=7.527e-16, s_score=8.723e-12),
    "glide_22k": dict(err=1.175e-03, s_dec=5.871e-16, s_raw=1.539e-12, s_ref=7.517e-16, s_score=1.255e-11),
    "const_48k": dict(err=2.466e-04, s_dec=2.513e-15, s_raw=2.088e-12, s_ref=7.202e-16, s_score=1.498e-11),
    "gap_8k": dict(err=3.112e-03, s_dec=0.000e+00, s_raw=1.778e-12, s_ref=6.365e-16, s_score=9.937e-13),
    "wide_8k": dict(err=1.639e-03, s_dec=1.510e-18, s_raw=9.863e-12, s_ref=8.803e-16, s_score=2.222e-11),
    "ragged_16k": dict(err=6.608e-03, s_dec=4.581e-16, s_raw=4.989e-12, s_ref=1.038e-14, s_score=1.885e-11),
    "short_16k": dict(err=0.000e+00, s_dec=3.651e-16, s_raw=8.188e-13, s_ref=5.068e-16, s_score=7.744e-13),
    "vowel_22k": dict(err=1.332e-03, s_dec=2.750e-16, s_raw=7.233e-14, s_ref=8.380e-16, s_score=6.439e-12),
}


def _harmonics(rng, f, fs, noise=NOISE):
    """Eight harmonics of the F0 track f (Hz per sample), random amplitudes and phases, on a noise floor."""
    ph = 2 * np.pi * np.cumsum(f) / fs
    y = sum(rng.uniform(0.05, 0.3) * np.sin(h * ph + rng.uniform(0, 6.28)) for h in range(1, 9))
    return y + noise * rng.standard_normal(len(f))


def _vowel(rng, T, fs, shiftms):
    order = 24
    mc = np.zeros((T, order + 1))
    mc[:, 0] = -3.0
    mc[:, 1:] = rng.standard_normal(order) * 0.5 / np.arange(1, order + 1)
    f0 = 180.0 + 25.0 * np.sin(np.arange(T) / 17.0)
    cap = np.full((T, R.n_bands(fs)), -25.0)
    y = R.synthesis(f0, mc, cap, None, fs, 1024, shiftms, 0.455)
    track = np.interp(np.arange(len(y)) / fs, np.arange(T) * shiftms / 1000.0, f0)
    return y + NOISE * rng.standard_normal(len(y)), track


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(fs, shiftms, utts=[dict(x, minf0, maxf0, track)]); track: the true F0 per sample (0 unvoiced) or None."""
    rng = np.random.default_rng(5150)
    out = {}

    def add(name, fs, shiftms, *utts):
        out[name] = dict(name=name, fs=fs, shiftms=shiftms,
                         utts=[dict(x=np.asarray(x, np.float64), minf0=lo, maxf0=hi, track=tr) for x, lo, hi, tr in utts])

    fs = 16000
    f = np.full(int(0.4 * fs), 151.3)
    add("const_16k", fs, 5, (_harmonics(rng, f, fs), 70, 400, f))
    fs = 22050
    f = np.linspace(120.0, 160.0, int(0.5 * fs))
    add("glide_22k", fs, 5, (_harmonics(rng, f, fs), 70, 400, f))
    fs = 48000
    f = np.full(int(0.35 * fs), 203.7)
    add("const_48k", fs, 10, (_harmonics(rng, f, fs), 70, 400, f))
    # voiced - digital silence - voiced as 16-bit PCM whose samples sum to exactly zero: removing the mean leaves the
    # silence at exactly 0.0, and a band-pass filter that lies inside it gives exact zeros by direct convolution and
    # rounding residue by FFT; the restatement's zero flush (harvest_ref.GATE) makes both the same
    fs = 8000
    f = np.full(int(0.5 * fs), 143.9)
    a, b = int(0.22 * fs), int(0.27 * fs)
    q = np.round(_harmonics(rng, f, fs) * 16384.0)
    q[a:b] = 0.0
    f[a:b] = 0.0
    q[5] -= q.sum()
    assert q.sum() == 0.0 and np.max(np.abs(q)) < 32768
    add("gap_8k", fs, 5, (q / 32768.0, 70, 400, f))
    f = np.linspace(210.0, 250.0, int(0.45 * fs))
    add("wide_8k", fs, 5, (_harmonics(rng, f, fs), 40, 700, f))
    fs = 16000
    f1 = np.linspace(230.0, 200.0, int(0.3 * fs))
    f2 = np.full(int(0.42 * fs) + 7, 96.4)
    add("ragged_16k", fs, 5, (_harmonics(rng, f1, fs), 70, 400, f1), (_harmonics(rng, f2, fs), 40, 700, f2))
    f = np.full(int(0.05 * fs), 180.0)  # 400 decimated samples; the longest filter of 70 - 400 Hz has 505 taps
    add("short_16k", fs, 5, (_harmonics(rng, f, fs), 70, 400, None))
    fs = 22050
    y, tr = _vowel(rng, 80, fs, 5.0)
    add("vowel_22k", fs, 5, (y, 70, 400, tr))
    return out


@functools.lru_cache(maxsize=None)
def stages(name, u=0, variant=False):
    """The restatement's stages of utterance u of a case, computed once and shared (read-only)."""
    c = cases()[name]
    w = c["utts"][u]
    f0, st = H.harvest(w["x"], c["fs"], w["minf0"], w["maxf0"], c["shiftms"], variant=variant, return_stages=True)
    st["f0"] = f0
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


def interior(track, fs, n_frames, period_ms, margin_ms=20):
    """Frames whose whole +-margin neighbourhood is voiced in the true track, and the true F0 there."""
    idx = np.minimum((np.arange(n_frames) * period_ms * fs) // 1000, len(track) - 1).astype(np.int64)
    m = int(margin_ms * fs / 1000)
    v = np.concatenate([[0.0], (track == 0).cumsum()])
    lo, hi = np.maximum(idx - m, 0), np.minimum(idx + m + 1, len(track))
    ok = (v[hi] - v[lo] == 0) & (idx - m >= 0) & (idx + m < len(track))
    return ok, track[idx]


def rel(a, b):
    """Largest |a - b| / |b| over the cells both fill, and the number of cells only one fills."""
    both = (a != 0) & (b != 0)
    d = float(np.max(np.abs(a[both] - b[both]) / np.abs(b[both]))) if both.any() else 0.0
    return d, int(np.sum((a != 0) != (b != 0)))


def measure(name):
    """What RECORDED holds for a case (the worst over its utterances)."""
    c = cases()[name]
    out = dict(err=0.0, s_dec=0.0, s_raw=0.0, s_ref=0.0, s_score=0.0, raw_flips=0, raw_cells=0, f0_flips=0)
    for u, w in enumerate(c["utts"]):
        a, b = stages(name, u), stages(name, u, True)
        out["s_dec"] = max(out["s_dec"], float(np.max(np.abs(a["yd"] - b["yd"])) / np.max(np.abs(a["yd"]))))
        d, fl = rel(b["raw"], a["raw"])
        out["s_raw"] = max(out["s_raw"], d)
        out["raw_flips"] += fl
        out["raw_cells"] += a["raw"].size
        # the refinement's own spread: both orders on the SAME candidate table
        rb, sb = H.refine(w["x"], c["fs"], a["cands"], a["cfg"]["floor"], a["cfg"]["ceil"], fft=True)
        out["s_ref"] = max(out["s_ref"], rel(rb, a["refined"])[0])
        out["s_score"] = max(out["s_score"], rel(sb, a["scores"])[0])
        out["f0_flips"] += int(np.sum((a["f0"] != 0) != (b["f0"] != 0))) + int(np.sum((a["f1"] != 0) != (b["f1"] != 0)))
        if w["track"] is not None:
            ok, true = interior(w["track"], c["fs"], len(a["f0"]), c["shiftms"])
            ok &= a["f0"] != 0
            if ok.any():
                out["err"] = max(out["err"], float(np.max(np.abs(a["f0"][ok] / true[ok] - 1.0))))
    return out


# ---------------------------------------------------------------------------------------------------------- hand-built tables
RAW_TABLE = dict(fs=8000, samples=160, minf0=40, maxf0=800)  # the utterance whose layout the table has


def raw_table():
    """A (185 channels, 21 frames) raw table, the layout of 20 ms at 40 - 800 Hz: frame 0 a run of exactly 9 channels, frame
    1 of exactly 10, frame 2 runs touching the first and the last channel, frame 3 two runs, frame 4 as many runs as
    there are slots (16 runs of 10 fill 185 channels), frames 17 - 20 runs whose overlap meets the utterance's end."""
    n_ch, T = 185, 21
    raw = np.zeros((n_ch, T))
    bf = 36.0 * 2.0 ** ((np.arange(n_ch) + 1.0) / 40)
    raw[20:29, 0] = bf[20:29]
    raw[20:30, 1] = bf[20:30] * 1.01
    raw[0:10, 2] = bf[0:10]  # channel 0 is forced empty: 9 left
    raw[n_ch - 11:, 2] = bf[n_ch - 11:]  # the last is forced empty: 10 left
    raw[5:40, 3] = bf[5:40]
    raw[60:75, 3] = bf[60:75] * 0.99
    for k in range(16):
        raw[1 + 11 * k:11 + 11 * k, 4] = bf[1 + 11 * k:11 + 11 * k]
    for i in range(17, 21):
        raw[30 + i:45 + i, i] = bf[30 + i:45 + i] * (1.0 + 0.001 * i)
    return raw


def contour_tables():
    """(cands, scores), each (frames, 112), and the frames of the structure: runs with an 8-frame gap (bridged) and a 9-frame
    gap (left open), a 5-frame run (dropped) and a 6-frame run (kept, then grown through lower-scored candidates under an
    erratic best candidate), and two runs that grow into each other and are merged by score."""
    T = 700
    c, s = np.zeros((T, H.NS)), np.zeros((T, H.NS))

    def run(a, b, f, slot=0, score=10.0):
        c[a:b, slot] = f + 0.02 * (np.arange(a, b) - a)
        s[a:b, slot] = score

    def erratic(a, b):  # a best candidate that jumps 3 % every frame: dropped by the jump rule
        c[a:b, 0] = np.where(np.arange(a, b) % 2 == 0, 300.0, 310.0)
        s[a:b, 0] = 20.0

    run(20, 80, 150.0)
    run(88, 150, 158.0)  # 8-frame gap 80 .. 87
    run(159, 230, 149.0)  # 9-frame gap 150 .. 158
    run(259, 265, 170.0)  # 5 frames once the jump rule has taken a run's first frame
    erratic(265, 300)
    run(265, 300, 170.1, slot=17, score=3.0)
    run(329, 336, 180.0)  # 6 frames
    erratic(336, 370)
    run(336, 370, 180.1, slot=17, score=3.0)
    run(420, 470, 120.0)
    erratic(470, 500)
    run(470, 500, 121.0, slot=33, score=4.0)
    run(500, 560, 122.0, score=12.0)
    run(600, 640, 200.0)
    run(640, 641, 260.0, slot=5)  # a lone candidate: unreliable, removed
    return c, s, dict(T=T, bridged=(80, 88), open=(150, 159), dropped=(260, 265), kept=(330, 336), merged=(420, 560))


def edges_reached():
    """Every case sits on the edge it is named for (host only)."""
    raw = raw_table()
    off = H.official_candidates(raw)
    assert np.count_nonzero(off[0]) == 0 and np.count_nonzero(off[1]) == 1
    assert np.count_nonzero(off[2]) == 1 and np.count_nonzero(off[3]) == 2 and np.count_nonzero(off[4]) == H.NC
    c, s, e = contour_tables()
    out, st = H.contour(c, s, return_steps=True)
    assert np.all(out[e["bridged"][0]:e["bridged"][1]] != 0) and np.all(out[e["open"][0]:e["open"][1]] == 0)
    assert np.all(st["step2"][e["dropped"][0]:e["dropped"][1]] == 0) and np.all(st["step1"][e["dropped"][0] + 1:e["dropped"][1]] != 0)
    assert np.all(st["step2"][e["kept"][0] + 1:e["kept"][1]] != 0)
    assert np.all(out[e["dropped"][0]:e["dropped"][1] + 20] == 0) and np.all(out[e["kept"][0] + 1:e["kept"][1] + 20] != 0)
    assert np.all(out[e["merged"][0] + 1:e["merged"][1] - 1] != 0)
    assert out[640] == 0 and c[640, 5] != 0
    # the runs counted at each step: 5- and 6-frame runs have exactly those lengths after the jump rule
    runs1 = {int(a): int(b - a + 1) for a, b in H._boundaries(st["step1"].copy())}
    assert runs1[e["dropped"][0]] == 5 and runs1[e["kept"][0]] == 6, runs1
    cs = cases()
    # one case per decimation ratio, a 40 - 700 Hz range, two ranges in one batch
    assert sorted({H.setup(c["fs"], 100, 70, 400)["r"] for c in cs.values()}) == [1, 2, 3, 6]
    assert any(w["minf0"] == 40 and w["maxf0"] == 700 for c in cs.values() for w in c["utts"])
    assert len({(w["minf0"], w["maxf0"]) for w in cs["ragged_16k"]["utts"]}) == 2
    assert all(len(w["x"]) <= 0.6 * c["fs"] + 8 for c in cs.values() for w in c["utts"])
    w = cs["short_16k"]["utts"][0]
    cfg = H.setup(16000, len(w["x"]), w["minf0"], w["maxf0"])
    assert cfg["nd"] < 2 * cfg["h"].max() + 1
    gap = stages("gap_8k")
    # the estimate reaches about 10 ms into the silence from both sides (220 .. 270 ms)
    assert np.all(gap["f1"][232:256] == 0) and np.all(gap["f1"][100:215] != 0) and np.all(gap["f1"][275:400] != 0)
    assert np.all(gap["yd"][int(0.22 * 8000):int(0.27 * 8000)] == 0.0)
    return True


if __name__ == "__main__":
    for name in cases():
        m = measure(name)
        print(f'    "{name}": dict(err={m["err"]:.3e}, s_dec={m["s_dec"]:.3e}, s_raw={m["s_raw"]:.3e}, '
              f's_ref={m["s_ref"]:.3e}, s_score={m["s_score"]:.3e}),  # raw flips {m["raw_flips"]} of {m["raw_cells"]}, '
              f'f0 flips {m["f0_flips"]}')
    print(edges_reached())
