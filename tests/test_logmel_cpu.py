"""The float64 reference of the log-mel tests (tests/logmel_cases.py) against independent facts, and the tolerance the
GPU tests derive from it (tests/test_gpu_logmel_shapes.py).  No GPU."""
import numpy as np

from tests import logmel_cases as C

CASES = C.cases()
BY = {c["name"]: c for c in CASES}


def test_unit_impulse_gives_the_window_tap_times_the_column_sums():
    """|rfft| of one unit impulse at sample n is window[n - lpad] in every bin, so each mel energy is that tap times
    the filter's sum of weights: pins the sample-to-window indexing of the reference without an FFT of its own."""
    for name in ("sweep_hamming", "sweep_win800", "r512_sweep_hamming"):
        c = BY[name]
        e = C.mel_energies(c, C.signal(c))  # (n_fft rows, 1 frame, n_mels)
        w = C.window64(c)
        want = w[:, None] * C.basis_of(c).astype(np.float64).sum(0)[None, :]
        assert e.shape == (c["n_fft"], 1, want.shape[1])
        assert np.abs(e[:, 0] - want).max() <= 1e-14 * want.max(), name
        lpad = (c["n_fft"] - c["win"]) // 2
        silent = C.silent_frames(e)[:, 0]
        assert silent.sum() == c["n_fft"] - c["win"] and silent[:lpad].all() and silent[lpad + c["win"]:].all()


def test_a_tone_on_a_bin_peaks_in_a_filter_over_that_bin():
    for name in ("tones", "r512_tones", "tones_basis_ends"):
        c = BY[name]
        nf = c["n_fft"]
        ks = [1, 37, nf // 2 - 1, nf // 2, 0] if c["sig"][1] == 5 else [1, nf // 2 - 1, nf // 2, 0]
        e = C.mel_energies(c, C.signal(c))
        fb = C.basis_of(c)
        for row, k in enumerate(ks):
            lobe = [j for j in (k - 1, k, k + 1) if 0 <= j <= nf // 2]  # the main lobe of a hann window
            for t in range(e.shape[1]):
                m = int(e[row, t].argmax())
                assert fb[lobe, m].any(), (name, k, t, m)
        # a tone exactly on bin k, hann window: |X[k]| = amp * sum(w) / 2 (twice that on bin 0 and on Nyquist)
        if "basis" in c:
            w = C.window64(c)
            x = C.signal(c)
            nyq = np.abs(np.fft.rfft(x[2, :nf].astype(np.float64) * w))[nf // 2]
            assert abs(nyq - 0.5 * abs(np.cos(0.3 * ((nf // 2) % 7))) * w.sum()) < 1e-5 * w.sum()
            assert abs(e[2, 0, 4] - nyq * float(fb[nf // 2, 4])) <= 1e-12 * nyq


def test_centred_frames_mirror_without_repeating_the_edge_sample():
    c = BY["centred_513"]
    x = C.signal(c)
    e = C.mel_energies(c, x)
    row = x[0].astype(np.float64)
    n, half = len(row), c["n_fft"] // 2
    padded = np.array([row[abs(i) if i < n else 2 * (n - 1) - i] for i in range(-half, n + half)])
    frames = np.stack([padded[t * c["hop"]:t * c["hop"] + c["n_fft"]] for t in range(C.n_frames(c))])
    want = np.abs(np.fft.rfft(frames * C.window64(c), axis=-1)) @ C.basis_of(c).astype(np.float64)
    assert e.shape == (1, 5, 80) and np.array_equal(e[0], want)


def test_every_edge_the_gpu_cases_are_meant_to_reach_is_reached():
    facts = C.edges_reached(CASES)
    assert all(facts.values()), facts
    assert sorted(C.ERRORS) == sorted(c["name"] for c in CASES)


def test_recorded_oracle_errors_are_the_oracles_own():
    """OracleLogMel (float32) against the float64 reference, every case.  torch.stft and the fp32 matmul order their
    additions differently from one CPU to the next (measured on two: 0.38 x .. 3.9 x the recorded value), so the oracle
    of this machine is held to what the kernels are held to - within FACTOR x the recorded error + FLOOR - and the
    recorded error may not be inflated either: no more than FACTOR x what this machine measures, + FLOOR.  None is
    above 1e-4, and the shapes agree."""
    bad = []
    for c in CASES:
        lin, log = C.oracle_error(c)
        r_lin, r_log = C.ERRORS[c["name"]]
        print(f'{c["name"]}: lin {lin} (recorded {r_lin}), log10 {log} (recorded {r_log})')
        for got, rec in ((lin, r_lin), (log, r_log)):
            assert (got is None) == (rec is None), c["name"]
            if got is None:
                continue
            assert max(got, rec) <= 1e-4, c["name"]
            if not (got <= C.FACTOR * rec + C.FLOOR and rec <= C.FACTOR * got + C.FLOOR):
                bad.append((c["name"], got, rec))
    assert not bad, bad


def test_silent_frames_of_the_oracle_are_exactly_the_silent_value():
    import torch

    for name in ("silence", "r512_silence", "scaler_silence", "sweep_win800"):
        c = BY[name]
        x = C.signal(c)
        with torch.no_grad():
            got = C.oracle(c)(torch.from_numpy(x)).numpy()
        silent = C.silent_frames(C.mel_energies(c, x))
        assert silent.any() and np.array_equal(got[silent], np.broadcast_to(C.silent_value(c), got[silent].shape)), name
    assert C.silent_value(BY["silence"]).tolist() == [-10.0] * 80


def test_log10_metric_is_unmasked_only_where_every_cell_is_within_1e3_of_its_frames_largest():
    for c in CASES:
        if "log" not in c["metrics"]:
            continue
        x = C.signal(c, C.host_rows(c))
        e = C.mel_energies(c, x)
        e = e[~C.silent_frames(e)]
        e = e[:, (C.basis_of(c) != 0).any(0)]  # (an all-zero filter gives log10(eps) in every implementation)
        ratio = float((np.maximum(e, C.EPS) / np.maximum(e, C.EPS).max(-1, keepdims=True)).min())
        print(f'{c["name"]}: smallest cell / largest of its frame {ratio:.3e}')
        assert ratio >= 1e-3, c["name"]


def test_product_slaney_basis_equals_the_oracles_bit_for_bit():
    from crank_amd.net.module.mlfb import slaney_mel_basis
    from oracle.modules import slaney_mel_basis as oracle_basis

    seen = set()
    for c in CASES:
        if "mel" not in c:
            continue
        key = (c["fs"], c["n_fft"]) + tuple(c["mel"])
        if key in seen:
            continue
        seen.add(key)
        a, b = slaney_mel_basis(*key), oracle_basis(*key)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (c["mel"][0], c["n_fft"] // 2 + 1)
        assert np.array_equal(a, b), key
    assert len(seen) >= 9
