"""Griffin-Lim without a GPU: the restatement tests/griffin_lim_ref.py against torch's STFT pair and against itself, the
mel inversion's rounding bound, every refusal of crank_amd/griffin_lim.py (raised before a device is touched) and the C ABI's
crk_gl_* entries in header, binding and built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import griffin_lim_cases as C
from tests import griffin_lim_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in C.CASES]
GL_SYMBOLS = ["crk_gl_create", "crk_gl_destroy", "crk_gl_workspace_bytes", "crk_gl_linear_spectrum", "crk_gl_run",
              "crk_gl_stft", "crk_gl_istft"]

# The ulp allowance `c` of 10 ** x in the mel inversion's bound (n_mels + c) 2^-53 sum |a| |b|: the float64 power function
# of the host's and of the device's maths library are each within 2 ulp = 4 units of 2^-53 of the exact power (the
# dot product itself, n_mels terms summed in any order with or without fused multiply-add, is within n_mels units).
POW_ULP_ALLOWANCE = 4


def linear_spectrum_bound(mlfb, pinv):
    a = np.power(np.longdouble(10.0), np.asarray(mlfb).astype(np.longdouble))
    return np.asarray((N_TERMS + POW_ULP_ALLOWANCE) * 2.0 ** -53 * (a @ np.abs(pinv).astype(np.longdouble).T), np.float64)


N_TERMS = C.N_MELS


def _signal(case, seed=5):
    return np.random.default_rng(seed).standard_normal(case["hop"] * (case["T"] - 1))


def _window(case):
    return torch.hann_window(case["win"], periodic=True, dtype=torch.float64)


@pytest.mark.parametrize("name", NAMES)
def test_restated_stft_and_istft_equal_torch(name):
    c = C.materialise(name)
    x = _signal(c)
    X = R.stft(x, c["hop"], c["win"])
    Xt = torch.stft(torch.from_numpy(x), R.N, c["hop"], c["win"], window=_window(c), center=True, pad_mode="reflect",
                    return_complex=True).numpy().T
    assert X.shape == (c["T"], R.K) == Xt.shape
    assert R.rel_l2(X, Xt) < 1e-12
    # a spectrum that is not the STFT of any signal, with imaginary parts at bin 0 and bin 512 (irfft drops them)
    rng = np.random.default_rng(6)
    Y = X + 0.3 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    y = R.istft(Y, c["hop"], c["win"])
    Yt = torch.from_numpy(np.ascontiguousarray(Y.T)).clone()
    Yt[0].imag.zero_()  # torch.istft's irfft ignores them as numpy's does; zeroed so that no backend can differ on it
    Yt[-1].imag.zero_()
    yt = torch.istft(Yt, R.N, c["hop"], c["win"], window=_window(c), center=True, length=c["hop"] * (c["T"] - 1)).numpy()
    assert y.shape == yt.shape == (c["hop"] * (c["T"] - 1),)
    assert R.rel_l2(y, yt) < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_istft_inverts_stft_on_the_interior(name):
    c = C.materialise(name)
    x = _signal(c)
    y = R.istft(R.stft(x, c["hop"], c["win"]), c["hop"], c["win"])
    # every sample of the trimmed signal is covered by a non-zero window (hop < win_length): the inverse is exact
    assert R.rel_l2(y, x) < 1e-12


def test_three_transforms_agree_on_a_frame():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, R.N))
    Xs = [t.rfft(x) for t in R.TRANSFORMS]
    assert all(X.shape == (3, R.K) for X in Xs)
    assert R.spread(Xs) < 1e-14
    Y = rng.standard_normal((3, R.K)) + 1j * rng.standard_normal((3, R.K))
    ys = [t.irfft(Y) for t in R.TRANSFORMS]
    assert all(y.shape == (3, R.N) and y.dtype == np.float64 for y in ys)
    assert R.spread(ys) < 1e-14
    assert R.rel_l2(R.Radix2FFT.irfft(R.Radix2FFT.rfft(x)), x) < 1e-14


@pytest.mark.parametrize("name", [n for n in NAMES if "zero" not in n])
def test_linear_spectrum_within_the_dot_product_bound(name):
    c = C.materialise(name)
    pinv = C.pinv_basis(c["fs"])
    ref = R.linear_spectrum(c["mlfb"], pinv, np.longdouble)
    err = np.abs(c["spc"] - np.asarray(ref, np.float64))
    assert (err <= linear_spectrum_bound(c["mlfb"], pinv)).all()


def test_the_negative_case_has_negative_cells_and_the_silent_case_is_tiny_but_not_zero():
    neg = C.materialise("hop128_negative_80")["spc"]
    assert 0.005 < (neg < 0).mean() < 0.5
    sil = C.materialise("hop128_silent_90")["S"]
    assert 0 < sil.max() < 1e-6
    assert not C.materialise("hop128_zero_20")["S"].any()
    for c in C.CASES:
        assert c["hop"] * (c["T"] - 1) > R.N // 2
    assert C.CASES[6]["hop"] * (C.CASES[6]["T"] - 2) <= R.N // 2 and C.CASES[7]["hop"] * (C.CASES[7]["T"] - 2) <= R.N // 2


def test_zero_spectrum_gives_exact_zeros():
    c = C.materialise("hop128_zero_20")
    y = R.griffin_lim(c["S"], c["angles"], 3, c["hop"], c["win"], clip=False)
    assert y.shape == (c["hop"] * (c["T"] - 1),) and not y.any() and np.isfinite(y).all()


def test_spectral_convergence_improves_on_every_case():
    snaps = C.all_snapshots()
    for c in C.CASES:
        if c["kind"] == "zero":
            continue
        m = C.materialise(c["name"])
        s = snaps[(c["name"], 0)]
        before = R.spectral_convergence(s[0], m["S"], c["hop"], c["win"])
        after = R.spectral_convergence(s[100], m["S"], c["hop"], c["win"])
        print(f"{c['name']}: spectral convergence {before:.3f} -> {after:.3f}")
        assert after < before, c["name"]


def test_spread_of_the_restatement_is_at_rounding_level():
    """The three transforms' results stay at the level the 100 iterations amplify float64 rounding to (a 1e-12 perturbation
    of the initial phases grows to 1e-9): a restatement whose transforms disagreed by more would be no yardstick."""
    snaps = C.all_snapshots()
    for c in C.CASES:
        for k in C.KS:
            sp = R.spread([snaps[(c["name"], i)][k] for i in range(len(R.TRANSFORMS))])
            print(f"{c['name']} k={k}: spread {sp:.3e}")
            assert sp < 1e-9, (c["name"], k)


def test_refusals_raise_before_a_device_is_touched():
    from crank_amd.griffin_lim import GriffinLim

    with pytest.raises(ValueError, match="1024"):
        GriffinLim(fftl=2048)
    with pytest.raises(ValueError, match="win_length"):
        GriffinLim(win_length=1025)
    with pytest.raises(ValueError, match="hann"):
        GriffinLim(window="hamming")
    with pytest.raises(ValueError, match="hop_size"):
        GriffinLim(hop_size=0)
    gl = GriffinLim(hop_size=128)
    T = 20
    ok = np.full((T, 80), -2.0)
    S = np.ones((T, 513))
    with pytest.raises(ValueError, match="80"):
        gl.mlfb2wav_batch([np.zeros((T, 79))])
    with pytest.raises(ValueError, match="80"):
        gl.linear_spectrum_batch([np.zeros((T, 81))])
    with pytest.raises(ValueError, match="at least 6 frames"):
        gl.mlfb2wav_batch([ok[:5]])
    with pytest.raises(ValueError, match="at least 6 frames"):
        gl.griffin_lim_batch([S[:5]])
    with pytest.raises(ValueError, match="n_iters"):
        gl.mlfb2wav_batch([ok], n_iters=-1)
    with pytest.raises(ValueError, match="n_iters"):
        gl.griffin_lim_batch([S], n_iters=-1)
    bad = ok.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        gl.mlfb2wav_batch([ok, bad])
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        gl.linear_spectrum_batch([bad])
    with pytest.raises(ValueError, match="angles"):
        gl.griffin_lim_batch([S], angles=[np.ones((T, 512), np.complex128)])
    with pytest.raises(ValueError, match="angles"):
        gl.griffin_lim_batch([S, S], angles=[np.ones((T, 513), np.complex128)])
    with pytest.raises(ValueError, match="512"):
        gl.stft_batch([np.zeros(512)])
    # a CPU device is refused as crank_amd.world refuses it, once the inputs are in order
    cpu = GriffinLim(hop_size=128, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        cpu.mlfb2wav_batch([ok])
    with pytest.raises(RuntimeError, match="GPU"):
        cpu.griffin_lim_batch([S])


def test_mlfb2wavf_logs_and_skips_non_finite_input(tmp_path, caplog):
    import logging

    from crank_amd.griffin_lim import mlfb2wavf

    bad = np.full((20, 80), np.nan)
    with caplog.at_level(logging.INFO):
        assert mlfb2wavf(bad, tmp_path / "sub" / "a.wav", hop_size=128) is None
    assert "ERROR" in caplog.text and (tmp_path / "sub").is_dir() and not (tmp_path / "sub" / "a.wav").exists()


def test_crk_gl_entries_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "crank_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(crk_gl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(GL_SYMBOLS), declared ^ set(GL_SYMBOLS)
    from crank_amd import _lib

    assert {s for s in _lib.SIGNATURES if s.startswith("crk_gl_")} == set(GL_SYMBOLS)
    lib_path = os.path.join(REPO, "crank_amd", "libcrank_hip.so")
    assert os.path.exists(lib_path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(lib_path)
    missing = [s for s in GL_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    # host-only entry: the workspace of n frames is two windowed frames and one complex spectrogram row per frame
    lib.crk_gl_workspace_bytes.restype = ctypes.c_longlong
    lib.crk_gl_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong]
    need = lib.crk_gl_workspace_bytes(2, 100, 100 * 128)
    assert 100 * (2 * 1024 * 8 + 513 * 16) <= need <= 100 * (2 * 1024 * 8 + 513 * 16) + 3 * 256
    assert lib.crk_gl_workspace_bytes(0, 100, 100) == -1 and lib.crk_gl_workspace_bytes(1, 0, 100) == -1
