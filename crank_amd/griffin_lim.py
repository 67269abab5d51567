"""Griffin-Lim waveform synthesis for log-mel models on the MI355X: what the reference's eval stage writes for
``output_feat_type: mlfb`` (basetrainer.py ``_save_decoded_mlfb`` -> ``crank.utils.mlfb2wavf`` -> ``mlfb2wav``:
``logmelspc_to_linearspc``, then librosa ``griffinlim`` with its defaults - momentum 0.99, random initial phases, centred
reflect-padded STFT, periodic Hann window - clipped to [-1, 1 - 2^-15]) and what ``crank/bin/griffin_lim.py`` runs.

Everything runs in the float64 HIP kernels of csrc/griffin_lim_kernels.hip (crk_gl_*), on a ragged batch of utterances per
call; CRANK_AMD_PRECISION does not apply.  There is no torch or CPU fallback: without the library every call raises.

Pinned: the kernels against the CPU restatement tests/griffin_lim_ref.py (sample by sample, within a multiple of the
restatement's own rounding spread), the restatement's ``stft`` / ``istft`` against ``torch.stft`` / ``torch.istft``, the mel
basis by the log-mel tests.  Unpinned: parity with librosa itself (it is not installed anywhere this project is tested);
the loop is restated from librosa's published algorithm.

Layouts: every spectrum here is frames first, (T, 513), also the initial phases (librosa's are (513, T)).  An utterance of T
frames gives hop_size * (T - 1) samples and needs hop_size * (T - 1) > fftl / 2, the condition ``torch.stft`` imposes on its
reflect padding.

Initial phases: utterance i of a call draws ``numpy.random.RandomState(seed + i).rand(513, T_i)`` on the host, the stream
librosa draws with ``random_state=seed``; ``seed=None`` uses numpy's global generator as the reference does.
"""
import ctypes
import logging
from pathlib import Path

import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, stream_ptr
from crank_amd._ragged import Workspace, f64, offsets, release, require_gpu, size_of

FFTL = 1024  # the only fftl the kernels implement (every recipe uses it)
K = FFTL // 2 + 1
MAX_MELS = 256
CLIP_LO, CLIP_HI = -1.0, 0.999969482421875
WS_BYTES_PER_FRAME = 2 * FFTL * 8 + K * 16  # two windowed frames and one complex spectrogram row


def _shape(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else np.asarray(x).shape


def _finite(x):
    if isinstance(x, torch.Tensor):
        return bool(torch.isfinite(x).all())
    return bool(np.isfinite(np.asarray(x)).all())


class GriffinLim:
    """``crank.utils.mlfb2wav`` with its arguments, run by the kernels on ragged batches.  ``workspace_cap``: the most
    workspace bytes one launch sequence may use (a larger batch runs in chunks of whole utterances, with the same bits);
    None takes half of the device's free memory at the first call."""

    def __init__(self, fs=22050, n_mels=80, fftl=FFTL, win_length=1024, hop_size=220, fmin=80, fmax=7600, window="hann",
                 device="cuda", workspace_cap=None):
        if int(fftl) != FFTL:
            raise ValueError(f"fftl {fftl}: only {FFTL} is supported")
        win_length = FFTL if win_length is None else int(win_length)
        if not 1 <= win_length <= FFTL:
            raise ValueError(f"win_length {win_length}: must lie in 1 .. fftl = {FFTL}")
        if window != "hann":
            raise ValueError(f"window {window!r}: only 'hann' is supported")
        if not 1 <= int(hop_size) <= FFTL:
            raise ValueError(f"hop_size {hop_size}: must lie in 1 .. {FFTL}")
        if not 1 <= int(n_mels) <= MAX_MELS:
            raise ValueError(f"n_mels {n_mels}: the kernels take 1 .. {MAX_MELS}")
        self.fs, self.n_mels, self.fftl, self.win_length, self.hop = int(fs), int(n_mels), FFTL, win_length, int(hop_size)
        self.fmin = 0 if fmin is None else fmin
        self.fmax = self.fs / 2 if fmax is None else fmax
        self.device = torch.device(device)
        self.workspace_cap = None if workspace_cap is None else int(workspace_cap)
        self.min_frames = FFTL // 2 // self.hop + 2  # the fewest frames with hop * (T - 1) > fftl / 2
        self._pinv = None
        self._handle = None
        self._workspace = Workspace(self.device)

    def __del__(self):
        release(self, "_handle", "crk_gl_destroy")

    # -- host tables
    def pinv_basis(self):
        """(513, n_mels) float64: numpy.linalg.pinv of the Slaney mel basis (librosa.filters.mel's float32 values)."""
        if self._pinv is None:
            from crank_amd.net.module.mlfb import slaney_mel_basis

            basis = slaney_mel_basis(self.fs, self.fftl, self.n_mels, self.fmin, self.fmax).astype(np.float64)
            self._pinv = np.ascontiguousarray(np.linalg.pinv(basis))
        return self._pinv

    def handle(self):
        if self._handle is None:
            self._on_device()
            p = self.pinv_basis()
            h = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                check(_lib.lib().crk_gl_create(self.fs, self.fftl, self.win_length, self.hop, self.n_mels,
                                               p.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)), "crk_gl_create")
            self._handle = h
        return self._handle

    def _on_device(self):
        require_gpu(self.device, "Griffin-Lim", "the synthesizer's device")

    def samples(self, frames):
        """Samples of an utterance of `frames` frames: librosa's istft length, hop * (frames - 1)."""
        return self.hop * (int(frames) - 1)

    # -- inputs
    def _check_frames(self, T, what):
        if self.samples(T) <= FFTL // 2:
            raise ValueError(f"{what} of {T} frames: hop_size {self.hop} needs at least {self.min_frames} frames "
                             f"(hop_size * (frames - 1) must exceed fftl / 2 = {FFTL // 2} for the reflect padding)")

    def _check_matrices(self, xs, width, what, min_frames=True):
        if not isinstance(xs, (list, tuple)) or len(xs) < 1:
            raise ValueError(f"{what}: a non-empty list of (frames, {width}) matrices is needed")
        for x in xs:
            shp = _shape(x)
            if len(shp) != 2 or shp[1] != width:
                raise ValueError(f"{what} must be (frames, {width}), got {shp}")
            if min_frames:
                self._check_frames(shp[0], what)
            elif shp[0] < 1:
                raise ValueError(f"{what} without frames")
        for x in xs:
            if not _finite(x):
                raise ValueError(f"{what} holds non-finite values")

    def _offsets(self, lens):
        return offsets(lens, self.device)

    # -- device resources
    def workspace_bytes(self, n_utts, total_frames, total_samples):
        return int(_lib.lib().crk_gl_workspace_bytes(int(n_utts), int(total_frames), int(total_samples)))

    def reserve(self, n_utts, total_frames, total_samples):
        """Workspace for a call of that size (kept and grown, never per call)."""
        need = self.workspace_bytes(n_utts, total_frames, total_samples)
        if need >= 0:
            self.handle()
        return self._workspace.ensure(need, "crk_gl_workspace_bytes")

    def _cap(self):
        if self.workspace_cap is None:
            self._on_device()
            self.workspace_cap = int(torch.cuda.mem_get_info(self.device)[0] // 2)
        return self.workspace_cap

    def _chunks(self, lens):
        """Runs of whole utterances (start, stop) whose workspace stays within the cap."""
        cap = self._cap()
        out, start, frames = [], 0, 0
        for i, T in enumerate(lens):
            if T * WS_BYTES_PER_FRAME + 1024 > cap:
                raise ValueError(f"an utterance of {T} frames needs {T * WS_BYTES_PER_FRAME + 1024} workspace bytes, "
                                 f"above the cap of {cap}")
            if frames and (frames + T) * WS_BYTES_PER_FRAME + 1024 > cap:
                out.append((start, i))
                start, frames = i, 0
            frames += T
        out.append((start, len(lens)))
        return out

    # -- the stages
    def linear_spectrum_batch(self, mlfbs, magnitude=True):
        """``logmelspc_to_linearspc`` of each (T, n_mels) log-mel: list of (T, 513) float64 on the device.  With
        ``magnitude`` (the default) its absolute value, what ``griffin_lim`` takes of it; else signed as the reference
        returns it (no clamp: cells may be negative)."""
        self._check_matrices(mlfbs, self.n_mels, "a log-mel matrix", min_frames=False)
        self._on_device()
        lens = [int(_shape(m)[0]) for m in mlfbs]
        x = torch.cat([f64(m, self.device) for m in mlfbs]).contiguous()
        S = torch.empty(sum(lens), K, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_gl_linear_spectrum(self.handle(), x.data_ptr(), sum(lens), int(bool(magnitude)),
                                                    S.data_ptr(), stream_ptr()), "crk_gl_linear_spectrum")
        return list(S.split(lens))

    def initial_angles(self, lens, seed=0):
        """Unit phasors exp(2 pi i r), r = RandomState(seed + i).rand(513, T_i) for utterance i (numpy's global generator
        when seed is None), as (T_i, 513) complex128 on the device."""
        out = []
        for i, T in enumerate(lens):
            r = (np.random if seed is None else np.random.RandomState(int(seed) + i)).rand(K, int(T))
            out.append(torch.as_tensor(np.exp(2j * np.pi * r).T.copy(), device=self.device))
        return out

    def griffin_lim_batch(self, spcs, n_iters=100, seed=0, angles=None, clip=True):
        """``griffin_lim`` of each (T, 513) linear spectrum (its absolute value is taken): list of float64 waveforms of
        hop * (T - 1) samples on the device, clipped to [-1, 1 - 2^-15] unless ``clip`` is False.  ``angles``: explicit
        initial unit phasors, one (T, 513) complex matrix per utterance, instead of the seeded draw."""
        if int(n_iters) < 0:
            raise ValueError(f"n_iters {n_iters}: must not be negative")
        self._check_matrices(spcs, K, "a linear spectrum")
        lens = [int(_shape(s)[0]) for s in spcs]
        if angles is not None:
            if not isinstance(angles, (list, tuple)) or len(angles) != len(spcs):
                raise ValueError("angles: one (frames, 513) complex matrix per utterance is needed")
            for a, T in zip(angles, lens):
                if _shape(a) != (T, K):
                    raise ValueError(f"angles must be ({T}, {K}) for an utterance of {T} frames, got {_shape(a)}")
            for a in angles:
                if not _finite(a):
                    raise ValueError("angles hold non-finite values")
        self._on_device()
        ys = []
        for lo, hi in self._chunks(lens):
            ang = (self.initial_angles(lens[lo:hi], None if seed is None else int(seed) + lo) if angles is None
                   else [f64(a, self.device, torch.complex128) for a in angles[lo:hi]])
            ys += self._run([f64(s, self.device).abs() for s in spcs[lo:hi]], ang, int(n_iters), bool(clip))
        return ys

    def _run(self, S, ang, n_iters, clip):
        lens = [int(s.shape[0]) for s in S]
        slens = [self.samples(T) for T in lens]
        F, N = sum(lens), sum(slens)
        ws = self.reserve(len(lens), F, N)
        Sc = torch.cat(S).contiguous()
        A = torch.view_as_real(torch.cat(ang).contiguous())
        foff, soff = self._offsets(lens), self._offsets(slens)
        y = torch.empty(N, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_gl_run(self.handle(), Sc.data_ptr(), A.data_ptr(), foff.data_ptr(), soff.data_ptr(),
                                        len(lens), F, N, n_iters, int(clip), y.data_ptr(), ws.data_ptr(), ws.numel(),
                                        stream_ptr()), "crk_gl_run")
        return list(y.split(slens))

    def mlfb2wav_batch(self, mlfbs, n_iters=100, seed=0):
        """``mlfb2wav`` of each (T, n_mels) log-mel: list of clipped float64 waveforms on the device."""
        if int(n_iters) < 0:
            raise ValueError(f"n_iters {n_iters}: must not be negative")
        self._check_matrices(mlfbs, self.n_mels, "a log-mel matrix")
        return self.griffin_lim_batch(self.linear_spectrum_batch(mlfbs), n_iters, seed)

    # -- the projections alone (tests)
    def stft_batch(self, waves):
        """librosa ``stft(y, n_fft, hop, win_length, window, center=True, pad_mode="reflect")`` of each waveform: list of
        (1 + len // hop, 513) complex128."""
        if not isinstance(waves, (list, tuple)) or len(waves) < 1:
            raise ValueError("waves must be a non-empty list")
        slens = [size_of(w) for w in waves]
        for n in slens:
            if n <= FFTL // 2:
                raise ValueError(f"a waveform of {n} samples: the reflect padding needs more than fftl / 2 = {FFTL // 2}")
        for w in waves:
            if not _finite(w):
                raise ValueError("a waveform holds non-finite values")
        self._on_device()
        lens = [1 + n // self.hop for n in slens]
        x = torch.cat([f64(w, self.device).reshape(-1) for w in waves]).contiguous()
        foff, soff = self._offsets(lens), self._offsets(slens)
        spec = torch.empty(sum(lens), K, 2, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_gl_stft(self.handle(), x.data_ptr(), foff.data_ptr(), soff.data_ptr(), len(lens),
                                         sum(lens), sum(slens), spec.data_ptr(), stream_ptr()), "crk_gl_stft")
        return list(torch.view_as_complex(spec).split(lens))

    def istft_batch(self, specs):
        """librosa ``istft(spec, hop, win_length, window, center=True)`` of each (T, 513) complex spectrum: list of float64
        waveforms of hop * (T - 1) samples."""
        self._check_matrices(specs, K, "a complex spectrum")
        self._on_device()
        lens = [int(_shape(s)[0]) for s in specs]
        slens = [self.samples(T) for T in lens]
        F, N = sum(lens), sum(slens)
        ws = self.reserve(len(lens), F, N)
        X = torch.view_as_real(torch.cat([f64(s, self.device, torch.complex128) for s in specs]).contiguous())
        foff, soff = self._offsets(lens), self._offsets(slens)
        y = torch.empty(N, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_gl_istft(self.handle(), X.data_ptr(), foff.data_ptr(), soff.data_ptr(), len(lens), F, N,
                                          y.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "crk_gl_istft")
        return list(y.split(slens))

    # -- eval outputs
    def vocode_eval_outputs(self, outputs, n_iters=100, seed=0):
        """Waveforms of the per-utterance dicts of ``trainer._store_features`` for an mlfb model ("feats": the
        de-normalised converted log-mel), synthesised as one ragged batch and clipped like mlfb2wav.  A dict of such lists
        (one per target speaker) gives a dict of lists."""
        if isinstance(outputs, dict):
            return {k: self.vocode_eval_outputs(v, n_iters, seed) for k, v in outputs.items()}
        return self.mlfb2wav_batch([d["feats"] for d in outputs], n_iters, seed)


# ---------------------------------------------------------------------------------------------------- the reference's names
def logmelspc_to_linearspc(lmspc, fs, n_mels, n_fft, fmin=None, fmax=None):
    """The reference's ``crank.utils.logmelspc_to_linearspc``: (T, n_mels) log-mel -> (T, n_fft / 2 + 1) linear spectrum,
    signed (no clamp), float64 numpy."""
    gl = GriffinLim(fs, n_mels, n_fft, fmin=fmin, fmax=fmax)
    return gl.linear_spectrum_batch([lmspc], magnitude=False)[0].cpu().numpy()


def griffin_lim(spc, n_fft, n_shift, win_length, window="hann", n_iters=100, seed=None):
    """The reference's ``crank.utils.griffin_lim``: (T, n_fft / 2 + 1) linear spectrum -> clipped waveform (float64 numpy).
    ``seed`` None draws the initial phases from numpy's global generator, as the reference does."""
    gl = GriffinLim(fftl=n_fft, win_length=win_length, hop_size=n_shift, window=window)
    return gl.griffin_lim_batch([spc], n_iters, seed)[0].cpu().numpy()


def mlfb2wav(mlfb, fs=22050, n_mels=80, fftl=1024, win_length=1024, hop_size=220, fmin=80, fmax=7600, window="hann",
             n_iters=100, seed=None):
    """The reference's ``crank.utils.mlfb2wav`` (float64 numpy, clipped to [-1, 1 - 2^-15])."""
    gl = GriffinLim(fs, n_mels, fftl, win_length, hop_size, fmin, fmax, window)
    return gl.mlfb2wav_batch([mlfb], n_iters, seed)[0].cpu().numpy()


def mlfb2wavf(mlfb, wavf, fs=22050, n_mels=80, fftl=1024, win_length=1024, hop_size=220, fmin=80, fmax=7600,
              window="hann", n_iters=100, seed=None):
    """The reference's ``crank.utils.mlfb2wavf`` without ``plot``: makes the parent directory and writes 16-bit PCM; an
    utterance with non-finite values (what librosa refuses) is logged and skipped."""
    from crank_amd.world import write_pcm16

    Path(wavf).parent.mkdir(parents=True, exist_ok=True)
    if not _finite(mlfb):
        logging.info("ERROR: GriffinLim for {}".format(str(wavf)))
        return
    write_pcm16(wavf, mlfb2wav(mlfb, fs, n_mels, fftl, win_length, hop_size, fmin, fmax, window, n_iters, seed), fs)
