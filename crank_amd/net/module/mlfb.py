"""Waveform -> log-mel: the on-the-fly layer (crank/net/module/mlfb.py:134-171, used when the
recipe sets ``use_raw``; ``center=False``) and the offline extraction of the recipe's stage 2
(``logmelfilterbank``: crank/feature/feature.py:126-145 calls the third-party
``parallel_wavegan.bin.preprocess.logmelfilterbank``; ``center=True``,
reflect padding).  STFT (LDS FFT), magnitude, mel projection, log10 and the optional
standardisation run in one HIP kernel (mlfb_kernels.hip).

Only the fixed-window variants are implemented ("hann", "hamming", ... =
``torch.<name>_window``); the trainable "param" / "conv" window variants of the
reference's STFTLayer (mlfb.py:64-90) are rejected.
"""
import ctypes

import numpy as np
import torch

from ... import _lib, ops
from ..._lib import check, stream_ptr
from ..._ragged import made, release, require_gpu, reset_streams


def slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax):
    """Mel filterbank with librosa.filters.mel's defaults (Slaney scale: linear below
    1 kHz at 200/3 Hz per mel, log above with step ln(6.4)/27; triangular filters on
    linspace(0, sr/2, 1+n_fft/2); area normalisation 2/(f[i+2]-f[i])), restated from
    the published definition.  Returns (n_mels, n_bins) f32."""
    f_sp = 200.0 / 3
    brk_hz = 1000.0
    brk_mel = brk_hz / f_sp
    step = np.log(6.4) / 27.0

    def to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= brk_hz, brk_mel + np.log(np.maximum(f, 1e-10) / brk_hz) / step, f / f_sp)

    def to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= brk_mel, brk_hz * np.exp(step * (m - brk_mel)), f_sp * m)

    bins = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    edges = to_hz(np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    rel = edges[:, None] - bins[None, :]
    fb = np.zeros((n_mels, bins.size))
    for i in range(n_mels):
        fb[i] = np.maximum(0.0, np.minimum(-rel[i] / width[i], rel[i + 2] / width[i + 1]))
    fb *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return fb.astype(np.float32)


class LogMelFilterBankLayer(torch.nn.Module):
    def __init__(self, fs=22050, hop_size=256, fft_size=1024, win_length=None, window="hann", center=True,
                 pad_mode="reflect", n_mels=80, fmin=None, fmax=None, scaler=None, eps=1.0e-10, device="cuda"):
        super().__init__()
        if window in ("param", "conv"):
            raise NotImplementedError("trainable STFT windows (mlfb.py:64-90) are not implemented")
        if center and pad_mode != "reflect":
            raise NotImplementedError("center=True is implemented for pad_mode='reflect' only")
        self.center = bool(center)
        self.fs, self.hop_size, self.fft_size = fs, hop_size, fft_size
        self.win_length = fft_size if win_length is None else win_length
        self.eps = eps
        fmin = 0 if fmin is None else fmin
        fmax = fs / 2 if fmax is None else fmax
        basis = slaney_mel_basis(fs, fft_size, n_mels, fmin, fmax)  # (n_mels, n_bins)
        self.mel_basis = torch.from_numpy(np.ascontiguousarray(basis.T)).to(device)  # (n_bins, n_mels)
        self.window = getattr(torch, f"{window}_window")(self.win_length, dtype=torch.float32, device=device)
        self.mean = self.std = None
        if scaler is not None:  # MLFBScalerLayer, mlfb.py:116-131
            self.mean = torch.from_numpy(np.asarray(scaler.mean_)).float().to(device)
            self.std = torch.from_numpy(np.asarray(scaler.var_)).float().sqrt().to(device)

    def forward(self, x):
        """x: (B, n_samples) -> (B, T, n_mels); T = 1 + (n_samples - fft_size)//hop, or 1 + n_samples//hop
        when centred (torch.stft's frame count over the padded signal)."""
        if self.center and x.shape[1] <= self.fft_size // 2:
            raise ValueError(f"reflect padding of {self.fft_size // 2} samples needs a longer signal than {x.shape[1]}")
        T = frames_ready(x.shape[1], self.fft_size, self.hop_size, self.center, end=True)
        return ops.logmel(x, T, self.fft_size, self.hop_size, self.win_length, self.window, self.mel_basis, self.eps,
                          self.mean, self.std, center=self.center)

    def streaming(self, n_streams, max_samples):
        """A ``StreamingLogMel`` with this layer's framing, basis and scaler: up to ``n_streams`` streams, ``max_samples``
        samples a push."""
        return StreamingLogMel(self, n_streams, max_samples)


def frames_ready(n_total, fft_size, hop_size, center, end=False):
    """Frames of an utterance that exist once ``n_total`` samples of it have arrived (``end``: it is over at ``n_total``)."""
    h = fft_size // 2
    if center:
        if n_total <= h:
            return 0  # reflect padding needs more than h samples: the offline call refuses such an utterance
        return 1 + n_total // hop_size if end else (n_total - h) // hop_size + 1
    return 0 if n_total < fft_size else (n_total - fft_size) // hop_size + 1


class StreamingLogMel:
    """``push`` takes the next samples of up to ``n_streams`` independent streams, at most ``max_samples`` each per push,
    and returns the log-mel frames that have become computable (csrc/logmel_stream_kernels.hip, ``crk_logmel_stream_*``).
    Stream i is row i of every argument.

    The frames of an utterance are those of the layer on the whole signal - the same count, and values within fp32
    rounding of the offline kernel's - and they do not depend, bit for bit, on how the signal is cut into pushes, on S
    or on the row.  A centred layer emits frame t once sample ``t * hop + fft_size // 2 - 1`` has arrived; the push that
    carries the stream's ``end`` flag emits the frames that need the right mirror and starts a new utterance.  An
    uncentred layer has nothing to flush: ``end`` only starts a new utterance.  The last ``fft_size`` samples and both
    counts of every stream stay on the device; a push launches two kernels, neither allocates nor reads back, and can be
    captured in a graph.  There is no torch or CPU fallback.

    ``n_frames`` goes straight into ``StreamingConverter.push(..., n_valid=n_frames)`` with ``feats`` as the chunk: build
    that converter with ``max_chunk >= max_frames``."""

    def __init__(self, layer, n_streams, max_samples):
        if n_streams < 1 or max_samples < 1:
            raise RuntimeError(f"n_streams = {n_streams}, max_samples = {max_samples}: both must be at least 1")
        self.layer, self.device = layer, layer.mel_basis.device
        require_gpu(self.device, "the streaming log-mel front end", "the layer's device")
        self.n_streams, self.max_samples = int(n_streams), int(max_samples)
        self.fft_size, self.hop_size, self.center = layer.fft_size, layer.hop_size, layer.center
        self.n_mels = int(layer.mel_basis.shape[1])
        h = ctypes.c_void_p()
        L = _lib.lib()
        with torch.cuda.device(self.device):
            check(L.crk_logmel_stream_create(
                layer.fft_size, layer.hop_size, layer.win_length, layer.window.contiguous().data_ptr(),
                layer.mel_basis.contiguous().data_ptr(), self.n_mels, float(layer.eps), _lib.ptr(layer.mean),
                _lib.ptr(layer.std), 1 if layer.center else 0, self.n_streams, self.max_samples, ctypes.byref(h)),
                "crk_logmel_stream_create")
            self._handle = made(h, "crk_logmel_stream_create")
        self.max_frames = int(L.crk_logmel_stream_max_frames(self._handle))

    def __del__(self):
        release(self, "_handle", "crk_logmel_stream_destroy")

    @property
    def state_bytes(self):
        return int(_lib.lib().crk_logmel_stream_state_bytes(self._handle))

    def frames_ready(self, n_total, end=False):
        """Frames of an utterance emitted once ``n_total`` samples of it were pushed (``end``: with the end flag)."""
        return frames_ready(n_total, self.fft_size, self.hop_size, self.center, end)

    def reset(self, streams=None):
        """``streams`` (all of them by default) start a new utterance; frames not emitted yet are dropped."""
        reset_streams(self._handle, "crk_logmel_stream_reset", streams, self.device)

    def empty_outputs(self, S):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns."""
        return {"feats": torch.empty(S, self.max_frames, self.n_mels, device=self.device),
                "n_frames": torch.empty(S, dtype=torch.int32, device=self.device)}

    def _flags(self, t, S, what):
        if t is None:
            return None
        if t.device.type != "cuda" or tuple(t.shape) != (S,) or t.dtype not in (torch.int32, torch.int64, torch.bool):
            raise ValueError(f"{what}: an integer ({S},) tensor on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.to(torch.int32).contiguous()

    def push(self, x, n_valid=None, end=None, out=None):
        """x (S, C) float32 samples, n_valid (S,) samples that count per stream (default: C; 0 is allowed), end (S,)
        non-zero where this push ends the stream's utterance.  Returns ``feats`` (S, max_frames, n_mels) and ``n_frames``
        (S,) int32: the frames written at the start of each stream's block; frames past ``n_frames`` are not written.
        S above ``n_streams`` or C above ``max_samples`` is refused by the library (RuntimeError) before anything runs.
        out: buffers to write into (``empty_outputs``), e.g. the static ones of a captured graph."""
        if x.dim() != 2 or x.device.type != "cuda" or x.dtype != torch.float32:
            raise ValueError(f"x: a float32 (S, C) tensor on the GPU, got {x.dtype} {tuple(x.shape)} on {x.device}")
        S, C = int(x.shape[0]), int(x.shape[1])
        x = x.contiguous()
        n_valid, end = self._flags(n_valid, S, "n_valid"), self._flags(end, S, "end")
        if out is None:
            out = self.empty_outputs(S)
        else:
            f, n = out["feats"], out["n_frames"]
            if (f.device.type != "cuda" or f.dtype != torch.float32 or tuple(f.shape) != (S, self.max_frames, self.n_mels)
                    or not f.is_contiguous() or n.device.type != "cuda" or n.dtype != torch.int32 or tuple(n.shape) != (S,)):
                raise ValueError(f"out: feats float32 ({S}, {self.max_frames}, {self.n_mels}) and n_frames int32 ({S},) on "
                                 "the GPU (empty_outputs)")
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_logmel_stream_push(
                self._handle, x.data_ptr(), C, _lib.ptr(n_valid), _lib.ptr(end), S, C, out["feats"].data_ptr(), self.n_mels,
                out["n_frames"].data_ptr(), stream_ptr()), "crk_logmel_stream_push")
        return out


_LAYERS = {}


def logmelfilterbank(audio, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80,
                     fmin=None, fmax=None, eps=1e-10, device="cuda"):
    """Offline log-mel of one utterance with the signature of the function the reference's feature
    extraction calls (crank/feature/feature.py:134-145): audio (n_samples,) -> (1 + n_samples // hop, num_mels)
    float32 ndarray.  The waveform crosses PCIe once; everything else happens in one kernel."""
    key = (sampling_rate, fft_size, hop_size, win_length, window, num_mels, fmin, fmax, eps, str(device))
    if key not in _LAYERS:
        _LAYERS[key] = LogMelFilterBankLayer(fs=sampling_rate, hop_size=hop_size, fft_size=fft_size, win_length=win_length,
                                             window=window, center=True, n_mels=num_mels, fmin=fmin, fmax=fmax, eps=eps,
                                             device=device)
    x = torch.as_tensor(np.asarray(audio, dtype=np.float32), device=device)[None]
    return _LAYERS[key](x)[0].cpu().numpy()
