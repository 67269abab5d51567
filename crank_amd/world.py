"""WORLD waveform synthesis for mel-cepstral models on the MI355X: what the reference's eval stage writes for
``output_feat_type: mcep`` (basetrainer.py ``_save_decoded_world`` -> ``crank.utils.world2wav`` -> sprocket
``Synthesizer.synthesis``: power modification, pysptk ``mc2sp``, pyworld ``decode_aperiodicity`` and ``synthesize``).

Everything runs in the float64 HIP kernels of csrc/world_kernels.hip (crk_world_*), on a ragged batch of utterances
per call; CRANK_AMD_PRECISION does not apply.  Parity with pyworld / pysptk / sprocket is unpinned (none is installed):
the tests compare with the CPU restatement tests/world_synth_ref.py.  There is no torch or CPU fallback: without the
library every call raises.

``WorldAnalyzer`` is the other direction, the spectral half of WORLD analysis (csrc/world_analysis_kernels.hip,
crk_wana_*): what the reference's ``crank/bin/evaluate_mcd.py`` runs on a converted waveform - ``low_cut_filter``, pyworld
``cheaptrick``, pysptk ``sp2mc``, sprocket ``spc2npow`` - for a ragged batch of waveforms.  It does NOT estimate F0
(Harvest is not implemented): the caller gives the contour, for converted speech the ``f0`` the eval stage stored with
the utterance, where the reference re-estimates it from the converted waveform.  Aperiodicity (D4C) is not implemented
either.  The oracle is tests/world_analysis_ref.py; parity with pyworld / pysptk is unpinned.
"""
import ctypes

import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, stream_ptr

FFTL = 1024  # the only fftl the kernels implement (every mcep recipe uses it)
K = FFTL // 2 + 1
MAX_ORDER1 = 128
PULSE_CAPACITY = 32768  # pulses per response buffer: 256 MiB of the workspace


def n_bands(fs):
    """Bands of WORLD's coded aperiodicity at fs: int(min(15000, fs/2 - 3000) / 3000)."""
    return int(min(15000.0, fs / 2.0 - 3000.0) / 3000.0)


def y_length(frames, fs, shiftms):
    """pyworld synthesize's output length for `frames` frames."""
    return int(frames * shiftms * fs / 1000)


def _f64(x, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=torch.float64)
    return torch.as_tensor(np.asarray(x, np.float64), device=device)


class WorldSynthesizer:
    """sprocket's ``Synthesizer(fs, fftl, shiftms)`` with ``synthesis(f0, mcep, codeap, rmcep)``, run by the kernels.
    ``alpha`` is the all-pass constant of the mel-cepstrum (the reference passes it to ``synthesis``)."""

    def __init__(self, fs=22050, fftl=FFTL, shiftms=5.0, alpha=0.42, device="cuda", pulse_capacity=PULSE_CAPACITY):
        if int(fftl) != FFTL:
            raise ValueError(f"fftl {fftl}: only {FFTL} is supported")
        if n_bands(fs) < 1:
            raise ValueError(f"fs {fs}: WORLD's coded aperiodicity needs fs above 12 kHz")
        self.fs, self.fftl, self.shiftms, self.alpha = int(fs), FFTL, float(shiftms), float(alpha)
        self.bands = n_bands(self.fs)
        self.device = torch.device(device)
        self.pulse_capacity = int(pulse_capacity)
        self._handles = {}  # order + 1 -> handle
        self._ws = None
        self._reserved = {}  # order + 1 -> samples the handle's noise table covers
        self.last_pulse_count = None

    def __del__(self):
        try:
            for h in self._handles.values():
                _lib.lib().crk_world_destroy(h)
        except Exception:
            pass

    def handle(self, order1):
        if order1 not in self._handles:
            h = _lib.lib().crk_world_create(self.fs, self.fftl, self.shiftms, self.alpha, order1, self.bands,
                                            self.pulse_capacity)
            if not h:
                raise RuntimeError("libcrank_hip: crk_world_create failed (unsupported configuration or HIP error)")
            self._handles[order1] = h
        return self._handles[order1]

    # -- inputs
    def _check(self, f0, mcep, codeap, rmcep):
        T = mcep.shape[0]
        if mcep.dim() != 2 or not 1 <= mcep.shape[1] <= MAX_ORDER1:
            raise ValueError(f"mcep must be (frames, 1..{MAX_ORDER1}), got {tuple(mcep.shape)}")
        if T < 2:
            raise ValueError(f"{T} frames: WORLD synthesis needs at least 2")
        if f0.numel() != T:
            raise ValueError(f"f0 has {f0.numel()} values for {T} frames")
        if codeap.dim() != 2 or codeap.shape[0] != T:
            raise ValueError(f"codeap must be (frames, bands), got {tuple(codeap.shape)}")
        if codeap.shape[1] != self.bands:
            raise ValueError(f"coded aperiodicity of {codeap.shape[1]} bands; fs {self.fs} has {self.bands}")
        if rmcep is not None and tuple(rmcep.shape) != tuple(mcep.shape):
            raise ValueError(f"rmcep {tuple(rmcep.shape)} and mcep {tuple(mcep.shape)} differ")

    def _batch(self, f0s, mceps, codeaps, rmceps):
        n = len(mceps)
        if n < 1 or len(f0s) != n or len(codeaps) != n:
            raise ValueError("f0s, mceps and codeaps must be lists of the same non-zero length")
        if rmceps is None:
            rmceps = [None] * n
        if len(rmceps) != n or (any(r is None for r in rmceps) and any(r is not None for r in rmceps)):
            raise ValueError("rmceps must be None or given for every utterance")
        dev = self.device
        f0s = [_f64(f, dev).reshape(-1) for f in f0s]
        mceps = [_f64(m, dev) for m in mceps]
        codeaps = [_f64(c, dev) for c in codeaps]
        rmceps = [None if r is None else _f64(r, dev) for r in rmceps]
        for f, m, c, r in zip(f0s, mceps, codeaps, rmceps):
            self._check(f, m, c, r)
        order1 = mceps[0].shape[1]
        if any(m.shape[1] != order1 for m in mceps):
            raise ValueError("every mcep of a batch must have the same order")
        lens = [m.shape[0] for m in mceps]
        ylens = [y_length(T, self.fs, self.shiftms) for T in lens]
        if min(ylens) < 1:
            raise ValueError("an utterance shorter than one output sample")
        self._on_device()
        foff = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=dev)
        soff = torch.tensor([0] + list(np.cumsum(ylens)), dtype=torch.int64, device=dev)
        cat = lambda xs: torch.cat(xs).contiguous()  # noqa: E731
        rm = None if rmceps[0] is None else cat(rmceps)
        return dict(f0=cat(f0s), mcep=cat(mceps), cap=cat(codeaps), rmcep=rm, order1=order1, lens=lens, ylens=ylens,
                    foff=foff, soff=soff)

    def _on_device(self):
        if self.device.type != "cuda":
            raise RuntimeError("WORLD synthesis runs in the HIP kernels: the synthesizer's device must be the GPU")

    # -- device resources
    def workspace_bytes(self, n_utts, total_frames, total_samples, order1=40):
        return int(_lib.lib().crk_world_workspace_bytes(self.handle(order1), n_utts, total_frames, total_samples))

    def reserve(self, n_utts, total_frames, total_samples, max_samples, order1=40):
        """Workspace for a call of that size and the noise table for utterances of up to max_samples samples (kept
        and grown, never per call)."""
        need = self.workspace_bytes(n_utts, total_frames, total_samples, order1)
        if need < 0:
            raise ValueError("crk_world_workspace_bytes: bad shape")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if max_samples > self._reserved.get(order1, 0):
            check(_lib.lib().crk_world_reserve(self.handle(order1), int(max_samples)), "crk_world_reserve")
            self._reserved[order1] = int(max_samples)
        return self._ws

    # -- synthesis
    def synthesis_batch(self, f0s, mceps, codeaps, rmceps=None):
        """Waveforms (float64, y_length(frames) samples, not clipped) of a ragged batch."""
        b = self._batch(f0s, mceps, codeaps, rmceps)
        h = self.handle(b["order1"])
        F, S = sum(b["lens"]), sum(b["ylens"])
        ws = self.reserve(len(b["lens"]), F, S, max(b["ylens"]), b["order1"])
        y = torch.empty(S, dtype=torch.float64, device=self.device)
        npulses = ctypes.c_longlong(0)
        rm = b["rmcep"]
        check(_lib.lib().crk_world_synthesis(h, b["f0"].data_ptr(), b["mcep"].data_ptr(), rm.data_ptr() if rm is not None else None,
                                             b["cap"].data_ptr(), b["order1"], self.bands, b["foff"].data_ptr(),
                                             b["soff"].data_ptr(), len(b["lens"]), F, S, max(b["ylens"]), y.data_ptr(),
                                             ctypes.addressof(npulses), ws.data_ptr(), ws.numel(), stream_ptr()),
              "crk_world_synthesis")
        self.last_pulse_count = int(npulses.value)
        return list(y.split(b["ylens"]))

    def synthesis(self, f0, mcep, codeap, rmcep=None):
        """sprocket ``synthesis(f0, mcep, ap, rmcep)`` for one utterance (coded aperiodicity)."""
        return self.synthesis_batch([f0], [mcep], [codeap], None if rmcep is None else [rmcep])[0]

    # -- the stages alone (tests)
    def frame_tables_batch(self, mceps, codeaps, rmceps=None):
        """Per utterance (sp, ap), each (frames, 513): the power-modified mc2sp and the decoded aperiodicity."""
        n = len(mceps)
        mceps = [_f64(m, self.device) for m in mceps]
        f0s = [torch.zeros(m.shape[0], dtype=torch.float64, device=self.device) for m in mceps]
        b = self._batch(f0s, mceps, codeaps, rmceps)
        F = sum(b["lens"])
        ws = self.reserve(n, F, sum(b["ylens"]), max(b["ylens"]), b["order1"])
        sp = torch.empty(F, K, dtype=torch.float64, device=self.device)
        ap = torch.empty_like(sp)
        rm = b["rmcep"]
        check(_lib.lib().crk_world_frames(self.handle(b["order1"]), b["mcep"].data_ptr(),
                                          rm.data_ptr() if rm is not None else None, b["cap"].data_ptr(), b["order1"],
                                          self.bands, F, sp.data_ptr(), ap.data_ptr(), ws.data_ptr(), ws.numel(),
                                          stream_ptr()), "crk_world_frames")
        return list(zip(sp.split(b["lens"]), ap.split(b["lens"])))

    def pulses_batch(self, f0s):
        """Per utterance (pulse samples, noise sizes, fractional shifts in seconds, vuv at each pulse) on the host."""
        dev = self.device
        f0s = [_f64(f, dev).reshape(-1) for f in f0s]
        lens = [f.numel() for f in f0s]
        if min(lens) < 2:
            raise ValueError("WORLD synthesis needs at least 2 frames")
        ylens = [y_length(T, self.fs, self.shiftms) for T in lens]
        self._on_device()
        foff = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=dev)
        soff = torch.tensor([0] + list(np.cumsum(ylens)), dtype=torch.int64, device=dev)
        S = sum(ylens)
        pos = torch.empty(S, dtype=torch.int32, device=dev)
        shift = torch.empty(S, dtype=torch.float64, device=dev)
        vuv = torch.empty(S, dtype=torch.uint8, device=dev)
        cnt = torch.empty(len(lens), dtype=torch.int64, device=dev)
        f0 = torch.cat(f0s).contiguous()
        check(_lib.lib().crk_world_pulses(self.handle(1), f0.data_ptr(), foff.data_ptr(), soff.data_ptr(), len(lens),
                                          pos.data_ptr(), shift.data_ptr(), vuv.data_ptr(), cnt.data_ptr(), stream_ptr()),
              "crk_world_pulses")
        out, s0 = [], 0
        for n, c in zip(ylens, cnt.tolist()):
            p = pos[s0:s0 + c].cpu().numpy().astype(np.int64)
            ns = np.zeros(c, np.int64)
            ns[:-1] = p[1:] - p[:-1]
            out.append((p, ns, shift[s0:s0 + c].cpu().numpy(), vuv[s0:s0 + c].cpu().numpy().astype(np.float64)))
            s0 += n
        return out

    # -- eval outputs
    def vocode_eval_outputs(self, outputs, clip=True):
        """Waveforms of the per-utterance dicts of ``trainer._store_features`` for an mcep model ("f0", "feats" with the
        0th coefficient, "cap", "rmcep"), synthesised as one ragged batch and clipped to [-1, 1] like world2wav.  A dict
        of such lists (one per target speaker) gives a dict of lists."""
        if isinstance(outputs, dict):
            return {k: self.vocode_eval_outputs(v, clip) for k, v in outputs.items()}
        for d in outputs:
            if d.get("cap") is None:
                raise ValueError("an mcep eval output without 'cap' (the batch has no coded aperiodicity)")
        f0s = [_f64(d["f0"], self.device).reshape(-1) for d in outputs]
        rm = [d.get("rmcep") for d in outputs]
        rm = None if all(r is None for r in rm) else rm
        ys = self.synthesis_batch(f0s, [d["feats"] for d in outputs], [d["cap"] for d in outputs], rm)
        return [y.clamp(-1.0, 1.0) for y in ys] if clip else ys


DRAWS_PER_FRAME = 2 * (FFTL // 2 - 1) + 1 + K  # the most randn values one CheapTrick frame draws
LOWCUT_TAPS = 255


class WorldAnalyzer:
    """sprocket's ``FeatureExtractor(analyzer="world", fs, fftl, shiftms)`` without F0 estimation and aperiodicity:
    CheapTrick spectral envelope, mel-cepstrum and normalised power of waveforms whose F0 contours are given, run by the
    kernels on a ragged batch.  Frame i of an utterance is centred at i * shiftms ms and ``len(f0)`` frames come back."""

    def __init__(self, fs=22050, fftl=FFTL, shiftms=5.0, device="cuda"):
        if int(fftl) != FFTL:
            raise ValueError(f"fftl {fftl}: only {FFTL} is supported")
        if not 8000 <= int(fs) <= 192000:
            raise ValueError(f"fs {fs}: the kernels take 8000 .. 192000 Hz")
        if not float(shiftms) > 0.0:
            raise ValueError(f"shiftms {shiftms}: must be positive")
        self.fs, self.fftl, self.shiftms = int(fs), FFTL, float(shiftms)
        self.device = torch.device(device)
        self._handles = {}  # (order + 1, alpha) -> handle
        self._reserved = {}  # handle key -> randn draws its table covers
        self._taps = {}  # cutoff -> device taps
        self._ws = None

    def __del__(self):
        try:
            for h in self._handles.values():
                _lib.lib().crk_wana_destroy(h)
        except Exception:
            pass

    def _on_device(self):
        if self.device.type != "cuda":
            raise RuntimeError("WORLD analysis runs in the HIP kernels: the analyzer's device must be the GPU")

    def handle(self, order1=1, alpha=0.0):
        key = (int(order1), float(alpha))
        if key not in self._handles:
            h = _lib.lib().crk_wana_create(self.fs, self.fftl, self.shiftms, key[1], key[0])
            if not h:
                raise RuntimeError("libcrank_hip: crk_wana_create failed (unsupported configuration or HIP error)")
            self._handles[key] = h
        return self._handles[key]

    # -- inputs
    def _batch(self, waves, f0s):
        n = len(waves)
        if n < 1 or len(f0s) != n:
            raise ValueError("waves and f0s must be lists of the same non-zero length")
        size = lambda a: int(a.numel() if isinstance(a, torch.Tensor) else np.asarray(a).size)  # noqa: E731
        lens, slens = [size(f) for f in f0s], [size(w) for w in waves]
        shift = self.shiftms / 1000.0 * self.fs
        for T, S in zip(lens, slens):
            if T < 1:
                raise ValueError("0 frames: an F0 contour needs at least 1 frame")
            if S < 1:
                raise ValueError("an empty waveform")
            if (T - 1) * shift > S + shift:
                raise ValueError(f"the last of {T} frames is centred at sample {(T - 1) * shift:.0f}, more than one "
                                 f"shift ({self.shiftms} ms) past the waveform's end ({S} samples)")
        self._on_device()
        dev = self.device
        f0 = torch.cat([_f64(f, dev).reshape(-1) for f in f0s]).contiguous()
        # the contours stay on the device; two flags come back
        flags = torch.stack([(~torch.isfinite(f0) | (f0 < 0)).any(), (f0 > self.fs / 4.0).any()]).tolist()
        if flags[0]:
            raise ValueError("F0 must be finite and not negative (0 marks an unvoiced frame)")
        if flags[1]:
            raise ValueError(f"F0 above fs / 4 = {self.fs / 4.0} Hz: the smoothing band would leave the spectrum")
        foff = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=dev)
        soff = torch.tensor([0] + list(np.cumsum(slens)), dtype=torch.int64, device=dev)
        return dict(f0=f0, lens=lens, slens=slens, foff=foff, soff=soff)

    def _waves(self, waves, dtype):
        dev = self.device
        xs = [w.detach().to(device=dev).reshape(-1) if isinstance(w, torch.Tensor)
              else torch.as_tensor(np.asarray(w).reshape(-1), device=dev) for w in waves]
        if len({x.dtype for x in xs}) > 1:
            xs = [x.to(dtype) for x in xs]
        return torch.cat(xs).to(dtype).contiguous()  # one cast of the batch, not one per utterance

    # -- device resources
    def reserve(self, n_utts, total_frames, total_samples, max_frames, order1=1, alpha=0.0):
        """Workspace for a call of that size and the randn table for utterances of up to max_frames frames (kept and
        grown, never per call).  Returns (workspace, the draw count the table is asked to cover)."""
        need = int(_lib.lib().crk_wana_workspace_bytes(n_utts, total_frames, total_samples))
        if need < 0:
            raise ValueError("crk_wana_workspace_bytes: bad shape")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        key = (int(order1), float(alpha))
        draws = int(max_frames) * DRAWS_PER_FRAME
        if draws > self._reserved.get(key, 0):
            check(_lib.lib().crk_wana_reserve(self.handle(*key), draws), "crk_wana_reserve")
            self._reserved[key] = draws
        return self._ws, draws

    # -- the stages
    def low_cut_batch(self, waves, cutoff=70):
        """The reference's ``low_cut_filter`` of each waveform cast to float32, as evaluate_mcd.py does: float64."""
        from scipy.signal import firwin

        if len(waves) < 1:
            raise ValueError("waves must be a non-empty list")
        slens = [int(w.numel() if isinstance(w, torch.Tensor) else np.asarray(w).size) for w in waves]
        if min(slens) < 1:
            raise ValueError("an empty waveform")
        self._on_device()
        if cutoff not in self._taps:
            taps = firwin(LOWCUT_TAPS, cutoff / (self.fs // 2), pass_zero=False)
            self._taps[cutoff] = torch.as_tensor(taps, dtype=torch.float64, device=self.device)
        x = self._waves(waves, torch.float32)
        soff = torch.tensor([0] + list(np.cumsum(slens)), dtype=torch.int64, device=self.device)
        y = torch.empty(x.numel(), dtype=torch.float64, device=self.device)
        check(_lib.lib().crk_wana_lowcut(self.handle(), x.data_ptr(), self._taps[cutoff].data_ptr(), LOWCUT_TAPS,
                                         soff.data_ptr(), len(slens), x.numel(), y.data_ptr(), stream_ptr()),
              "crk_wana_lowcut")
        return list(y.split(slens))

    def cheaptrick_batch(self, waves, f0s):
        """pyworld ``cheaptrick`` of each waveform (taken as float64, no low cut) at its F0 contour: list of (T, 513)."""
        b = self._batch(waves, f0s)
        x = self._waves(waves, torch.float64)
        F, S = sum(b["lens"]), sum(b["slens"])
        ws, draws = self.reserve(len(b["lens"]), F, S, max(b["lens"]))
        sp = torch.empty(F, K, dtype=torch.float64, device=self.device)
        check(_lib.lib().crk_wana_cheaptrick(self.handle(), x.data_ptr(), b["f0"].data_ptr(), b["foff"].data_ptr(),
                                             b["soff"].data_ptr(), len(b["lens"]), F, S, draws, sp.data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream_ptr()), "crk_wana_cheaptrick")
        return list(sp.split(b["lens"]))

    def mcep_batch(self, waves, f0s, dim=34, alpha=0.455, low_cut=70, return_sp=False):
        """sprocket ``FeatureExtractor.mcep(dim, alpha)`` of each waveform: list of (T, dim + 1).  ``low_cut``: the cutoff
        of the reference's low-cut filter applied first (waveform cast to float32, as evaluate_mcd.py does); None
        analyses the waveform as given."""
        order1 = int(dim) + 1
        if not 1 <= order1 <= MAX_ORDER1:
            raise ValueError(f"dim + 1 = {order1}: the kernels take 1 .. {MAX_ORDER1} coefficients")
        if not abs(float(alpha)) < 1.0:
            raise ValueError(f"alpha {alpha}: the all-pass constant must lie in (-1, 1)")
        b = self._batch(waves, f0s)
        if low_cut is None:
            x = self._waves(waves, torch.float64)
        else:
            x = torch.cat(self.low_cut_batch(waves, low_cut))
        F, S = sum(b["lens"]), sum(b["slens"])
        ws, draws = self.reserve(len(b["lens"]), F, S, max(b["lens"]), order1, alpha)
        mc = torch.empty(F, order1, dtype=torch.float64, device=self.device)
        sp = torch.empty(F, K, dtype=torch.float64, device=self.device) if return_sp else None
        check(_lib.lib().crk_wana_mcep(self.handle(order1, alpha), x.data_ptr(), b["f0"].data_ptr(), b["foff"].data_ptr(),
                                       b["soff"].data_ptr(), len(b["lens"]), F, S, draws, order1, mc.data_ptr(),
                                       _lib.ptr(sp), ws.data_ptr(), ws.numel(), stream_ptr()), "crk_wana_mcep")
        if return_sp:
            return list(mc.split(b["lens"])), list(sp.split(b["lens"]))
        return list(mc.split(b["lens"]))

    def npow_of_sp_batch(self, sps):
        """sprocket ``spc2npow`` of each (T, 513) envelope: list of (T,) in dB over the utterance's mean power."""
        self._on_device()
        sps = [_f64(s, self.device) for s in sps]
        lens = [int(s.shape[0]) for s in sps]
        if not lens or min(lens) < 1 or any(s.dim() != 2 or s.shape[1] != K for s in sps):
            raise ValueError(f"spectral envelopes must be (frames >= 1, {K})")
        F = sum(lens)
        ws, _ = self.reserve(len(lens), F, 1, 1)
        sp = torch.cat(sps).contiguous()
        foff = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=self.device)
        out = torch.empty(F, dtype=torch.float64, device=self.device)
        check(_lib.lib().crk_wana_npow(self.handle(), sp.data_ptr(), foff.data_ptr(), len(lens), F, out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream_ptr()), "crk_wana_npow")
        return list(out.split(lens))

    def npow_batch(self, waves, f0s):
        """sprocket ``FeatureExtractor.npow()`` of each waveform: list of (T,)."""
        return self.npow_of_sp_batch(self.cheaptrick_batch(waves, f0s))

    def analyze_mcep(self, wave, f0, dim=34, alpha=0.455, low_cut=70):
        """One utterance: evaluate_mcd.py's ``get_world_features`` with the F0 given."""
        return self.mcep_batch([wave], [f0], dim, alpha, low_cut)[0]

    def frame_shapes_batch(self, f0s):
        """Per utterance the integers the CheapTrick kernel forms for every frame (debug; on the host): dict of origin,
        half, dc_limit, boundary, offset."""
        self._on_device()
        dev = self.device
        f0s = [_f64(f, dev).reshape(-1) for f in f0s]
        lens = [int(f.numel()) for f in f0s]
        if not lens or min(lens) < 1:
            raise ValueError("an F0 contour needs at least 1 frame")
        F = sum(lens)
        foff = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=dev)
        f0 = torch.cat(f0s).contiguous()
        shapes = torch.empty(F, 4, dtype=torch.int32, device=dev)
        off = torch.empty(F, dtype=torch.int64, device=dev)
        check(_lib.lib().crk_wana_frame_shapes(self.handle(), f0.data_ptr(), foff.data_ptr(), len(lens), F,
                                               shapes.data_ptr(), off.data_ptr(), stream_ptr()), "crk_wana_frame_shapes")
        cuts = np.cumsum(lens)[:-1]
        out = []
        for s, o in zip(np.split(shapes.cpu().numpy().astype(np.int64), cuts), np.split(off.cpu().numpy(), cuts)):
            out.append(dict(origin=s[:, 0], half=s[:, 1], dc_limit=s[:, 2], boundary=s[:, 3], offset=o))
        return out

    # -- eval outputs
    def mcep_of_eval_outputs(self, waves, outputs, dim=34, alpha=0.455, low_cut=70):
        """Mel-cepstra of the waveforms ``ParallelWaveGANVocoder.vocode_eval_outputs`` returned for the per-utterance
        dicts ``outputs`` of ``trainer._store_features`` (their "f0" is the converted contour the model was conditioned
        on), analysed as one ragged batch on the device.  A dict of lists (one per target speaker) gives a dict of lists."""
        if isinstance(outputs, dict):
            return {k: self.mcep_of_eval_outputs(waves[k], v, dim, alpha, low_cut) for k, v in outputs.items()}
        if len(waves) != len(outputs):
            raise ValueError("one waveform per eval output is needed")
        return self.mcep_batch(list(waves), [d["f0"] for d in outputs], dim, alpha, low_cut)


def world2wav(f0, mcep, codeap, rmcep=None, wavf=None, fs=22050, fftl=1024, shiftms=10, alpha=0.455):
    """The reference's ``crank.utils.world2wav``: the synthesis clipped to [-1, 1], written to `wavf` (16-bit PCM)
    when given, else returned (float64 numpy)."""
    wav = WorldSynthesizer(fs, fftl, shiftms, alpha).synthesis(f0, mcep, codeap, rmcep).clamp(-1.0, 1.0)
    wav = wav.cpu().numpy()
    if wavf is None:
        return wav
    write_pcm16(wavf, wav, fs)


def write_pcm16(path, wav, fs):
    from scipy.io import wavfile

    from crank_amd.bin.pwg_decode import to_pcm16

    wavfile.write(str(path), int(fs), to_pcm16(wav))
