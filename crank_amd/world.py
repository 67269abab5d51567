"""WORLD waveform synthesis for mel-cepstral models on the MI355X: what the reference's eval stage writes for
``output_feat_type: mcep`` (basetrainer.py ``_save_decoded_world`` -> ``crank.utils.world2wav`` -> sprocket
``Synthesizer.synthesis``: power modification, pysptk ``mc2sp``, pyworld ``decode_aperiodicity`` and ``synthesize``).

Everything runs in the float64 HIP kernels of csrc/world_kernels.hip (crk_world_*), on a ragged batch of utterances
per call; CRANK_AMD_PRECISION does not apply.  Parity with pyworld / pysptk / sprocket is unpinned (none is installed):
the tests compare with the CPU restatement tests/world_synth_ref.py.  There is no torch or CPU fallback: without the
library every call raises.

``WorldAnalyzer`` is the other direction, the spectral half of WORLD analysis (csrc/world_analysis_kernels.hip,
crk_wana_*): what the reference's ``crank/bin/evaluate_mcd.py`` runs on a converted waveform - ``low_cut_filter``, pyworld
``cheaptrick``, pysptk ``sp2mc``, sprocket ``spc2npow`` - for a ragged batch of waveforms.  Its stage methods take the F0 contour from
the caller; ``analyze_batch`` estimates it first with ``HarvestF0``, as the reference does.  Aperiodicity is pyworld
``d4c`` and ``code_aperiodicity`` (csrc/d4c_kernels.hip, crk_wana_d4c*: ``d4c_batch``, ``codeap_batch``,
``code_aperiodicity_batch``) at 13640 .. 24052 Hz, and ``cap_postprocess_batch`` the recipe's ``ccap`` / ``cap_uv``.  The
oracles are tests/world_analysis_ref.py and tests/d4c_ref.py; parity with pyworld / pysptk is unpinned.

``HarvestF0`` is pyworld ``harvest`` (csrc/f0_kernels.hip, crk_f0_*) for a ragged batch of waveforms with a search range
each, and ``continuous_f0_batch`` the reference's ``convert_continuos_f0`` with ``lf0`` / ``lcf0``.  The oracle is
tests/harvest_ref.py; parity with pyworld is unpinned.  ``StreamingF0`` runs it on a window around
each block of a live stream's frames and finishes the contour into the ``lcf0`` / ``uv`` rows streaming conversion takes
(csrc/f0_stream_kernels.hip, crk_f0_stream_*; the definition is tests/f0_stream_ref.py).

``StreamingMcep`` (``WorldAnalyzer.streaming``) is ``mcep_batch`` frame by frame from live streams of samples and F0 rows,
bit for bit (csrc/wana_stream_kernels.hip, crk_wana_stream_*; the definition is tests/wana_stream_ref.py, DESIGN.md
section 6o); ``analysis_capacities`` sizes its ring and its F0 queue.

``StreamingWorldSynthesizer`` (``WorldSynthesizer.streaming``) is ``synthesis_batch`` sample by sample from live streams of
frame rows, bit for bit (csrc/world_stream_kernels.hip, crk_wsyn_stream_*; the definition is tests/wsyn_stream_ref.py,
DESIGN.md section 6p); ``synthesis_capacities`` sizes its row queue, its sample ring and what one push can add and emit.
"""
import ctypes

import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, stream_ptr
from crank_amd._ragged import Workspace, f64, made, offsets, release, require_gpu, reset_streams, size_of

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
        self._workspace = Workspace(self.device)
        self._reserved = {}  # order + 1 -> samples the handle's noise table covers
        self.last_pulse_count = None

    def __del__(self):
        release(self, "_handles", "crk_world_destroy")

    def handle(self, order1):
        if order1 not in self._handles:
            self._handles[order1] = made(_lib.lib().crk_world_create(self.fs, self.fftl, self.shiftms, self.alpha, order1,
                                                                     self.bands, self.pulse_capacity), "crk_world_create")
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
        f0s = [f64(f, dev).reshape(-1) for f in f0s]
        mceps = [f64(m, dev) for m in mceps]
        codeaps = [f64(c, dev) for c in codeaps]
        rmceps = [None if r is None else f64(r, dev) for r in rmceps]
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
        foff = offsets(lens, dev)
        soff = offsets(ylens, dev)
        cat = lambda xs: torch.cat(xs).contiguous()  # noqa: E731
        rm = None if rmceps[0] is None else cat(rmceps)
        return dict(f0=cat(f0s), mcep=cat(mceps), cap=cat(codeaps), rmcep=rm, order1=order1, lens=lens, ylens=ylens,
                    foff=foff, soff=soff)

    def _on_device(self):
        require_gpu(self.device, "WORLD synthesis", "the synthesizer's device")

    # -- device resources
    def workspace_bytes(self, n_utts, total_frames, total_samples, order1=40):
        return int(_lib.lib().crk_world_workspace_bytes(self.handle(order1), n_utts, total_frames, total_samples))

    def reserve(self, n_utts, total_frames, total_samples, max_samples, order1=40):
        """Workspace for a call of that size and the noise table for utterances of up to max_samples samples (kept
        and grown, never per call)."""
        ws = self._workspace.ensure(self.workspace_bytes(n_utts, total_frames, total_samples, order1),
                                    "crk_world_workspace_bytes")
        if max_samples > self._reserved.get(order1, 0):
            check(_lib.lib().crk_world_reserve(self.handle(order1), int(max_samples)), "crk_world_reserve")
            self._reserved[order1] = int(max_samples)
        return ws

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
        mceps = [f64(m, self.device) for m in mceps]
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
        f0s = [f64(f, dev).reshape(-1) for f in f0s]
        lens = [f.numel() for f in f0s]
        if min(lens) < 2:
            raise ValueError("WORLD synthesis needs at least 2 frames")
        ylens = [y_length(T, self.fs, self.shiftms) for T in lens]
        self._on_device()
        foff = offsets(lens, dev)
        soff = offsets(ylens, dev)
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

    def streaming(self, n_streams, max_rows_in, order1, **kw):
        """A ``StreamingWorldSynthesizer`` at this synthesizer's fs, shiftms, alpha and device (with a handle of its
        own: no call on this object can move the table a captured push reads)."""
        kw.setdefault("device", self.device)
        return StreamingWorldSynthesizer(self.fs, self.shiftms, n_streams, max_rows_in, order1, self.alpha, **kw)

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
        f0s = [f64(d["f0"], self.device).reshape(-1) for d in outputs]
        rm = [d.get("rmcep") for d in outputs]
        rm = None if all(r is None for r in rm) else rm
        ys = self.synthesis_batch(f0s, [d["feats"] for d in outputs], [d["cap"] for d in outputs], rm)
        return [y.clamp(-1.0, 1.0) for y in ys] if clip else ys


DRAWS_PER_FRAME = 2 * (FFTL // 2 - 1) + 1 + K  # the most randn values one CheapTrick frame draws
LOWCUT_TAPS = 255


D4C_FFT = 2048  # both of D4C's transforms at the supported rates
D4C_FS_MIN, D4C_FS_MAX = 13640, 24052
D4C_MAX_BANDS = 3


def d4c_fft_sizes(fs):
    """(Love-Train, D4C) transform sizes of WORLD at fs."""
    return (2 ** (1 + int(np.log2(3.0 * fs / 40.0 + 1))), 2 ** (1 + int(np.log2(4.0 * fs / 47.0 + 1))))


def check_d4c_fs(fs):
    lt, d4 = d4c_fft_sizes(fs)
    if (lt, d4) != (D4C_FFT, D4C_FFT):
        raise ValueError(f"fs {fs}: D4C would need a {lt}-point Love-Train transform and a {d4}-point one; the kernels "
                         f"implement {D4C_FFT} for both ({D4C_FS_MIN} <= fs <= {D4C_FS_MAX})")


def d4c_draws_per_frame(fs):
    """The most randn values one D4C frame draws: the Love-Train window at 40 Hz and the general pass's three at 47 Hz."""
    return (2 * int(1.5 * fs / 40.0 + 0.5) + 1) + 3 * (2 * int(2.0 * fs / 47.0 + 0.5) + 1)


class WorldAnalyzer:
    """sprocket's ``FeatureExtractor(analyzer="world", fs, fftl, shiftms)``: CheapTrick spectral envelope, mel-cepstrum,
    normalised power and D4C aperiodicity (plain and coded) of waveforms whose F0 contours are given, run by the kernels
    on a ragged batch; ``analyze_batch`` estimates the contours with Harvest first.  Frame i of an utterance is centred at i * shiftms ms and ``len(f0)`` frames come back."""

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
        self._workspace = Workspace(self.device)
        self._harvest = None

    def __del__(self):
        release(self, "_handles", "crk_wana_destroy")

    def _on_device(self):
        require_gpu(self.device, "WORLD analysis", "the analyzer's device")

    def handle(self, order1=1, alpha=0.0):
        key = (int(order1), float(alpha))
        if key not in self._handles:
            self._handles[key] = made(_lib.lib().crk_wana_create(self.fs, self.fftl, self.shiftms, key[1], key[0]),
                                      "crk_wana_create")
        return self._handles[key]

    # -- inputs
    def _batch(self, waves, f0s):
        n = len(waves)
        if n < 1 or len(f0s) != n:
            raise ValueError("waves and f0s must be lists of the same non-zero length")
        lens, slens = [size_of(f) for f in f0s], [size_of(w) for w in waves]
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
        f0 = torch.cat([f64(f, dev).reshape(-1) for f in f0s]).contiguous()
        # the contours stay on the device; two flags come back
        flags = torch.stack([(~torch.isfinite(f0) | (f0 < 0)).any(), (f0 > self.fs / 4.0).any()]).tolist()
        if flags[0]:
            raise ValueError("F0 must be finite and not negative (0 marks an unvoiced frame)")
        if flags[1]:
            raise ValueError(f"F0 above fs / 4 = {self.fs / 4.0} Hz: the smoothing band would leave the spectrum")
        foff = offsets(lens, dev)
        soff = offsets(slens, dev)
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
        ws = self._workspace.ensure(int(_lib.lib().crk_wana_workspace_bytes(n_utts, total_frames, total_samples)),
                                    "crk_wana_workspace_bytes")
        key = (int(order1), float(alpha))
        draws = int(max_frames) * DRAWS_PER_FRAME
        if draws > self._reserved.get(key, 0):
            check(_lib.lib().crk_wana_reserve(self.handle(*key), draws), "crk_wana_reserve")
            self._reserved[key] = draws
        return ws, draws

    # -- the stages
    def low_cut_batch(self, waves, cutoff=70):
        """The reference's ``low_cut_filter`` of each waveform cast to float32, as evaluate_mcd.py does: float64."""
        from scipy.signal import firwin

        if len(waves) < 1:
            raise ValueError("waves must be a non-empty list")
        slens = [size_of(w) for w in waves]
        if min(slens) < 1:
            raise ValueError("an empty waveform")
        self._on_device()
        if cutoff not in self._taps:
            taps = firwin(LOWCUT_TAPS, cutoff / (self.fs // 2), pass_zero=False)
            self._taps[cutoff] = torch.as_tensor(taps, dtype=torch.float64, device=self.device)
        x = self._waves(waves, torch.float32)
        soff = offsets(slens, self.device)
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
        sps = [f64(s, self.device) for s in sps]
        lens = [int(s.shape[0]) for s in sps]
        if not lens or min(lens) < 1 or any(s.dim() != 2 or s.shape[1] != K for s in sps):
            raise ValueError(f"spectral envelopes must be (frames >= 1, {K})")
        F = sum(lens)
        ws, _ = self.reserve(len(lens), F, 1, 1)
        sp = torch.cat(sps).contiguous()
        foff = offsets(lens, self.device)
        out = torch.empty(F, dtype=torch.float64, device=self.device)
        check(_lib.lib().crk_wana_npow(self.handle(), sp.data_ptr(), foff.data_ptr(), len(lens), F, out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream_ptr()), "crk_wana_npow")
        return list(out.split(lens))

    def npow_batch(self, waves, f0s):
        """sprocket ``FeatureExtractor.npow()`` of each waveform: list of (T,)."""
        return self.npow_of_sp_batch(self.cheaptrick_batch(waves, f0s))

    # -- aperiodicity
    def _d4c(self, waves, f0s, threshold, low_cut, want_ap, want_cap):
        check_d4c_fs(self.fs)
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must be a number")
        b = self._batch(waves, f0s)
        x = self._waves(waves, torch.float64) if low_cut is None else torch.cat(self.low_cut_batch(waves, low_cut))
        n, F, S = len(b["lens"]), sum(b["lens"]), sum(b["slens"])
        ws, draws = self.reserve_d4c(n, F, max(b["lens"]))
        dev = self.device
        ap = torch.empty(F, K, dtype=torch.float64, device=dev) if want_ap else None
        cap = torch.empty(F, n_bands(self.fs), dtype=torch.float64, device=dev) if want_cap else None
        check(_lib.lib().crk_wana_d4c(self.handle(), x.data_ptr(), b["f0"].data_ptr(), b["foff"].data_ptr(),
                                      b["soff"].data_ptr(), n, F, S, draws, threshold, _lib.ptr(ap), _lib.ptr(cap),
                                      ws.data_ptr(), ws.numel(), stream_ptr()), "crk_wana_d4c")
        return [None if t is None else list(t.split(b["lens"])) for t in (ap, cap)]

    def reserve_d4c(self, n_utts, total_frames, max_frames):
        """Workspace of a D4C call of that size and the randn table for utterances of up to max_frames frames (a frame
        draws at most ``d4c_draws_per_frame(fs)`` values).  Returns (workspace, the draw count the table covers)."""
        ws = self._workspace.ensure(int(_lib.lib().crk_wana_d4c_workspace_bytes(n_utts, total_frames)),
                                    "crk_wana_d4c_workspace_bytes")
        key = (1, 0.0)
        draws = int(max_frames) * d4c_draws_per_frame(self.fs)
        if draws > self._reserved.get(key, 0):
            check(_lib.lib().crk_wana_reserve(self.handle(*key), draws), "crk_wana_reserve")
            self._reserved[key] = draws
        return ws, draws

    def d4c_batch(self, waves, f0s, threshold=0.85, low_cut=None):
        """pyworld ``d4c(x, f0, time_axis, fs, threshold, fft_size=1024)`` of each waveform at its F0 contour: list of
        (T, 513).  ``low_cut`` as in ``mcep_batch`` (None: the waveform as given, float64)."""
        return self._d4c(waves, f0s, threshold, low_cut, True, False)[0]

    def codeap_batch(self, waves, f0s, threshold=0.85, low_cut=None):
        """sprocket ``FeatureExtractor.codeap()``: pyworld ``code_aperiodicity`` of the D4C table, list of (T, bands) in
        dB.  The 513-bin table is not formed: a band reads the two bins around its knot."""
        return self._d4c(waves, f0s, threshold, low_cut, False, True)[1]

    def code_aperiodicity_batch(self, aps):
        """pyworld ``code_aperiodicity(ap, fs)`` of each (T, 513) table: list of (T, bands) in dB."""
        bands = n_bands(self.fs)
        if bands < 1:
            raise ValueError(f"fs {self.fs}: WORLD's coded aperiodicity has no band below fs / 2 - 3 kHz")
        if bands > D4C_MAX_BANDS:
            raise ValueError(f"fs {self.fs}: {bands} bands; the kernels code up to {D4C_MAX_BANDS}")
        lens = [int(a.shape[0]) for a in aps]
        if not lens or min(lens) < 1 or any(a.dim() != 2 or a.shape[1] != K for a in aps):
            raise ValueError(f"aperiodicity tables must be (frames >= 1, {K})")
        self._on_device()
        ap = torch.cat([f64(a, self.device) for a in aps]).contiguous()
        cap = torch.empty(sum(lens), bands, dtype=torch.float64, device=self.device)
        check(_lib.lib().crk_wana_d4c_code(self.handle(), ap.data_ptr(), sum(lens), cap.data_ptr(), stream_ptr()),
              "crk_wana_d4c_code")
        return list(cap.split(lens))

    def d4c_frame_shapes_batch(self, waves, f0s, threshold=0.85):
        """Per utterance what the D4C kernels form before the general pass (debug; on the host): dict of origin, half_lt,
        half_gb, origin_c1, origin_c2, dc_limit, bound_half, bound_full, passed, lt_offset, gb_offset."""
        check_d4c_fs(self.fs)
        b = self._batch(waves, f0s)
        x = self._waves(waves, torch.float64)
        n, F, S = len(b["lens"]), sum(b["lens"]), sum(b["slens"])
        ws, draws = self.reserve_d4c(n, F, max(b["lens"]))
        dev = self.device
        shapes = torch.empty(F, 8, dtype=torch.int32, device=dev)
        passed = torch.empty(F, dtype=torch.int32, device=dev)
        lt, gb = (torch.empty(F, dtype=torch.int64, device=dev) for _ in range(2))
        check(_lib.lib().crk_wana_d4c_frame_shapes(self.handle(), x.data_ptr(), b["f0"].data_ptr(), b["foff"].data_ptr(),
                                                   b["soff"].data_ptr(), n, F, S, draws, float(threshold), shapes.data_ptr(),
                                                   passed.data_ptr(), lt.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), stream_ptr()), "crk_wana_d4c_frame_shapes")
        cuts = np.cumsum(b["lens"])[:-1]
        host = lambda t: np.split(t.cpu().numpy().astype(np.int64), cuts)  # noqa: E731
        names = ("origin", "half_lt", "half_gb", "origin_c1", "origin_c2", "dc_limit", "bound_half", "bound_full")
        out = []
        for s, p, a, g in zip(host(shapes), host(passed), host(lt), host(gb)):
            d = {k: s[:, i] for i, k in enumerate(names)}
            d.update(passed=p.astype(bool), lt_offset=a, gb_offset=g)
            out.append(d)
        return out

    def streaming(self, n_streams, max_samples, max_f0_in, f0_capacity=None, ring_capacity=None, f0_lag_ms=0.0, **kw):
        """A ``StreamingMcep`` at this analyzer's fs, shiftms and device: ``mcep_batch`` frame by frame from live
        streams.  Capacities not given are ``analysis_capacities`` for F0 rows that lag the signal by ``f0_lag_ms``;
        ``kw``: dim, alpha, low_cut, max_utt_frames, scaler, use_mcep_0th."""
        ring, queue = analysis_capacities(self.fs, self.shiftms, f0_lag_ms, max_samples, max_f0_in)
        return StreamingMcep(self.fs, self.shiftms, n_streams, max_samples, max_f0_in,
                             queue if f0_capacity is None else f0_capacity, ring if ring_capacity is None else ring_capacity,
                             device=self.device, **kw)

    def analyze_mcep(self, wave, f0, dim=34, alpha=0.455, low_cut=70):
        """One utterance: evaluate_mcd.py's ``get_world_features`` with the F0 given."""
        return self.mcep_batch([wave], [f0], dim, alpha, low_cut)[0]

    def frame_shapes_batch(self, f0s):
        """Per utterance the integers the CheapTrick kernel forms for every frame (debug; on the host): dict of origin,
        half, dc_limit, boundary, offset."""
        self._on_device()
        dev = self.device
        f0s = [f64(f, dev).reshape(-1) for f in f0s]
        lens = [int(f.numel()) for f in f0s]
        if not lens or min(lens) < 1:
            raise ValueError("an F0 contour needs at least 1 frame")
        F = sum(lens)
        foff = offsets(lens, dev)
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


    def analyze_batch(self, waves, minf0s, maxf0s, low_cut=70, return_ap=False):
        """sprocket ``FeatureExtractor.analyze`` for each waveform: the reference's low cut (None: none), Harvest at the
        utterance's search range, CheapTrick at that F0 and, with ``return_ap``, D4C.  Returns (f0s, sps) or
        (f0s, sps, aps): lists of (T,), (T, 513) and (T, 513)."""
        if return_ap:
            check_d4c_fs(self.fs)
        if self.shiftms != round(self.shiftms):
            raise ValueError(f"shiftms {self.shiftms}: Harvest takes an integer frame period")
        if self._harvest is None:
            self._harvest = HarvestF0(self.fs, int(self.shiftms), self.device)
        self._harvest.check(waves, minf0s, maxf0s)
        xs = [f64(w, self.device).reshape(-1) for w in waves] if low_cut is None else self.low_cut_batch(waves, low_cut)
        f0s = self._harvest.harvest_batch(xs, minf0s, maxf0s)
        if return_ap:
            return f0s, self.cheaptrick_batch(xs, f0s), self.d4c_batch(xs, f0s)
        return f0s, self.cheaptrick_batch(xs, f0s)


HARVEST_MAX_CHANNELS = 192  # F0_MAX_CH
HARVEST_SLOTS = 112  # candidates per 1 ms frame after the overlap (F0_NS)
HARVEST_MIN_SAMPLES = 64


class HarvestF0:
    """pyworld ``harvest(x, fs, f0_floor=minf0, f0_ceil=maxf0, frame_period=shiftms)`` for a ragged batch, each utterance
    with its own search range (the reference takes it per speaker from spkr.yml).  All float64, on the device."""

    def __init__(self, fs=22050, shiftms=5, device="cuda"):
        if int(fs) != fs or not 8000 <= int(fs) <= 48000:
            raise ValueError(f"fs {fs}: Harvest takes 8000 .. 48000 Hz")
        if int(shiftms) != shiftms or not 1 <= int(shiftms) <= 1000:
            raise ValueError(f"shiftms {shiftms}: Harvest takes an integer frame period in ms")
        self.fs, self.shiftms = int(fs), int(shiftms)
        self.device = torch.device(device)
        self.r = int(min(12, max(1, np.floor(self.fs / 8000.0 + 0.5))))
        self.fs_d = self.fs / self.r
        self._h = None
        self._workspace = Workspace(self.device)
        self._events = 0

    def __del__(self):
        release(self, "_h", "crk_f0_destroy")

    @property
    def _ws(self):
        return self._workspace.buf

    def handle(self):
        if self._h is None:
            require_gpu(self.device, "Harvest")
            from scipy.signal import cheby1

            b, a = cheby1(3, 0.05, 0.8 / self.r)
            co = (ctypes.c_double * 8)(*[float(v) for v in list(b) + list(a)])
            self._h = made(_lib.lib().crk_f0_create(self.fs, self.shiftms, co), "crk_f0_create")
        return self._h

    # -- inputs
    def check(self, waves, minf0s, maxf0s):
        """The supported envelope, before any launch."""
        n = len(waves)
        if n < 1 or len(minf0s) != n or len(maxf0s) != n:
            raise ValueError("waves, minf0s and maxf0s must be lists of the same non-zero length")
        for w, lo, hi in zip(waves, minf0s, maxf0s):
            if size_of(w) < HARVEST_MIN_SAMPLES:
                raise ValueError(f"a waveform of {size_of(w)} samples: Harvest needs at least {HARVEST_MIN_SAMPLES}")
            if not (np.isfinite(lo) and np.isfinite(hi) and 40.0 <= lo < hi <= 800.0):
                raise ValueError(f"search range {lo} .. {hi} Hz: Harvest takes 40 <= minf0 < maxf0 <= 800")

    def _layout(self, lens, minf0s, maxf0s):
        """The batch's integers, formed once on the host in float64 / int64 (the kernels trust them): utt, range, chan_bf,
        chan as include/crank_hip.h lays them out, and the totals."""
        fs, r, fs_d = self.fs, self.r, self.fs_d
        utt = np.zeros((len(lens), 12), np.int64)
        rng = np.zeros((len(lens), 2))
        bfs, chans = [], []
        s0 = d0 = t0 = c0 = r0 = o0 = e0 = 0
        for u, (n, lo, hi) in enumerate(zip(lens, minf0s, maxf0s)):
            floor, ceil = 0.9 * float(lo), 1.1 * float(hi)
            n_ch = 1 + int(np.log2(ceil / floor) * 40)
            if n_ch > HARVEST_MAX_CHANNELS:
                raise ValueError(f"{n_ch} channels: the kernels take {HARVEST_MAX_CHANNELS}")
            bf = floor * 2.0 ** ((np.arange(n_ch) + 1.0) / 40)
            nd, T1 = -(-n // r), int(1000.0 * n / fs) + 1
            To = int(1000.0 * n / fs / self.shiftms) + 1
            h = np.floor(2.0 * fs_d / bf + 0.5).astype(np.int64)
            # a band-passed signal crosses zero about bf times a second in each direction; 3 bf and 16 spare
            cap = np.minimum(nd, (3.0 * bf * nd / fs_d).astype(np.int64) + 16)
            off = e0 + 4 * (np.cumsum(cap) - cap)
            chans.append(np.stack([h, off, cap, np.full(n_ch, u, np.int64)], 1))
            bfs.append(bf)
            utt[u, :11] = (s0, n, d0, nd, t0, T1, c0, n_ch, r0, o0, To)
            rng[u] = (floor, ceil)
            s0, d0, t0, c0, r0, o0 = s0 + n, d0 + nd, t0 + T1, c0 + n_ch, r0 + n_ch * T1, o0 + To
            e0 += 4 * int(cap.sum())
        dev = self.device
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
        return dict(utt=up(utt), range=up(rng), chan_bf=up(np.concatenate(bfs)), chan=up(np.concatenate(chans)),
                    host=utt, n=len(lens), S=s0, D=d0, F=t0, C=c0, R=r0, O=o0, E=e0)

    def _batch(self, waves, minf0s, maxf0s):
        self.check(waves, minf0s, maxf0s)
        self.handle()
        xs = [f64(w, self.device).reshape(-1) for w in waves]
        L = self._layout([int(x.numel()) for x in xs], minf0s, maxf0s)
        L["x"] = torch.cat(xs).contiguous()
        self.reserve(L["n"], L["S"], L["F"], L["C"], L["E"])
        return L

    @staticmethod
    def _split(t, L, col):
        """Rows of t per utterance: col 3 decimated samples, 5 the 1 ms frames, 10 the output frames."""
        return list(t.split([int(v) for v in L["host"][:, col]]))

    # -- device resources
    def reserve(self, n_utts, total_samples, total_frames, total_channels, total_events):
        """Workspace for a call of that size and the handle's event storage (kept and grown, never per call)."""
        ws = self._workspace.ensure(int(_lib.lib().crk_f0_workspace_bytes(n_utts, total_samples, total_frames,
                                                                          total_channels)), "crk_f0_workspace_bytes")
        if total_events > self._events:
            check(_lib.lib().crk_f0_reserve(self.handle(), int(total_events)), "crk_f0_reserve")
            self._events = int(total_events)
        return ws

    @staticmethod
    def _status(status):
        if bool(status.any()):
            raise RuntimeError("Harvest: an event stream overflowed its capacity (more than 3 zero crossings per period of "
                               "a channel's centre frequency)")

    # -- the estimator
    def harvest_batch(self, waves, minf0s, maxf0s):
        """F0 contours (float64, int(1000 n / fs / shiftms) + 1 frames, 0 = unvoiced) of a ragged batch."""
        L = self._batch(waves, minf0s, maxf0s)
        f0 = torch.empty(L["O"], dtype=torch.float64, device=self.device)
        status = torch.empty(L["n"], dtype=torch.int32, device=self.device)
        ws = self._ws
        check(_lib.lib().crk_f0_harvest(self._h, L["x"].data_ptr(), L["utt"].data_ptr(), L["range"].data_ptr(),
                                        L["chan_bf"].data_ptr(), L["chan"].data_ptr(), L["n"], L["S"], L["C"], L["F"],
                                        L["E"], L["O"], f0.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                        stream_ptr()), "crk_f0_harvest")
        self._status(status)
        return self._split(f0, L, 10)

    def harvest(self, wave, minf0, maxf0):
        return self.harvest_batch([wave], [minf0], [maxf0])[0]

    # -- the stages alone (tests)
    def decimate_batch(self, waves, minf0s, maxf0s):
        """Per utterance the zero-phase low-passed, decimated, mean-free signal the band-pass filters run on."""
        L = self._batch(waves, minf0s, maxf0s)
        yd = torch.empty(L["D"], dtype=torch.float64, device=self.device)
        ws = self._ws
        check(_lib.lib().crk_f0_decimate(self._h, L["x"].data_ptr(), L["utt"].data_ptr(), L["n"], L["S"], yd.data_ptr(),
                                         ws.data_ptr(), ws.numel(), stream_ptr()), "crk_f0_decimate")
        return self._split(yd, L, 3)

    def raw_candidates_batch(self, waves, minf0s, maxf0s, decimated=None):
        """Per utterance the (channels, 1 ms frames) raw candidate table; ``decimated``: the signals to filter instead of
        this object's own decimation of ``waves``."""
        yds = self.decimate_batch(waves, minf0s, maxf0s) if decimated is None else [f64(y, self.device) for y in decimated]
        L = self._batch(waves, minf0s, maxf0s)
        if [int(y.numel()) for y in yds] != [int(v) for v in L["host"][:, 3]]:
            raise ValueError("decimated signals must have ceil(samples / r) samples")
        yd = torch.cat(yds).contiguous()
        raw = torch.empty(L["R"], dtype=torch.float64, device=self.device)
        status = torch.empty(L["n"], dtype=torch.int32, device=self.device)
        ws = self._ws
        check(_lib.lib().crk_f0_raw_candidates(self._h, yd.data_ptr(), L["utt"].data_ptr(), L["range"].data_ptr(),
                                               L["chan_bf"].data_ptr(), L["chan"].data_ptr(), L["n"], L["C"], L["F"],
                                               L["E"], raw.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                               stream_ptr()), "crk_f0_raw_candidates")
        self._status(status)
        h = L["host"]
        return [t.view(int(h[u, 7]), int(h[u, 5])) for u, t in enumerate(raw.split([int(v) for v in h[:, 7] * h[:, 5]]))]

    def _tables(self, L, tables):
        ts = [f64(t, self.device) for t in tables]
        for u, t in enumerate(ts):
            if tuple(t.shape) != (int(L["host"][u, 5]), HARVEST_SLOTS):
                raise ValueError(f"a candidate table must be (1 ms frames, {HARVEST_SLOTS}), got {tuple(t.shape)}")
        return torch.cat(ts).contiguous()

    def candidates_batch(self, waves, minf0s, maxf0s, raws):
        """Per utterance the (1 ms frames, 112) candidate table of a raw table: run means, overlapped over +-3 frames."""
        L = self._batch(waves, minf0s, maxf0s)
        rs = [f64(t, self.device) for t in raws]
        for u, t in enumerate(rs):
            if tuple(t.shape) != (int(L["host"][u, 7]), int(L["host"][u, 5])):
                raise ValueError("a raw table must be (channels, 1 ms frames)")
        raw = torch.cat([t.reshape(-1) for t in rs]).contiguous()
        out = torch.empty(L["F"], HARVEST_SLOTS, dtype=torch.float64, device=self.device)
        ws = self._ws
        check(_lib.lib().crk_f0_candidates(self._h, raw.data_ptr(), L["utt"].data_ptr(), L["n"], L["F"], out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream_ptr()), "crk_f0_candidates")
        return self._split(out, L, 5)

    def refine_batch(self, waves, minf0s, maxf0s, cands):
        """Per utterance (refined F0, score), each (1 ms frames, 112), of a candidate table on the undecimated waveform."""
        L = self._batch(waves, minf0s, maxf0s)
        c = self._tables(L, cands)
        ref, sc = torch.empty_like(c), torch.empty_like(c)
        check(_lib.lib().crk_f0_refine(self._h, L["x"].data_ptr(), c.data_ptr(), L["utt"].data_ptr(),
                                       L["range"].data_ptr(), L["n"], L["F"], ref.data_ptr(), sc.data_ptr(), stream_ptr()),
              "crk_f0_refine")
        return list(zip(self._split(ref, L, 5), self._split(sc, L, 5)))

    def contour_batch(self, waves, minf0s, maxf0s, refined, scores):
        """Per utterance the 1 ms contour of the refined candidate and score tables."""
        L = self._batch(waves, minf0s, maxf0s)
        c, s = self._tables(L, refined), self._tables(L, scores)
        f1 = torch.empty(L["F"], dtype=torch.float64, device=self.device)
        ws = self._ws
        check(_lib.lib().crk_f0_contour(self._h, c.data_ptr(), s.data_ptr(), L["utt"].data_ptr(), L["n"], L["F"],
                                        f1.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "crk_f0_contour")
        return self._split(f1, L, 5)


def continuous_f0_batch(f0s, device="cuda", return_filled=False):
    """The reference's ``convert_continuos_f0`` and feature.py:86-88 for each contour: (uv float32, cf0, lf0, lcf0), with
    its quirk: the ends of the contour are overwritten with the first / last voiced value before lf0 = log(f0 + 1e-10) is
    taken (``return_filled`` appends that contour).  A contour without a voiced frame raises ValueError (the reference:
    IndexError)."""
    dev = torch.device(device)
    require_gpu(dev, "continuous_f0_batch")
    f0s = [f64(f, dev).reshape(-1) for f in f0s]
    lens = [int(f.numel()) for f in f0s]
    if not lens or min(lens) < 1:
        raise ValueError("an F0 contour needs at least 1 frame")
    F = sum(lens)
    f0 = torch.cat(f0s).contiguous()
    foff = offsets(lens, dev)
    uv = torch.empty(F, dtype=torch.float32, device=dev)
    filled, cf0, lf0, lcf0 = (torch.empty(F, dtype=torch.float64, device=dev) for _ in range(4))
    status = torch.empty(len(lens), dtype=torch.int32, device=dev)
    check(_lib.lib().crk_f0_continuous(f0.data_ptr(), foff.data_ptr(), len(lens), F, uv.data_ptr(), filled.data_ptr(),
                                       cf0.data_ptr(), lf0.data_ptr(), lcf0.data_ptr(), status.data_ptr(), stream_ptr()),
          "crk_f0_continuous")
    bad = status.nonzero().reshape(-1).tolist()
    if bad:
        raise ValueError(f"utterance {bad[0]} has no voiced frame")
    outs = [t.split(lens) for t in ((uv, cf0, lf0, lcf0, filled) if return_filled else (uv, cf0, lf0, lcf0))]
    return [tuple(o[u] for o in outs) for u in range(len(lens))]


class StreamingF0:
    """``push`` takes the next samples of ``len(minf0s)`` independent streams, at most ``max_samples`` each per push, and
    returns the ``lcf0`` / ``uv`` rows ``StreamingConverter.push`` takes for a ``decoder_f0`` model, already converted to
    the target speaker and scaled (csrc/f0_stream_kernels.hip, ``crk_f0_stream_*``).  Stream i is
    row i of every argument and has its own search range.

    Harvest is not streamed bit for bit (its contour rules reach arbitrarily far along a voiced run): the 1 ms frames of a
    stream are cut into blocks of ``block_ms``, and block j's contour is Harvest - this module's kernels, through
    ``HarvestF0(fs, 1)`` - of the window from ``back_ms`` before the block to ``ahead_ms`` after it, truncated at the
    stream's start and, at the ``end`` flag, at its last sample.  A block is emitted by the push that completes its
    window, so the algorithmic latency is at most ``ahead_ms + block_ms``.  Output frame t sits at 1 ms frame
    ``t * shiftms`` (``HarvestF0``'s grid), or with ``hop_size`` at the 1 ms frame nearest ``t * hop_size`` samples (the
    centre of ``StreamingLogMel``'s centred frame t); give exactly one.  With ``low_cut`` the stream is first filtered by
    ``crank.utils.low_cut_filter`` with zero history at its start, bit for bit ``WorldAnalyzer.low_cut_batch`` of the whole
    signal.  The outputs do not depend on how the signal is cut into pushes.

    The sample history, the counts and the carry of every stream stay on the device; ``n_valid`` and ``end`` are host
    integers, so the host knows which blocks are ready.  A push with no ready block is one launch, nothing is read back,
    and an overflowing Harvest event stream sets a sticky flag that ``status()`` raises on.  A push cannot be captured in a
    graph (what it launches depends on the counts).  There is no torch or CPU fallback."""

    def __init__(self, fs, minf0s, maxf0s, spk_lcf0_mean, spk_lcf0_std, max_samples, shiftms=None, hop_size=None,
                 lcf0_scaler=None, back_ms=300, ahead_ms=100, block_ms=80, low_cut=70, device="cuda"):
        if (shiftms is None) == (hop_size is None):
            raise ValueError("the output frame grid is exactly one of shiftms and hop_size")
        if int(fs) != fs or not 8000 <= int(fs) <= 48000:
            raise ValueError(f"fs {fs}: Harvest takes 8000 .. 48000 Hz")
        fs = int(fs)
        grid = shiftms if hop_size is None else hop_size
        if int(grid) != grid or int(grid) < 1 or (shiftms is not None and grid > 1000):
            raise ValueError(f"shiftms / hop_size {grid}: a positive integer (shiftms at most 1000)")
        if hop_size is not None and 1000 * int(hop_size) < fs:
            raise ValueError(f"hop_size {hop_size}: below 1 ms at {fs} Hz, finer than the 1 ms contour")
        for name, ms in (("back_ms", back_ms), ("ahead_ms", ahead_ms), ("block_ms", block_ms)):
            if int(ms) != ms or not 1 <= int(ms) <= 10000 or (int(ms) * fs) % 1000:
                raise ValueError(f"{name} {ms}: whole milliseconds in 1 .. 10000 that end on a whole sample at {fs} Hz")
        if min(int(back_ms), int(block_ms)) * fs // 1000 < HARVEST_MIN_SAMPLES:
            raise ValueError(f"back_ms {back_ms}, block_ms {block_ms}: each window must hold Harvest's {HARVEST_MIN_SAMPLES} samples")
        if len(minf0s) < 1 or len(minf0s) != len(maxf0s):
            raise ValueError("minf0s and maxf0s must be lists of the same non-zero length")
        for lo, hi in zip(minf0s, maxf0s):
            if not (np.isfinite(lo) and np.isfinite(hi) and 40.0 <= lo < hi <= 800.0):
                raise ValueError(f"search range {lo} .. {hi} Hz: Harvest takes 40 <= minf0 < maxf0 <= 800")
        if int(max_samples) < 1:
            raise ValueError(f"max_samples = {max_samples}: must be at least 1")
        self.device = torch.device(device)
        require_gpu(self.device, "streaming F0")
        self.fs, self.n_streams, self.max_samples = fs, len(minf0s), int(max_samples)
        self.minf0s, self.maxf0s = [float(v) for v in minf0s], [float(v) for v in maxf0s]
        self.shiftms, self.hop_size = (int(shiftms), None) if hop_size is None else (None, int(hop_size))
        self.back_ms, self.ahead_ms, self.block_ms = int(back_ms), int(ahead_ms), int(block_ms)
        self.spk_mean = f64(spk_lcf0_mean, self.device).reshape(-1).contiguous()
        self.spk_std = f64(spk_lcf0_std, self.device).reshape(-1).contiguous()
        if self.spk_mean.numel() < 1 or self.spk_mean.numel() != self.spk_std.numel():
            raise ValueError("spk_lcf0_mean and spk_lcf0_std: one value per speaker each")
        self.lcf0_scaler = None if lcf0_scaler is None else (float(lcf0_scaler[0]), float(lcf0_scaler[1]))
        self._harvest = HarvestF0(fs, 1, self.device)
        self._rounds = {}  # (ready streams, window lengths) -> the round's tables; one entry in steady lock-step
        taps, n_taps = None, 0
        if low_cut is not None:
            from scipy.signal import firwin

            n_taps = LOWCUT_TAPS
            taps = (ctypes.c_double * n_taps)(*firwin(n_taps, low_cut / (fs // 2), pass_zero=False))
        h = ctypes.c_void_p()
        L = _lib.lib()
        with torch.cuda.device(self.device):
            self._harvest.handle()
            check(L.crk_f0_stream_create(fs, self.back_ms, self.ahead_ms, self.block_ms, self.shiftms or 0,
                                         self.hop_size or 0, taps, n_taps, self.n_streams, self.max_samples,
                                         ctypes.byref(h)), "crk_f0_stream_create")
            self._handle = made(h, "crk_f0_stream_create")
        self.max_frames = int(L.crk_f0_stream_max_frames(self._handle))
        self.max_rounds = int(L.crk_f0_stream_max_rounds(self._handle))

    def __del__(self):
        release(self, "_handle", "crk_f0_stream_destroy")

    @property
    def state_bytes(self):
        return int(_lib.lib().crk_f0_stream_state_bytes(self._handle))

    def reset(self, streams=None):
        """``streams`` (all of them by default) return to their start state; blocks not emitted yet are dropped."""
        reset_streams(self._handle, "crk_f0_stream_reset", streams, self.device)

    def status(self):
        """Synchronises; raises if a Harvest event stream overflowed in a window of any stream since its last reset."""
        flags = (ctypes.c_int * self.n_streams)()
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_f0_stream_status(self._handle, flags, stream_ptr()), "crk_f0_stream_status")
        bad = [s for s in range(self.n_streams) if flags[s] & 2]
        if bad:
            raise RuntimeError(f"streaming F0: the tables of streams {bad} did not fit the device's counts")
        HarvestF0._status(torch.tensor([f & 1 for f in flags]))

    def empty_outputs(self, S, raw=False, cv_f0=False):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns; ``raw`` (the contour) and
        ``cv_f0`` (exp(cv_lcf0) uv) are float64 and optional."""
        out = {"lcf0": torch.empty(S, self.max_frames, 1, device=self.device),
               "uv": torch.empty(S, self.max_frames, 1, device=self.device),
               "n_frames": torch.empty(S, dtype=torch.int32, device=self.device)}
        for name, want in (("raw", raw), ("cv_f0", cv_f0)):
            if want:
                out[name] = torch.empty(S, self.max_frames, 1, dtype=torch.float64, device=self.device)
        return out

    def _host_ints(self, v, S, C, what):
        if v is None:
            return None, None
        a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
        if a.shape != (S,) or a.dtype.kind not in "iub":
            raise ValueError(f"{what}: {S} host integers, got {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a, np.int32)
        if what == "n_valid" and (a.min() < 0 or a.max() > C):
            raise ValueError(f"n_valid: 0 .. {C}")
        return a, torch.as_tensor(a, device=self.device)

    def _spk(self, t, S, what):
        if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.int32
                or tuple(t.shape) != (S,)):
            raise ValueError(f"{what}: an int32 ({S},) tensor on the GPU")
        return t.contiguous()

    def _round(self, ids, lens):
        key = (tuple(ids), tuple(lens))
        r = self._rounds.get(key)
        if r is None:
            if len(self._rounds) >= 256:  # a stream's first back_ms and ragged schedules make new layouts; steady state one
                self._rounds.clear()
            L = self._harvest._layout(list(lens), [self.minf0s[s] for s in ids], [self.maxf0s[s] for s in ids])
            L["ids"] = torch.as_tensor(np.asarray(ids, np.int32), device=self.device)
            L["desc"] = _lib.F0StreamRound(L["ids"].data_ptr(), L["utt"].data_ptr(), L["range"].data_ptr(),
                                           L["chan_bf"].data_ptr(), L["chan"].data_ptr(), L["n"], L["S"], L["C"], L["F"],
                                           L["E"])
            r = self._rounds[key] = L
        return r

    def push(self, x, org_spk, cv_spk, n_valid=None, end=None, out=None):
        """x (S, C) float32 samples on the GPU; n_valid, end: S host integers (default: C, 0; n_valid may be 0) - the
        samples that count per stream and non-zero where this push ends the stream's utterance; org_spk, cv_spk int32
        (S,) on the GPU.  Returns ``lcf0`` and ``uv`` (S, max_frames, 1) float32 and ``n_frames`` (S,) int32: the frames
        written at the start of each stream's rows; frames past ``n_frames`` are not written.  Anything refused leaves
        outputs and state untouched.  out: buffers to write into (``empty_outputs``)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.device.type != "cuda" or x.dtype != torch.float32:
            raise ValueError("x: a float32 (S, C) tensor on the GPU")
        S, C = int(x.shape[0]), int(x.shape[1])
        if S != self.n_streams:
            raise ValueError(f"x: {S} rows for {self.n_streams} streams")
        x = x.contiguous()
        nv_h, nv_d = self._host_ints(n_valid, S, C, "n_valid")
        end_h, end_d = self._host_ints(end, S, C, "end")
        org_spk, cv_spk = self._spk(org_spk, S, "org_spk"), self._spk(cv_spk, S, "cv_spk")
        if out is None:
            out = self.empty_outputs(S)
        else:
            for name, dt in (("lcf0", torch.float32), ("uv", torch.float32), ("raw", torch.float64), ("cv_f0", torch.float64)):
                t = out.get(name)
                if t is None and name in ("raw", "cv_f0"):
                    continue
                if (t is None or t.device.type != "cuda" or t.dtype != dt or tuple(t.shape) != (S, self.max_frames, 1)
                        or not t.is_contiguous()):
                    raise ValueError(f"out[{name!r}]: {dt} ({S}, {self.max_frames}, 1) on the GPU (empty_outputs)")
            n = out.get("n_frames")
            if n is None or n.device.type != "cuda" or n.dtype != torch.int32 or tuple(n.shape) != (S,):
                raise ValueError(f"out['n_frames']: int32 ({S},) on the GPU (empty_outputs)")
        L = _lib.lib()
        ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        n_rounds = ctypes.c_int()
        round_n = (ctypes.c_int * self.max_rounds)()
        ids = (ctypes.c_int * (self.max_rounds * S))()
        lens = (ctypes.c_longlong * (self.max_rounds * S))()
        check(L.crk_f0_stream_plan(self._handle, ip(nv_h), ip(end_h), S, C, ctypes.byref(n_rounds), round_n, ids, lens),
              "crk_f0_stream_plan")
        rounds = [self._round(ids[r * S:r * S + round_n[r]], lens[r * S:r * S + round_n[r]]) for r in range(n_rounds.value)]
        descs = (_lib.F0StreamRound * max(len(rounds), 1))(*[r["desc"] for r in rounds])
        ws = None
        for r in rounds:
            ws = self._harvest.reserve(r["n"], r["S"], r["F"], r["C"], r["E"])
        mean, scale = self.lcf0_scaler or (0.0, 1.0)
        with torch.cuda.device(self.device):
            check(L.crk_f0_stream_push(
                self._handle, self._harvest.handle(), x.data_ptr(), C, ip(nv_h), ip(end_h), _lib.ptr(nv_d), _lib.ptr(end_d),
                S, C, descs, len(rounds), org_spk.data_ptr(), cv_spk.data_ptr(), self.spk_mean.data_ptr(),
                self.spk_std.data_ptr(), int(self.spk_mean.numel()), mean, scale, 1 if self.lcf0_scaler else 0,
                out["lcf0"].data_ptr(), out["uv"].data_ptr(), out["n_frames"].data_ptr(), _lib.ptr(out.get("raw")),
                _lib.ptr(out.get("cv_f0")), _lib.ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()),
                "crk_f0_stream_push")
        return out


WINDOW_REACH = FFTL // 2 - 1  # the furthest a CheapTrick window reaches either side of its frame's origin


def analysis_capacities(fs, shiftms, f0_lag_ms, max_samples, max_f0_in, reach=WINDOW_REACH):
    """(ring_capacity, f0_capacity) of a ``StreamingMcep`` that can never set flag 1 or 2 while the F0 rows lag the signal
    by at most ``f0_lag_ms`` and do not lead it.  With n the samples and ``rows`` the rows a stream holds after a push,
    origin_k frame k's origin and L = ceil(f0_lag_ms fs / 1000): every frame with origin_k + L <= n has its row, no row
    has origin_k > n, and an end push brings at most the rows the offline call takes (k shift <= n + shift).  Closed form,
    with M = max(L, reach + 1) and C = max_samples:

    * a frame leaves in the first push after which its row is there and n >= origin + reach + 1; before that push
      n <= origin + M - 1, so after it n <= origin + M - 1 + C while the window starts at origin - reach or later: the
      ring holds ``M - 1 + C + reach`` samples;
    * before a push every frame with origin + M <= n has left, after it the rows reach k shift <= n + C + shift at the
      most: the waiting rows have k shift within a closed span of C + M + shift - 0.499 (the 0.499: origins are k shift
      + 0.001 rounded to nearest), ``floor((C + M - 0.499) / shift) + 2`` rows.

    ``max_f0_in`` only bounds what a push can bring (at least one row).  tests/wana_stream_ref.py tries every history at
    toy sizes (``reach`` is the toy's window)."""
    fs, C = int(fs), int(max_samples)
    shift = float(shiftms) / 1000.0 * fs
    if not shift > 0.0 or C < 1 or int(max_f0_in) < 1 or not float(f0_lag_ms) >= 0.0 or int(reach) < 0:
        raise ValueError("analysis_capacities: shiftms > 0, max_samples >= 1, max_f0_in >= 1, f0_lag_ms >= 0")
    L = int(np.ceil(float(f0_lag_ms) * fs / 1000.0))
    M = max(L, int(reach) + 1)
    return M - 1 + C + int(reach), int(np.floor((C + M - 0.499) / shift)) + 2


class StreamingMcep:
    """``push`` takes the next samples and the next F0 rows of ``n_streams`` independent streams and returns the frames
    ``WorldAnalyzer.mcep_batch`` writes for the whole utterance at the same contour, bit for bit, as soon as each frame's
    window is complete (csrc/wana_stream_kernels.hip, ``crk_wana_stream_*``; the definition is tests/wana_stream_ref.py,
    DESIGN.md section 6o).  Stream i is row i of every argument; row k of a stream's utterance is frame k.

    Frame i leaves in the first push after which its F0 row has arrived and the stream holds ``origin_i + 512`` samples
    (the longest half window plus one: readiness never depends on the F0), or in the push whose ``end`` flag is set, where
    every waiting frame leaves with its window clamped at the stream's final length and the stream returns to its start
    state.  ``feats`` are the rows a generator takes: columns ``first:`` of the mel-cepstrum (``first`` = 0 with
    ``use_mcep_0th``, else 1), with ``scaler`` = (mean, scale) of ``dim + 1`` values as ``(mcep - mean) / scale`` in
    float64, rounded once to float32.

    The low-cut filtered signal (a power-of-two float64 ring of at least ``ring_capacity`` samples), the waiting F0 rows
    (at most ``f0_capacity``), the counts and the randn draw offset stay on the device; ``n_valid``, ``n_f0`` and ``end`` are
    device tensors and nothing is read back, so a push - four launches - can be captured in a graph.
    ``analysis_capacities`` gives capacities that cannot overflow for a given F0 lag.  Sticky flags, raised by
    ``status()``: 1 a frame's window start had left the ring (the frame is dropped and counted in ``n_dropped``), 2 the
    F0 queue overflowed (the newest rows are dropped and counted), 4 an utterance outgrew ``max_utt_frames`` (the randn
    table; the frame is emitted with the draw offset clamped), 8 rows past the end of the signal at an end push (dropped and counted),
    16 an F0 row not finite, negative or above fs / 4 (analysed as unvoiced).  There is no torch or CPU fallback."""

    FLAGS = {1: "a frame's window had left the sample ring (F0 rows came later than ring_capacity allows)",
             2: "the F0 queue overflowed (f0_capacity)",
             4: "an utterance drew past the randn table (max_utt_frames)",
             8: "F0 rows past the end of the signal at an end push",
             16: "an F0 row not finite, negative or above fs / 4"}

    def __init__(self, fs, shiftms, n_streams, max_samples, max_f0_in, f0_capacity, ring_capacity, dim=34, alpha=0.455,
                 low_cut=70, max_utt_frames=6000, scaler=None, use_mcep_0th=False, device="cuda"):
        if int(fs) != fs or not 8000 <= int(fs) <= 192000:
            raise ValueError(f"fs {fs}: the kernels take 8000 .. 192000 Hz")
        if not float(shiftms) > 0.0:
            raise ValueError(f"shiftms {shiftms}: must be positive")
        order1 = int(dim) + 1
        if not 1 <= order1 <= MAX_ORDER1:
            raise ValueError(f"dim + 1 = {order1}: the kernels take 1 .. {MAX_ORDER1} coefficients")
        if not abs(float(alpha)) < 1.0:
            raise ValueError(f"alpha {alpha}: the all-pass constant must lie in (-1, 1)")
        if not use_mcep_0th and order1 < 2:
            raise ValueError("dim 0 without use_mcep_0th leaves no feature column")
        sizes = dict(n_streams=n_streams, max_samples=max_samples, max_f0_in=max_f0_in, f0_capacity=f0_capacity,
                     ring_capacity=ring_capacity, max_utt_frames=max_utt_frames)
        for name, v in sizes.items():
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name} = {v}: must be a positive integer")
        if int(n_streams) > 65535 or max(int(f0_capacity), int(max_f0_in)) > 65536 or int(ring_capacity) > 1 << 26:
            raise ValueError("at most 65535 streams, 65536 F0 rows and a ring of 2^26 samples")
        if int(ring_capacity) < int(max_samples):
            raise ValueError(f"ring_capacity {ring_capacity} below max_samples {max_samples}")
        if int(max_utt_frames) * DRAWS_PER_FRAME > 1 << 31:
            raise ValueError(f"max_utt_frames {max_utt_frames}: the randn table holds 2^31 draws")
        self.device = torch.device(device)
        require_gpu(self.device, "streaming WORLD analysis")
        self.fs, self.shiftms, self.dim, self.alpha = int(fs), float(shiftms), int(dim), float(alpha)
        self.low_cut, self.use_mcep_0th = low_cut, bool(use_mcep_0th)
        self.first = 0 if self.use_mcep_0th else 1
        self.n_streams, self.max_samples, self.max_f0_in = int(n_streams), int(max_samples), int(max_f0_in)
        self.f0_capacity, self.ring_capacity, self.max_utt_frames = int(f0_capacity), int(ring_capacity), int(max_utt_frames)
        self._mean = self._scale = None
        if scaler is not None:
            self._mean, self._scale = (f64(v, self.device).reshape(-1).contiguous() for v in scaler)
            if self._mean.numel() != order1 or self._scale.numel() != order1:
                raise ValueError(f"scaler: mean and scale of {order1} values each")
        taps, n_taps = None, 0
        if low_cut is not None:
            from scipy.signal import firwin

            n_taps = LOWCUT_TAPS
            taps = (ctypes.c_double * n_taps)(*firwin(n_taps, low_cut / (self.fs // 2), pass_zero=False))
        L = _lib.lib()
        self._handle = self._wana = None
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            # a Wana handle of its own: its randn table is reserved once, here, and no offline call grows it
            self._wana = made(L.crk_wana_create(self.fs, FFTL, self.shiftms, self.alpha, order1), "crk_wana_create")
            check(L.crk_wana_stream_create(self._wana, taps, n_taps, self.n_streams, self.max_samples, self.max_f0_in,
                                           self.f0_capacity, self.ring_capacity, self.max_utt_frames,
                                           1 if self.use_mcep_0th else 0, ctypes.byref(h)), "crk_wana_stream_create")
            self._handle = made(h, "crk_wana_stream_create")
        self.max_frames = int(L.crk_wana_stream_max_frames(self._handle))

    def __del__(self):
        release(self, "_handle", "crk_wana_stream_destroy")
        release(self, "_wana", "crk_wana_destroy")

    @property
    def state_bytes(self):
        return int(_lib.lib().crk_wana_stream_state_bytes(self._handle))

    def reset(self, streams=None):
        """``streams`` (all of them by default) return to their start state; waiting frames are dropped, flags cleared."""
        reset_streams(self._handle, "crk_wana_stream_reset", streams, self.device)

    def flags(self):
        """Synchronises; the sticky flag word of every stream (host list)."""
        flags = (ctypes.c_int * self.n_streams)()
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_wana_stream_status(self._handle, flags, stream_ptr()), "crk_wana_stream_status")
        return list(flags)

    def status(self):
        """Synchronises; raises if any stream has set a flag since its last reset."""
        bad = {s: f for s, f in enumerate(self.flags()) if f}
        if bad:
            what = "; ".join(f"stream {s}: " + ", ".join(t for b, t in self.FLAGS.items() if f & b) for s, f in bad.items())
            raise RuntimeError(f"streaming WORLD analysis: {what}")

    def empty_outputs(self, S=None, sp=False):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns; ``sp`` (the spectral envelope) is
        optional."""
        S = self.n_streams if S is None else int(S)
        dev, F = self.device, self.max_frames
        out = {"mcep": torch.empty(S, F, self.dim + 1, dtype=torch.float64, device=dev),
               "feats": torch.empty(S, F, self.dim + 1 - self.first, dtype=torch.float32, device=dev)}
        if sp:
            out["sp"] = torch.empty(S, F, K, dtype=torch.float64, device=dev)
        for name in ("n_frames", "first", "n_dropped"):
            out[name] = torch.empty(S, dtype=torch.int32, device=dev)
        return out

    def _dev_ints(self, v, S, what):
        if v is None:
            return None
        if (not isinstance(v, torch.Tensor) or v.device.type != "cuda" or v.dtype != torch.int32
                or tuple(v.shape) != (S,)):
            raise ValueError(f"{what}: an int32 ({S},) tensor on the GPU (or None)")
        return v.contiguous()

    def push(self, x, f0, n_valid=None, n_f0=None, end=None, out=None):
        """x (S, C) float32 samples and f0 (S, R) or (S, R, 1) float64 rows (raw contour, 0 = unvoiced) on the GPU, C <=
        max_samples, R <= max_f0_in (either may be 0); n_valid, n_f0, end: int32 (S,) on the GPU or None (C, R, 0) - the
        samples and rows that count per stream and non-zero where this push ends the stream's utterance.  Returns
        ``mcep`` (S, max_frames, dim + 1) float64, ``feats`` (S, max_frames, dim + 1 - first) float32, ``sp`` (S,
        max_frames, 513) float64 if ``out`` holds one, and ``n_frames``, ``first``, ``n_dropped`` int32 (S,): the frames
        written at the start of each stream's rows; rows at and past ``n_frames`` are not written.  Anything refused
        leaves outputs and state untouched.  out: buffers to write into (``empty_outputs``)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.device.type != "cuda" or x.dtype != torch.float32:
            raise ValueError("x: a float32 (S, C) tensor on the GPU")
        S, C = int(x.shape[0]), int(x.shape[1])
        if S != self.n_streams:
            raise ValueError(f"x: {S} rows for {self.n_streams} streams")
        if C > self.max_samples:
            raise ValueError(f"x: {C} samples per push, max_samples is {self.max_samples}")
        if (not isinstance(f0, torch.Tensor) or f0.device.type != "cuda" or f0.dtype != torch.float64
                or f0.dim() not in (2, 3) or f0.shape[0] != S or (f0.dim() == 3 and f0.shape[2] != 1)):
            raise ValueError(f"f0: a float64 ({S}, R) or ({S}, R, 1) tensor on the GPU")
        R = int(f0.shape[1])
        if R > self.max_f0_in:
            raise ValueError(f"f0: {R} rows per push, max_f0_in is {self.max_f0_in}")
        x, f0 = x.contiguous(), f0.reshape(S, R).contiguous()
        n_valid, n_f0, end = (self._dev_ints(v, S, what) for v, what in ((n_valid, "n_valid"), (n_f0, "n_f0"), (end, "end")))
        if out is None:
            out = self.empty_outputs(S)
        else:
            F = self.max_frames
            for name, dt, w in (("mcep", torch.float64, self.dim + 1), ("feats", torch.float32, self.dim + 1 - self.first),
                                ("sp", torch.float64, K)):
                t = out.get(name)
                if t is None and name == "sp":
                    continue
                if (t is None or t.device.type != "cuda" or t.dtype != dt or tuple(t.shape) != (S, F, w)
                        or not t.is_contiguous()):
                    raise ValueError(f"out[{name!r}]: {dt} ({S}, {F}, {w}) on the GPU (empty_outputs)")
            for name in ("n_frames", "first", "n_dropped"):
                t = out.get(name)
                if t is None or t.device.type != "cuda" or t.dtype != torch.int32 or tuple(t.shape) != (S,):
                    raise ValueError(f"out[{name!r}]: int32 ({S},) on the GPU (empty_outputs)")
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_wana_stream_push(
                self._handle, x.data_ptr(), C, _lib.ptr(n_valid), C, f0.data_ptr(), R, _lib.ptr(n_f0), R, _lib.ptr(end), S,
                _lib.ptr(self._mean), _lib.ptr(self._scale), out["mcep"].data_ptr(), _lib.ptr(out.get("sp")),
                out["feats"].data_ptr(), out["n_frames"].data_ptr(), out["first"].data_ptr(), out["n_dropped"].data_ptr(),
                stream_ptr()), "crk_wana_stream_push")
        return out


def longest_pulse_interval(fs, shiftms, fftl=FFTL):
    """The most samples between two consecutive pulses of WORLD's time base away from an utterance's last frame.  A
    pulse lies at i where the phase total crosses a multiple of 2 pi inside sample i + 1's increment, so an interval is
    one more than the longest run of increments that sum to less than one cycle.  The slowest steady contour is the
    lowest F0 the time base keeps, L = fs // fftl + 1 (anything below is unvoiced and pulses at 500 Hz): fs / L
    increments per cycle.  Next to an unvoiced row a voiced row's F0 is interpolated down to half over the voiced half
    of the frame (frame fraction s < 0.5 falling, s > 0.5 rising; s = 0.5 is unvoiced); such a ramp falls short of L by
    L times the sum of min(s, 1 - s) over its samples: h (h + 1) / (2 shift) increments' worth with h = floor(shift / 2)
    when the frame holds a whole number `shift` of samples (a sample at s = 0.5 counted on both sides: its fraction is a
    rounded quotient), and below shift / 8 + 1 / 2 otherwise.  A run holds two ramps
    (one each end) and no more: between two others lies a whole unvoiced frame, whose 500 Hz repay both while 500 >=
    1.25 L.  So with d the two ramps' shortfall a run has fewer than fs / L + d increments: the interval is at most
    ceil(fs / L + d)."""
    fs, shift = int(fs), float(shiftms) / 1000.0 * int(fs)
    lowest = fs // int(fftl) + 1
    if not 500.0 >= 1.25 * lowest:
        raise ValueError(f"fs {fs}: the lowest F0 {lowest} Hz is too close to the unvoiced pulse rate")
    if shift == int(shift):
        h = int(shift) // 2
        d = h * (h + 1) / shift
    else:
        d = shift / 4.0 + 1.0
    return int(np.ceil(fs / lowest + d))


def synthesis_capacities(fs, shiftms, max_rows_in, f0_ceil=1000.0, fftl=FFTL):
    """Capacities of a ``StreamingWorldSynthesizer`` that can never set flag 1, 2, 32 or 64 while every F0 row lies within
    ``f0_ceil``: a dict of ``rows`` (the row queue), ``ring`` (the sample ring), ``pulses`` (the pulses one push adds)
    and ``out`` (the samples one push emits, ``max_out``).  Closed forms, with shift = shiftms fs / 1000 samples per
    frame, r = max_rows_in, a = fftl / 2 - 1 and b = fftl / 2 (a pulse at s covers s - a .. s + b), I =
    ``longest_pulse_interval`` and n(R) = ceil((R - 1) shift) the time front after R rows:

    * the front's own comparison of rounded times puts n(R) at that value or one past it, so a push moves the front by
      at most D = ceil(r shift) + 1, an end push by at most D_end = floor((r + 1) shift) (to y_length(R + r) = floor((R +
      r) shift); 1 more where shift is no whole number and the product can round up to one);
    * the pending pulse P has no successor among the n samples with a phase, and its successor comes within I: P >=
      n - 1 - I.  No sample at or past P - a has left, so before a push at most I + 1 + a samples with a phase are
      held.  A push needs the ring up to the reach of the last pulse it can find, n' - 2 + b, an end push up to
      y_length: ``ring`` = I + a + max(D + b, D_end + 1);
    * at an end everything held leaves: ``out`` = I + 1 + a + D_end (a push that does not end emits at most D + I);
    * a held row is one the pending pulse or the front still reads, from floor(P / fs / fp) on, a rounded quotient that
      can fall one below floor(P / shift); with n >= (R - 1) shift that is 2 + ceil((I + 1) / shift) rows, and a push
      brings r more: ``rows``;
    * a push adds at most the pulses it finds (and at an end the pending one besides).  D increments at no more than F =
      max(f0_ceil, 500) Hz (unvoiced samples pulse at 500 Hz) cross floor(D F / fs) + 1 multiples at the most.  In an
      utterance's last frame the extrapolated knot reaches 2 f0_ceil - or goes negative, which is slower: its
      increments sum to at most f0_ceil (shift + (shift + 1) / 2) / fs cycles, or 500 shift / fs: ``pulses`` = max(floor(D F
      / fs) + 1, floor(((D_end - shift) F + max(f0_ceil (3 shift + 1) / 2, 500 shift)) / fs) + 2).

    tests/test_wsyn_stream_cpu.py walks row histories at toy sizes (``fftl`` is the toy's) and finds, for each capacity,
    a history that overflows one unit less."""
    fs, r, N = int(fs), int(max_rows_in), int(fftl)
    shift = float(shiftms) / 1000.0 * fs
    if not shift >= 2.0 or r < 1 or not 0.0 < float(f0_ceil) <= fs / 4.0 or N < 4:
        raise ValueError("synthesis_capacities: shiftms fs / 1000 >= 2, max_rows_in >= 1, 0 < f0_ceil <= fs / 4")
    a, b = N // 2 - 1, N // 2
    interval = longest_pulse_interval(fs, shiftms, N)
    D = int(np.ceil(r * shift)) + 1
    D_end = int(np.floor((r + 1) * shift)) + (0 if shift == int(shift) else 1)
    F = max(float(f0_ceil), 500.0)
    last = max(float(f0_ceil) * (3.0 * shift + 1.0) / 2.0, 500.0 * shift)
    return {"rows": 2 + int(np.ceil((interval + 1) / shift)) + r,
            "ring": interval + a + max(D + b, D_end + 1),
            "pulses": max(int(np.floor(D * F / fs)) + 1, int(np.floor(((D_end - shift) * F + last) / fs)) + 2),
            "out": interval + 1 + a + D_end}


class StreamingWorldSynthesizer:
    """``push`` takes the next frame rows of ``n_streams`` independent streams - F0, mel-cepstrum, coded aperiodicity, and
    the rmcep rows with ``power_mod`` - and returns the samples ``WorldSynthesizer.synthesis_batch`` writes for the whole
    utterance, bit for bit under any cut, as soon as no pulse can reach them any more (csrc/world_stream_kernels.hip,
    ``crk_wsyn_stream_*``; the definition is tests/wsyn_stream_ref.py).  Stream i is row i of every
    argument; row k of a stream's utterance is frame k.

    After a push with R rows so far the time base has run over every sample whose frame is at most R - 2 (its next row
    is there).  A pulse at i is found when sample i + 1 has its phase and added when its successor is found, which gives
    its noise size.  Sample i leaves once i + 511 < B, B the pending pulse (found, not added) or else the last sample
    with a phase: readiness depends on the contour, so the count comes back as a device int32.  The push whose ``end``
    flag is set runs the front to ``y_length(R)`` with the offline clamp and extrapolated knot, adds the last pulse with
    noise size 0, emits every sample and returns the stream to its start state.

    The open rows, the phase carry, the pending pulse and a float64 ring of the samples still open stay on the device;
    ``n_rows`` and ``end`` are device tensors and nothing is read back, so a push - five launches, six with
    ``power_mod`` - can be captured in a graph.  ``capacities`` defaults to ``synthesis_capacities`` (which cannot
    overflow within ``f0_ceil``); the randn table is reserved once, for ``max_utt_samples``, on a handle of the stream's
    own.  Sticky flags, raised by ``status()``: 1 the sample ring overflowed, 2 the row queue overflowed (the newest rows
    are dropped and counted in ``n_dropped``), 4 an utterance outgrew ``max_utt_samples`` (the noise offset is clamped),
    8 an end push on a stream holding a single row (dropped and counted; nothing leaves), 16 an F0 row not finite,
    negative or above ``f0_ceil`` (synthesised as unvoiced), 32 a push found more pulses than its budget, 64 more samples
    were ready than ``max_out``.  There is no torch or CPU fallback."""

    FLAGS = {1: "the sample ring overflowed (capacities['ring'])",
             2: "the row queue overflowed (capacities['rows'])",
             4: "an utterance's noise offsets passed the randn table (max_utt_samples)",
             8: "an end push on a stream holding one row",
             16: "an F0 row not finite, negative or above f0_ceil",
             32: "a push found more pulses than its budget (capacities['pulses'])",
             64: "more samples were ready than max_out (capacities['out'])"}

    def __init__(self, fs, shiftms, n_streams, max_rows_in, order1, alpha, power_mod=False, f0_ceil=1000.0,
                 max_utt_samples=1 << 21, capacities=None, device="cuda"):
        if int(fs) != fs or n_bands(int(fs)) < 1 or int(fs) > 192000:
            raise ValueError(f"fs {fs}: WORLD's coded aperiodicity needs 12000 < fs <= 192000 Hz")
        if not float(shiftms) * int(fs) / 1000.0 >= 2.0:
            raise ValueError(f"shiftms {shiftms}: a frame must hold at least 2 samples")
        if not 1 <= int(order1) <= MAX_ORDER1:
            raise ValueError(f"order1 {order1}: the kernels take 1 .. {MAX_ORDER1} coefficients")
        if not abs(float(alpha)) < 1.0:
            raise ValueError(f"alpha {alpha}: the all-pass constant must lie in (-1, 1)")
        if not 0.0 < float(f0_ceil) <= int(fs) / 4.0:
            raise ValueError(f"f0_ceil {f0_ceil}: must lie in (0, fs / 4]")
        if capacities is None:
            capacities = synthesis_capacities(fs, shiftms, max_rows_in, f0_ceil)
        caps = {k: capacities[k] for k in ("rows", "ring", "pulses", "out")}
        sizes = dict(n_streams=n_streams, max_rows_in=max_rows_in, max_utt_samples=max_utt_samples, **caps)
        for name, v in sizes.items():
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name} = {v}: must be a positive integer")
        if (int(n_streams) > 65535 or int(max_rows_in) > 4096 or int(caps["rows"]) > 65536 or int(caps["pulses"]) > 65535
                or max(int(caps["ring"]), int(caps["out"])) > 1 << 24 or int(max_utt_samples) > 1 << 31):
            raise ValueError("at most 65535 streams, 4096 rows a push, 65536 queued rows, 65535 pulses a push, a ring and "
                             "an output of 2^24 samples, utterances of 2^31 samples")
        if int(caps["rows"]) < 2 or int(caps["ring"]) < FFTL:
            raise ValueError(f"capacities: at least 2 rows and a ring of {FFTL} samples")
        self.device = torch.device(device)
        require_gpu(self.device, "streaming WORLD synthesis")
        self.fs, self.shiftms, self.alpha, self.order1 = int(fs), float(shiftms), float(alpha), int(order1)
        self.bands = n_bands(self.fs)
        self.n_streams, self.max_rows_in, self.power_mod = int(n_streams), int(max_rows_in), bool(power_mod)
        self.f0_ceil, self.max_utt_samples = float(f0_ceil), int(max_utt_samples)
        self.capacities = {k: int(v) for k, v in caps.items()}
        L = _lib.lib()
        self._handle = self._world = None
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            # a World handle of its own: its randn table is reserved once, here, and no offline call grows it
            self._world = made(L.crk_world_create(self.fs, FFTL, self.shiftms, self.alpha, self.order1, self.bands, 1),
                               "crk_world_create")
            c = self.capacities
            check(L.crk_wsyn_stream_create(self._world, self.n_streams, self.max_rows_in, c["rows"], c["ring"], c["pulses"],
                                           c["out"], self.f0_ceil, 1 if self.power_mod else 0, self.max_utt_samples,
                                           ctypes.byref(h)), "crk_wsyn_stream_create")
            self._handle = made(h, "crk_wsyn_stream_create")
        self.max_out = int(L.crk_wsyn_stream_max_out(self._handle))

    def __del__(self):
        release(self, "_handle", "crk_wsyn_stream_destroy")
        release(self, "_world", "crk_world_destroy")

    def state_bytes(self):
        return int(_lib.lib().crk_wsyn_stream_state_bytes(self._handle))

    def reset(self, streams=None):
        """``streams`` (all of them by default) return to their start state; open samples are dropped, flags cleared."""
        reset_streams(self._handle, "crk_wsyn_stream_reset", streams, self.device)

    def flags(self):
        """Synchronises; the sticky flag word of every stream (host list)."""
        flags = (ctypes.c_int * self.n_streams)()
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_wsyn_stream_status(self._handle, flags, stream_ptr()), "crk_wsyn_stream_status")
        return list(flags)

    def status(self):
        """Synchronises; raises if any stream has set a flag since its last reset."""
        bad = {s: f for s, f in enumerate(self.flags()) if f}
        if bad:
            what = "; ".join(f"stream {s}: " + ", ".join(t for b, t in self.FLAGS.items() if f & b) for s, f in bad.items())
            raise RuntimeError(f"streaming WORLD synthesis: {what}")

    def empty_outputs(self):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns."""
        S, dev = self.n_streams, self.device
        return {"y": torch.empty(S, self.max_out, dtype=torch.float64, device=dev),
                "n_samples": torch.empty(S, dtype=torch.int32, device=dev),
                "n_dropped": torch.empty(S, dtype=torch.int32, device=dev)}

    def _rows(self, t, S, R, width, what):
        shape = (S, R) if width is None else (S, R, width)
        ok = isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.float64
        if ok and width is None and tuple(t.shape) == (S, R, 1):
            t = t.reshape(S, R)
        if not ok or tuple(t.shape) != shape:
            raise ValueError(f"{what}: a float64 {shape} tensor on the GPU")
        return t.contiguous()

    def _dev_ints(self, v, S, what):
        if v is None:
            return None
        if (not isinstance(v, torch.Tensor) or v.device.type != "cuda" or v.dtype != torch.int32
                or tuple(v.shape) != (S,)):
            raise ValueError(f"{what}: an int32 ({S},) tensor on the GPU (or None)")
        return v.contiguous()

    def push(self, f0, mcep, codeap, rmcep=None, n_rows=None, end=None, out=None, clip=False):
        """f0 (S, R) or (S, R, 1), mcep (S, R, order1), codeap (S, R, bands) and, with ``power_mod``, rmcep (S, R, order1):
        float64 on the GPU, R <= max_rows_in (R may be 0); n_rows, end: int32 (S,) on the GPU or None (R, 0) - the rows
        that count per stream and non-zero where this push ends the stream's utterance.  Returns ``y`` (S, max_out)
        float64 (not clipped; ``clip=True`` clamps to [-1, 1] as ``world2wav`` does) and ``n_samples``, ``n_dropped``
        int32 (S,): the samples written at the start of each stream's row and the rows dropped; columns at and past
        ``n_samples`` are not written.  Anything refused raises ValueError before any launch and leaves outputs and
        state untouched.  out: buffers to write into (``empty_outputs``)."""
        S = self.n_streams
        if not isinstance(f0, torch.Tensor) or f0.dim() not in (2, 3) or f0.shape[0] != S:
            raise ValueError(f"f0: a float64 ({S}, R) or ({S}, R, 1) tensor on the GPU")
        R = int(f0.shape[1])
        if R > self.max_rows_in:
            raise ValueError(f"f0: {R} rows per push, max_rows_in is {self.max_rows_in}")
        if (rmcep is not None) != self.power_mod:
            raise ValueError("rmcep: given exactly when the handle was made with power_mod")
        f0 = self._rows(f0, S, R, None, "f0")
        mcep = self._rows(mcep, S, R, self.order1, "mcep")
        codeap = self._rows(codeap, S, R, self.bands, "codeap")
        if rmcep is not None:
            rmcep = self._rows(rmcep, S, R, self.order1, "rmcep")
        n_rows, end = (self._dev_ints(v, S, what) for v, what in ((n_rows, "n_rows"), (end, "end")))
        if out is None:
            out = self.empty_outputs()
        else:
            t = out.get("y")
            if (t is None or t.device.type != "cuda" or t.dtype != torch.float64 or tuple(t.shape) != (S, self.max_out)
                    or not t.is_contiguous()):
                raise ValueError(f"out['y']: float64 ({S}, {self.max_out}) on the GPU (empty_outputs)")
            for name in ("n_samples", "n_dropped"):
                t = out.get(name)
                if t is None or t.device.type != "cuda" or t.dtype != torch.int32 or tuple(t.shape) != (S,):
                    raise ValueError(f"out[{name!r}]: int32 ({S},) on the GPU (empty_outputs)")
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_wsyn_stream_push(
                self._handle, f0.data_ptr(), mcep.data_ptr(), codeap.data_ptr(), _lib.ptr(rmcep), _lib.ptr(n_rows), R,
                _lib.ptr(end), S, 1 if clip else 0, out["y"].data_ptr(), out["n_samples"].data_ptr(),
                out["n_dropped"].data_ptr(), stream_ptr()), "crk_wsyn_stream_push")
        return out


def cap_postprocess_batch(caps, device="cuda"):
    """The recipe's post-processing of coded aperiodicity (feature.py:98-107) for each (T, bands) table: per band column
    every frame equal to the column's maximum is set to 0, then ``convert_continuos_f0`` of the column.  Returns per
    utterance (cap, ccap, cap_uv), float64 / float64 / float32; ``cap`` is the column as that function left it (its ends
    filled in place).  A column without a non-zero frame raises ValueError like ``continuous_f0_batch``."""
    dev = torch.device(device)
    caps = [f64(c, dev) for c in caps]
    if not caps or any(c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 1 for c in caps):
        raise ValueError("coded aperiodicity must be (frames >= 1, bands >= 1)")
    cols = []
    for c in caps:
        c = torch.where(c == c.max(0, keepdim=True).values, torch.zeros_like(c), c)
        cols += list(c.t().contiguous())
    outs = continuous_f0_batch(cols, dev, return_filled=True)
    res, i = [], 0
    for c in caps:
        o = outs[i:i + c.shape[1]]
        i += c.shape[1]
        res.append((torch.stack([t[4] for t in o], 1), torch.stack([t[1] for t in o], 1), torch.stack([t[0] for t in o], 1)))
    return res


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
