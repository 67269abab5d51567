"""The live conversion loop on the MI355X: pushes of samples in, pushes of converted samples out.

``LiveConverter`` owns the four streaming stages - ``StreamingLogMel`` and ``StreamingF0`` (the front ends),
``StreamingConverter`` (or, with ``lookahead=True``, ``LookaheadConverter`` for the recipe's default non-causal generators)
and ``StreamingVocoder`` - and what connects them on the device (csrc/join_kernels.hip,
DESIGN.md section 6m):

``FrameJoin`` (``crk_join_*``) pairs the rows of two inputs that arrive at different delays.  Log-mel frame t arrives
about ``n_fft / 2`` samples behind the signal, its ``[lcf0, uv]`` row up to ``ahead_ms + block_ms`` behind it: the rows of
the earlier side wait in a per-stream ring on the device until their partners arrive, and each push emits the pairs that
are complete.  No count is read back and nothing is allocated; a push is two launches and can be captured in a graph.

``crk_feat_renorm`` de-scales the decoded rows with crank's scaler and normalises them with the vocoder's statistics in
one launch, on the rows that count, with the bits of ``voc.normalize(dec * scale + mean)``.

There is no torch or CPU fallback.
"""
import ctypes

import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, stream_ptr
from crank_amd._ragged import made, release, require_gpu, reset_streams
from crank_amd.stream import LookaheadConverter, StreamingConverter, check_lookahead_conf, check_stream_conf


def join_capacities(fs, n_fft, hop, center, back_ms=300, ahead_ms=100, block_ms=80, max_samples=None):
    """``(cap_a, cap_b)``: the most log-mel frames that wait for their F0 rows, and the most F0 rows that wait for their
    log-mel frames, after any push - over every sample count n an utterance can stand at (pushes of 1 .. ``max_samples``
    samples reach every n, so the bound does not depend on ``max_samples``).  With L = ``n_fft / 2`` (centred; ``n_fft``
    uncentred), Bs / As the block and the look-ahead in samples and u = fs / 2000 (half a 1 ms frame: output frame t sits
    at the 1 ms frame nearest t * hop samples):

    * log-mel has emitted ``(n - L) // hop + 1`` frames (0 while n <= L centred, n < L uncentred; ``mlfb.frames_ready``);
    * J = ``max(0, (n - As) // Bs)`` blocks are complete and F0 has emitted the frames below 1 ms frame ``J * block_ms``:
      ``ceil((J * Bs - u) / hop)`` of them (``back_ms`` moves no boundary).

    Log-mel leads the most one sample before a block completes, n = (J + 1) Bs + As - 1:
    ``cap_a = floor((Bs + As - 1 - L + u) / hop) + 1``.  F0 leads the most at the sample that completes a block, n = J Bs + As:
    at most ``(L - As - u + hop - 1) / hop`` once log-mel has started, and what the blocks below log-mel's first frame
    hold before it.  Both are upper bounds that some n attains within one row."""
    fs, n_fft, hop = int(fs), int(n_fft), int(hop)
    Bs, As = int(block_ms) * fs // 1000, int(ahead_ms) * fs // 1000
    L = n_fft // 2 if center else n_fft
    den = 2000 * hop
    cap_a = max(0, (2000 * (Bs + As - 1 - L) + fs) // den + 1)

    def f0_rows(J):  # ceil((2000 J Bs - fs) / den)
        return 0 if J < 1 else -((fs - 2000 * J * Bs) // den)

    started = max(0, (2000 * (L - As + hop - 1) - fs - 1) // den)
    n_before = L if center else L - 1  # the last count at which log-mel has no frame
    before = f0_rows(max(0, (n_before - As) // Bs)) if n_before >= As else 0
    return int(cap_a), int(max(started, before))


def join_max_frames(cap_a, cap_b, max_in_a, max_in_b):
    """The most pairs one push can emit: no more than what waits plus what arrives, on either side."""
    return min(cap_a + max_in_a, cap_b + max_in_b)


def _int32(t, S, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.int32 or tuple(t.shape) != (S,):
        raise ValueError(f"{what}: an int32 ({S},) tensor on the GPU")
    return t.contiguous()


class FrameJoin:
    """``push`` takes the new rows of two inputs of up to ``n_streams`` streams - A rows of ``width_a`` floats, at most
    ``max_in_a`` a push, and B rows of ``width_b`` floats, at most ``max_in_b`` - and returns the pairs that are complete:
    row j of both outputs is pair ``first + j`` of the stream's utterance.  The surplus of the longer side waits on the
    device, at most ``cap_a`` / ``cap_b`` rows (either may be 0); more than that is lost and sets a sticky flag that
    ``status()`` raises on.  A stream's ``end`` flag discards its surplus (``n_dropped``) and starts it over at pair 0.
    Stream i is row i of every argument.  Two launches a push, nothing allocated, nothing read back: capturable."""

    def __init__(self, n_streams, width_a, width_b, max_in_a, max_in_b, cap_a, cap_b, device="cuda"):
        args = dict(n_streams=n_streams, width_a=width_a, width_b=width_b, max_in_a=max_in_a, max_in_b=max_in_b)
        for name, v in args.items():
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name} = {v}: must be at least 1")
        for name, v in (("cap_a", cap_a), ("cap_b", cap_b)):
            if int(v) != v or int(v) < 0:
                raise ValueError(f"{name} = {v}: must be at least 0")
        self.device = torch.device(device)
        require_gpu(self.device, "the frame join")
        self.n_streams, self.width_a, self.width_b = int(n_streams), int(width_a), int(width_b)
        self.max_in_a, self.max_in_b, self.cap_a, self.cap_b = int(max_in_a), int(max_in_b), int(cap_a), int(cap_b)
        h = ctypes.c_void_p()
        L = _lib.lib()
        with torch.cuda.device(self.device):
            check(L.crk_join_create(self.n_streams, self.width_a, self.width_b, self.max_in_a, self.max_in_b, self.cap_a,
                                    self.cap_b, ctypes.byref(h)), "crk_join_create")
            self._handle = made(h, "crk_join_create")
        self.max_frames = int(L.crk_join_max_frames(self._handle))
        if self.max_frames != join_max_frames(self.cap_a, self.cap_b, self.max_in_a, self.max_in_b):
            raise RuntimeError(f"crk_join_max_frames = {self.max_frames}")

    def __del__(self):
        release(self, "_handle", "crk_join_destroy")

    @property
    def state_bytes(self):
        return int(_lib.lib().crk_join_state_bytes(self._handle))

    def reset(self, streams=None):
        """``streams`` (all of them by default) drop what waits, start at pair 0 and clear their overflow flags."""
        ids = None if streams is None else [int(s) for s in streams]
        if ids is not None and any(not 0 <= i < self.n_streams for i in ids):
            raise ValueError(f"streams {ids}: stream ids are 0 .. {self.n_streams - 1}")
        reset_streams(self._handle, "crk_join_reset", ids, self.device)

    def status(self):
        """Synchronises; raises if a ring of any stream lost rows since the stream's last reset."""
        flags = (ctypes.c_int * self.n_streams)()
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_join_status(self._handle, flags, stream_ptr()), "crk_join_status")
        bad = [(s, "A" if flags[s] == 1 else "B" if flags[s] == 2 else "A and B") for s in range(self.n_streams) if flags[s]]
        if bad:
            raise RuntimeError(f"frame join: rows were lost (stream, ring) {bad}: more than cap_a = {self.cap_a} / cap_b = "
                               f"{self.cap_b} rows had to wait")

    def empty_outputs(self, S):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns."""
        dev = self.device
        return {"a": torch.empty(S, self.max_frames, self.width_a, device=dev),
                "b": torch.empty(S, self.max_frames, self.width_b, device=dev),
                "n_frames": torch.empty(S, dtype=torch.int32, device=dev),
                "first": torch.empty(S, dtype=torch.int32, device=dev),
                "n_dropped": torch.empty(S, dtype=torch.int32, device=dev)}

    def _rows(self, t, S, rows, width, what):
        """A float32 (S, rows, width) tensor on the GPU whose rows are contiguous and whose streams are `rows` rows apart."""
        if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32
                or tuple(t.shape) != (S, rows, width) or t.stride(2) != 1 or t.stride(1) < width
                or t.stride(0) != rows * t.stride(1)):
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: a float32 ({S}, {rows}, {width}) tensor on the GPU with contiguous rows, got {got}")
        return t

    def push(self, a, n_a, b, n_b, end=None, out=None):
        """a (S, max_in_a, width_a) and b (S, max_in_b, width_b) float32 (a row stride above the width is allowed: a slice
        of the last dimension), n_a / n_b (S,) int32: the rows at the start of each stream's block that are new; end (S,)
        int32, non-zero where this push ends the stream's utterance.  Returns ``a`` (S, max_frames, width_a), ``b``
        (S, max_frames, width_b), ``n_frames``, ``first`` and ``n_dropped`` (S,) int32; rows at and past ``n_frames`` are not
        written.  out: buffers to write into (``empty_outputs``), e.g. the static ones of a captured graph."""
        S = int(a.shape[0]) if isinstance(a, torch.Tensor) and a.dim() == 3 else -1
        if S < 1:
            raise ValueError("a: a float32 (S, max_in_a, width_a) tensor on the GPU")
        a = self._rows(a, S, self.max_in_a, self.width_a, "a")
        b = self._rows(b, S, self.max_in_b, self.width_b, "b")
        n_a, n_b = _int32(n_a, S, "n_a"), _int32(n_b, S, "n_b")
        end = None if end is None else _int32(end, S, "end")
        if out is None:
            out = self.empty_outputs(S)
        else:
            self._rows(out.get("a"), S, self.max_frames, self.width_a, "out['a']")
            self._rows(out.get("b"), S, self.max_frames, self.width_b, "out['b']")
            for name in ("n_frames", "first", "n_dropped"):
                _int32(out.get(name), S, f"out[{name!r}]")
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_join_push(
                self._handle, a.data_ptr(), a.stride(1), n_a.data_ptr(), b.data_ptr(), b.stride(1), n_b.data_ptr(),
                _lib.ptr(end), S, out["a"].data_ptr(), out["a"].stride(1), out["b"].data_ptr(), out["b"].stride(1),
                self.max_frames, out["n_frames"].data_ptr(), out["first"].data_ptr(), out["n_dropped"].data_ptr(),
                stream_ptr()), "crk_join_push")
        return out


def feat_renorm(x, scale, mean, vmean, vscale, n_valid, out):
    """out[s, j] = ((x[s, j] * scale + mean) - vmean) / vscale for j < n_valid[s] (``crk_feat_renorm``): x, out (S, C, D)
    float32 contiguous on the GPU, the four vectors (D,) float32, n_valid (S,) int32.  Rows past ``n_valid`` are not written."""
    if (x.dim() != 3 or x.device.type != "cuda" or x.dtype != torch.float32 or not x.is_contiguous() or out.shape != x.shape
            or out.device != x.device or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError("x, out: float32 (S, C, D) contiguous tensors on the GPU of one shape")
    S, C, D = (int(v) for v in x.shape)
    for name, v in (("scale", scale), ("mean", mean), ("vmean", vmean), ("vscale", vscale)):
        if v.device != x.device or v.dtype != torch.float32 or tuple(v.shape) != (D,) or not v.is_contiguous():
            raise ValueError(f"{name}: a float32 ({D},) tensor on the GPU")
    n_valid = _int32(n_valid, S, "n_valid")
    with torch.cuda.device(x.device):
        check(_lib.lib().crk_feat_renorm(x.data_ptr(), D, scale.data_ptr(), mean.data_ptr(), vmean.data_ptr(),
                                         vscale.data_ptr(), n_valid.data_ptr(), S, C, D, out.data_ptr(), D, stream_ptr()),
              "crk_feat_renorm")
    return out


class LiveConverter:
    """wave -> (log-mel, F0) -> join -> causal generator -> vocoder, for ``n_streams`` concurrent streams: ``push`` takes
    the next samples of every stream and returns the converted samples that have become computable.

    ``G`` a ``VQVAE2`` with ``causal: true``; ``layer`` the ``LogMelFilterBankLayer`` of its features (centred, with crank's
    ``mlfb`` scaler); ``vocoder`` a ``ParallelWaveGANVocoder`` loaded with its statistics; ``scaler`` crank's scaler dict
    (``scaler["mlfb"]``: ``mean_`` / ``scale_`` de-scale the decoded rows; ``scaler["lcf0"]``, when there, scales the F0
    rows).  With ``decoder_f0`` a ``StreamingF0`` on the layer's hop (``minf0s`` / ``maxf0s`` per stream,
    ``spk_lcf0_mean`` / ``spk_lcf0_std`` per speaker, ``**f0_grid``: ``fs``, ``back_ms``, ``ahead_ms``, ``block_ms``,
    ``low_cut``) and a ``FrameJoin`` sized by ``join_capacities``; the converter and the vocoder take
    ``max_chunk = join.max_frames`` frames a push.  Without it there is no F0 stage and no join.

    The emitted samples do not depend on how the signal is cut into pushes when ``noise`` is given (zeros, or the caller's
    own tape); noise drawn on the device (``noise=None``) is drawn per push, so the waveform then depends on the cut.
    ``lookahead=True`` takes a generator built with ``causal: false`` (the recipe's default) instead: the conversion stage is
    a ``LookaheadConverter`` that follows its input ``lookahead_frames(conf)`` frames behind (66 for the default shapes, 383
    ms at 22.05 kHz with hop 128 - ``latency_ms`` counts them) and ends utterances itself under the join's end flag.  A push
    that ends an utterance emits up to ``max_out = max_chunk + lookahead`` frames, so the vocoder stage, the noise argument
    and the output buffers are ``max_out`` frames (``max_out * hop`` samples) wide; without the keyword ``max_out`` is
    ``max_chunk``.  The samples are those of the offline forward of the whole utterance through the vocoder.

    Refused with NotImplementedError, naming the key: what ``check_stream_conf`` (``check_lookahead_conf`` with
    ``lookahead=True``) refuses, ``encoder_f0`` (it needs the
    unconverted rows, which ``StreamingF0`` does not emit in the same pass), an ``input_size`` that is not the layer's
    ``n_mels`` and an ``output_size`` that is not the vocoder's ``aux_channels``."""

    def __init__(self, G, layer, vocoder, n_streams, max_samples, minf0s=None, maxf0s=None, spk_lcf0_mean=None,
                 spk_lcf0_std=None, scaler=None, lookahead=False, **f0_grid):
        from crank_amd.world import StreamingF0

        conf = G.conf
        self.lookahead = bool(lookahead)
        (check_lookahead_conf if self.lookahead else check_stream_conf)(conf, G.spkr_size)
        if conf["encoder_f0"]:
            raise NotImplementedError("encoder_f0 = true: the encoder takes the unconverted lcf0 / uv rows, which StreamingF0 "
                                      "does not emit in the same pass")
        n_mels = int(layer.mel_basis.shape[1])
        if conf["input_size"] != n_mels:
            raise NotImplementedError(f"input_size = {conf['input_size']}: the log-mel layer emits n_mels = {n_mels}")
        if conf["output_size"] != vocoder.aux_channels:
            raise NotImplementedError(f"output_size = {conf['output_size']}: the vocoder takes aux_channels = "
                                      f"{vocoder.aux_channels}")
        if int(n_streams) < 1 or int(max_samples) < 1:
            raise ValueError(f"n_streams = {n_streams}, max_samples = {max_samples}: both must be at least 1")
        if vocoder.hop_size != layer.hop_size:
            raise ValueError(f"the vocoder's hop_size {vocoder.hop_size} is not the layer's {layer.hop_size}")
        if vocoder.mean is None:
            raise ValueError("the vocoder was loaded without stats: its normalisation is part of the loop")
        if scaler is None or "mlfb" not in scaler:
            raise ValueError("scaler: crank's scaler dict with the 'mlfb' entry that de-scales the decoded rows")
        self.device = dev = torch.device(vocoder.device)
        require_gpu(dev, "live conversion", "the vocoder's device")
        self.G, self.layer, self.vocoder, self.conf = G, layer, vocoder, conf
        self.n_streams, self.max_samples, self.hop_size = int(n_streams), int(max_samples), int(layer.hop_size)
        self.decoder_f0 = bool(conf["decoder_f0"])
        fs = f0_grid.pop("fs", None) or getattr(layer, "fs", None) or vocoder.sampling_rate
        if fs is None:
            raise ValueError("fs: the sampling rate is known to neither the layer nor the vocoder; give fs=")
        self.fs = int(fs)
        S = self.n_streams
        f32 = lambda v: torch.as_tensor(np.asarray(v, np.float32), device=dev).reshape(-1).contiguous()  # noqa: E731
        self._scale, self._mean = f32(scaler["mlfb"].scale_), f32(scaler["mlfb"].mean_)
        self._vmean, self._vscale = vocoder.mean.reshape(-1).contiguous(), vocoder.scale.reshape(-1).contiguous()
        D = conf["output_size"]
        if any(int(v.numel()) != D for v in (self._scale, self._mean, self._vmean, self._vscale)):
            raise ValueError(f"scaler['mlfb'] and the vocoder's statistics must hold output_size = {D} values each")
        self.sl = layer.streaming(S, self.max_samples)
        self.sf = self.join = None
        self._front_ms = 1000.0 * (layer.fft_size // 2 if layer.center else layer.fft_size) / self.fs
        if self.decoder_f0:
            if minf0s is None or maxf0s is None or len(minf0s) != S or len(maxf0s) != S:
                raise ValueError(f"minf0s, maxf0s: one search range per stream ({S}) for a decoder_f0 model")
            lc = scaler.get("lcf0") if hasattr(scaler, "get") else None
            lcf0_scaler = None if lc is None else (float(np.ravel(lc.mean_)[0]), float(np.ravel(lc.scale_)[0]))
            self.sf = sf = StreamingF0(self.fs, minf0s, maxf0s, spk_lcf0_mean, spk_lcf0_std, self.max_samples,
                                       hop_size=self.hop_size, lcf0_scaler=lcf0_scaler, device=dev, **f0_grid)
            cap_a, cap_b = join_capacities(self.fs, layer.fft_size, self.hop_size, layer.center, sf.back_ms, sf.ahead_ms,
                                           sf.block_ms, self.max_samples)
            self.join = FrameJoin(S, n_mels, 2, self.sl.max_frames, sf.max_frames, cap_a, cap_b, dev)
            self.max_chunk = self.join.max_frames
            self._front_ms = max(self._front_ms, sf.ahead_ms + sf.block_ms + 0.5)  # (a frame sits at the NEAREST 1 ms frame)
        else:
            if f0_grid:
                raise ValueError(f"{sorted(f0_grid)}: the F0 grid of a model without decoder_f0")
            self.max_chunk = self.sl.max_frames
        # the frames one push can hand to the vocoder: with look-ahead an end push flushes the frames the converter holds back
        if self.lookahead:
            self.conv = LookaheadConverter(G, S, self.max_chunk, dev)
            self.max_out = self.conv.max_out
        else:
            self.conv = StreamingConverter(G, S, self.max_chunk, dev)
            self.max_out = self.max_chunk
        self.sv = vocoder.streaming(S, self.max_out)
        # what a push writes between the stages: made here, never in push
        self._nv = torch.zeros(S, dtype=torch.int32, device=dev)
        self._end = torch.zeros(S, dtype=torch.int32, device=dev)
        self._spk = torch.zeros(S, dtype=torch.int64, device=dev)
        self._first = torch.zeros(S, dtype=torch.int32, device=dev)  # (without a join: the frames emitted so far)
        self._goes_on = torch.zeros(S, dtype=torch.bool, device=dev)  # (without a join: the stream's end flag is 0)
        self._fr = self.sl.empty_outputs(S)
        self._conv_out = self.conv.empty_outputs(S) if self.lookahead else self.conv.empty_outputs(S, self.max_chunk)
        self._c = torch.zeros(S, self.max_out, D, device=dev)
        self._zero_noise = None
        if self.decoder_f0:
            self._f0 = self.sf.empty_outputs(S)
            self._b = torch.zeros(S, self.sf.max_frames, 2, device=dev)
            self._j = self.join.empty_outputs(S)

    @property
    def state_bytes(self):
        stages = [self.sl, self.conv, self.sv] + ([self.sf, self.join] if self.decoder_f0 else [])
        return sum(st.state_bytes for st in stages)

    @property
    def latency_ms(self):
        """The worst-case algorithmic delay from a sample to its converted sample: the later front end (half a window,
        or F0's look-ahead plus a block), the generator's look-ahead when ``lookahead=True``, then the vocoder's look-ahead.
        The length of a push and the push times add to it."""
        frames = self.sv.lookahead + (self.conv.lookahead if self.lookahead else 0)
        return self._front_ms + 1000.0 * frames * self.hop_size / self.fs

    def reset(self, streams=None):
        """``streams`` (all of them by default) start a new utterance in every stage; what they hold is dropped."""
        for st in (self.sl, self.sf, self.join, self.conv, self.sv):
            if st is not None:
                st.reset(streams)
        if streams is None:
            self._first.zero_()
        else:
            for s in streams:
                self._first[int(s)].zero_()

    def status(self):
        """Synchronises; raises on StreamingF0's flags and on a join ring that lost rows."""
        if self.decoder_f0:
            self.sf.status()
            self.join.status()

    def empty_outputs(self, S, decoded=False):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns; ``decoded``: also the decoded rows
        (scaled, as the generator emits them), their count and the utterance's frame index of the first one."""
        out = self.sv.empty_outputs(S, self.max_out)
        if decoded:
            out.update(decoded=torch.empty(S, self.max_out, self.conf["output_size"], device=self.device),
                       n_frames=torch.empty(S, dtype=torch.int32, device=self.device),
                       first=torch.empty(S, dtype=torch.int32, device=self.device))
        return out

    def _host_ints(self, v, S, fill, what):
        if isinstance(v, torch.Tensor) and v.device.type != "cpu":
            raise ValueError(f"{what}: {S} HOST integers; a tensor on {v.device} would have to be read back every push")
        a = np.full(S, fill, np.int32) if v is None else np.asarray(v)
        if a.shape != (S,) or a.dtype.kind not in "iub":
            raise ValueError(f"{what}: {S} host integers, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a, np.int32)

    def push(self, wave, org_spk, cv_spk, n_valid=None, end=None, noise=None, out=None):
        """wave (S, C) float32 samples on the GPU, S = ``n_streams``, C <= ``max_samples``; org_spk / cv_spk int32 (S,) on
        the GPU; n_valid, end: S host integers (default: C, 0) - the samples that count per stream and non-zero where this
        push ends the stream's utterance; noise (S, max_out * hop) float32 or None (drawn on the device per push: the
        waveform then depends on the cut).  Returns ``wave`` (S, (max_out + the vocoder's lookahead) * hop) and ``n_out`` (S,) int32 as
        ``StreamingVocoder.push`` does; with ``out=`` buffers from ``empty_outputs(S, decoded=True)`` also ``decoded``,
        ``n_frames`` and ``first`` (the frame index of ``decoded[:, 0]`` in its utterance)."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.device.type != "cuda" or wave.dtype != torch.float32:
            raise ValueError("wave: a float32 (S, C) tensor on the GPU")
        S, C = int(wave.shape[0]), int(wave.shape[1])
        if S != self.n_streams or not 1 <= C <= self.max_samples:
            raise ValueError(f"wave: ({S}, {C}) for n_streams = {self.n_streams} and max_samples = {self.max_samples}")
        nv_h, end_h = self._host_ints(n_valid, S, C, "n_valid"), self._host_ints(end, S, 0, "end")
        if nv_h.min() < 0 or nv_h.max() > C:
            raise ValueError(f"n_valid: 0 .. {C}")
        org_spk, cv_spk = _int32(org_spk, S, "org_spk"), _int32(cv_spk, S, "cv_spk")
        N = self.max_out * self.hop_size
        if noise is not None and (noise.device.type != "cuda" or noise.dtype != torch.float32 or tuple(noise.shape) != (S, N)):
            raise ValueError(f"noise: a float32 ({S}, {N}) tensor on the GPU")
        if out is None:
            out = self.empty_outputs(S)
        with torch.cuda.device(self.device):
            self._nv.copy_(torch.from_numpy(nv_h))
            self._end.copy_(torch.from_numpy(end_h))
            self._spk.copy_(cv_spk)
            fr = self.sl.push(wave, n_valid=self._nv, end=self._end, out=self._fr)
            if self.decoder_f0:
                f0 = self.sf.push(wave, org_spk, cv_spk, n_valid=nv_h, end=end_h, out=self._f0)
                torch.cat([f0["lcf0"], f0["uv"]], dim=-1, out=self._b)
                j = self.join.push(fr["feats"], fr["n_frames"], self._b, f0["n_frames"], end=self._end, out=self._j)
                feats, n, first, cond = j["a"], j["n_frames"], j["first"], j["b"]
            else:
                feats, n, first, cond = fr["feats"], fr["n_frames"], self._first, None
            conv_out = self._conv_out if "decoded" not in out else dict(self._conv_out, decoded=out["decoded"])
            if self.lookahead:  # the converter ends utterances itself and says which frames leave
                res = self.conv.push(feats, None, None, self._spk, n_valid=n, end=self._end, lcf0_uv=cond, out=conv_out)
                dec, n, first = res["decoded"], res["n_out"], res["first"]
            else:
                dec = self.conv.push(feats, None, None, self._spk, n_valid=n, lcf0_uv=cond, out=conv_out)["decoded"]
            feat_renorm(dec, self._scale, self._mean, self._vmean, self._vscale, n, self._c)
            res = self.sv.push(self._c, noise, n_valid=n, end=self._end, out={"wave": out["wave"], "n_out": out["n_out"]})
            if "n_frames" in out:
                out["n_frames"].copy_(n)
                out["first"].copy_(first)
            if not self.decoder_f0 and not self.lookahead:  # the frames emitted so far, for `first`: 0 again behind an end
                torch.eq(self._end, 0, out=self._goes_on)
                self._first.add_(n).mul_(self._goes_on)
            ended = [] if self.lookahead else [s for s in range(S) if end_h[s]]
            if ended:  # the causal converter carries no end flag: its layers' history starts over
                self.conv.reset(ended)
        out["wave"], out["n_out"] = res["wave"], res["n_out"]
        return out
