"""Streaming conversion on the MI355X, with a causal generator and, at a fixed look-ahead, with a non-causal one:
``VQVAE2.forward`` (encoders, quantizers, decoders, no EMA update) for chunks of new frames of many concurrent streams, one
launch per push (csrc/stream_kernels.hip, ``crk_stream_*``).

A generator trained with ``causal: true`` computes frame t from input frames <= t, so conversion can follow a speaker who
is still talking.  ``StreamingConverter`` keeps, per stream and per residual layer, the last ``(kernel_size - 1) *
dilation`` frames of that layer's input on the device and computes only the new frames of a push.  The outputs do not
depend on how an utterance is cut into pushes - bit for bit - and equal the offline forward within fp32 rounding
(the kernels are fp32 throughout; ``CRANK_AMD_PRECISION`` does not apply).  There is no torch or CPU fallback.

The stages either side are in the package too: ``LogMelFilterBankLayer.streaming`` (``crank_amd.net.module.mlfb.
StreamingLogMel``) turns pushes of samples into the scaled log-mel frames that have become computable - its ``n_frames``
is this class's ``n_valid``, so build the converter with ``max_chunk >= StreamingLogMel.max_frames`` - and
``crank_amd.vocoder.StreamingVocoder`` turns the decoded chunks into sound, 16 frames behind them.

The ``lcf0`` / ``uv`` rows of a ``decoder_f0`` model come from ``crank_amd.world.StreamingF0``: Harvest on a window around
each block of 80 ms of the same pushes of samples, converted to the target speaker and scaled, at most 180 ms behind the
signal - ``crank_amd.live.LiveConverter`` holds the log-mel frames on the device until their F0 frames arrive and runs all
four stages in one call.

A generator trained with the recipe's default ``causal: false`` needs ``lookahead_frames(conf)`` frames after frame t for
its output at t (66 for the default shapes).  ``LookaheadConverter`` follows its input at that delay - the same slots as the
causal kernel, the residual taken from the same frame's input, edges masked by position, and per-stream rings on the device
for what waits for a delayed layer (csrc/stream_la_kernels.hip, ``crk_lstream_*``) - and returns the
offline forward of the whole utterance, bit for bit however it is cut.  ``LiveConverter(lookahead=True)`` is the live loop on it.

Where things live: ``_Converter`` owns what the two classes share - the native handle of one family of entry points
(``crk_stream_*`` / ``crk_lstream_*``), ``_prepare``, ``state_bytes``, ``reset`` (``_ragged.reset_streams``, the reset of
every streaming class of the package) and ``_inputs``, the checks of a push's arguments; a class keeps its outputs
(``empty_outputs``, ``LookaheadConverter._check_out``) and the library call of its ``push``.  On the native side
csrc/stream_common.h holds the handle base and the functions both families' entry points are made of.

What stays with the caller: ``encoder_f0`` conditioning (the same rows unconverted: ``StreamingF0`` with ``cv_spk = org_spk``),
and ``use_raw`` models, which ``check_stream_conf`` refuses: feed them scaled features.
"""
import ctypes

import torch

from crank_amd import _lib
from crank_amd._lib import StreamDesc, check, stream_ptr
from crank_amd._ragged import made, release, require_gpu, reset_streams

MAX_STACKS = 3
MAX_CHANNELS = 128      # inputs, outputs, conditioning and the last decoder's concatenated input (stream_kernels.hip)
MAX_KERNEL_SIZE = 5     # as net/module/pwg.py
MAX_HALO = 64           # (kernel_size - 1) * dilation of a layer: the rows in front of a tile in LDS
VQ_DIMS = (16, 32, 64, 128)  # as net/module/vqvae2.py


def receptive_chain(conf):
    """Frames of context in front of a frame that the generator's output depends on: the sum over the encoder and decoder
    stacks of (kernel_size - 1) * sum of dilations (132 for the default shapes: 48 + 18 + 18 + 48)."""
    total = 0
    for n in range(conf["n_vq_stacks"]):
        dil = sum(2 ** (i % conf["n_layers"][n]) for i in range(conf["n_layers"][n] * conf["n_layers_stacks"][n]))
        total += 2 * (conf["kernel_size"][n] - 1) * dil
    return total


def lookahead_frames(conf):
    """Frames after frame t that a generator built with ``causal: false`` needs for its output at t: half its receptive
    chain (66 for the default shapes) - what ``LookaheadConverter`` stays behind its input."""
    return receptive_chain(conf) // 2


def check_stream_conf(conf, spkr_size):
    """Refuse what cannot be streamed, naming the configuration key.  Touches neither the library nor the device."""
    if not conf["causal"]:
        raise NotImplementedError(
            f"causal = {conf['causal']}: only a generator built with causal: true can be streamed - this one's output at "
            f"frame t needs {lookahead_frames(conf)} frames after t (its stacks look as far ahead as behind); "
            f"LookaheadConverter follows it at that delay")
    _check_limits(conf, spkr_size, odd_kernels=False)


def check_lookahead_conf(conf, spkr_size):
    """Refuse what ``LookaheadConverter`` cannot follow, naming the configuration key: the limits of ``check_stream_conf``,
    ``causal: true`` (that is ``StreamingConverter``'s) and even kernel sizes (their padding is not symmetric).  Touches
    neither the library nor the device."""
    if conf["causal"]:
        raise NotImplementedError(f"causal = {conf['causal']}: a generator built with causal: true needs no look-ahead; "
                                  f"StreamingConverter streams it without delay")
    _check_limits(conf, spkr_size, odd_kernels=True)


def _check_limits(conf, spkr_size, odd_kernels):
    """The shapes the streaming kernels take, causal or not."""
    if conf["use_raw"]:
        raise NotImplementedError("use_raw = true: the on-the-fly log-mel layer is not streamed; feed scaled features")
    nst = conf["n_vq_stacks"]
    if not 1 <= nst <= MAX_STACKS:
        raise NotImplementedError(f"n_vq_stacks = {nst}: the streaming kernel takes 1 .. {MAX_STACKS}")
    for n in range(nst):
        if conf["emb_dim"][n] not in VQ_DIMS:
            raise NotImplementedError(f"emb_dim[{n}] = {conf['emb_dim'][n]}: the streaming kernel supports emb_dim in {VQ_DIMS}")
        k = conf["kernel_size"][n]
        if not 1 <= k <= MAX_KERNEL_SIZE:
            raise NotImplementedError(f"kernel_size[{n}] = {k}: the streaming kernel takes 1 .. {MAX_KERNEL_SIZE}")
        if odd_kernels and k % 2 == 0:
            raise NotImplementedError(f"kernel_size[{n}] = {k}: the look-ahead kernel takes odd kernel sizes (a non-causal "
                                      f"layer pads (k - 1) / 2 * dilation frames on both sides)")
        halo = (k - 1) * 2 ** (conf["n_layers"][n] - 1)
        if halo > MAX_HALO:
            raise NotImplementedError(f"n_layers[{n}] = {conf['n_layers'][n]} with kernel_size[{n}] = {k}: a layer would keep "
                                      f"{halo} frames of history, above the {MAX_HALO} the streaming kernel holds")
    d_aux = (2 if conf["decoder_f0"] else 0) + (conf["spkr_embedding_size"] if conf["use_spkr_embedding"] else spkr_size)
    for key, ch in (("input_size", conf["input_size"]), ("output_size", conf["output_size"]),
                    ("emb_dim", sum(conf["emb_dim"][:nst])),
                    ("spkr_embedding_size" if conf["use_spkr_embedding"] else "use_spkr_embedding", d_aux)):
        if not 1 <= ch <= MAX_CHANNELS:
            raise NotImplementedError(f"{key}: {ch} channels (for emb_dim: their sum; for the speaker key: the last decoder's "
                                      f"conditioning), the streaming kernel takes 1 .. {MAX_CHANNELS}")
    if spkr_size < 1:
        raise NotImplementedError(f"spkr_size = {spkr_size}: the last decoder is conditioned on a speaker")


def _stream_desc(G, causal):
    """``crk_stream_desc`` of generator ``G``: shapes, and element offsets into its flat parameter block."""
    conf, nst = G.conf, G.conf["n_vq_stacks"]
    d = StreamDesc()
    d.n_stacks, d.in_ch, d.out_ch = nst, conf["input_size"], conf["output_size"]
    for n in range(nst):
        d.emb_dim[n], d.emb_size[n] = conf["emb_dim"][n], conf["emb_size"][n]
        d.cb_off[n] = G.quantizers[n].cb_offset
        d.enc_base[n], d.dec_base[n] = G.encoders[n].base, G.decoders[n].base
    d.causal, d.enc_f0, d.dec_f0 = causal, int(bool(conf["encoder_f0"])), int(bool(conf["decoder_f0"]))
    d.spk_onehot = int(not conf["use_spkr_embedding"])
    d.spk_dim = conf["spkr_embedding_size"] if conf["use_spkr_embedding"] else G.spkr_size
    d.n_spk = G.spkr_size
    d.spk_off = G.emb_offset if conf["use_spkr_embedding"] else 0
    return d


class _Converter:
    """What the two converters share: the native handle of one family (entry points ``<_prefix>_*``, a ``crk_stream_desc``
    with ``causal = _causal``, configurations ``_check_conf`` lets through), its weights' preparation, ``reset`` and the
    checks of a push's inputs.  A subclass adds its outputs and the one library call of ``push``."""
    _prefix = _causal = _check_conf = _what = None

    def __init__(self, G, n_streams, max_chunk, device="cuda"):
        conf = G.conf
        self._check_conf(conf, G.spkr_size)
        if n_streams < 1 or max_chunk < 1:
            raise ValueError(f"n_streams = {n_streams}, max_chunk = {max_chunk}: both must be at least 1")
        self.device = torch.device(device)
        require_gpu(self.device, self._what, "the converter's device")
        self.G, self.conf, self.n_streams, self.max_chunk = G, conf, int(n_streams), int(max_chunk)
        self.nst = nst = conf["n_vq_stacks"]
        self.dims = [conf["emb_dim"][n] for n in range(nst)]
        d = _stream_desc(G, causal=self._causal)
        nets = ctypes.c_void_p * nst
        enc = nets(*[G.encoders[n].net.handle for n in range(nst)])
        dec = nets(*[G.decoders[n].net.handle for n in range(nst)])
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self._call("create", ctypes.byref(d), enc, dec, ctypes.byref(h))
            self._handle = made(h, self._prefix + "_create")
            self._call("reserve", self._handle, self.n_streams, self.max_chunk)
        self._prepared = None
        self._ptrs = ctypes.c_void_p * nst

    def _call(self, name, *args):
        """The family's entry point ``name``; RuntimeError unless it returns CRK_OK."""
        entry = f"{self._prefix}_{name}"
        check(getattr(_lib.lib(), entry)(*args), entry)

    def __del__(self):
        release(self, "_handle", self._prefix + "_destroy")

    @property
    def state_bytes(self):
        """What the handle keeps on the device for ``n_streams`` streams: layer history and, behind a look-ahead, frame
        counters and the rings of what waits for a delayed layer."""
        return int(getattr(_lib.lib(), self._prefix + "_state_bytes")(self._handle, self.n_streams))

    def _prepare(self):
        """Effective weights for the generator's current parameters; again after any parameter or codebook write."""
        G = self.G
        key = (G.version, G.codebook_epoch, G.flat.data_ptr())
        if key != self._prepared:
            self._call("prepare", self._handle, G.flat.data_ptr(), G.version, stream_ptr())
            self._prepared = key

    def reset(self, streams=None):
        """``streams`` (all of them by default) drop what they hold - the carried history, behind a look-ahead also the
        frame count: their next frame is frame 0 of an utterance."""
        reset_streams(self._handle, self._prefix + "_reset", streams, self.device)

    def _f32(self, t, S, C, last, what):
        if t is None:
            raise ValueError(f"{what} is required by this configuration")
        if t.device.type != "cuda" or t.dtype != torch.float32 or tuple(t.shape) != (S, C, last):
            raise ValueError(f"{what}: a float32 ({S}, {C}, {last}) tensor on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.contiguous()

    def _inputs(self, feats, lcf0, uv, spkr, n_valid, enc_lcf0_uv, lcf0_uv, end=None):
        """The inputs of a push, checked: S, C, feats, the decoder's and the encoder's (S, C, 2) conditioning rows (None
        where the model takes none) and n_valid, end as int32 (None stays None)."""
        S, C = int(feats.shape[0]), int(feats.shape[1])
        conf = self.conf
        feats = self._f32(feats, S, C, conf["input_size"], "feats")
        dcond = None
        if lcf0_uv is not None:
            if lcf0 is not None or uv is not None:
                raise ValueError("lcf0_uv: the packed rows replace lcf0 and uv; give one form, not both")
            if not conf["decoder_f0"]:
                raise ValueError("lcf0_uv: this model has decoder_f0 = false and takes no F0 rows")
            dcond = self._f32(lcf0_uv, S, C, 2, "lcf0_uv")
        elif conf["decoder_f0"]:
            dcond = torch.cat([self._f32(lcf0, S, C, 1, "lcf0"), self._f32(uv, S, C, 1, "uv")], dim=-1)
        econd = self._f32(enc_lcf0_uv, S, C, 2, "enc_lcf0_uv") if conf["encoder_f0"] else None
        if spkr.device.type != "cuda" or spkr.dtype != torch.int64 or tuple(spkr.shape) != (S,):
            raise ValueError(f"spkr: an int64 ({S},) tensor on the GPU, got {spkr.dtype} {tuple(spkr.shape)} on {spkr.device}")
        flags = []
        for name, v in (("n_valid", n_valid), ("end", end)):
            if v is not None:
                if v.device.type != "cuda" or tuple(v.shape) != (S,):
                    raise ValueError(f"{name}: an integer ({S},) tensor on the GPU")
                v = v.to(torch.int32).contiguous()
            flags.append(v)
        return (S, C, feats, dcond, econd, *flags)


class StreamingConverter(_Converter):
    """``push`` runs generator ``G`` (a ``VQVAE2`` with ``causal: true``) on the next frames of up to ``n_streams``
    independent streams, at most ``max_chunk`` frames each per push.  Stream i is row i of every argument."""
    _prefix, _causal, _check_conf, _what = "crk_stream", 1, staticmethod(check_stream_conf), "streaming conversion"

    def empty_outputs(self, S, C):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns."""
        dev = self.device
        return {"decoded": torch.empty(S, C, self.conf["output_size"], device=dev),
                "qidx": [torch.empty(S, C, dtype=torch.int64, device=dev) for _ in range(self.nst)],
                "encoded": [torch.empty(S, C, D, device=dev) for D in self.dims]}

    def push(self, feats, lcf0, uv, spkr, n_valid=None, enc_lcf0_uv=None, out=None, lcf0_uv=None):
        """feats (S, C, input_size) scaled features, lcf0 / uv (S, C, 1) the scaled (already converted) F0 contour and the
        voicing flags - or, with both of them None, lcf0_uv (S, C, 2) the two packed as ``FrameJoin`` emits them, which is
        passed to the kernel as it is (giving both forms, or lcf0_uv to a model without ``decoder_f0``, is a ValueError) -,
        spkr (S,) int64 target speakers, n_valid (S,)
        frames that count per stream (default: C), enc_lcf0_uv (S, C, 2) the encoder's conditioning when ``encoder_f0``.
        Returns ``decoded`` (S, C, output_size),
        ``qidx`` [(S, C) int64 per stack, bottom first] and ``encoded`` [(S, C, emb_dim) per stack: the quantizer's input] -
        the keys of ``VQVAE2.make_dict``.  Rows at and past ``n_valid`` are not written.  out: buffers to write into
        (``empty_outputs``), e.g. the static ones of a captured graph."""
        S, C, feats, dcond, econd, n_valid, _ = self._inputs(feats, lcf0, uv, spkr, n_valid, enc_lcf0_uv, lcf0_uv)
        out = self.empty_outputs(S, C) if out is None else out
        with torch.cuda.device(self.device):
            self._prepare()
            self._call("push", self._handle, feats.data_ptr(), feats.shape[-1], _lib.ptr(dcond), 2, _lib.ptr(econd), 2,
                       spkr.data_ptr(), _lib.ptr(n_valid), S, C, out["decoded"].data_ptr(),
                       self._ptrs(*[t.data_ptr() for t in out["qidx"]]), self._ptrs(*[t.data_ptr() for t in out["encoded"]]),
                       stream_ptr())
        return out


class LookaheadConverter(_Converter):
    """``push`` runs generator ``G`` (a ``VQVAE2`` with ``causal: false``, the recipe's default) on the next frames of up to
    ``n_streams`` independent streams, at most ``max_chunk`` frames each per push, and returns the frames whose whole
    future context has arrived: it follows its input ``lookahead = lookahead_frames(conf)`` frames behind (66 for the
    default shapes: 383 ms at 22.05 kHz with hop 128).  After T frames of an utterance ``max(0, T - lookahead)`` have been
    emitted; a push with the stream's ``end`` flag emits the rest - up to ``max_out = max_chunk + lookahead`` rows, at the
    cost of ``n_valid + lookahead`` frames - and starts the stream over.  What is emitted is the offline forward of the
    whole utterance, bit for bit however it is cut into pushes (csrc/stream_la_kernels.hip, ``crk_lstream_*``; DESIGN.md
    section 6n).  Stream i is row i of every argument.  There is no torch or CPU fallback."""
    _prefix, _causal, _check_conf = "crk_lstream", 0, staticmethod(check_lookahead_conf)
    _what = "look-ahead streaming conversion"

    def __init__(self, G, n_streams, max_chunk, device="cuda"):
        super().__init__(G, n_streams, max_chunk, device)
        self.lookahead = lookahead_frames(self.conf)
        self.max_out = self.max_chunk + self.lookahead
        la = int(_lib.lib().crk_lstream_lookahead(self._handle))
        if la != self.lookahead:
            raise RuntimeError(f"crk_lstream_lookahead = {la}, not {self.lookahead}")

    def empty_outputs(self, S):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns: ``max_out`` rows per stream."""
        dev, R = self.device, self.max_out
        return {"decoded": torch.empty(S, R, self.conf["output_size"], device=dev),
                "qidx": [torch.empty(S, R, dtype=torch.int64, device=dev) for _ in range(self.nst)],
                "encoded": [torch.empty(S, R, D, device=dev) for D in self.dims],
                "n_out": torch.empty(S, dtype=torch.int32, device=dev),
                "first": torch.empty(S, dtype=torch.int32, device=dev)}

    def _check_out(self, out, S):
        """Every buffer of ``out`` as ``empty_outputs(S)`` makes it: the kernel writes up to ``max_out`` rows per stream."""
        R = self.max_out
        want = [("decoded", out.get("decoded"), (S, R, self.conf["output_size"]), torch.float32),
                ("n_out", out.get("n_out"), (S,), torch.int32), ("first", out.get("first"), (S,), torch.int32)]
        for key, dims, dtype in (("qidx", [()] * self.nst, torch.int64), ("encoded", [(D,) for D in self.dims], torch.float32)):
            bufs = out.get(key)
            if not isinstance(bufs, (list, tuple)) or len(bufs) != self.nst:
                raise ValueError(f"out[{key!r}]: a list of {self.nst} tensors (empty_outputs({S}))")
            want += [(f"{key}[{n}]", t, (S, R) + dims[n], dtype) for n, t in enumerate(bufs)]
        for name, t, shape, dtype in want:
            if (not isinstance(t, torch.Tensor) or t.device != out["decoded"].device or t.device.type != "cuda"
                    or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
                got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"out[{name}]: a contiguous {dtype} {shape} tensor on the GPU, max_out = {R} rows per stream "
                                 f"(empty_outputs({S})), got {got}")

    def push(self, feats, lcf0, uv, spkr, n_valid=None, end=None, enc_lcf0_uv=None, out=None, lcf0_uv=None):
        """The arguments of ``StreamingConverter.push`` (feats (S, C, input_size), lcf0 / uv (S, C, 1) or the packed lcf0_uv
        (S, C, 2), spkr (S,) int64, n_valid (S,), enc_lcf0_uv), and end (S,): non-zero where this push carries the last
        frames of the stream's utterance (``n_valid`` may be 0 there).  The speaker of a frame is the ``spkr`` of the push
        that delivered it.  Returns ``decoded`` (S, max_out, output_size), ``qidx`` [(S, max_out) int64 per stack, bottom
        first], ``encoded`` [(S, max_out, emb_dim) per stack] and ``n_out``, ``first`` (S,) int32 on the device: row j of
        every output is frame ``first + j`` of the stream's utterance, rows at and past ``n_out`` are not written.
        out: buffers to write into (``empty_outputs``), e.g. the static ones of a captured graph."""
        S, C, feats, dcond, econd, n_valid, end = self._inputs(feats, lcf0, uv, spkr, n_valid, enc_lcf0_uv, lcf0_uv, end)
        out = self.empty_outputs(S) if out is None else out
        self._check_out(out, S)
        with torch.cuda.device(self.device):
            self._prepare()
            self._call("push", self._handle, feats.data_ptr(), feats.shape[-1], _lib.ptr(dcond), 2, _lib.ptr(econd), 2,
                       spkr.data_ptr(), _lib.ptr(n_valid), _lib.ptr(end), S, C, self.max_out, out["decoded"].data_ptr(),
                       self._ptrs(*[t.data_ptr() for t in out["qidx"]]), self._ptrs(*[t.data_ptr() for t in out["encoded"]]),
                       out["n_out"].data_ptr(), out["first"].data_ptr(), stream_ptr())
        return out
