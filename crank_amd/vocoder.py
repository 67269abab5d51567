"""Parallel WaveGAN vocoder inference on the MI355X: recipe stage 6 (egs/vaevc/template/run.sh:173-241, voc=PWG).

The stage normalises the converted log-mel with the vocoder's statistics (``parallel-wavegan-normalize``) and runs
``parallel-wavegan-decode``: the published ``ParallelWaveGANGenerator.inference(c, x)``.  Here the whole generator -
ConvInUpsampleNetwork aux path and the gated residual stack - runs in the HIP kernels of csrc/vocoder_kernels.hip
(crk_voc_*), on a ragged batch of utterances per call.  Weight norm is folded (g v / ||v||) once, on load.

Parity against the third-party package is unpinned (it is not installed): the tests compare with the CPU restatement
tests/pwg_vocoder_ref.py.  There is no torch fallback: without the library every call raises.
"""
import ctypes

import numpy as np
import torch

from crank_amd import _lib, ops
from crank_amd._lib import check, stream_ptr
from crank_amd._ragged import Workspace, made, offsets, release, require_gpu, reset_streams

MAX_AUX = 128
MAX_SCALE = 16
MAX_SCALES = 8

# ParallelWaveGANGenerator's published defaults (generator_params keys)
GENERATOR_DEFAULTS = dict(
    in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128,
    skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True,
    use_causal_conv=False, upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork",
    upsample_params={"upsample_scales": [4, 4, 4, 4]},
)


def generator_params(config):
    """The generator's parameters with the published defaults filled in; NotImplementedError for what the kernels do
    not implement."""
    gtype = config.get("generator_type", "ParallelWaveGANGenerator")
    if gtype != "ParallelWaveGANGenerator":
        raise NotImplementedError(f"generator_type {gtype!r}: only ParallelWaveGANGenerator")
    p = dict(GENERATOR_DEFAULTS)
    p.update(config.get("generator_params") or {})
    up = dict(p["upsample_params"] or {})
    unknown = set(p) - set(GENERATOR_DEFAULTS)
    if unknown:
        raise NotImplementedError(f"generator_params {sorted(unknown)}")

    def refuse(cond, what):
        if cond:
            raise NotImplementedError(what)

    refuse(p["use_causal_conv"], "use_causal_conv (causal PWG)")
    refuse(not p["upsample_conditional_features"], "upsample_conditional_features=False")
    refuse(p["upsample_net"] != "ConvInUpsampleNetwork", f"upsample_net {p['upsample_net']!r}")
    refuse(up.get("nonlinear_activation") is not None, "a nonlinearity in the upsampling network")
    refuse(up.get("freq_axis_kernel_size", 1) != 1, "freq_axis_kernel_size != 1")
    refuse(up.get("interpolate_mode", "nearest") != "nearest", "interpolate_mode other than nearest")
    refuse(set(up) - {"upsample_scales", "nonlinear_activation", "nonlinear_activation_params", "interpolate_mode",
                      "freq_axis_kernel_size"}, f"upsample_params {sorted(up)}")
    refuse((p["residual_channels"], p["gate_channels"], p["skip_channels"]) != (64, 128, 64),
           "residual / gate / skip widths other than 64 / 128 / 64")
    refuse(p["in_channels"] != 1 or p["out_channels"] != 1, "in / out channels other than 1")
    refuse(p["kernel_size"] != 3, "kernel_size other than 3")
    refuse(not 1 <= p["aux_channels"] <= MAX_AUX, f"aux_channels outside 1..{MAX_AUX}")
    refuse(p["aux_context_window"] < 0, "negative aux_context_window")
    refuse(p["layers"] < 1 or p["stacks"] < 1 or p["layers"] % p["stacks"], "layers not a multiple of stacks")
    refuse(p["layers"] // p["stacks"] > 30, "more than 30 layers per stack")
    scales = [int(s) for s in up.get("upsample_scales", [])]
    refuse(not 1 <= len(scales) <= MAX_SCALES, f"1..{MAX_SCALES} upsample scales")
    refuse(any(not 1 <= s <= MAX_SCALE for s in scales), f"an upsample scale outside 1..{MAX_SCALE}")
    p["upsample_params"] = dict(up, upsample_scales=scales)
    return p


def lookahead_frames(params):
    """Frames a streamed generator runs behind its input (``StreamingVocoder``): win + ceil((D + A) / H), with H the hop,
    D the sum of the layers' dilations and A = sum_i H / prod_{j<i} s_j the forward reach of the upsampling network in
    samples (each stage can ask for one more input sample of its own rate).  16 for the published default
    (D = 3069, A = 340, H = 256, win = 2)."""
    scales = [int(s) for s in params["upsample_params"]["upsample_scales"]]
    lps = params["layers"] // params["stacks"]
    D = sum(2 ** (l % lps) for l in range(params["layers"]))
    H, A, rate = int(np.prod(scales)), 0, 1
    for s in scales:
        A += H // rate
        rate *= s
    return int(params["aux_context_window"]) + -(-(D + A) // H)


def expected_keys(p):
    """(module prefix, has bias) of every conv of the generator, in the order of crk_voc_create's parameter block."""
    b = bool(p["bias"])
    keys = [("first_conv.", b), ("upsample_net.conv_in.", False)]
    keys += [(f"upsample_net.upsample.up_layers.{2 * i + 1}.", False) for i in range(len(p["upsample_params"]["upsample_scales"]))]
    for l in range(p["layers"]):
        keys += [(f"conv_layers.{l}.conv.", b), (f"conv_layers.{l}.conv1x1_aux.", False),
                 (f"conv_layers.{l}.conv1x1_out.", b), (f"conv_layers.{l}.conv1x1_skip.", b)]
    keys += [("last_conv_layers.1.", b), ("last_conv_layers.3.", b)]
    return keys


def fold_state_dict(state, p):
    """prefix -> (weight, bias or None), fp32 on the CPU, weight norm folded exactly as torch's remove_weight_norm does.
    Raises KeyError on a missing and ValueError on an unexpected key."""
    state = {k: v for k, v in state.items()}
    used, out = set(), {}
    for prefix, has_bias in expected_keys(p):
        if prefix + "weight" in state:
            w = state[prefix + "weight"].detach().float().cpu()
            used.add(prefix + "weight")
        elif prefix + "weight_g" in state and prefix + "weight_v" in state:
            g, v = state[prefix + "weight_g"].detach().float().cpu(), state[prefix + "weight_v"].detach().float().cpu()
            w = torch._weight_norm(v, g, 0)
            used.update((prefix + "weight_g", prefix + "weight_v"))
        else:
            raise KeyError(f"generator state dict has no {prefix}weight (nor weight_g / weight_v)")
        bias = None
        if has_bias:
            if prefix + "bias" not in state:
                raise KeyError(f"generator state dict has no {prefix}bias")
            bias = state[prefix + "bias"].detach().float().cpu()
            used.add(prefix + "bias")
        out[prefix] = (w, bias)
    extra = sorted(set(state) - used)
    if extra:
        raise ValueError(f"generator state dict has keys this generator does not have: {extra[:8]}")
    return out


def _param_block(p, w):
    """The fp32 host block crk_voc_create reads (include/crank_hip.h)."""
    aux, K = p["aux_channels"], 2 * p["aux_context_window"] + 1
    parts = []

    def put(t, shape):
        t = torch.zeros(shape) if t is None else t
        if tuple(t.shape) != tuple(shape) and t.numel() == int(np.prod(shape)):
            t = t.reshape(shape)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"parameter of shape {tuple(t.shape)}, expected {tuple(shape)}")
        parts.append(t.reshape(-1))

    fw, fb = w["first_conv."]
    put(fw, (64, 1, 1)); put(fb, (64,))
    put(w["upsample_net.conv_in."][0], (aux, aux, K))
    for i, s in enumerate(p["upsample_params"]["upsample_scales"]):
        put(w[f"upsample_net.upsample.up_layers.{2 * i + 1}."][0], (1, 1, 1, 2 * s + 1))
    for l in range(p["layers"]):
        cw, cb = w[f"conv_layers.{l}.conv."]
        put(cw, (128, 64, 3)); put(cb, (128,))
        put(w[f"conv_layers.{l}.conv1x1_aux."][0], (128, aux, 1))
        ow, ob = w[f"conv_layers.{l}.conv1x1_out."]
        put(ow, (64, 64, 1)); put(ob, (64,))
        sw, sb = w[f"conv_layers.{l}.conv1x1_skip."]
        put(sw, (64, 64, 1)); put(sb, (64,))
    w1, b1 = w["last_conv_layers.1."]
    put(w1, (64, 64, 1)); put(b1, (64,))
    w2, b2 = w["last_conv_layers.3."]
    put(w2, (1, 64, 1)); put(b2, (1,))
    return torch.cat(parts).contiguous()


def load_stats(stats):
    """(mean, scale) of the vocoder's feature statistics: ``stats.npy`` ([mean, scale]) or ``stats.h5``."""
    if stats is None:
        return None
    if isinstance(stats, (tuple, list)) and len(stats) == 2:
        return np.asarray(stats[0], np.float32), np.asarray(stats[1], np.float32)
    if str(stats).endswith(".npy"):
        a = np.load(stats)
        return np.asarray(a[0], np.float32), np.asarray(a[1], np.float32)
    try:
        import h5py
    except ImportError as e:  # pragma: no cover - environment dependent
        raise RuntimeError("reading stats.h5 needs h5py; pass stats.npy ([mean, scale]) instead") from e
    with h5py.File(stats, "r") as fp:
        return np.asarray(fp["mean"][:], np.float32), np.asarray(fp["scale"][:], np.float32)


def load_config(config):
    if isinstance(config, dict):
        return config
    import yaml

    with open(config) as f:
        return yaml.load(f, Loader=yaml.SafeLoader)


class ParallelWaveGANVocoder:
    """The generator of a Parallel WaveGAN checkpoint, run by the HIP kernels."""

    def __init__(self, params, weights, hop_size, sampling_rate=None, stats=None, device="cuda"):
        self.params = params
        self.weights = weights  # prefix -> (folded weight, bias): what remove_weight_norm() leaves
        self.scales = list(params["upsample_params"]["upsample_scales"])
        self.hop_size = int(hop_size)
        if int(np.prod(self.scales)) != self.hop_size:
            raise NotImplementedError(f"prod(upsample_scales) = {int(np.prod(self.scales))} != hop_size {self.hop_size}")
        self.sampling_rate = sampling_rate
        self.aux_channels = params["aux_channels"]
        self.device = torch.device(device)
        self.block = _param_block(params, weights)
        self.mean = self.scale = None
        if stats is not None:
            mean, scale = load_stats(stats)
            self.mean = torch.as_tensor(mean, dtype=torch.float32, device=self.device)
            self.scale = torch.as_tensor(scale, dtype=torch.float32, device=self.device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(0)
        self._handle = None
        self._workspace = Workspace(self.device)

    @classmethod
    def from_checkpoint(cls, checkpoint, config, stats=None, device="cuda"):
        cfg = load_config(config)
        p = generator_params(cfg)
        ck = torch.load(checkpoint, map_location="cpu") if not isinstance(checkpoint, dict) else checkpoint
        state = ck["model"]["generator"]
        return cls(p, fold_state_dict(state, p), cfg["hop_size"], cfg.get("sampling_rate"), stats, device)

    # -- device resources
    def handle(self):
        if self._handle is None:
            p = self.params
            sc = (ctypes.c_int * len(self.scales))(*self.scales)
            self._handle = made(_lib.lib().crk_voc_create(p["layers"], p["stacks"], p["aux_channels"],
                                                          p["aux_context_window"], ctypes.addressof(sc), len(self.scales),
                                                          self.block.data_ptr()), "crk_voc_create")
        return self._handle

    def workspace_bytes(self, n_utts, total_frames):
        return int(_lib.lib().crk_voc_workspace_bytes(self.handle(), n_utts, total_frames))

    def reserve(self, n_utts, total_frames):
        """Device workspace for a call of n_utts utterances / total_frames frames (kept and grown, never per call)."""
        return self._workspace.ensure(self.workspace_bytes(n_utts, total_frames), "crk_voc_workspace_bytes")

    def __del__(self):
        release(self, "_handle", "crk_voc_destroy")

    def manual_seed(self, seed):
        self.generator.manual_seed(int(seed))
        return self

    # -- stage 6
    def normalize(self, feats):
        """``parallel-wavegan-normalize``: (feat - mean) / scale with the vocoder's statistics, on the device."""
        if self.mean is None:
            raise RuntimeError("the vocoder was loaded without stats")
        f = torch.as_tensor(feats, dtype=torch.float32).to(self.device)
        return (f - self.mean) / self.scale

    def _batch(self, cs):
        cs = [torch.as_tensor(c, dtype=torch.float32).to(self.device) for c in cs]
        for c in cs:
            if c.dim() != 2 or c.shape[1] != self.aux_channels or c.shape[0] < 1:
                raise ValueError(f"c must be (frames >= 1, {self.aux_channels}), got {tuple(c.shape)}")
        lens = [int(c.shape[0]) for c in cs]
        off = offsets(lens, self.device)
        return torch.cat(cs).contiguous(), off, lens

    def upsample_batch(self, cs):
        """The aux path alone (conv_in + upsampling network, fp32): per utterance (frames * hop, aux)."""
        c, off, lens = self._batch(cs)
        F = sum(lens)
        ws = self.reserve(len(lens), F)
        out = torch.empty(F * self.hop_size, self.aux_channels, device=self.device)
        check(_lib.lib().crk_voc_upsample(self.handle(), c.data_ptr(), off.data_ptr(), len(lens), F, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream_ptr()), "crk_voc_upsample")
        return list(out.split([n * self.hop_size for n in lens]))

    def inference_batch(self, cs, xs=None):
        """Waveforms (frames * hop,) of a ragged batch of (frames, aux) features; xs: per utterance noise
        (frames * hop[, 1]) or None (drawn on the device from ``self.generator``)."""
        c, off, lens = self._batch(cs)
        F, N = sum(lens), sum(lens) * self.hop_size
        if xs is None:
            noise = torch.randn(N, generator=self.generator, device=self.device)
        else:
            xs = [torch.as_tensor(x, dtype=torch.float32).to(self.device).reshape(-1) for x in xs]
            if len(xs) != len(lens) or any(x.numel() != n * self.hop_size for x, n in zip(xs, lens)):
                raise ValueError("each x must hold frames * hop_size samples")
            noise = torch.cat(xs).contiguous()
        ws = self.reserve(len(lens), F)
        out = torch.empty(N, device=self.device)
        flags = ops.CRK_FLAG_PRECISE if ops.get_precision() in ("bf16x3", "bf16x3f") else 0
        check(_lib.lib().crk_voc_forward(self.handle(), c.data_ptr(), off.data_ptr(), len(lens), F, noise.data_ptr(),
                                         out.data_ptr(), ws.data_ptr(), ws.numel(), flags, stream_ptr()),
              "crk_voc_forward")
        return list(out.split([n * self.hop_size for n in lens]))

    def streaming(self, n_streams, max_chunk):
        """A ``StreamingVocoder`` on this generator's weights: up to ``n_streams`` streams, ``max_chunk`` frames a push."""
        return StreamingVocoder(self, n_streams, max_chunk)

    def inference(self, c, x=None):
        """The published ``inference(c, x)``: c (frames, aux) -> waveform (frames * hop,)."""
        return self.inference_batch([c], None if x is None else [x])[0]

    def vocode_eval_outputs(self, outputs):
        """Waveforms of the per-utterance dicts of ``trainer.eval()`` / ``_store_features`` ("feats": de-normalised by
        crank's scaler): normalised with the vocoder's statistics, then decoded as one ragged batch.  A dict of
        such lists (one per target speaker) gives a dict of lists."""
        if isinstance(outputs, dict):
            return {k: self.vocode_eval_outputs(v) for k, v in outputs.items()}
        return self.inference_batch([self.normalize(d["feats"]) for d in outputs])



class StreamingVocoder:
    """``push`` vocodes the next frames of up to ``n_streams`` independent streams, at most ``max_chunk`` frames each per
    push (csrc/voc_stream_kernels.hip, ``crk_voc_stream_*``).  Stream i is row i of every argument.

    The generator is not causal, so a stream runs ``lookahead`` frames behind its input: after T frames of an utterance
    it has emitted max(0, T - lookahead) * hop samples, and the push that carries the stream's ``end`` flag emits the rest
    and starts a new utterance.  The emitted samples equal ``inference_batch`` on the whole utterance with the same noise
    bit for bit, in every precision and however the utterance is cut into pushes.  Every layer's history and every
    position stay on the device; a push neither allocates nor reads back.  There is no torch or CPU fallback."""

    def __init__(self, vocoder, n_streams, max_chunk):
        if n_streams < 1 or max_chunk < 1:
            raise ValueError(f"n_streams = {n_streams}, max_chunk = {max_chunk}: both must be at least 1")
        self.vocoder, self.device = vocoder, vocoder.device
        require_gpu(self.device, "streaming vocoding", "the vocoder's device")
        self.n_streams, self.max_chunk = int(n_streams), int(max_chunk)
        self.hop_size, self.aux_channels = vocoder.hop_size, vocoder.aux_channels
        self.lookahead = lookahead_frames(vocoder.params)
        h = ctypes.c_void_p()
        L = _lib.lib()
        with torch.cuda.device(self.device):
            check(L.crk_voc_stream_create(vocoder.handle(), self.n_streams, self.max_chunk, ctypes.byref(h)),
                  "crk_voc_stream_create")
            self._handle = made(h, "crk_voc_stream_create")
        if int(L.crk_voc_stream_lookahead(self._handle)) != self.lookahead:
            raise RuntimeError(f"crk_voc_stream_lookahead = {L.crk_voc_stream_lookahead(self._handle)}, "
                               f"lookahead_frames = {self.lookahead}")

    def __del__(self):
        release(self, "_handle", "crk_voc_stream_destroy")

    @property
    def state_bytes(self):
        return int(_lib.lib().crk_voc_stream_state_bytes(self._handle))

    def reset(self, streams=None):
        """``streams`` (all of them by default) start a new utterance; what they had not emitted yet is dropped."""
        ids = None if streams is None else [int(s) for s in streams]
        if ids is not None and any(not 0 <= i < self.n_streams for i in ids):
            raise ValueError(f"streams {ids}: stream ids are 0 .. {self.n_streams - 1}")
        reset_streams(self._handle, "crk_voc_stream_reset", ids, self.device)

    def empty_outputs(self, S, C):
        """Output buffers of one push, in the form ``push(out=...)`` takes and returns."""
        return {"wave": torch.empty(S, (C + self.lookahead) * self.hop_size, device=self.device),
                "n_out": torch.empty(S, dtype=torch.int32, device=self.device)}

    def _flags(self, t, S, what):
        if t is None:
            return None
        if t.device.type != "cuda" or tuple(t.shape) != (S,) or t.dtype not in (torch.int32, torch.int64, torch.bool):
            raise ValueError(f"{what}: an integer ({S},) tensor on the GPU, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.to(torch.int32).contiguous()

    def push(self, c, noise=None, n_valid=None, end=None, out=None):
        """c (S, C, aux) normalised features, noise (S, C * hop) or None (drawn on the device from the vocoder's
        generator), n_valid (S,) frames that count per stream (default: C), end (S,) non-zero where this push ends the
        stream's utterance.  Returns ``wave`` (S, (C + lookahead) * hop) and ``n_out`` (S,) int32: the samples written at
        the start of each row; samples past ``n_out`` are not written.  out: buffers to write into (``empty_outputs``),
        e.g. the static ones of a captured graph."""
        if c.dim() != 3:
            raise ValueError(f"c: a float32 (S, C, {self.aux_channels}) tensor on the GPU, got {tuple(c.shape)}")
        S, C = int(c.shape[0]), int(c.shape[1])
        if c.device.type != "cuda" or c.dtype != torch.float32 or tuple(c.shape) != (S, C, self.aux_channels):
            raise ValueError(f"c: a float32 ({S}, {C}, {self.aux_channels}) tensor on the GPU, got {c.dtype} "
                             f"{tuple(c.shape)} on {c.device}")
        if not 1 <= S <= self.n_streams:
            raise ValueError(f"S = {S}: this StreamingVocoder holds n_streams = {self.n_streams}")
        if not 1 <= C <= self.max_chunk:
            raise ValueError(f"C = {C}: a push takes 1 .. max_chunk = {self.max_chunk} frames")
        N = C * self.hop_size
        if noise is None:
            noise = torch.randn(S, N, generator=self.vocoder.generator, device=self.device)
        elif noise.device.type != "cuda" or noise.dtype != torch.float32 or tuple(noise.shape) != (S, N):
            raise ValueError(f"noise: a float32 ({S}, {N}) tensor on the GPU, got {noise.dtype} {tuple(noise.shape)} on "
                             f"{noise.device}")
        n_valid, end = self._flags(n_valid, S, "n_valid"), self._flags(end, S, "end")
        if out is None:
            out = self.empty_outputs(S, C)
        else:
            w, n = out["wave"], out["n_out"]
            if (w.device.type != "cuda" or w.dtype != torch.float32 or tuple(w.shape) != (S, (C + self.lookahead) * self.hop_size)
                    or not w.is_contiguous() or n.device.type != "cuda" or n.dtype != torch.int32 or tuple(n.shape) != (S,)):
                raise ValueError(f"out: wave float32 ({S}, {(C + self.lookahead) * self.hop_size}) and n_out int32 ({S},) "
                                 "on the GPU (empty_outputs)")
        flags = ops.CRK_FLAG_PRECISE if ops.get_precision() in ("bf16x3", "bf16x3f") else 0
        with torch.cuda.device(self.device):
            check(_lib.lib().crk_voc_stream_push(
                self._handle, c.contiguous().data_ptr(), noise.contiguous().data_ptr(), _lib.ptr(n_valid), _lib.ptr(end),
                S, C, out["wave"].data_ptr(), out["n_out"].data_ptr(), flags, stream_ptr()), "crk_voc_stream_push")
        return out
