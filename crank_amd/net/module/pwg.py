"""HIP-backed convolutional stacks with the constructor surface of the third-party
`parallel_wavegan` classes crank instantiates (call sites
crank/net/module/vqvae2.py:237-273, crank/net/module/spkradv.py:49-60,
crank/bin/train.py:78-128).  The arithmetic is in libcrank_hip.so (net.hip).
"""
import torch

from ... import ops
from .flat import FlatModel, net_keys

KIND_GENERATOR, KIND_RESIDUAL_D, KIND_PLAIN = 0, 1, 2
MAX_CHANNELS = 128  # input, output and conditioning channels of one stack (crk_net_create)
MAX_KERNEL_SIZE = 5
MAX_PLAIN_LAYERS = 8  # plain chains: layer i has dilation i; deeper chains' data gradients are wrong


def _pad32(c):
    return (c + 31) // 32 * 32


def wgrad_one_tap_group(cout, cin, k, dil):
    """Whether the weight-gradient kernel takes all k taps of a conv in ONE table entry (conv_kernels.hip wgrad_expand:
    at most 10 MFMA tiles per wave, and the conv-input rows of a 64-frame chunk within 11 passes of the workgroup).
    Several tap groups give wrong weight gradients ("Kernel sizes above 5")."""
    nct, nit = _pad32(cout) // 32, _pad32(cin) // 32
    nctp = 1 if nct <= 1 else (2 if nct <= 2 else 4)
    rows_per_pass = 256 // (_pad32(cin) // 4)
    return k * nit <= 10 * (4 // nctp) and -(-(64 + (k - 1) * dil) // rows_per_pass) <= 11


PER_LAYER_LDS_LIMIT = 160 * 1024  # conv_kernels.hip launch_conv
FUSED_MAX_AUX = 64  # the fused gated kernels' conditioning chunk (stack_fwd_plan, stack_bwd_plan, stack_wgrad_supported)


def per_layer_gated_lds_bytes(kernel_size, dilation, aux_channels, precise):
    """LDS bytes of the per-layer gated forward kernel for one block (conv_kernels.hip conv_fill_lds, MODE_RESFWD): the
    input tile with its halo, the conditioning tile, one weight chunk and the z tile, each as a hi plane and - in
    split-operand arithmetic - a lo plane."""
    def al16(n):
        return (n + 15) // 16 * 16

    aux_pad = 0 if aux_channels <= 0 else (64 if aux_channels <= 64 else (aux_channels + 15) // 16 * 16)
    rows = 128 + (kernel_size - 1) * dilation
    stride = lambda ch: ch * 2 + 16  # noqa: E731
    one = (al16(rows * stride(64)) + (al16(128 * stride(aux_pad)) if aux_pad else 0) + al16(128 * stride(max(64, aux_pad)))
           + al16(128 * stride(64)))
    return (2 if precise else 1) * one


def _conv_shapes(kind, cin, cout, layers, stacks, conv_ch):
    """(cout, cin, dilation) of every conv with more than one tap (net.hip crk_net_create)."""
    if kind == KIND_PLAIN:  # dilation = layer index (1 for the first and the last conv)
        chans = [cin] + [conv_ch] * (layers - 1)
        return [(cout if i == layers - 1 else conv_ch, chans[i], 1 if i in (0, layers - 1) else i) for i in range(layers)]
    lps = layers // max(stacks, 1)  # gated blocks: the dilated 64 -> 128 conv, dilation 2^(l mod layers per stack)
    return [(128, 64, 2 ** (l % lps)) for l in range(layers)]


class HipStack:
    """One stack living at `base` inside its owner's flat parameter block."""

    def __init__(self, kind, in_channels, out_channels, kernel_size, layers, stacks=1, aux_channels=0,
                 conv_channels=64, use_causal_conv=False, bias=True, negative_slope=0.2, dropout=0.0):
        self.kind = kind
        self.layers, self.stacks, self.kernel_size = layers, stacks, kernel_size
        # the library's channel limit (crk_net_create): refused here with its reason instead of as a failed handle
        for name, ch in (("in_channels", in_channels), ("out_channels", out_channels), ("aux_channels", aux_channels)):
            if ch > MAX_CHANNELS:
                raise NotImplementedError(f"{name}={ch}: the HIP conv stacks take at most {MAX_CHANNELS} channels")
        # wider kernels compute wrong values ("Kernel sizes above 5"): refused, not run
        if kernel_size > MAX_KERNEL_SIZE:
            raise NotImplementedError(f"kernel_size={kernel_size}: the HIP conv stacks are verified up to kernel_size "
                                      f"{MAX_KERNEL_SIZE} only")
        if kind == KIND_PLAIN and layers > MAX_PLAIN_LAYERS:
            raise NotImplementedError(f"layers={layers}: plain conv chains are verified up to {MAX_PLAIN_LAYERS} layers only "
                                      f"(dilation {MAX_PLAIN_LAYERS - 2})")
        for cout, cin, dil in _conv_shapes(kind, in_channels, out_channels, layers, stacks, conv_channels):
            if not wgrad_one_tap_group(cout, cin, kernel_size, dil):
                raise NotImplementedError(
                    f"a {cin} -> {cout} conv of kernel {kernel_size} at dilation {dil}: its weight gradient would be split "
                    f"into tap groups, which the HIP conv stacks do not compute correctly yet (DESIGN.md)")
        # A conditioning chunk wider than FUSED_MAX_AUX channels always runs on the per-layer kernels, and there its tiles fit
        # the LDS in plain bf16 only (aux 65, kernel 5: 164992 bytes with lo planes; aux 128: 214144): such a stack computes in
        # plain bf16 and refuses the split-operand arithmetics when it is called ("What reaches the per-layer kernels")
        self.plain_bf16_only = None
        if kind != KIND_PLAIN and aux_channels > FUSED_MAX_AUX:
            need = max(per_layer_gated_lds_bytes(kernel_size, dil, aux_channels, True)
                       for _, _, dil in _conv_shapes(kind, in_channels, out_channels, layers, stacks, conv_channels))
            if need > PER_LAYER_LDS_LIMIT:
                self.plain_bf16_only = (f"{aux_channels} conditioning channels: more than {FUSED_MAX_AUX} run on the per-layer "
                                        f"kernels, whose split-operand tiles need {need} bytes of LDS ({PER_LAYER_LDS_LIMIT} "
                                        f"available) - plain bf16 only")
        self.net = ops.HipNet(
            kind=kind, in_ch=in_channels, out_ch=out_channels, kernel_size=kernel_size, layers=layers,
            stacks=max(stacks, 1), res_ch=64, gate_ch=128, skip_ch=64, aux_ch=max(aux_channels, 0),
            conv_ch=conv_channels, causal=int(bool(use_causal_conv)), use_bias=int(bool(bias)),
            slope=float(negative_slope), dropout=float(dropout),
        )
        self.owner, self.base = None, 0

    @property
    def n_params(self):
        return self.net.n_params

    def entries(self, prefix, base):
        return [(prefix + k, base + off, shp) for (k, off, shp) in net_keys(self.kind, self.net.convs)]

    def bind(self, owner, base):
        self.owner, self.base = owner, base
        owner.register_net(self.net, base)

    @torch.no_grad()
    def init_parameters(self):
        """PWG init: kaiming-normal(relu) v, g = ||v||, bias 0."""
        flat = self.owner.flat.data
        for (cout, cin, k, off_b, off_g, off_v, dil, role, layer) in self.net.convs:
            v = torch.randn(cout, cin * k, device=flat.device) * float((2.0 / (cin * k)) ** 0.5)
            flat[self.base + off_v: self.base + off_v + cout * cin * k] = v.reshape(-1)
            flat[self.base + off_g: self.base + off_g + cout] = v.norm(dim=1)
            if off_b >= 0:
                flat[self.base + off_b: self.base + off_b + cout] = 0.0

    @property
    def receptive_field_size(self):
        lpc = self.layers // self.stacks
        return (self.kernel_size - 1) * sum(2 ** (i % lpc) for i in range(self.layers)) + 1

    def __call__(self, x, c=None, dx_scale=1.0, out=None):
        """x: (B,T,in) channel-last; c: (B,T,aux) or None -> (B,T,out); out = (buffer, column): see ops.net_apply."""
        if self.plain_bf16_only and ops.get_precision() != "bf16":
            raise NotImplementedError(f"precision {ops.get_precision()}: {self.plain_bf16_only}")
        return ops.net_apply(self.net, self.owner, self.base, x, c, dx_scale, out=out)

    def ce(self, x, target, dx_scale=1.0, ignore_index=-100):
        """Mean cross entropy of this stack's output against `target` (B,T) as one op (ops.net_ce): what
        nn.CrossEntropyLoss(ignore_index)(stack(x).reshape(-1, classes), target.reshape(-1)) returns."""
        return ops.net_ce(self.net, self.owner, self.base, x, target, dx_scale, ignore_index)


class _StandaloneStack(FlatModel):
    """A model that is exactly one stack (speaker classifier C, discriminator D).
    Called like the reference calls them: (B,C,T) in, (B,C_out,T) out."""

    def __init__(self, stack, device):
        super().__init__()
        self.stack = stack
        self._alloc(stack.entries("", 0), stack.n_params, device)
        stack.bind(self, 0)
        stack.init_parameters()

    def forward(self, x):
        y = self.stack(x.transpose(1, 2))
        return y.transpose(1, 2)

    def forward_ce(self, x, target, ignore_index=-100):
        """cross entropy of forward(x) (B,C_out,T) against target (B,T) as one op (not in the reference: its trainers
        compose the two, trainer_vqvae.py:186-198); stacks without dropout only."""
        return self.stack.ce(x.transpose(1, 2), target, ignore_index=ignore_index)


class ParallelWaveGANDiscriminator(_StandaloneStack):
    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2}, bias=True,
                 use_weight_norm=True, device="cuda"):
        if dilation_factor != 1 or nonlinear_activation != "LeakyReLU" or not use_weight_norm:
            raise NotImplementedError("only the configuration crank uses is implemented "
                                      "(dilation_factor=1, LeakyReLU, weight norm)")
        stack = HipStack(KIND_PLAIN, in_channels, out_channels, kernel_size, layers, conv_channels=conv_channels,
                         bias=bias, negative_slope=nonlinear_activation_params.get("negative_slope", 0.2))
        super().__init__(stack, device)


class ResidualParallelWaveGANDiscriminator(_StandaloneStack):
    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64,
                 gate_channels=128, skip_channels=64, dropout=0.0, bias=True, use_weight_norm=True,
                 use_causal_conv=False, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, device="cuda"):
        if (residual_channels, gate_channels, skip_channels) != (64, 128, 64) or not use_weight_norm:
            raise NotImplementedError("channel widths are fixed at 64/128/64 as in crank/bin/train.py:108-118")
        stack = HipStack(KIND_RESIDUAL_D, in_channels, out_channels, kernel_size, layers, stacks=stacks,
                         use_causal_conv=use_causal_conv, bias=bias, dropout=dropout,
                         negative_slope=nonlinear_activation_params.get("negative_slope", 0.2))
        super().__init__(stack, device)
