"""Test-side CPU restatement of the Parallel WaveGAN generator WITH its upsampling network (the vocoder of recipe stage 6,
egs/vaevc/template/run.sh:173-241): the published ``ConvInUpsampleNetwork`` / ``UpsampleNetwork`` / ``Stretch2d`` /
``Conv2d`` and ``ParallelWaveGANGenerator.inference()``, composed with ``oracle.pwg.ResidualBlock`` / ``Conv1d1x1``.

The aux path (conv_in + upsampling) always runs in fp32 torch; under ``oracle.pwg.bf16_emulation`` the residual stack
and the tail round their conv operands to bf16 the way the HIP kernels do.  Parity of this restatement against the
third-party ``parallel_wavegan`` package is UNPINNED: the package is not installed here, exactly as for oracle/pwg.py.

Upstream notice: the classes restated here (argument lists, attribute and state-dict key names, layer arithmetic) are
those of kan-bayashi/ParallelWaveGAN, published under the MIT License, Copyright (c) 2019 Tomoki Hayashi.  No upstream
source text is in this file; the permission notice of that licence applies to the design it follows:
"Permission is hereby granted, free of charge, to any person obtaining a copy of this software and associated
documentation files (the "Software"), to deal in the Software without restriction ... THE SOFTWARE IS PROVIDED "AS IS",
WITHOUT WARRANTY OF ANY KIND".
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.pwg import Conv1d1x1, ResidualBlock


class PlainConv1d(nn.Conv1d):
    """The published Conv1d (kaiming-normal weight, zero bias) without bf16 emulation: the aux path stays fp32."""

    def reset_parameters(self):
        nn.init.kaiming_normal_(self.weight, nonlinearity="relu")
        if self.bias is not None:
            nn.init.constant_(self.bias, 0.0)


class Conv2d(nn.Conv2d):
    """Published Conv2d of the upsampling network: weight 1 / prod(kernel_size), zero bias."""

    def reset_parameters(self):
        self.weight.data.fill_(1.0 / np.prod(self.kernel_size))
        if self.bias is not None:
            nn.init.constant_(self.bias, 0.0)


class Stretch2d(nn.Module):
    def __init__(self, x_scale, y_scale, mode="nearest"):
        super().__init__()
        self.x_scale, self.y_scale, self.mode = x_scale, y_scale, mode

    def forward(self, x):
        return F.interpolate(x, scale_factor=(self.y_scale, self.x_scale), mode=self.mode)


class UpsampleNetwork(nn.Module):
    def __init__(self, upsample_scales, nonlinear_activation=None, nonlinear_activation_params={},
                 interpolate_mode="nearest", freq_axis_kernel_size=1, use_causal_conv=False):
        super().__init__()
        self.use_causal_conv = use_causal_conv
        self.up_layers = nn.ModuleList()
        for scale in upsample_scales:
            self.up_layers += [Stretch2d(scale, 1, interpolate_mode)]
            assert (freq_axis_kernel_size - 1) % 2 == 0
            freq_axis_padding = (freq_axis_kernel_size - 1) // 2
            kernel_size = (freq_axis_kernel_size, scale * 2 + 1)
            padding = (freq_axis_padding, scale * 2) if use_causal_conv else (freq_axis_padding, scale)
            self.up_layers += [Conv2d(1, 1, kernel_size=kernel_size, padding=padding, bias=False)]
            if nonlinear_activation is not None:
                self.up_layers += [getattr(nn, nonlinear_activation)(**nonlinear_activation_params)]

    def forward(self, c):
        c = c.unsqueeze(1)
        for f in self.up_layers:
            if self.use_causal_conv and isinstance(f, Conv2d):
                c = f(c)[..., : c.size(-1)]
            else:
                c = f(c)
        return c.squeeze(1)


class ConvInUpsampleNetwork(nn.Module):
    def __init__(self, upsample_scales, nonlinear_activation=None, nonlinear_activation_params={},
                 interpolate_mode="nearest", freq_axis_kernel_size=1, aux_channels=80, aux_context_window=0,
                 use_causal_conv=False):
        super().__init__()
        self.aux_context_window = aux_context_window
        self.use_causal_conv = use_causal_conv and aux_context_window > 0
        kernel_size = aux_context_window + 1 if use_causal_conv else 2 * aux_context_window + 1
        self.conv_in = PlainConv1d(aux_channels, aux_channels, kernel_size=kernel_size, bias=False)
        self.upsample = UpsampleNetwork(upsample_scales, nonlinear_activation, nonlinear_activation_params,
                                        interpolate_mode, freq_axis_kernel_size, use_causal_conv)

    def forward(self, c):
        c_ = self.conv_in(c)
        c = c_[:, :, : -self.aux_context_window] if self.use_causal_conv else c_
        return self.upsample(c)


class PWGVocoderRef(nn.Module):
    """ParallelWaveGANGenerator with upsample_conditional_features=True (ConvInUpsampleNetwork)."""

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64,
                 gate_channels=128, skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0, bias=True,
                 use_weight_norm=True, use_causal_conv=False, upsample_conditional_features=True,
                 upsample_net="ConvInUpsampleNetwork", upsample_params={"upsample_scales": [4, 4, 4, 4]}):
        super().__init__()
        assert upsample_conditional_features and upsample_net == "ConvInUpsampleNetwork"
        self.aux_channels, self.aux_context_window = aux_channels, aux_context_window
        self.layers, self.stacks, self.kernel_size = layers, stacks, kernel_size
        lps = layers // stacks
        self.first_conv = Conv1d1x1(in_channels, residual_channels, bias=True)
        up = dict(upsample_params)
        up.update({"use_causal_conv": use_causal_conv, "aux_channels": aux_channels,
                   "aux_context_window": aux_context_window})
        self.upsample_net = ConvInUpsampleNetwork(**up)
        self.upsample_factor = int(np.prod(up["upsample_scales"]))
        self.conv_layers = nn.ModuleList(
            [ResidualBlock(kernel_size=kernel_size, residual_channels=residual_channels, gate_channels=gate_channels,
                           skip_channels=skip_channels, aux_channels=aux_channels, dilation=2 ** (l % lps),
                           dropout=dropout, bias=bias, use_causal_conv=use_causal_conv) for l in range(layers)])
        self.last_conv_layers = nn.ModuleList([nn.ReLU(inplace=True), Conv1d1x1(skip_channels, skip_channels, bias=True),
                                               nn.ReLU(inplace=True), Conv1d1x1(skip_channels, out_channels, bias=True)])
        if use_weight_norm:
            self.apply_weight_norm()

    def apply_weight_norm(self):
        def _f(m):
            if isinstance(m, (nn.Conv1d, nn.Conv2d)):
                nn.utils.weight_norm(m)

        self.apply(_f)

    def remove_weight_norm(self):
        def _f(m):
            try:
                nn.utils.remove_weight_norm(m)
            except ValueError:
                return

        self.apply(_f)

    def forward(self, x, c):
        c = self.upsample_net(c)
        assert c.size(-1) == x.size(-1)
        x = self.first_conv(x)
        skips = 0
        for f in self.conv_layers:
            x, h = f(x, c)
            skips = skips + h
        x = skips * math.sqrt(1.0 / len(self.conv_layers))
        for f in self.last_conv_layers:
            x = f(x)
        return x

    def upsample_aux(self, c):
        """The aux path alone: (T, aux) -> (T * hop, aux), after the replicate padding inference() applies."""
        c = c.transpose(1, 0).unsqueeze(0)
        c = nn.ReplicationPad1d(self.aux_context_window)(c)
        return self.upsample_net(c)[0].transpose(1, 0)

    def inference(self, c, x=None):
        """(T, aux) -> (T * hop,); x: (T * hop,) noise or None (torch.randn)."""
        if x is None:
            x = torch.randn(len(c) * self.upsample_factor)
        x = x.reshape(1, 1, -1).to(c)
        c = c.transpose(1, 0).unsqueeze(0)
        c = nn.ReplicationPad1d(self.aux_context_window)(c)
        return self.forward(x, c).reshape(-1)


def brute_force_upsample(c, conv_in_w, kernels, scales, window):
    """(T, aux) -> (T * hop, aux) by explicit loops: replicate pad, conv_in, then per stage repeat each value s times and
    correlate with the (2s+1)-tap kernel over zero padding (float64)."""
    c = np.asarray(c, np.float64)
    T, A = c.shape
    idx = np.clip(np.arange(-window, T + window), 0, T - 1)
    cp = c[idx]
    K = 2 * window + 1
    h = np.zeros((T, A))
    for t in range(T):
        for k in range(K):
            h[t] += np.asarray(conv_in_w, np.float64)[:, :, k] @ cp[t + k]
    for s, w in zip(scales, kernels):
        w = np.asarray(w, np.float64).reshape(-1)
        st = np.repeat(h, s, axis=0)
        L = st.shape[0]
        pad = np.concatenate([np.zeros((s, A)), st, np.zeros((s, A))])
        h = np.zeros((L, A))
        for t in range(L):
            for k in range(2 * s + 1):
                h[t] += w[k] * pad[t + k]
    return h


def random_generator(seed, **params):
    """A randomly initialised generator (weight norm on) with non-trivial biases and norms."""
    torch.manual_seed(seed)
    g = PWGVocoderRef(**params)
    with torch.no_grad():
        for name, p in g.named_parameters():
            if name.endswith("bias"):
                p.uniform_(-0.1, 0.1)
            elif name.endswith("weight_g"):
                p.mul_(torch.empty_like(p).uniform_(0.5, 1.5))
            elif "up_layers" in name and name.endswith("weight_v"):
                p.add_(torch.empty_like(p).uniform_(-0.2, 0.2))
    return g.eval()


def checkpoint_of(g):
    return {"model": {"generator": g.state_dict()}, "steps": 0}
