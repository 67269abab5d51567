"""Test-side float64 restatement of the streaming vocoder's frontier scheme (csrc/voc_stream_kernels.hip), with
absolute arrays and no rings: every stage of the generator - conv_in, each upsampling stage, each residual layer - keeps the
position up to which its output exists, a push moves every frontier from its value at T0 frames to its value at T1 (to the
utterance's end when the push ends it), and a stage computes the positions in between from operands addressed by their
absolute position.  Arrays start as NaN, so a stage that reads a position nobody has computed yet poisons what it emits.

The weights are those of a ``tests.pwg_vocoder_ref.PWGVocoderRef`` whose weight norm has been removed."""
import math

import numpy as np


def geometry(layers, stacks, scales, win):
    """H, per-layer dilations, D, A and the look-ahead LA = win + ceil((D + A) / H), as the issue defines them."""
    lps = layers // stacks
    dil = [2 ** (l % lps) for l in range(layers)]
    H = int(np.prod(scales))
    A, rate = 0, 1
    for s in scales:
        A += H // rate
        rate *= s
    D = sum(dil)
    return H, dil, D, A, win + -(-(D + A) // H)


def _np(t):
    return t.detach().double().numpy()


class ChunkedVocoderRef:
    def __init__(self, g, max_frames):
        up = g.upsample_net
        self.win = g.aux_context_window
        self.scales = [m.x_scale for m in up.upsample.up_layers if hasattr(m, "x_scale")]
        self.layers = len(g.conv_layers)
        self.H, self.dil, self.D, self.A, self.LA = geometry(self.layers, g.stacks, self.scales, self.win)
        self.aux = g.aux_channels
        self.first_w, self.first_b = _np(g.first_conv.weight).reshape(-1), _np(g.first_conv.bias)
        self.cin_w = _np(up.conv_in.weight)  # [aux][aux][2 win + 1]
        self.up_w = [_np(m.weight).reshape(-1) for m in up.upsample.up_layers if hasattr(m, "weight")]
        self.lw = [dict(conv=_np(f.conv.weight), conv_b=_np(f.conv.bias), aux=_np(f.conv1x1_aux.weight)[:, :, 0],
                        out=_np(f.conv1x1_out.weight)[:, :, 0], out_b=_np(f.conv1x1_out.bias),
                        skip=_np(f.conv1x1_skip.weight)[:, :, 0], skip_b=_np(f.conv1x1_skip.bias)) for f in g.conv_layers]
        self.t1_w, self.t1_b = _np(g.last_conv_layers[1].weight)[:, :, 0], _np(g.last_conv_layers[1].bias)
        self.t2_w, self.t2_b = _np(g.last_conv_layers[3].weight)[:, :, 0], _np(g.last_conv_layers[3].bias)
        self.max_frames = max_frames
        self.reset()

    def reset(self):
        Tm, nan = self.max_frames, np.nan
        self.T = 0
        self.c = np.full((Tm, self.aux), nan)
        rates = np.cumprod([1] + self.scales)
        self.u = [np.full((Tm * int(r), self.aux), nan) for r in rates]  # u[0]: conv_in's output, u[-1]: the conditioning
        self.noise = np.full(Tm * self.H, nan)
        self.x = [None] + [np.full((Tm * self.H, 64), nan) for _ in range(1, self.layers)]
        self.skip = np.full((Tm * self.H, 64), nan)

    # -- frontiers: a function of the frames received and of whether the utterance has ended
    def f_frames(self, T, e):
        return T if e else max(0, T - self.win)

    def f_stage(self, T, e, i):
        p, rate = self.f_frames(T, e), 1
        for j in range(i):
            rate *= self.scales[j]
            p = T * rate if e else max(0, (p - 1) * self.scales[j])
        return p

    def f_x(self, T, e, l):
        """frontier of x_l, the input of layer l (l = layers: the last layer's own reach)"""
        return T * self.H if e else max(0, self.f_stage(T, e, len(self.scales)) - sum(self.dil[:l]))

    def f_emit(self, T, e):
        return T * self.H if e else max(0, T - self.LA) * self.H

    def push(self, c_new, noise_new, end=False):
        c_new, noise_new = np.asarray(c_new, np.float64), np.asarray(noise_new, np.float64).reshape(-1)
        T0, T1 = self.T, self.T + len(c_new)
        assert len(noise_new) == len(c_new) * self.H and T1 <= self.max_frames
        self.c[T0:T1] = c_new
        self.noise[T0 * self.H:T1 * self.H] = noise_new
        big = 1 << 60
        # conv_in: replicate padding at the utterance's edges, by position
        E = T1 if end else big
        K = 2 * self.win + 1
        for f in range(self.f_frames(T0, False), self.f_frames(T1, end)):
            acc = np.zeros(self.aux)
            for k in range(K):
                acc += self.cin_w[:, :, k] @ self.c[min(max(f - self.win + k, 0), E - 1)]
            self.u[0][f] = acc
        # upsampling stages: nearest stretch and the (2s + 1)-tap kernel over zeros outside [0, E)
        rate = 1
        for i, s in enumerate(self.scales):
            rate *= s
            E = T1 * rate if end else big
            lo, hi = self.f_stage(T0, False, i + 1), self.f_stage(T1, end, i + 1)
            t = np.arange(lo, hi)
            acc = np.zeros((hi - lo, self.aux))
            for k in range(2 * s + 1):
                tt = t + k - s
                ok = (tt >= 0) & (tt < E)
                acc[ok] += self.up_w[i][k] * self.u[i][tt[ok] // s]
            self.u[i + 1][lo:hi] = acc
        cond = self.u[-1]
        # residual layers
        E = T1 * self.H if end else big
        out = np.zeros(0)
        for l, w in enumerate(self.lw):
            last = l + 1 == self.layers
            lo = self.f_emit(T0, False) if last else self.f_x(T0, False, l + 1)
            hi = self.f_emit(T1, end) if last else self.f_x(T1, end, l + 1)
            n = np.arange(lo, hi)

            def xin(m):
                if l == 0:
                    return self.noise[m][:, None] * self.first_w[None] + self.first_b[None]
                return self.x[l][m]

            a = np.tile(w["conv_b"], (hi - lo, 1)) + cond[n] @ w["aux"].T
            for k in range(3):
                m = n + (k - 1) * self.dil[l]
                ok = (m >= 0) & (m < E)
                a[ok] += xin(m[ok]) @ w["conv"][:, :, k].T
            z = np.tanh(a[:, :64]) / (1.0 + np.exp(-a[:, 64:]))
            s_ = z @ w["skip"].T + w["skip_b"]
            sk = s_ if l == 0 else self.skip[n] + s_
            if not last:
                self.skip[n] = sk
                self.x[l + 1][n] = (z @ w["out"].T + w["out_b"] + xin(n)) * math.sqrt(0.5)
            else:
                y = np.maximum(sk * math.sqrt(1.0 / self.layers), 0.0)
                y = np.maximum(y @ self.t1_w.T + self.t1_b, 0.0)
                out = (y @ self.t2_w.T + self.t2_b).reshape(-1)
        if end:
            self.reset()
        else:
            self.T = T1
        return out
