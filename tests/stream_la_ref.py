"""A chunked, stateful float64 restatement of look-ahead streaming for non-causal generators (TEST INFRASTRUCTURE): the
scheme csrc/stream_la_kernels.hip implements, stated independently of the GPU and by POSITION.

Slot u of a stream is its u-th step since the utterance began; T slots have received a frame.  A non-causal residual layer
pads h = (k - 1) / 2 * dil zeros on both sides, so its output at slot u is frame u - delay, delay the sum of h over the
layer and every layer before it in the chain enc[0] .. enc[top], dec[top] .. dec[0].  A push walks every layer over its
slots; a push with the end flag runs LA further slots on zero input, emits every remaining frame and starts over.

Every quantity lives in an absolute array indexed by the utterance's frame, initialised to NaN: a layer that reads a frame
inside [0, E) that nobody computed poisons what is emitted.  A frame outside [0, E) - E the utterance's length, out of
reach until the end flag - reads as zero wherever a layer takes it.  tests/test_stream_la_cpu.py holds it to the oracle's
offline ``VQVAE2.forward`` of each whole utterance in float64."""
import math

import torch

import oracle.modules
from tests.stream_ref import _b, _w

FAR = 1 << 30  # E while the utterance's end is not in reach


def _lin(x, wb):
    y = x @ wb[0].t()
    return y if wb[1] is None else y + wb[1]


def _frames(lo, hi, E):
    """The frames of [lo, hi) inside the utterance."""
    return range(max(lo, 0), max(min(hi, E), max(lo, 0)))


def _read(arr, frames, E):
    """Rows of the absolute array at `frames` (a list): zero outside [0, E), the array's value (NaN: not computed) inside."""
    out = torch.zeros(len(frames), arr.shape[1], dtype=torch.float64)
    for i, fr in enumerate(frames):
        if 0 <= fr < E:
            out[i] = arr[fr]
    return out


class _Net:
    """One non-causal ParallelWaveGANGenerator (oracle/pwg.py) with an absolute array per layer."""

    def __init__(self, net, cap):
        self.first = (_w(net.first_conv)[:, :, 0], _b(net.first_conv))
        self.layers = []
        for blk in net.conv_layers:
            assert not blk.use_causal_conv
            k, dil = blk.conv.kernel_size[0], blk.conv.dilation[0]
            assert k % 2 == 1
            aux = None if blk.conv1x1_aux is None else _w(blk.conv1x1_aux)[:, :, 0]
            self.layers.append(dict(w=_w(blk.conv), b=_b(blk.conv), k=k, dil=dil, h=(k - 1) // 2 * dil, aux=aux,
                                    out=(_w(blk.conv1x1_out)[:, :, 0], _b(blk.conv1x1_out)),
                                    skip=(_w(blk.conv1x1_skip)[:, :, 0], _b(blk.conv1x1_skip))))
        self.last1 = (_w(net.last_conv_layers[1])[:, :, 0], _b(net.last_conv_layers[1]))
        self.last2 = (_w(net.last_conv_layers[3])[:, :, 0], _b(net.last_conv_layers[3]))
        self.delay = sum(y["h"] for y in self.layers)
        self.cap, self.out_ch = cap, self.last2[0].shape[0]
        self.clear()

    def clear(self):
        nan = lambda w: torch.full((self.cap, w), float("nan"), dtype=torch.float64)  # noqa: E731
        self.x = [nan(64) for _ in range(len(self.layers) + 1)]  # x[0]: the first conv's output; x[l + 1]: layer l's
        self.skip = nan(64)
        self.out = nan(self.out_ch)

    def push(self, src, cond, u0, u1, delay, E):
        """Slots [u0, u1): `src` the absolute array of the net's input, whose frame u - delay is in reach at slot u; cond
        the absolute array of its conditioning rows or None.  Fills self.out for frames [u0, u1) - (delay + self.delay)."""
        F = list(_frames(u0 - delay, u1 - delay, E))
        if F:
            self.x[0][F] = _lin(src[F], self.first)
        for l, y in enumerate(self.layers):
            delay += y["h"]
            F = list(_frames(u0 - delay, u1 - delay, E))
            if not F:
                continue
            g = 0 if y["b"] is None else y["b"]
            for j in range(y["k"]):  # tap j reads frame t + (j - (k - 1) / 2) * dil
                off = (j - (y["k"] - 1) // 2) * y["dil"]
                g = g + _read(self.x[l], [fr + off for fr in F], E) @ y["w"][:, :, j].t()
            if cond is not None:
                g = g + cond[F] @ y["aux"].t()
            z = torch.tanh(g[:, :64]) * torch.sigmoid(g[:, 64:])
            s = _lin(z, y["skip"])
            self.skip[F] = s if l == 0 else self.skip[F] + s  # (layer order: the offline order of additions)
            self.x[l + 1][F] = (_lin(z, y["out"]) + self.x[l][F]) * math.sqrt(0.5)
        F = list(_frames(u0 - delay, u1 - delay, E))
        if F:
            hid = torch.relu(self.skip[F] * math.sqrt(1.0 / len(self.layers)))
            self.out[F] = _lin(torch.relu(_lin(hid, self.last1)), self.last2)
        return delay


class LookaheadRef:
    """One stream of ``orac`` (an OracleVQVAE2 with causal: false), float64; utterances of at most ``cap`` frames."""

    def __init__(self, orac, cap=256):
        conf = orac.conf
        self.nst, self.cap = conf["n_vq_stacks"], cap
        self.enc = [_Net(n, cap) for n in orac.encoders]
        self.dec = [_Net(n, cap) for n in orac.decoders]
        self.cb = [q.embedding.weight.detach().double() for q in orac.quantizers]
        self.la = sum(n.delay for n in self.enc + self.dec)
        self.in_ch = self.enc[0].first[0].shape[1]
        self.aux_d = None if self.dec[0].layers[0]["aux"] is None else self.dec[0].layers[0]["aux"].shape[1]
        self.aux_e = None if self.enc[0].layers[0]["aux"] is None else self.enc[0].layers[0]["aux"].shape[1]
        self._clear()

    def _clear(self):
        nan = lambda w, dt=torch.float64: torch.full((self.cap, w), float("nan") if dt == torch.float64 else -1, dtype=dt)  # noqa: E731
        self.T = 0
        self.x = nan(self.in_ch)
        self.cd = None if self.aux_d is None else nan(self.aux_d)
        self.ce = None if self.aux_e is None else nan(self.aux_e)
        self.xq = [nan(cb.shape[1]) for cb in self.cb]   # the quantizers' inputs ("encoded")
        self.q = [nan(cb.shape[1]) for cb in self.cb]    # the quantized rows
        self.idx = [nan(1, torch.int64) for _ in self.cb]
        self.cat = nan(sum(cb.shape[1] for cb in self.cb))
        for n in self.enc + self.dec:
            n.clear()

    def push(self, x, dec_cond, enc_cond=None, end=False):
        """x (C, input_size) the next frames (C may be 0), dec_cond (C, aux of the last decoder), enc_cond (C, 2) or None;
        end: these are the utterance's last frames.  Returns first, decoded, qidx, encoded of the frames that leave:
        frames [first, first + n_out)."""
        C, T = x.shape[0], self.T
        E = T + C if end else FAR
        u0, u1 = T, T + C + (self.la if end else 0)
        assert u1 <= self.cap + self.la
        self.x[T: T + C] = x.double()
        if self.cd is not None:
            self.cd[T: T + C] = dec_cond.double()
        if self.ce is not None:
            self.ce[T: T + C] = enc_cond.double()
        delay, src = 0, self.x
        for n in range(self.nst):
            delay = self.enc[n].push(src, self.ce if n == 0 else None, u0, u1, delay, E)
            src = self.enc[n].out
        dec_out = None
        for n in reversed(range(self.nst)):
            F = list(_frames(u0 - delay, u1 - delay, E))
            if F:
                self.xq[n][F] = self.enc[n].out[F] if dec_out is None else self.enc[n].out[F] + dec_out[F]
                self.idx[n][F, 0] = oracle.modules.vq_nearest(self.xq[n][F], self.cb[n])
                e = self.cb[n][self.idx[n][F, 0]]
                self.q[n][F] = self.xq[n][F] + (e - self.xq[n][F])
                if n == 0:
                    self.cat[F] = torch.cat([self.q[m][F] for m in reversed(range(self.nst))], 1)
            if n != 0:
                delay = self.dec[n].push(self.q[n], None, u0, u1, delay, E)
                dec_out = self.dec[n].out
            else:
                delay = self.dec[0].push(self.cat, self.cd, u0, u1, delay, E)
        assert delay == self.la
        first = max(T - self.la, 0)
        last = min(max(u1 - self.la, 0), E)
        sl = slice(first, max(last, first))
        res = (first, self.dec[0].out[sl].clone(), [i[sl, 0].clone() for i in self.idx], [e[sl].clone() for e in self.xq])
        if end:
            self._clear()
        else:
            self.T = T + C
        return res
