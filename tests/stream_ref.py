"""A chunked, stateful float64 restatement of the causal generator (TEST INFRASTRUCTURE): what csrc/stream_kernels.hip
implements, stated independently of the GPU.  Every residual layer keeps the last (kernel_size - 1) * dilation frames of
its input, zero at the start - the left zero padding of the oracle's causal convolution - and a push computes only its
new frames.  tests/test_stream_cpu.py holds it to the oracle's offline ``VQVAE2.forward`` in float64."""
import contextlib
import math

import torch

import oracle.modules


def _w(conv):
    """Effective weight of a weight-normed conv: g * v / ||v||."""
    return torch._weight_norm(conv.weight_v.detach().double(), conv.weight_g.detach().double(), 0)


def _b(conv):
    return None if conv.bias is None else conv.bias.detach().double()


class _Net:
    """One causal ParallelWaveGANGenerator (oracle/pwg.py) on frames-first rows, with its layers' carried inputs."""

    def __init__(self, net):
        self.first = (_w(net.first_conv)[:, :, 0], _b(net.first_conv))
        self.layers = []
        for blk in net.conv_layers:
            assert blk.use_causal_conv
            k, dil = blk.conv.kernel_size[0], blk.conv.dilation[0]
            aux = None if blk.conv1x1_aux is None else _w(blk.conv1x1_aux)[:, :, 0]
            self.layers.append(dict(w=_w(blk.conv), b=_b(blk.conv), k=k, dil=dil, aux=aux,
                                    out=(_w(blk.conv1x1_out)[:, :, 0], _b(blk.conv1x1_out)),
                                    skip=(_w(blk.conv1x1_skip)[:, :, 0], _b(blk.conv1x1_skip)),
                                    state=torch.zeros((k - 1) * dil, 64, dtype=torch.float64)))
        self.last1 = (_w(net.last_conv_layers[1])[:, :, 0], _b(net.last_conv_layers[1]))
        self.last2 = (_w(net.last_conv_layers[3])[:, :, 0], _b(net.last_conv_layers[3]))

    @staticmethod
    def _lin(x, wb):
        y = x @ wb[0].t()
        return y if wb[1] is None else y + wb[1]

    def push(self, x, c):
        C = x.shape[0]
        x = self._lin(x, self.first)
        skips = 0
        for y in self.layers:
            halo = (y["k"] - 1) * y["dil"]
            xin = torch.cat([y["state"], x], 0)  # row r is frame r - halo
            g = 0 if y["b"] is None else y["b"]
            for j in range(y["k"]):  # tap j reads frame t - (k - 1 - j) * dil
                g = g + xin[j * y["dil"]: j * y["dil"] + C] @ y["w"][:, :, j].t()
            y["state"] = xin[xin.shape[0] - halo:].clone()
            if c is not None:
                g = g + c @ y["aux"].t()
            z = torch.tanh(g[:, :64]) * torch.sigmoid(g[:, 64:])
            skips = skips + self._lin(z, y["skip"])
            x = (self._lin(z, y["out"]) + x) * math.sqrt(0.5)
        h = torch.relu(skips * math.sqrt(1.0 / len(self.layers)))
        return self._lin(torch.relu(self._lin(h, self.last1)), self.last2)


class StreamRef:
    """One stream of ``orac`` (an OracleVQVAE2 with causal: true), float64."""

    def __init__(self, orac):
        self.nst = orac.conf["n_vq_stacks"]
        self.enc = [_Net(n) for n in orac.encoders]
        self.dec = [_Net(n) for n in orac.decoders]
        self.cb = [q.embedding.weight.detach().double() for q in orac.quantizers]

    def push(self, x, dec_cond, enc_cond=None):
        """x (C, input_size), dec_cond (C, aux of the last decoder), enc_cond (C, 2) or None -> decoded, qidx, encoded
        (bottom stack first, encoded = the quantizers' inputs)."""
        enc, cur = [], x.double()
        for n in range(self.nst):
            cur = self.enc[n].push(cur, enc_cond.double() if (n == 0 and enc_cond is not None) else None)
            enc.append(cur)
        dec, qxs, qidx = 0, [], [None] * self.nst
        for n in reversed(range(self.nst)):
            enc[n] = enc[n] + dec
            qidx[n] = oracle.modules.vq_nearest(enc[n], self.cb[n])
            e = self.cb[n][qidx[n]]
            qxs.append(enc[n] + (e - enc[n]))
            dec = self.dec[n].push(qxs[-1], None) if n != 0 else self.dec[0].push(torch.cat(qxs, 1), dec_cond.double())
        return dec, qidx, enc


class _KeepsDtype(torch.Tensor):
    def float(self):
        return self.as_subclass(torch.Tensor)


class _F:
    """torch.nn.functional with a one_hot whose ``.float()`` keeps float64: the oracle's quantizer looks its code rows up
    as ``one_hot(idx).float() @ codebook``, a row selection in any precision."""

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    @staticmethod
    def one_hot(idx, n):
        return torch.nn.functional.one_hot(idx, n).double().as_subclass(_KeepsDtype)


@contextlib.contextmanager
def oracle_in_float64():
    """Lets an ``OracleVQVAE2.double()`` run its forward: nothing but the dtype of the quantizer's one-hot changes."""
    real = oracle.modules.F
    oracle.modules.F = _F()
    try:
        yield
    finally:
        oracle.modules.F = real
