"""Shared inputs of the streaming-conversion tests (tests/test_stream_cpu.py, tests/test_gpu_stream.py): seeded causal
generators through the oracle's constructor, codebooks drawn around the quantizers' own inputs, S = 3 streams of T = 150 frames
(more than the 132-frame receptive chain of the default stacks: the last frames depend on every layer's carried state),
the oracle's offline causal forward on them, the per-frame code margins and the chunk schedules."""
import functools

import numpy as np
import torch

from tests.helpers import fill_models, load_yaml, make_batch

T = 150
S = 3
N_SPK = 4
MARGIN = 1e-4        # relative gap between the best and the second-best code below which a frame is left out
MAX_LEFT_OUT = 0.02  # ... and the share of frames that may be

_MIXED = (1, 7, 16, 2, 33, 1)


def _cut(sizes, total=T):
    out, done = [], 0
    for c in sizes:
        if done >= total:
            break
        out.append(min(c, total - done))
        done += out[-1]
    assert done == total
    return out


SCHEDULES = {
    "c1": [1] * T,
    "c3": _cut([3] * T),
    "c16": _cut([16] * T),
    "c40": _cut([40] * T),
    "mixed": _cut(_MIXED * T),
    "whole": [T],
}


def dedup_rows(w):
    """Codebook rows with every exact duplicate of an earlier row removed (a tie is one code for a margin)."""
    _, first = np.unique(w, axis=0, return_index=True)
    return w[np.sort(first)]


def margins(x, w):
    """(second-best - best) / best squared distance of every row of x (N, D) to the distinct rows of w, in float64."""
    x, w = np.asarray(x, np.float64), dedup_rows(np.asarray(w, np.float64))
    d = (x * x).sum(1)[:, None] - 2.0 * x @ w.T + (w * w).sum(1)[None]
    d.sort(axis=1)
    return (d[:, 1] - d[:, 0]) / np.maximum(d[:, 0], 1e-300)


def downstream(mask, reach):
    """mask (S, T) spread `reach` frames forward in time: the frames a causal chain of that receptive field can carry a
    difference at a marked frame to."""
    out = mask.copy()
    for s, t in zip(*np.nonzero(mask)):
        out[s, t: t + reach + 1] = True
    return out


class Fixture:
    def __init__(self, over):
        from crank_amd.stream import receptive_chain
        from oracle.modules import OracleVQVAE2

        self.conf = conf = load_yaml(None, causal=True, **over)
        self.nst = nst = conf["n_vq_stacks"]
        self.orac = orac = OracleVQVAE2(conf, spkr_size=N_SPK).eval()
        fill_models({"G": orac})
        b = make_batch(S, T, N_SPK, in_dim=conf["input_size"], seed=77, full_length=True)
        self.x, self.lcf0, self.uv = b["in_feats"], b["cv_lcf0"], b["uv"]
        self.spk = b["cv_h"][:, 0].clone()
        self.enc_cond = torch.cat([b["lcf0"], b["uv"]], -1) if conf["encoder_f0"] else None
        self.reach = receptive_chain(conf)
        # Codebooks the quantizers' inputs land well inside the cells of: top stack first (a stack's input depends on the
        # codebooks above it), code rows are frames of that input moved by a tenth of its spread, the rest of the book at
        # the input's magnitude.  Where the book is smaller than the fixture (emb_size < S * T) most frames meet codes that
        # were not made for them; the first seed whose margins leave out no more than the tests allow is taken.
        for seed in range(99, 99 + 16):
            self._draw_codebooks(seed)
            self.ref = self.offline(orac)
            self._margins()
            if self.left_out <= MAX_LEFT_OUT:
                break
        self.state = {k: v.clone() for k, v in orac.state_dict().items()}

    def _draw_codebooks(self, seed):
        orac, rs = self.orac, np.random.RandomState(seed)
        with torch.no_grad():
            enc = orac.encode(self.x.transpose(1, 2), enc_h=None if self.enc_cond is None else self.enc_cond.transpose(1, 2))
            dec = 0
            for n in reversed(range(self.nst)):
                xn = enc[n] + dec  # (S, D, T)
                rows = xn.transpose(1, 2).reshape(S * T, -1)
                w = orac.quantizers[n].embedding.weight
                K, spread = w.shape[0], float(rows.std())
                book = torch.from_numpy(rs.standard_normal(tuple(w.shape)).astype(np.float32)) * spread
                pick = torch.from_numpy(rs.permutation(S * T)[: min(K, S * T)])
                book[: len(pick)] = rows[pick] + 0.1 * spread * torch.from_numpy(
                    rs.standard_normal((len(pick), w.shape[1])).astype(np.float32))
                w.copy_(book[torch.from_numpy(rs.permutation(K))])
                if n != 0:
                    dec = orac.decoders[n](orac.quantizers[n](xn, use_ema=False)[1], c=None)

    def _margins(self):
        nst = self.nst
        self.codebooks = [self.orac.quantizers[n].embedding.weight.detach().numpy().copy() for n in range(nst)]
        low = [margins(self.ref["encoded"][n].reshape(S * T, -1).numpy(), self.codebooks[n]).reshape(S, T) <= MARGIN
               for n in range(nst)]
        # a low-margin frame of stack n is left out for stack n, and with everything behind it in the receptive chain for the
        # stacks below n and the decoded features
        self.keep_q, above = [None] * nst, np.zeros((S, T), bool)
        for n in reversed(range(nst)):
            self.keep_q[n] = ~(low[n] | above)
            above = above | downstream(low[n], self.reach)
        self.keep_dec = ~above
        self.left_out = (sum(int((~k).sum()) for k in self.keep_q) + int((~self.keep_dec).sum())) / ((nst + 1) * S * T)

    def dec_cond(self):
        """The last decoder's conditioning as the oracle and the offline forward take it, and their spkrvec."""
        parts = [self.lcf0, self.uv] if self.conf["decoder_f0"] else []
        h = self.spk[:, None].expand(S, T).contiguous()
        if self.conf["use_spkr_embedding"]:
            return (torch.cat(parts, -1) if parts else None), h
        return torch.cat(parts + [torch.nn.functional.one_hot(h, N_SPK).float()], -1), None

    def offline(self, model, dtype=torch.float32):
        dec_h, h = self.dec_cond()
        cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
        with torch.no_grad():
            return model(cast(self.x), cast(self.enc_cond), cast(dec_h), spkrvec=h, use_ema=False)


@functools.lru_cache(maxsize=None)
def _fixture(items):
    return Fixture(dict(items))


def fixture(**over):
    """One Fixture per configuration, built once per process and left unchanged."""
    return _fixture(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in over.items())))


# configurations off the default (test 8 of the issue), by name
VARIANTS = {
    "nvq1": dict(n_vq_stacks=1),
    "nvq3": dict(n_vq_stacks=3, emb_dim=(64, 32, 32)),  # (the last decoder takes sum(emb_dim) <= 128 channels)
    "encf0": dict(encoder_f0=True),
    "onehot": dict(use_spkr_embedding=False),
    "k333": dict(kernel_size=(3, 3, 3)),
    "dim32": dict(emb_dim=(32, 32, 32), emb_size=(64, 64, 64)),
    "mcep35": dict(input_feat_type="mcep", output_feat_type="mcep", input_size=35, output_size=35),
}
