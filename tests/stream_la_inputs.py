"""Shared inputs of the look-ahead streaming tests (tests/test_stream_la_cpu.py, tests/test_gpu_stream_la.py,
tests/test_gpu_live_la.py): the fixtures of tests/stream_inputs.py with ``causal: false`` - the same seeded generators, batch
and codebook draw, the oracle's offline NON-causal forward on them - and margins spread ``lookahead_frames`` frames to both
sides of a low-margin frame: a non-causal chain carries a difference as far back as forward."""
import functools

import numpy as np
import torch

from tests.helpers import fill_models, load_yaml, make_batch
from tests.stream_inputs import MARGIN, MAX_LEFT_OUT, N_SPK, S, SCHEDULES, T, VARIANTS, Fixture, margins  # noqa: F401

# the smallest configuration with every mechanism: two stacks, one layer stack of dilations 1 and 2 per net, look-ahead 12,
# rings of different depths (delays 3, 6, 9, 12)
SMALL = dict(n_layers_stacks=(1, 1, 1), kernel_size=(3, 3, 3))


def around(mask, reach):
    """mask (S, T) spread `reach` frames to both sides: the frames a non-causal chain that looks `reach` frames each way
    can carry a difference at a marked frame to."""
    out = mask.copy()
    for s, t in zip(*np.nonzero(mask)):
        out[s, max(t - reach, 0): t + reach + 1] = True
    return out


class LaFixture(Fixture):
    def __init__(self, over):
        from crank_amd.stream import lookahead_frames
        from oracle.modules import OracleVQVAE2

        self.conf = conf = load_yaml(None, causal=False, **over)
        self.nst = conf["n_vq_stacks"]
        self.orac = orac = OracleVQVAE2(conf, spkr_size=N_SPK).eval()
        fill_models({"G": orac})
        b = make_batch(S, T, N_SPK, in_dim=conf["input_size"], seed=77, full_length=True)
        self.x, self.lcf0, self.uv = b["in_feats"], b["cv_lcf0"], b["uv"]
        self.spk = b["cv_h"][:, 0].clone()
        self.enc_cond = torch.cat([b["lcf0"], b["uv"]], -1) if conf["encoder_f0"] else None
        self.la = self.reach = lookahead_frames(conf)
        for seed in range(99, 99 + 16):  # (the draw of tests/stream_inputs.py, on the non-causal quantizer inputs)
            self._draw_codebooks(seed)
            self.ref = self.offline(orac)
            self._margins()
            if self.left_out <= MAX_LEFT_OUT:
                break
        self.state = {k: v.clone() for k, v in orac.state_dict().items()}

    def _margins(self):
        nst = self.nst
        self.codebooks = [self.orac.quantizers[n].embedding.weight.detach().numpy().copy() for n in range(nst)]
        low = [margins(self.ref["encoded"][n].reshape(S * T, -1).numpy(), self.codebooks[n]).reshape(S, T) <= MARGIN
               for n in range(nst)]
        # a low-margin frame of stack n is left out for stack n, and with everything within the look-ahead on either side
        # for the stacks below n and the decoded features
        self.keep_q, near = [None] * nst, np.zeros((S, T), bool)
        for n in reversed(range(nst)):
            self.keep_q[n] = ~(low[n] | near)
            near = near | around(low[n], self.la)
        self.keep_dec = ~near
        self.left_out = (sum(int((~k).sum()) for k in self.keep_q) + int((~self.keep_dec).sum())) / ((nst + 1) * S * T)

    def offline_part(self, model, s, lo, hi, dtype=torch.float32, x=None, lcf0=None, uv=None, enc_cond=None):
        """The offline forward of frames [lo, hi) of stream s as an utterance of their own (batch of one); x, lcf0, uv,
        enc_cond: replacements for the fixture's rows of that stream."""
        dec_h, h = self.dec_cond()
        pick = lambda t, own: None if t is None else (t[s] if own is None else own)[None, lo:hi].to(dtype)  # noqa: E731
        if self.conf["decoder_f0"] and (lcf0 is not None or uv is not None):
            own = torch.cat([self.lcf0[s] if lcf0 is None else lcf0, self.uv[s] if uv is None else uv], -1)
            dec_own = own if self.conf["use_spkr_embedding"] else torch.cat([own, dec_h[s][:, 2:]], -1)
        else:
            dec_own = None
        with torch.no_grad():
            return model(pick(self.x, x), pick(self.enc_cond, enc_cond), pick(dec_h, dec_own),
                         spkrvec=None if h is None else h[s][None, lo:hi], use_ema=False)


@functools.lru_cache(maxsize=None)
def _fixture(items):
    return LaFixture(dict(items))


def fixture(**over):
    """One LaFixture per configuration, built once per process and left unchanged."""
    return _fixture(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in over.items())))
