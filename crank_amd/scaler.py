"""Fitting StandardScalers on the device: what sklearn's ``StandardScaler.partial_fit``, called once per utterance in
file order (the reference's ``Scaler.fit``, crank/bin/extract_statistics.py:27-40), leaves in ``mean_`` / ``var_`` /
``n_samples_seen_``, computed over a corpus packed in HBM by the kernels of csrc/scaler_fit_kernels.hip.

``ScalerFit`` is the two launches: ``moments`` (every utterance's n, sum and corrected two-pass sum of squares, float64)
and ``merge`` (sklearn's update walked over each group's utterances in order, bit for bit sklearn's given the same
moments).  ``scale_`` is formed on the host from the downloaded statistics by sklearn's rule (``scale_of``), and
``make_scaler`` wraps the numbers in a real ``StandardScaler`` when sklearn imports, in a ``FittedScaler`` otherwise.
There is no CPU path: without the library or the GPU every device call raises.
"""
import ctypes

import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, stream_ptr
from crank_amd._ragged import require_gpu

TILE = 64  # SF_TILE
ALIGN = 256


def scale_of(mean, var, n):
    """sklearn's ``scale_`` (preprocessing/_data.py: ``_is_constant_feature`` then ``_handle_zeros_in_scale``): sqrt(var),
    and 1 where the variance is within the two-pass algorithm's error bound of zero."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return scale


def _float_copy(X):
    """A writable copy that keeps float32 / float64 and makes everything else float64, as sklearn's validation does."""
    X = np.asarray(X)
    return np.array(X, dtype=X.dtype if X.dtype in (np.float32, np.float64) else np.float64)


class FittedScaler:
    """The attributes of a fitted sklearn ``StandardScaler`` and its two transforms, for machines without sklearn."""

    def __init__(self, mean, var, n):
        self.mean_ = np.array(mean, np.float64).reshape(-1)
        self.var_ = np.array(var, np.float64).reshape(-1)
        self.n_samples_seen_ = int(n)
        self.scale_ = scale_of(self.mean_, self.var_, self.n_samples_seen_)
        self.n_features_in_ = int(self.mean_.size)
        self.with_mean = self.with_std = self.copy = True

    def transform(self, X):
        X = _float_copy(X)
        X -= self.mean_
        X /= self.scale_
        return X

    def inverse_transform(self, X):
        X = _float_copy(X)
        X *= self.scale_
        X += self.mean_
        return X


def make_scaler(mean, var, n):
    """A fitted ``sklearn.preprocessing.StandardScaler`` carrying the given statistics (so that the reference can load
    the pickle), or a ``FittedScaler`` when sklearn does not import."""
    fitted = FittedScaler(mean, var, n)
    try:
        from sklearn.preprocessing import StandardScaler
    except ImportError:
        return fitted
    ss = StandardScaler()
    ss.mean_, ss.var_, ss.scale_ = fitted.mean_, fitted.var_, fitted.scale_
    ss.n_samples_seen_, ss.n_features_in_ = fitted.n_samples_seen_, fitted.n_features_in_
    return ss


def csr(groups):
    """[[utterance, ...], ...] -> (group_start int64, group_utts int32) numpy arrays."""
    start = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    utts = np.asarray([u for g in groups for u in g], dtype=np.int32).reshape(-1)
    return start, utts


class ScalerFit:
    """The workspace of a corpus of ``U`` utterances and ``D`` columns, and the two launches that fill and read it.
    ``lens``: frames of each utterance in file order (each at least 1)."""

    def __init__(self, lens, D, device="cuda"):
        self.device = torch.device(device)
        self.lens = [int(n) for n in lens]
        self.U, self.D = len(self.lens), int(D)
        if self.U < 1 or self.D < 1:
            raise ValueError("fitting a scaler needs at least one utterance and one column")
        for u, n in enumerate(self.lens):
            if n < 1:
                raise ValueError(f"utterance {u} is empty: sklearn refuses a partial_fit of 0 samples")
        require_gpu(self.device, "fitting a scaler")
        self.start_host = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.start = torch.as_tensor(self.start_host, device=self.device)
        self.tiles = (self.D + TILE - 1) // TILE
        need = int(_lib.lib().crk_scaler_workspace_bytes(self.U, self.D))
        if need < 0:
            raise ValueError("crk_scaler_workspace_bytes: bad shape")
        self.ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        up = lambda b: (b + ALIGN - 1) // ALIGN * ALIGN  # noqa: E731
        o_n = up(self.U * self.tiles * 4)
        o_sum = o_n + up(self.U * 8)
        o_m2 = o_sum + up(self.U * self.D * 8)
        assert o_m2 + up(self.U * self.D * 8) == need, "workspace layout differs from include/crank_hip.h"
        # views of the workspace, as the header lays it out
        self.status = self.ws[: self.U * self.tiles * 4].view(torch.int32).view(self.U, self.tiles)
        self.n = self.ws[o_n : o_n + self.U * 8].view(torch.int64)
        self.sum = self.ws[o_sum : o_sum + self.U * self.D * 8].view(torch.float64).view(self.U, self.D)
        self.m2 = self.ws[o_m2 : o_m2 + self.U * self.D * 8].view(torch.float64).view(self.U, self.D)

    def launch_moments(self, x, col0=0, ws_bytes=None):
        """The launch alone (capturable): x (F_total, ld) float32 on the device, columns [col0, col0 + D).  Returns the
        library's code."""
        if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or x.device.type != "cuda":
            raise ValueError("x must be a 2-D float32 device tensor with unit column stride")
        if x.shape[0] != int(self.start_host[-1]):
            raise ValueError(f"x has {x.shape[0]} frames, the utterances {int(self.start_host[-1])}")
        return _lib.lib().crk_scaler_moments(x.data_ptr(), x.stride(0), int(col0), self.D, x.shape[0], self.start.data_ptr(),
                                             self.start_host.ctypes.data_as(ctypes.c_void_p), self.U, self.ws.data_ptr(),
                                             self.ws.numel() if ws_bytes is None else int(ws_bytes), stream_ptr())

    def moments(self, x, col0=0):
        """Fill the workspace from x; a non-finite value raises ValueError (sklearn's nansum branch is not offered).
        Returns (n, sum, m2): views of the workspace, (U,) int64 and (U, D) float64."""
        check(self.launch_moments(x, col0), "crk_scaler_moments")
        bad = self.status.amax(dim=1).nonzero().reshape(-1).tolist()  # the one synchronisation of a fit
        if bad:
            if int(self.status[bad[0]].max()) == 2:
                raise RuntimeError(f"utterance {bad[0]}: the device offsets do not match the host's")
            raise ValueError(f"utterance {bad[0]} holds a NaN or an infinite value: it cannot be fitted")
        return self.n, self.sum, self.m2

    def set_moments(self, n, s, m2):
        """Put given moments into the workspace (what ``moments`` would have left)."""
        dev = self.device
        self.n.copy_(torch.as_tensor(np.array(n, np.int64).reshape(self.U), device=dev))
        self.sum.copy_(torch.as_tensor(np.array(s, np.float64).reshape(self.U, self.D), device=dev))
        self.m2.copy_(torch.as_tensor(np.array(m2, np.float64).reshape(self.U, self.D), device=dev))

    def prepare_merge(self, groups):
        """Device and host copies of the groups and the output tensors: what ``launch_merge`` takes."""
        if not groups:
            raise ValueError("no group to merge")
        for g, members in enumerate(groups):
            if len(members) < 1:
                raise ValueError(f"group {g} has no utterance")
            if min(members) < 0 or max(members) >= self.U:
                raise ValueError(f"group {g} names an utterance outside 0 .. {self.U - 1}")
        gs, gu = csr(groups)
        dev, G = self.device, len(groups)
        return dict(gs=gs, gu=gu, gs_dev=torch.as_tensor(gs, device=dev), gu_dev=torch.as_tensor(gu, device=dev), G=G,
                    mean=torch.empty(G, self.D, dtype=torch.float64, device=dev),
                    var=torch.empty(G, self.D, dtype=torch.float64, device=dev),
                    count=torch.empty(G, dtype=torch.int64, device=dev))

    def launch_merge(self, p, ws_bytes=None):
        return _lib.lib().crk_scaler_merge(self.ws.data_ptr(), self.ws.numel() if ws_bytes is None else int(ws_bytes), self.U,
                                           self.D, p["gs_dev"].data_ptr(), p["gu_dev"].data_ptr(),
                                           p["gs"].ctypes.data_as(ctypes.c_void_p), p["gu"].ctypes.data_as(ctypes.c_void_p),
                                           p["G"], p["mean"].data_ptr(), p["var"].data_ptr(), p["count"].data_ptr(),
                                           stream_ptr())

    def merge(self, groups):
        """sklearn's running statistics after the utterances of each group, in the order given: (mean (G, D), var (G, D),
        count (G,)) on the device."""
        p = self.prepare_merge(groups)
        check(self.launch_merge(p), "crk_scaler_merge")
        return p["mean"], p["var"], p["count"]

