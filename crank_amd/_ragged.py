"""Plumbing the ragged-batch and streaming families share (world.py, griffin_lim.py, vocoder.py, stream.py, live.py,
net/module/mlfb.py, bin/evaluate_mcd.py): offset tensors, input conversion, the grow-only workspace, the device check, the
lifetime of a native handle and the reset of a streaming handle's streams."""
import ctypes

import numpy as np
import torch

from crank_amd import _lib


def offsets(lens, device):
    """int64 [0, cumsum(lens)]: where each utterance starts in the concatenated batch, and the total."""
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=device)


def f64(x, device, dtype=torch.float64):
    """A tensor or anything numpy takes, on ``device`` as ``dtype``."""
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype)
    return torch.as_tensor(np.asarray(x), device=device).to(dtype)


def size_of(x):
    return int(x.numel() if isinstance(x, torch.Tensor) else np.asarray(x).size)


def require_gpu(device, what, whose="the device"):
    if device.type != "cuda":
        raise RuntimeError(f"{what} runs in the HIP kernels: {whose} must be the GPU")


class Workspace:
    """A grow-only uint8 device buffer, kept between calls."""

    def __init__(self, device):
        self.device, self.buf = device, None

    def ensure(self, need, what):
        """The buffer, at least ``need`` bytes; ``what`` names the library's sizing function that returned ``need``."""
        if need < 0:
            raise ValueError(f"{what}: bad shape")
        if self.buf is None or self.buf.numel() < need:
            self.buf = None  # the old block goes before the larger one comes
            self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.buf


def made(handle, create):
    """``handle`` as the library's ``create`` returned it, or RuntimeError when that is null."""
    if not handle:
        raise RuntimeError(f"libcrank_hip: {create} failed (unsupported configuration or HIP error)")
    return handle


def reset_streams(handle, entry, streams, device):
    """The body of a streaming class's ``reset``: the library's ``entry`` (``crk_*_reset``) on ``streams``, or on every
    stream of ``handle`` when that is None, in the current stream of ``device``.  Validates no id: an id the handle does
    not have is the library's CRK_ERR_ARG (a RuntimeError), raised before anything is zeroed."""
    ids = None if streams is None else [int(s) for s in streams]
    arr = None if ids is None else (ctypes.c_int * max(len(ids), 1))(*ids)
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.lib(), entry)(handle, arr, 0 if ids is None else len(ids), _lib.stream_ptr()), entry)


def release(owner, attr, destroy):
    """The body of an owner's ``__del__``: hands the handle, or the dict of handles, in ``owner.attr`` to the library's
    ``destroy``.  Never raises: ``__init__`` may have failed before the attribute existed, the interpreter may be going."""
    try:
        hs = getattr(owner, attr)
        for h in hs.values() if isinstance(hs, dict) else [hs]:
            if h:
                getattr(_lib.lib(), destroy)(h)
    except Exception:
        pass
