"""MCD between converted and ground-truth mel-cepstra (crank/bin/evaluate_mcd.py:45-79) for a batch of
utterance pairs in one launch: voiced-frame selection on the host (the features come from files), FastDTW
alignment and the distortion on the device (crk_mcd_fastdtw, one wavefront per pair).

The reference's file handling (HDF5, feats.scp lookup, per-pair summary) is not reproduced; ``mcd_fastdtw`` takes the
arrays ``calculate()`` works on.  ``mcd_fastdtw_from_waveforms`` is the branch for models that write waveforms
(``output_feat_type: mlfb``; evaluate_mcd.py:26-42, 56-57): low cut and WORLD spectral analysis of all converted
waveforms in one batch on the device (crank_amd.world.WorldAnalyzer), then ``mcd_fastdtw``.  With ``cv_f0s=None`` the F0 of
the converted waveform is re-estimated by Harvest (crank_amd.world.HarvestF0) as the reference does; a given contour (the
one the eval stage stored with the utterance and the model was conditioned on) is used as it is.
"""
import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, ptr, stream_ptr
from crank_amd._ragged import offsets


def mcd_fastdtw(cv_mceps, cv_f0s, gt_mceps, gt_f0s, radius=1, return_paths=False, device="cuda"):
    """Lists of per-utterance arrays: mcep (n, D), f0 (n,) or (n, 1).  Returns the list of MCDs in dB
    (and the warping paths as (len, 2) int arrays)."""
    P = len(cv_mceps)
    if not (P == len(cv_f0s) == len(gt_mceps) == len(gt_f0s)) or P == 0:
        raise ValueError("need the same, non-zero number of converted and ground-truth utterances")
    cv, gt = [], []
    for m, f, out in [(a, b, cv) for a, b in zip(cv_mceps, cv_f0s)] + [(a, b, gt) for a, b in zip(gt_mceps, gt_f0s)]:
        m = np.asarray(m, dtype=np.float64)
        out.append(np.ascontiguousarray(m[np.where(np.asarray(f).reshape(-1) > 0)[0]]))  # evaluate_mcd.py:64-67
    D = cv[0].shape[1]
    for a in cv + gt:
        if a.ndim != 2 or a.shape[1] != D:
            raise ValueError("all mel-cepstra must be (frames, D) with the same D")
        if a.shape[0] == 0:
            raise ValueError("an utterance has no voiced frame")
        if not np.isfinite(a).all():
            # the package's backtrack dies on these (KeyError); the kernel would return a truncated path and a NaN
            raise ValueError("a voiced frame holds a non-finite value")
    nx, ny = [a.shape[0] for a in cv], [a.shape[0] for a in gt]
    dev = torch.device(device)
    up = lambda arrs: torch.as_tensor(np.concatenate(arrs), device=dev)  # noqa: E731
    x, y, xo, yo = up(cv), up(gt), offsets(nx, dev), offsets(ny, dev)
    L = _lib.lib()
    mx, my = max(nx), max(ny)
    nbytes = L.crk_mcd_scratch_bytes(P, mx, my, D, radius)
    if nbytes < 0:
        raise ValueError("unsupported sizes")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mcd = torch.empty(P, dtype=torch.float64, device=dev)
    plen = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    stride = 2 * (mx + my)
    paths = torch.empty(P, stride, dtype=torch.int32, device=dev) if return_paths else None
    check(L.crk_mcd_fastdtw(ptr(x), ptr(xo), ptr(y), ptr(yo), P, D, radius, mx, my, ptr(mcd), ptr(plen), ptr(paths), stride,
                            ptr(scratch), ptr(status), stream_ptr()), "mcd_fastdtw")
    if int(status.max()) != 0:
        raise RuntimeError("crk_mcd_fastdtw: a pair exceeded the scratch sizing")
    vals = mcd.cpu().tolist()
    if not return_paths:
        return vals
    lens = plen.cpu().tolist()
    pc = paths.cpu().numpy()
    return vals, [pc[i, : 2 * lens[i]].reshape(-1, 2) for i in range(P)]


def mcd_fastdtw_from_waveforms(cv_waves, cv_f0s, gt_mceps, gt_f0s, conf, radius=1, return_paths=False, device="cuda",
                               analyzer=None, f0_ranges=None):
    """MCD of converted WAVEFORMS against ground-truth mel-cepstra.  cv_waves: per-utterance waveforms at
    conf["feature"]["fs"]; cv_f0s: their F0 contours (one value per analysis frame of shiftms; > 0 voiced), which set the
    number of frames and select the voiced ones; gt_mceps / gt_f0s as in ``mcd_fastdtw``.  The 0th coefficient stays in,
    as in the reference.  cv_f0s=None: the contours are re-estimated from the low-cut converted waveforms, as the reference
    does, and f0_ranges = [(minf0, maxf0), ...], the target speakers' search ranges, is required."""
    from crank_amd.world import WorldAnalyzer

    feat = conf["feature"]
    if analyzer is None:
        analyzer = WorldAnalyzer(feat["fs"], feat["fftl"], feat["shiftms"], device=device)
    if cv_f0s is None:
        if f0_ranges is None or len(f0_ranges) != len(cv_waves):
            raise ValueError("cv_f0s=None needs f0_ranges, one (minf0, maxf0) per converted waveform")
        cv_f0s, _ = analyzer.analyze_batch(cv_waves, [r[0] for r in f0_ranges], [r[1] for r in f0_ranges], low_cut=70)
    cv_mceps = analyzer.mcep_batch(cv_waves, cv_f0s, feat["mcep_dim"], feat["mcep_alpha"], low_cut=70)
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    return mcd_fastdtw([to_np(m) for m in cv_mceps], [to_np(f) for f in cv_f0s], gt_mceps, gt_f0s, radius, return_paths,
                       device)
