"""The log-mel front end (crank_amd/csrc/mlfb_kernels.hip: logmel_wave_kernel + lm_prep_kernel for n_fft 1024,
logmel_kernel for every other size and under CRK_LOGMEL_WAVE=0) beyond the one configuration of test_gpu_ops.py.

Every case of tests/logmel_cases.py against its float64 reference, no cell left out, within 10 x the fp32 oracle's own
error + 2^-21 (the recorded ERRORS; tests/test_logmel_cpu.py reproduces them); silent frames bit for bit; then the
properties that need no tolerance (rows of a batch against rows alone at 1, 8 and 32 frame pairs per wave, reads past
the last frame, reflect padding and window padding against the same done on the host, the 8 table slots, streams, graph
capture - also as the first call of a process) and the refusals of the entry point.

The switch between the two kernels is read once per process, so the n_fft 1024 cases of the radix-2 kernel run in a
child process (one at a time, results through an .npz)."""
import functools
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import logmel_cases as C
from tests.helpers import REPO

pytestmark = pytest.mark.gpu

CASES = C.cases()
BY = {c["name"]: c for c in CASES}
IN_PROCESS = [c["name"] for c in CASES if c["kernel"] != "radix2_env"]
ENV_CASES = [c["name"] for c in CASES if c["kernel"] == "radix2_env"]


# ------------------------------------------------------------------------------------------------------ running a case
@functools.lru_cache(maxsize=None)
def sig(name):
    return C.signal(BY[name])


def device_args(case, window=None):
    """(window, basis, mean, std) of a case on the GPU, as LogMelFilterBankLayer builds them."""
    if window is None:
        window = getattr(torch, f"{case['window']}_window")(case["win"], dtype=torch.float32, device="cuda")
    fb = torch.from_numpy(C.basis_of(case)).cuda()
    mean = std = None
    if case["scaler"]:
        s = C.Scaler()
        mean = torch.from_numpy(s.mean_).float().cuda()
        std = torch.from_numpy(s.var_).float().sqrt().cuda()
    return window, fb, mean, std


def call(case, x, T=None, center=None, window=None, win=None, dev=None):
    """ops.logmel with the case's framing on float32 rows x (numpy or cuda tensor); T, center, window overridable.
    dev: device_args() built beforehand (inside a capture nothing may be copied from the host)."""
    from crank_amd import ops

    xg = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    center = case["center"] if center is None else center
    if T is None:
        T = C.n_frames(dict(case, center=center), xg.shape[1])
    w, fb, mean, std = device_args(case, window) if dev is None else dev
    return ops.logmel(xg, T, case["n_fft"], case["hop"], case["win"] if win is None else win, w, fb, C.EPS, mean, std,
                      center=center)


def run_case(case, x=None):
    """What the product returns for a case: the layer for a Slaney basis, ops.logmel for a synthetic one."""
    from crank_amd.net.module.mlfb import LogMelFilterBankLayer

    x = C.signal(case) if x is None else x
    if "basis" in case:
        return call(case, x).cpu().numpy()
    n_mels, fmin, fmax = case["mel"]
    layer = LogMelFilterBankLayer(fs=case["fs"], hop_size=case["hop"], fft_size=case["n_fft"], win_length=case["win"],
                                  window=case["window"], center=case["center"], n_mels=n_mels, fmin=fmin, fmax=fmax,
                                  scaler=C.Scaler() if case["scaler"] else None, eps=C.EPS)
    return layer(torch.from_numpy(x).cuda()).cpu().numpy()


_GOT = {}


def got(name):
    if name not in _GOT:
        _GOT[name] = run_case(BY[name], sig(name))
    return _GOT[name]


def check_against_float64(case, out, x, tag):
    """Both metrics of a result against the float64 reference of the same rows within the case's bounds; silent frames
    exactly the silent value.  Returns (lin, log)."""
    energies = C.mel_energies(case, x)
    assert out.shape == energies.shape and out.dtype == np.float32, (out.shape, energies.shape)
    assert np.isfinite(out).all()
    silent = C.silent_frames(energies)
    if silent.any():
        want = np.broadcast_to(C.silent_value(case), out[silent].shape)
        assert np.array_equal(out[silent], want), (case["name"], "silent frames", float(np.abs(out[silent] - want).max()))
    if case["sig"][0] == "silence":
        assert silent.all()
    lin, log = C.metrics(case, out, energies)
    b_lin, b_log = C.bounds(case["name"])
    print(f'{tag} {case["name"]}: lin {lin} (bound {b_lin}), log10 {log} (bound {b_log}), silent frames {int(silent.sum())}')
    for v, b in ((lin, b_lin), (log, b_log)):
        assert (v is None) == (b is None) or silent.all()
        if v is not None:
            assert v <= b, (case["name"], v, b)
    return lin, log


def test_the_edges_are_reached_before_anything_runs():
    facts = C.edges_reached(CASES)
    assert all(facts.values()), facts
    assert sorted(C.ERRORS) == sorted(BY)


# ------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("name", IN_PROCESS)
def test_case_against_float64(name):
    case = BY[name]
    check_against_float64(case, got(name), sig(name), "wave   " if case["kernel"] == "wave" else "radix-2")


# --------------------------------------------------------------------------------------------------- bit for bit
def _rows_alone(name, rows):
    """Rows of a batch against the same rows computed alone (one row: ppw = 1 for every T of the cases)."""
    case, x, full = BY[name], sig(name), got(name)
    assert (C.n_frames(case) + 1) // 2 <= C.LM_WAVES_PER_ROUND  # a single row gets one frame pair per wave
    for r in rows:
        alone = run_case(case, x[r:r + 1])
        assert alone.shape[1:] == full.shape[1:]
        bad = int((alone[0] != full[r]).sum())
        assert bad == 0, (name, r, bad, float(np.abs(alone[0] - full[r]).max()))


@pytest.mark.parametrize("name,rows", [("B64_bench", (0, 1, 31, 63)), ("B270_ppw_cap", (0, 134, 135, 269)),
                                        ("T37_B3", (0, 1, 2)), ("B5_T129_hop1024", (0, 2, 4)), ("centred_B4", (0, 1, 2, 3)),
                                        ("scaler_centred", (0, 1)), ("r512_T37_B3", (0, 1, 2)), ("r512_centred_B3", (0, 1, 2)),
                                        ("r512_win400", (0, 2))])
def test_every_row_of_a_batch_equals_the_row_alone(name, rows):
    _rows_alone(name, rows)


@pytest.mark.parametrize("name", ["fs22050_hop221", "T1", "T37_B3", "r512_T37_B3", "r2048_hop300_win1200"])
def test_nothing_is_read_past_the_last_frame(name):
    """A row padded to a larger n_samples with T unchanged gives the same bits."""
    case, x = BY[name], sig(name)
    T = C.n_frames(case)
    rng = np.random.default_rng(7)
    for extra in (1, 777):
        xp = np.concatenate([x, (1e3 * rng.standard_normal((x.shape[0], extra))).astype(np.float32)], 1)
        assert np.array_equal(call(case, xp, T=T).cpu().numpy(), call(case, x, T=T).cpu().numpy()), (name, extra)


@pytest.mark.parametrize("name", ["centred_513", "centred_600", "centred_B4", "centred_60s_24k", "r512_centred_B3"])
def test_centred_equals_uncentred_on_the_input_mirrored_on_the_host(name):
    case, x = BY[name], sig(name)
    a = call(case, x).cpu().numpy()
    xp = np.pad(x, ((0, 0), (case["n_fft"] // 2,) * 2), mode="reflect")
    b = call(case, xp, T=C.n_frames(case), center=False).cpu().numpy()
    assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["win800_hamming", "win1023", "win2", "r512_win400", "r2048_hop300_win1200"])
def test_short_window_equals_the_window_zero_padded_on_the_host(name):
    case, x = BY[name], sig(name)
    w = getattr(torch, f"{case['window']}_window")(case["win"], dtype=torch.float32, device="cuda")
    lpad = (case["n_fft"] - case["win"]) // 2
    full = torch.zeros(case["n_fft"], device="cuda")
    full[lpad:lpad + case["win"]] = w
    a = call(case, x, window=w).cpu().numpy()
    b = call(case, x, window=full, win=case["n_fft"]).cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a, got(name)) or "basis" in case  # (the layer builds the same window)


def test_the_eight_table_slots_and_two_streams():
    """24 calls alternating three bases of different n_mels (three times round the 8 slots of lm_prep_kernel's tables)
    each return their first call's bits; so do two calls with different bases on two streams."""
    names = ["fs22050_hop128", "mel20_0_11025", "basis_fill40"]
    assert len({C.basis_of(BY[n]).shape[1] for n in names}) == 3
    first = [call(BY[n], sig(n)).cpu().numpy() for n in names]
    for i in range(24):
        out = call(BY[names[i % 3]], sig(names[i % 3]))
        assert np.array_equal(out.cpu().numpy(), first[i % 3]), i
    xs = [torch.from_numpy(sig(n)).cuda() for n in names[:2]]
    args = [device_args(BY[n]) for n in names[:2]]  # (allocated on the default stream, in front of the side streams)
    torch.cuda.synchronize()
    from crank_amd import ops

    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for rep in range(4):
        for n, x, (w, fb, mean, std), s in zip(names[:2], xs, args, streams):
            c = BY[n]
            with torch.cuda.stream(s):
                outs.append((n, ops.logmel(x, C.n_frames(c), c["n_fft"], c["hop"], c["win"], w, fb, C.EPS, mean, std, center=False)))
    torch.cuda.synchronize()
    for n, o in outs:
        assert np.array_equal(o.cpu().numpy(), first[names.index(n)]), n


def _capture(fn):
    """fn() recorded into one linear graph on a side stream; returns (graph, what fn returned)."""
    from crank_amd.net.trainer.basetrainer import hold_collector_for_capture

    gc_was_on = hold_collector_for_capture()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream(), capture_error_mode="thread_local"):
            out = fn()
    finally:
        if gc_was_on:
            gc.enable()
    return g, out


@pytest.mark.parametrize("name", ["fs22050_hop221", "r512_win400"])
def test_captured_call_replayed_on_a_new_input_equals_the_eager_call(name):
    case = BY[name]
    x = sig(name)
    x2 = np.ascontiguousarray(x[:, ::-1]) * np.float32(0.5)
    want1, want2 = call(case, x).cpu().numpy(), call(case, x2).cpu().numpy()
    assert not np.array_equal(want1, want2)
    buf = torch.from_numpy(x).cuda()
    dev = device_args(case)
    torch.cuda.synchronize()
    g, out = _capture(lambda: call(case, buf, dev=dev))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want1)
    buf.copy_(torch.from_numpy(x2).cuda())
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want2)
    del g


# ------------------------------------------------------------------------------------------------- child processes
_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from tests import logmel_cases as C
from tests import test_gpu_logmel_shapes as G
mode, path, names = sys.argv[1], sys.argv[2], sys.argv[3:]
out = {}
if mode == "cases":
    for n in names:
        out[n] = G.run_case(G.BY[n])
else:
    # the library is loaded and the inputs are on the GPU, but no log-mel call has been made by this process
    from crank_amd import ops
    ops.vq_apply(torch.randn(2, 50, 64, device="cuda"), torch.randn(512, 64, device="cuda"))
    case = G.BY[names[0]]
    x = C.signal(case)
    bufs = [torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(x[:, ::-1])).cuda()]
    dev = G.device_args(case)
    torch.cuda.synchronize()
    if mode == "capture_first":
        g, res = G._capture(lambda: G.call(case, bufs[0], dev=dev))
        out["eager_after_capture"] = G.call(case, bufs[1], dev=dev).cpu().numpy()  # (before any replay)
        g.replay()
        torch.cuda.synchronize()
        out["replayed"] = res.cpu().numpy()
        del g
    else:
        out["replayed"] = G.call(case, bufs[0], dev=dev).cpu().numpy()
        out["eager_after_capture"] = G.call(case, bufs[1], dev=dev).cpu().numpy()
np.savez(path, **out)
"""


def _child(tmp_path, tag, mode, names, env=None):
    f = tmp_path / f"{tag}.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD % REPO, mode, str(f)] + list(names), env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(f)


@pytest.mark.parametrize("name", ["fs22050_hop128"])
def test_first_logmel_call_of_a_process_inside_a_capture(tmp_path, name):
    """The twiddle table of the wave kernel was once filled by a launch behind a process-wide flag: a first call inside
    a capture recorded the fill instead of running it.  A child whose first log-mel call is captured (an eager call
    follows before any replay, then the replay) against a child that makes the same two calls eagerly."""
    a = _child(tmp_path, "capture_first", "capture_first", [name])
    b = _child(tmp_path, "eager", "eager", [name])
    for k in ("eager_after_capture", "replayed"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["replayed"], got(name))


def test_n_fft_1024_through_both_kernels(tmp_path):
    """The n_fft 1024 cases of the radix-2 kernel (CRK_LOGMEL_WAVE=0) and the same through the wave kernel (=1): both
    within their float64 bounds, and the radix-2 result within 10 x oracle error + floor of the wave kernel's."""
    r2 = _child(tmp_path, "wave0", "cases", ENV_CASES, env={"CRK_LOGMEL_WAVE": "0"})
    wv = _child(tmp_path, "wave1", "cases", ENV_CASES, env={"CRK_LOGMEL_WAVE": "1"})
    assert len(ENV_CASES) >= 4
    differ = 0
    for n in ENV_CASES:
        case = BY[n]
        x = C.signal(case)
        check_against_float64(case, r2[n], x, "radix-2")
        check_against_float64(case, wv[n], x, "wave   ")
        a, b = r2[n].astype(np.float64), wv[n].astype(np.float64)
        lin = float((np.abs(10.0 ** a - 10.0 ** b) / (10.0 ** b).max(-1, keepdims=True)).max())
        log = float(np.abs(a - b).max())
        b_lin, b_log = C.bounds(n)
        print(f"radix-2 against wave {n}: lin {lin} (bound {b_lin}), log10 {log} (bound {b_log})")
        assert lin <= b_lin, (n, lin, b_lin)
        if b_log is not None:
            assert log <= b_log, (n, log, b_log)
        differ += int(not np.array_equal(r2[n], wv[n]))
    assert differ > 0  # two kernels: the switch reached the child (the same kernel twice would agree bit for bit)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_reach_python_and_leave_the_output_untouched():
    from crank_amd import _lib, ops

    L = _lib.lib()
    case = BY["fs22050_hop128"]
    x = torch.from_numpy(sig("fs22050_hop128")).cuda()
    B, n = x.shape
    w, fb, _, _ = device_args(case)
    w4096 = torch.ones(4096, device="cuda")
    fb_wide = torch.ones(513, 257, device="cuda")
    good = dict(B=B, n=n, T=C.n_frames(case), n_fft=1024, hop=128, win=1024, n_mels=80, center=0)
    bad = [dict(n_fft=1000, win=1000), dict(n_fft=4096, win=4096), dict(win=1025), dict(n_mels=257), dict(center=1, n=512),
           dict(center=1, n=300), dict(hop=0), dict(hop=-128), dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(n_fft=1, win=1),
           dict(n_fft=0, win=0), dict(win=0), dict(win=-5), dict(n_mels=0)]
    sentinel = 12345.0
    out = torch.full((B, good["T"], 257), sentinel, device="cuda")
    for over in bad:
        a = dict(good, **over)
        rc = L.crk_logmel_fwd(x.data_ptr(), n, a["B"], a["n"], a["T"], a["n_fft"], a["hop"], a["win"], w4096.data_ptr(),
                              fb_wide.data_ptr(), a["n_mels"], C.EPS, 0, 0, out.data_ptr(), 257, a["center"], _lib.stream_ptr())
        assert rc == 1, (over, rc)  # CRK_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    # the same through ops.logmel: an exception, not a result
    for kw in (dict(n_fft=1000, win_length=1000), dict(n_fft=4096, win_length=4096), dict(n_fft=1024, win_length=1025),
               dict(n_fft=1024, win_length=1024, hop=0), dict(n_fft=1024, win_length=1024, T=0), dict(n_fft=1024, win_length=0)):
        a = dict(dict(T=good["T"], hop=128), **kw)
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.logmel(x, a["T"], a["n_fft"], a["hop"], a["win_length"], w4096, fb, C.EPS)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.logmel(x, good["T"], 1024, 128, 1024, w, fb_wide, C.EPS)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.logmel(x[:, :512].contiguous(), 5, 1024, 128, 1024, w, fb, C.EPS, center=True)
    from crank_amd.net.module.mlfb import logmelfilterbank

    with pytest.raises(ValueError):
        logmelfilterbank(sig("fs22050_hop128")[0, :512], 22050, fft_size=1024, hop_size=128, num_mels=80, fmin=80, fmax=7600)
    # and the call still works afterwards
    assert np.array_equal(call(case, x).cpu().numpy(), got("fs22050_hop128"))
