"""Griffin-Lim on the device (crank_amd/griffin_lim.py, csrc/griffin_lim_kernels.hip) against the CPU restatement
tests/griffin_lim_ref.py on the cases of tests/griffin_lim_cases.py.

The yardstick of every waveform comparison is the restatement's own rounding: the spread of a case is the largest pairwise
relative-L2 distance between the restatement's results with its three FFT routines (numpy, torch, a plain radix-2 transform
of the kernels' class), computed here on the CPU, never taken from the kernels.  The kernels must lie within MARGIN = 8
spreads of the restatement (its numpy-FFT run): what the spread does not contain is fused multiply-add in the butterflies and
the device's hypot / reciprocal in the phase normalisation, a small constant factor.

Measured on an MI355X (distance to the restatement / spread), the full table is profiles/griffin_lim_ratio_table.csv:
see DESIGN.md section 6d.
"""
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import griffin_lim_cases as C
from tests import griffin_lim_ref as R
from tests.test_griffin_lim_cpu import linear_spectrum_bound

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8
NT = len(R.TRANSFORMS)
_GL = {}


def _gl(key, **kw):
    from crank_amd.griffin_lim import GriffinLim

    if kw:
        return GriffinLim(key[0], C.N_MELS, R.N, key[2], key[1], C.FMIN, C.FMAX, **kw)
    if key not in _GL:
        _GL[key] = GriffinLim(key[0], C.N_MELS, R.N, key[2], key[1], C.FMIN, C.FMAX)
    return _GL[key]


def _groups():
    groups = {}
    for c in C.CASES:
        groups.setdefault(C.config_key(c), []).append(C.materialise(c["name"]))
    return groups


def _np(ys):
    return [y.cpu().numpy() for y in ys]


def _check(label, got, results):
    """got within MARGIN spreads of results[0]; results: the restatement's waveforms, one per transform."""
    sp = R.spread(results)
    dist = R.rel_l2(got, results[0])
    ratio = dist / sp if sp else (0.0 if dist == 0.0 else float("inf"))
    print(f"GLROW,{label},{sp:.3e},{dist:.3e},{ratio:.2f}")
    return None if dist <= MARGIN * sp else f"{label}: distance {dist:.3e} > {MARGIN} x spread {sp:.3e} (ratio {ratio:.2f})"


def test_projections_alone_match_the_restatement():
    bad = []
    for key, cases in _groups().items():
        gl = _gl(key)
        rng = np.random.default_rng(11)
        xs = [rng.standard_normal(c["hop"] * (c["T"] - 1)) for c in cases]
        Xs = gl.stft_batch(xs)
        Ys = []
        for c, x, X in zip(cases, xs, _np(Xs)):
            refs = [R.stft(x, c["hop"], c["win"], t) for t in R.TRANSFORMS]
            assert X.shape == refs[0].shape
            bad.append(_check(f"stft {c['name']}", X, refs))
            Ys.append(refs[0] + 0.3 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)))
        ys = gl.istft_batch(Ys)
        for c, Y, y in zip(cases, Ys, _np(ys)):
            refs = [R.istft(Y, c["hop"], c["win"], t) for t in R.TRANSFORMS]
            assert y.shape == refs[0].shape
            bad.append(_check(f"istft {c['name']}", y, refs))
        # a waveform whose length is no multiple of the hop: 1 + len // hop frames, the reflection at its true end
        c = cases[0]
        x = rng.standard_normal(c["hop"] * (c["T"] - 1) + c["hop"] // 2 + 1)
        X = gl.stft_batch([x])[0].cpu().numpy()
        bad.append(_check(f"stft ragged end {c['name']}", X, [R.stft(x, c["hop"], c["win"], t) for t in R.TRANSFORMS]))
    assert not [b for b in bad if b], [b for b in bad if b]


def test_mel_inversion_within_the_dot_product_bound():
    for key, cases in _groups().items():
        cases = [c for c in cases if c["mlfb"] is not None]
        gl = _gl(key)
        signed = _np(gl.linear_spectrum_batch([c["mlfb"] for c in cases], magnitude=False))
        mags = _np(gl.linear_spectrum_batch([c["mlfb"] for c in cases]))
        for c, s, m in zip(cases, signed, mags):
            pinv = C.pinv_basis(c["fs"])
            assert np.array_equal(gl.pinv_basis(), pinv)
            ref = np.asarray(R.linear_spectrum(c["mlfb"], pinv, np.longdouble), np.float64)
            bound = linear_spectrum_bound(c["mlfb"], pinv)
            err = np.abs(s - ref)
            worst = float((err[bound > 0] / bound[bound > 0]).max())  # bins no filter reaches have a zero row: 0 <= 0
            print(f"{c['name']}: worst error / bound {worst:.3f}")
            assert (err <= bound).all(), c["name"]
            assert np.array_equal(m, np.abs(s))
            if c["kind"] == "rough":
                assert (s < 0).any()


@pytest.mark.parametrize("k", C.KS)
def test_iteration_within_eight_spreads_of_the_restatement(k):
    snaps = C.all_snapshots()
    bad = []
    for key, cases in _groups().items():
        gl = _gl(key)
        ys = _np(gl.griffin_lim_batch([c["S"] for c in cases], n_iters=k, angles=[c["angles"] for c in cases], clip=False))
        for c, y in zip(cases, ys):
            refs = [snaps[(c["name"], i)][k] for i in range(NT)]
            assert y.shape == refs[0].shape == (c["hop"] * (c["T"] - 1),)
            assert np.isfinite(y).all(), c["name"]
            if c["kind"] == "zero":
                assert not y.any() and not refs[0].any()
            bad.append(_check(f"k={k} {c['name']}", y, refs))
    assert not [b for b in bad if b], [b for b in bad if b]


def test_seeded_phases_are_those_of_the_restatement():
    key = (22050, 128, 1024)
    cases = [c for c in _groups()[key] if c["mlfb"] is not None and c["T"] <= 100]
    assert len(cases) >= 3
    gl = _gl(key)
    pinv = C.pinv_basis(22050)
    bad = []
    for seed in (0, 7):
        ys = _np(gl.mlfb2wav_batch([c["mlfb"] for c in cases], n_iters=10, seed=seed))
        for i, (c, y) in enumerate(zip(cases, ys)):
            refs = [R.mlfb2wav(c["mlfb"], pinv, c["hop"], c["win"], 10, seed + i, t) for t in R.TRANSFORMS]
            bad.append(_check(f"seed {seed}+{i} {c['name']}", y, refs))
    assert not [b for b in bad if b], [b for b in bad if b]
    # the reference's names, one utterance: numpy, clipped, the same bits as the batch entry
    from crank_amd import griffin_lim as G

    c = cases[0]
    y = G.mlfb2wav(c["mlfb"], c["fs"], C.N_MELS, R.N, c["win"], c["hop"], C.FMIN, C.FMAX, n_iters=10, seed=0)
    assert isinstance(y, np.ndarray) and np.array_equal(y, _np(gl.mlfb2wav_batch([c["mlfb"]], 10, 0))[0])
    spc = G.logmelspc_to_linearspc(c["mlfb"], c["fs"], C.N_MELS, R.N, C.FMIN, C.FMAX)
    assert np.array_equal(spc, _np(gl.linear_spectrum_batch([c["mlfb"]], magnitude=False))[0])
    assert np.array_equal(G.griffin_lim(spc, R.N, c["hop"], c["win"], n_iters=10, seed=0), y)
    np.random.seed(3)
    a = G.griffin_lim(spc, R.N, c["hop"], c["win"], n_iters=2)
    np.random.seed(3)
    b = _np(gl.griffin_lim_batch([spc], 2, angles=[np.exp(2j * np.pi * np.random.rand(R.K, c["T"])).T]))[0]
    assert np.array_equal(a, b)


def test_bits_do_not_depend_on_the_batch_or_the_chunking():
    key = (22050, 128, 1024)
    base = _groups()[key]
    cases = base + [base[1], base[0]]
    assert len(cases) == 7
    S, A = [c["S"] for c in cases], [c["angles"] for c in cases]
    gl = _gl(key)
    first = gl.griffin_lim_batch(S, 10, angles=A, clip=False)
    again = gl.griffin_lim_batch(S, 10, angles=A, clip=False)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for i in (0, 2, 5):
        alone = gl.griffin_lim_batch([S[i]], 10, angles=[A[i]], clip=False)[0]
        assert torch.equal(alone, first[i]), cases[i]["name"]
    # a cap that holds the longest utterance and little more: several chunks of whole utterances
    from crank_amd.griffin_lim import WS_BYTES_PER_FRAME

    small = _gl(key, workspace_cap=450 * WS_BYTES_PER_FRAME)
    lens = [c["T"] for c in cases]
    assert len(small._chunks(lens)) >= 3
    chunked = small.griffin_lim_batch(S, 10, angles=A, clip=False)
    assert all(torch.equal(a, b) for a, b in zip(first, chunked))
    seeded = gl.griffin_lim_batch(S, 3, seed=5)
    assert all(torch.equal(a, b) for a, b in zip(seeded, small.griffin_lim_batch(S, 3, seed=5)))
    with pytest.raises(ValueError, match="cap"):
        _gl(key, workspace_cap=100 * WS_BYTES_PER_FRAME).griffin_lim_batch(S, 1, angles=A)


def test_outputs_are_clipped_like_the_reference():
    key = (22050, 128, 1024)
    cases = [c for c in _groups()[key] if c["mlfb"] is not None]
    gl = _gl(key)
    lo, hi = -1.0, 0.999969482421875
    for y in gl.mlfb2wav_batch([c["mlfb"] for c in cases], 5, seed=1):
        assert float(y.min()) >= lo and float(y.max()) <= hi
    c = cases[0]
    loud = [c["S"] * 5e3 / c["S"].max()]
    raw = gl.griffin_lim_batch(loud, 5, angles=[c["angles"]], clip=False)[0]
    cl = gl.griffin_lim_batch(loud, 5, angles=[c["angles"]])[0]
    assert float(raw.max()) > 1.0 and float(raw.min()) < -1.0
    assert float(cl.max()) == hi and float(cl.min()) == lo
    assert torch.equal(cl, raw.clamp(lo, hi))


def _raw_run(gl, S, A, lens, n_iter, y, ws, ws_bytes):
    from crank_amd import _lib

    slens = [gl.samples(T) for T in lens]
    foff, soff = gl._offsets(lens), gl._offsets(slens)
    rc = _lib.lib().crk_gl_run(gl.handle(), S.data_ptr(), A.data_ptr(), foff.data_ptr(), soff.data_ptr(), len(lens),
                               sum(lens), sum(slens), n_iter, 0, y.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_short_workspace_is_refused_and_the_compute_entry_does_not_allocate():
    from crank_amd import _lib

    key = (22050, 128, 1024)
    cases = _groups()[key][:3]
    gl = _gl(key)
    lens = [c["T"] for c in cases]
    F, N = sum(lens), sum(gl.samples(T) for T in lens)
    S = torch.cat([torch.as_tensor(c["S"]) for c in cases]).cuda().contiguous()
    A = torch.view_as_real(torch.cat([torch.as_tensor(c["angles"]) for c in cases]).cuda().contiguous())
    need = gl.workspace_bytes(len(lens), F, N)
    ws = gl.reserve(len(lens), F, N)
    assert ws.numel() >= need > 0
    y = torch.full((N,), 123.0, dtype=torch.float64, device="cuda")
    assert _raw_run(gl, S, A, lens, 2, y, ws, need - 1) == 1  # CRK_ERR_ARG
    assert bool((y == 123.0).all()), "a refused call launched something"
    assert _raw_run(gl, S, A, lens, 2, y, ws, need) == 0  # warm: every kernel's code object is loaded
    lib = _lib.lib()
    before, free = lib.crk_debug_alloc_count(), torch.cuda.mem_get_info()[0]
    assert _raw_run(gl, S, A, lens, 10, y, ws, need) == 0
    assert lib.crk_debug_alloc_count() == before and torch.cuda.mem_get_info()[0] == free
    ref = gl.griffin_lim_batch([c["S"] for c in cases], 10, angles=[c["angles"] for c in cases], clip=False)
    assert torch.equal(y, torch.cat(ref))


def _dicts(cases, cv):
    return [{"feats": torch.as_tensor(c["mlfb"], dtype=torch.float32).cuda(), "flbl": f"spk{i}/utt{i}",
             "org_spkr_name": f"spk{i}", "cv_spkr_name": cv} for i, c in enumerate(cases)]


def test_trainer_saves_decoded_mlfb_and_the_cli_converts_a_directory(tmp_path):
    from scipy.io import wavfile

    from crank_amd.bin.pwg_decode import to_pcm16
    from crank_amd.griffin_lim import mlfb2wav
    from crank_amd.net.trainer.basetrainer import BaseTrainer
    from crank_amd.utils import load_yaml

    conf = load_yaml()
    fc = conf["feature"]
    assert (fc["fs"], fc["hop_size"], fc["win_length"], fc["mlfb_dim"], fc["n_iteration"]) == (22050, 128, 1024, 80, 100)
    cases = [c for c in _groups()[(22050, 128, 1024)] if c["mlfb"] is not None and c["T"] <= 100]
    trainer = NS(conf=conf, device=torch.device("cuda"))
    dicts = {"cvA": _dicts(cases[:2], "cvA"), "cvB": _dicts(cases[2:3], "cvB")}
    paths = BaseTrainer._save_decoded_mlfb(trainer, dicts, tmp_path / "wav", n_iters=4, seed=2)
    flat = [d for v in dicts.values() for d in v]
    assert [str(p.relative_to(tmp_path / "wav")) for p in paths] == [
        f"{d['flbl']}_org-{d['org_spkr_name']}_cv-{d['cv_spkr_name']}.wav" for d in flat]
    for i, (p, d) in enumerate(zip(paths, flat)):
        sr, data = wavfile.read(p)
        T = d["feats"].shape[0]
        assert sr == fc["fs"] and data.dtype == np.int16 and data.shape == (fc["hop_size"] * (T - 1),)
        want = mlfb2wav(d["feats"].cpu().numpy(), fc["fs"], fc["mlfb_dim"], fc["fftl"], fc["win_length"], fc["hop_size"],
                        fc["fmin"], fc["fmax"], n_iters=4, seed=2 + i)
        assert np.array_equal(data, to_pcm16(want))
    # n_iters defaults to the configuration's feature.n_iteration
    short = NS(conf={"feature": dict(fc, n_iteration=3)}, device=torch.device("cuda"))
    p3 = BaseTrainer._save_decoded_mlfb(short, dicts["cvB"], tmp_path / "wav3")
    d = dicts["cvB"][0]
    want = mlfb2wav(d["feats"].cpu().numpy(), fc["fs"], fc["mlfb_dim"], fc["fftl"], fc["win_length"], fc["hop_size"],
                    fc["fmin"], fc["fmax"], n_iters=3, seed=0)
    assert np.array_equal(wavfile.read(p3[0])[1], to_pcm16(want))

    # the CLI: a directory of .npy files (one of them not finite: logged and skipped), <stem>.wav out
    root, out = tmp_path / "feats", tmp_path / "cli"
    root.mkdir()
    for i, c in enumerate(cases[:2]):
        np.save(root / f"f{i}.npy", c["mlfb"].astype(np.float32))
    np.save(root / "bad.npy", np.full((20, 80), np.nan, np.float32))
    confp = tmp_path / "conf.yml"
    confp.write_text("feature:\n  n_iteration: 3\n")
    r = subprocess.run([sys.executable, "-m", "crank_amd.bin.griffin_lim", "--conf", str(confp), "--rootdir", str(root),
                        "--outdir", str(out), "--seed", "4"], cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    assert sorted(p.name for p in out.iterdir()) == ["f0.wav", "f1.wav"]
    for i, c in enumerate(cases[:2]):
        sr, data = wavfile.read(out / f"f{i}.wav")
        want = mlfb2wav(c["mlfb"].astype(np.float32), fc["fs"], 80, 1024, 1024, 128, fc["fmin"], fc["fmax"], n_iters=3,
                        seed=4 + i)
        assert sr == 22050 and np.array_equal(data, to_pcm16(want))
