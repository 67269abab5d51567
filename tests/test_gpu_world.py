"""WORLD synthesis for mcep models (crk_world_*, csrc/world_kernels.hip) against the CPU restatement
tests/world_synth_ref.py, on ragged batches of 2, 3, 57 and 400 frames.  The restatement's parity against pyworld /
pysptk / sprocket is unpinned (none of them is installed)."""
import functools

import numpy as np
import pytest
import torch

from tests import world_synth_ref as R
from tests.world_inputs import utterance

pytestmark = pytest.mark.gpu

LENS = [2, 3, 57, 400]
CONFIGS = {"22k": (22050, 35, 0.455), "24k": (24000, 37, 0.466)}
SHIFTS = [10.0, 5.80499]


@functools.lru_cache(maxsize=None)
def _inputs(cfg):
    fs, order1, _ = CONFIGS[cfg]
    rng = np.random.default_rng({"22k": 1, "24k": 2}[cfg])
    return [utterance(rng, T, order1, R.n_bands(fs)) for T in LENS]


@functools.lru_cache(maxsize=None)
def _synth(cfg, shiftms):
    from crank_amd.world import WorldSynthesizer

    fs, _, alpha = CONFIGS[cfg]
    return WorldSynthesizer(fs, 1024, shiftms, alpha)


@functools.lru_cache(maxsize=None)
def _ref(cfg, shiftms, with_r):
    fs, _, alpha = CONFIGS[cfg]
    out = []
    for f0, mc, cap, rm in _inputs(cfg):
        sp, ap = R.frame_tables(mc, cap, rm if with_r else None, fs, 1024, alpha)
        out.append((sp, ap, R.pulses(f0, fs, 1024, shiftms), R.synthesize(f0, sp, ap, fs, shiftms)))
    return out


def _run(cfg, shiftms, with_r, idx=None):
    syn = _synth(cfg, shiftms)
    ins = _inputs(cfg) if idx is None else [_inputs(cfg)[i] for i in idx]
    f0s, mcs, caps, rms = zip(*ins)
    ys = syn.synthesis_batch(list(f0s), list(mcs), list(caps), list(rms) if with_r else None)
    torch.cuda.synchronize()
    return [y.cpu().numpy() for y in ys]


CASES = [(c, s, r) for c in CONFIGS for s in SHIFTS for r in (False, True)]


@pytest.mark.parametrize("cfg,with_r", [(c, r) for c in CONFIGS for r in (False, True)])
def test_frame_tables_match_restatement(cfg, with_r):
    _, _, alpha = CONFIGS[cfg]
    syn = _synth(cfg, 10.0)
    ins = _inputs(cfg)
    got = syn.frame_tables_batch([i[1] for i in ins], [i[2] for i in ins], [i[3] for i in ins] if with_r else None)
    for (sp, ap), (rsp, rap, _, _) in zip(got, _ref(cfg, 10.0, with_r)):
        sp, ap = sp.cpu().numpy(), ap.cpu().numpy()
        assert np.abs(sp / rsp - 1).max() < 1e-12
        assert np.abs(ap / rap - 1).max() < 1e-12


@pytest.mark.parametrize("cfg,shiftms", [(c, s) for c in CONFIGS for s in SHIFTS])
def test_pulse_positions_identical(cfg, shiftms):
    syn = _synth(cfg, shiftms)
    got = syn.pulses_batch([i[0] for i in _inputs(cfg)])
    for (pos, ns, shift, vuv), (_, _, (rpos, rns, rshift, rvuv, _), _) in zip(got, _ref(cfg, shiftms, False)):
        assert np.array_equal(pos, rpos)
        assert np.array_equal(ns, rns)
        assert np.array_equal(vuv, rvuv)
        assert np.array_equal(shift, rshift)


@pytest.mark.parametrize("cfg,shiftms,with_r", CASES)
def test_waveforms_match_restatement(cfg, shiftms, with_r):
    fs = CONFIGS[cfg][0]
    ys = _run(cfg, shiftms, with_r)
    for T, y, (_, _, _, ry) in zip(LENS, ys, _ref(cfg, shiftms, with_r)):
        assert y.shape == (R.y_length(T, fs, shiftms),) == ry.shape
        assert np.isfinite(y).all()
        den = np.linalg.norm(ry)
        if den == 0:  # a single pulse (the last one of its utterance) responds with zeros
            assert np.array_equal(y, ry)
        else:
            assert np.linalg.norm(y - ry) / den < 1e-9, (T, np.linalg.norm(y - ry) / den)


@pytest.mark.parametrize("cfg,with_r", [("22k", True), ("24k", False)])
def test_ragged_batch_bit_identical_to_single_calls_and_repeats(cfg, with_r):
    batch = _run(cfg, 5.80499, with_r)
    again = _run(cfg, 5.80499, with_r)
    for a, b in zip(batch, again):
        assert np.array_equal(a, b)
    for i, y in enumerate(batch):
        assert np.array_equal(_run(cfg, 5.80499, with_r, [i])[0], y)


def test_small_pulse_capacity_gives_the_same_bits():
    """A call whose pulses need several rounds of the response buffer sums in the same order."""
    from crank_amd.world import WorldSynthesizer

    fs, _, alpha = CONFIGS["22k"]
    syn = WorldSynthesizer(fs, 1024, 10.0, alpha, pulse_capacity=37)
    f0s, mcs, caps, rms = zip(*_inputs("22k"))
    ys = syn.synthesis_batch(list(f0s), list(mcs), list(caps), list(rms))
    assert syn.last_pulse_count > 37
    for a, b in zip(ys, _run("22k", 10.0, True)):
        assert np.array_equal(a.cpu().numpy(), b)


def test_no_allocation_after_reserve():
    from crank_amd import _lib

    syn = _synth("24k", 10.0)
    f0s, mcs, caps, rms = zip(*_inputs("24k"))
    syn.synthesis_batch(list(f0s), list(mcs), list(caps), list(rms))
    torch.cuda.synchronize()
    lib = _lib.lib()
    before = lib.crk_debug_alloc_count()
    syn.synthesis_batch(list(f0s), list(mcs), list(caps), list(rms))
    torch.cuda.synchronize()
    assert lib.crk_debug_alloc_count() == before


def test_refusals():
    from crank_amd.world import WorldSynthesizer

    with pytest.raises(ValueError):
        WorldSynthesizer(22050, 2048, 10.0, 0.455)
    syn = _synth("22k", 10.0)
    f0, mc, cap, rm = _inputs("22k")[2]
    with pytest.raises(ValueError):
        syn.synthesis(f0, mc, cap[:, :1])
    with pytest.raises(ValueError):
        syn.synthesis(f0[:1], mc[:1], cap[:1])


def test_stargan_mcep_eval_outputs_synthesise_and_save(tmp_path):
    """trainer.eval() of the untrained stargan_mcep golden scenario -> _store_features (batch with mcep_0th and cap)
    -> vocode_eval_outputs: finite waveforms of int(T * shiftms * fs / 1000) samples; _save_decoded_world writes
    readable 16-bit WAVs named as the reference names them."""
    from types import SimpleNamespace as NS

    from scipy.io import wavfile

    from crank_amd.world import WorldSynthesizer
    from tests.helpers import make_batch, run_golden_case
    from tests.test_gpu_step import _hip_factories

    _, _, trainer, fx, _ = run_golden_case("stargan_mcep", *_hip_factories(), device="cuda", steps=0)
    conf = trainer.conf
    fc = conf["feature"]
    B, T, n_spkrs = [int(v) for v in fx["meta_B_T_nspk_seed_steps"]][:3]
    batch = make_batch(B, T, n_spkrs, in_dim=conf["input_size"], seed=3, device="cuda", use_raw=conf["use_raw"],
                       fftl=fc["fftl"], hop_size=fc["hop_size"])
    batch.setdefault("flbl", [f"u{n}" for n in range(B)])
    batch.setdefault("org_spkr_name", [f"spk{int(h)}" for h in batch["org_h"][:, 0].tolist()])
    g = torch.Generator().manual_seed(7)
    batch["mcep_0th"] = (torch.randn(B, T, 1, generator=g) * 0.2 - 2.0).cuda()
    batch["cap"] = torch.where(batch["uv"].cpu() > 0, torch.full((B, T, R.n_bands(fc["fs"])), -20.0), torch.zeros(B, T, 1)).cuda()
    lcf0 = NS(mean_=np.array([5.0]), scale_=np.array([0.5]), var_=np.array([0.25]))
    trainer.scaler = {"lcf0": lcf0, **{s: {"lcf0": lcf0} for s in trainer.spkrs}}
    trainer._stats = None
    out = trainer.eval(batch)
    name = sorted(out)[0]
    dicts = trainer._store_features(batch, {"decoded": out[name]}, name)
    assert all(d["rmcep"] is not None and d["feats"].shape[-1] == conf["output_size"] + 1 for d in dicts)
    syn = WorldSynthesizer(fc["fs"], fc["fftl"], fc["shiftms"], fc["mcep_alpha"])
    wavs = syn.vocode_eval_outputs(dicts)
    assert len(wavs) == len(dicts)
    for d, y in zip(dicts, wavs):
        assert y.shape == (int(d["feats"].shape[0] * fc["shiftms"] * fc["fs"] / 1000),)
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 1.0
    paths = trainer._save_decoded_world({name: dicts}, tmp_path)
    assert [str(p.relative_to(tmp_path)) for p in paths] == [f"{d['flbl']}_org-{d['org_spkr_name']}_cv-{name}.wav"
                                                             for d in dicts]
    for p, y in zip(paths, wavs):
        sr, data = wavfile.read(p)
        assert sr == fc["fs"] and data.dtype == np.int16 and data.shape == tuple(y.shape)
