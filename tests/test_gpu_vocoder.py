"""Parallel WaveGAN vocoder inference (crk_voc_*, csrc/vocoder_kernels.hip) against the CPU restatement
tests/pwg_vocoder_ref.py, on ragged batches of 1, 3, 17 and 40 frames.  The restatement's parity against the
third-party parallel_wavegan package is unpinned (the package is not installed)."""
import functools

import numpy as np
import pytest
import torch

from oracle.pwg import bf16_emulation
from tests.pwg_vocoder_ref import checkpoint_of, random_generator

pytestmark = pytest.mark.gpu

LENS = [1, 3, 17, 40]
CONFIGS = {
    "hop128": dict(upsample_params={"upsample_scales": [4, 4, 8]}),
    "hop256": dict(upsample_params={"upsample_scales": [4, 4, 4, 4]}),
    "small": dict(layers=6, stacks=2, upsample_params={"upsample_scales": [2, 4, 4]}),
}


def _hop(name):
    return int(np.prod(CONFIGS[name]["upsample_params"]["upsample_scales"]))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(restated generator without weight norm, vocoder, features, noises, fp32 waveforms, bf16-emulated waveforms)."""
    from crank_amd.vocoder import ParallelWaveGANVocoder

    params = CONFIGS[name]
    g = random_generator(11, **params)
    cfg = {"generator_params": params, "hop_size": _hop(name), "sampling_rate": 22050}
    voc = ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(g), cfg, device="cuda")
    g.remove_weight_norm()
    gen = torch.Generator().manual_seed(5)
    cs = [torch.randn(T, 80, generator=gen) for T in LENS]
    xs = [torch.randn(T * _hop(name), generator=gen) for T in LENS]
    with torch.no_grad():
        ref = [g.inference(c, x) for c, x in zip(cs, xs)]
        with bf16_emulation():
            emu = [g.inference(c, x) for c, x in zip(cs, xs)]
    return g, voc, cs, xs, ref, emu


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_aux_path_alone_matches_fp32_restatement(name):
    g, voc, cs, _, _, _ = _case(name)
    got = voc.upsample_batch(cs)
    torch.cuda.synchronize()
    for c, u in zip(cs, got):
        with torch.no_grad():
            r = g.upsample_aux(c)
        assert u.shape == r.shape
        assert _rel(u, r) <= 1e-5, (len(c), _rel(u, r))
        hop = _hop(name)  # edge frames on their own
        assert _rel(u[:hop], r[:hop]) <= 1e-5 and _rel(u[-hop:], r[-hop:]) <= 1e-5


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16x3_waveform_within_1e3_of_fp32(name):
    from crank_amd import ops

    _, voc, cs, xs, ref, _ = _case(name)
    ops.set_precision("bf16x3")
    try:
        got = voc.inference_batch(cs, xs)
    finally:
        ops.set_precision("bf16")
    for T, y, r in zip(LENS, got, ref):
        assert y.shape == (T * _hop(name),)
        assert _rel(y, r) <= 1e-3, (T, _rel(y, r))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16_waveform_error_within_twice_the_emulation_error(name):
    from crank_amd import ops

    _, voc, cs, xs, ref, emu = _case(name)
    ops.set_precision("bf16")
    got = voc.inference_batch(cs, xs)
    for T, y, r, e in zip(LENS, got, ref, emu):
        assert torch.isfinite(y).all()
        assert _rel(y, r) <= 2 * _rel(e, r), (T, _rel(y, r), _rel(e, r))


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_ragged_batch_is_bit_identical_alone_and_reordered(prec):
    from crank_amd import ops

    _, voc, cs, xs, _, _ = _case("hop128")
    ops.set_precision(prec)
    try:
        batch = voc.inference_batch(cs, xs)
        alone = [voc.inference(c, x) for c, x in zip(cs, xs)]
        order = [2, 0, 3, 1]
        shuffled = voc.inference_batch([cs[i] for i in order], [xs[i] for i in order])
    finally:
        ops.set_precision("bf16")
    for i in range(len(cs)):
        assert torch.equal(batch[i], alone[i]), i
        assert torch.equal(batch[order[i]], shuffled[i]), i


def test_seeded_noise_is_reproducible_and_lengths_are_frames_times_hop():
    _, voc, cs, _, _, _ = _case("small")
    voc.manual_seed(123)
    a = voc.inference_batch(cs)
    b = voc.inference(cs[2])
    voc.manual_seed(123)
    a2 = voc.inference_batch(cs)
    b2 = voc.inference(cs[2])
    for T, y, y2 in zip(LENS, a, a2):
        assert y.shape == (T * _hop("small"),) and torch.equal(y, y2)
    assert torch.equal(b, b2) and not torch.equal(b, a[2])


def test_forward_does_not_allocate_after_the_workspace_is_reserved():
    from crank_amd import _lib

    _, voc, cs, xs, _, _ = _case("hop128")
    voc.reserve(len(cs), sum(LENS))
    voc.inference_batch(cs, xs)
    torch.cuda.synchronize()
    lib = _lib.lib()
    before = lib.crk_debug_alloc_count()
    out = voc.inference_batch(cs, xs)
    torch.cuda.synchronize()
    assert lib.crk_debug_alloc_count() == before
    assert sum(o.numel() for o in out) == sum(LENS) * _hop("hop128")


def test_untrained_vqvae_eval_outputs_vocode_to_finite_waveforms():
    """trainer.eval() of an untrained small VQVAE2 -> _store_features -> vocode_eval_outputs: finite waveforms of
    frames * hop samples per utterance."""
    from crank_amd.vocoder import ParallelWaveGANVocoder
    from tests.helpers import make_batch, run_golden_case
    from tests.test_gpu_step import _hip_factories

    from types import SimpleNamespace as NS

    _, _, trainer, fx, _ = run_golden_case("vqvae", *_hip_factories(), device="cuda", steps=0)
    conf = trainer.conf
    B, T, n_spkrs = [int(v) for v in fx["meta_B_T_nspk_seed_steps"]][:3]
    batch = make_batch(B, T, n_spkrs, in_dim=conf["input_size"], seed=3, device="cuda", use_raw=conf["use_raw"],
                       fftl=conf["feature"]["fftl"], hop_size=conf["feature"]["hop_size"])
    batch.setdefault("flbl", [f"u{n}" for n in range(B)])
    batch.setdefault("org_spkr_name", [f"spk{int(h)}" for h in batch["org_h"][:, 0].tolist()])
    # the decode side needs the feature / F0 scalers (sklearn StandardScaler attributes)
    lcf0 = NS(mean_=np.array([5.0]), scale_=np.array([0.5]), var_=np.array([0.25]))
    D = int(conf["output_size"]) if "output_size" in conf else int(conf["input_size"])
    scaler = {"mlfb": NS(mean_=np.full(D, -2.0), scale_=np.full(D, 1.5), var_=np.full(D, 2.25)), "lcf0": lcf0}
    scaler.update({s: {"lcf0": lcf0} for s in trainer.spkrs})
    trainer.scaler = scaler
    trainer._stats = None
    out = trainer.eval(batch)
    name = sorted(out)[0]
    dicts = trainer._store_features(batch, {"decoded": out[name]}, name)
    D = int(dicts[0]["feats"].shape[-1])
    params = dict(CONFIGS["small"], aux_channels=D)
    g = random_generator(4, **params)
    voc = ParallelWaveGANVocoder.from_checkpoint(checkpoint_of(g), {"generator_params": params, "hop_size": 32},
                                                 stats=(np.zeros(D), np.ones(D)), device="cuda")
    wavs = voc.vocode_eval_outputs(dicts)
    assert len(wavs) == len(dicts)
    for d, y in zip(dicts, wavs):
        assert y.shape == (d["feats"].shape[0] * 32,) and bool(torch.isfinite(y).all())
