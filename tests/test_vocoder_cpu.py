"""Parallel WaveGAN vocoder (recipe stage 6): checkpoint loading, refusals, the restated upsampler and the CLI, on CPU.

The restatement (tests/pwg_vocoder_ref.py) follows the published parallel_wavegan generator; its parity against the
third-party package is unpinned - the package is not installed here."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests.pwg_vocoder_ref import brute_force_upsample, checkpoint_of, random_generator

SMALL = dict(layers=6, stacks=2, aux_channels=80, aux_context_window=2, upsample_params={"upsample_scales": [2, 4, 4]})


def _write(tmp_path, g, params, hop, stats=True):
    ck = tmp_path / "checkpoint.pkl"
    torch.save(checkpoint_of(g), ck)
    cfg = tmp_path / "config.yml"
    cfg.write_text(yaml.safe_dump({"generator_params": params, "hop_size": hop, "sampling_rate": 22050}))
    st = None
    if stats:
        st = tmp_path / "stats.npy"
        np.save(st, np.stack([np.linspace(-5, 0, 80), np.linspace(1, 2, 80)]).astype(np.float32))
    return str(ck), str(cfg), None if st is None else str(st)


def test_from_checkpoint_maps_every_key_and_folds_weight_norm(tmp_path):
    """Every conv of the published layout is found; the folded weights equal the restatement's remove_weight_norm()
    weights at 1e-7; the statistics are read from stats.npy."""
    from crank_amd.vocoder import ParallelWaveGANVocoder

    g = random_generator(0, **SMALL)
    ck, cfg, st = _write(tmp_path, g, SMALL, 32)
    voc = ParallelWaveGANVocoder.from_checkpoint(ck, cfg, stats=st, device="cpu")
    plain = random_generator(0, **SMALL)
    plain.load_state_dict(g.state_dict())
    plain.remove_weight_norm()
    ref = plain.state_dict()
    seen = set()
    for prefix, (w, b) in voc.weights.items():
        r = ref[prefix + "weight"]
        assert w.shape == r.shape, prefix
        assert torch.allclose(w, r, rtol=0, atol=1e-7 * float(r.abs().max())), prefix
        seen.add(prefix + "weight")
        if b is not None:
            assert torch.equal(b, ref[prefix + "bias"])
            seen.add(prefix + "bias")
    assert seen == set(ref), set(ref) ^ seen
    assert voc.hop_size == 32 and voc.sampling_rate == 22050
    assert np.allclose(voc.mean.numpy(), np.linspace(-5, 0, 80)) and np.allclose(voc.scale.numpy(), np.linspace(1, 2, 80))
    f = torch.randn(5, 80)
    assert torch.allclose(voc.normalize(f), (f - voc.mean) / voc.scale)
    # plain (already removed) weights load to the same block
    ck2 = tmp_path / "plain.pkl"
    torch.save(checkpoint_of(plain), ck2)
    voc2 = ParallelWaveGANVocoder.from_checkpoint(str(ck2), cfg, device="cpu")
    assert torch.allclose(voc2.block, voc.block, rtol=0, atol=1e-7)
    n_conv = 1 + 1 + 3 + 4 * 6 + 2
    assert len(voc.weights) == n_conv


def test_from_checkpoint_refuses_missing_and_extra_keys(tmp_path):
    from crank_amd.vocoder import ParallelWaveGANVocoder

    g = random_generator(1, **SMALL)
    _, cfg, _ = _write(tmp_path, g, SMALL, 32, stats=False)
    sd = g.state_dict()
    missing = {k: v for k, v in sd.items() if k != "conv_layers.3.conv1x1_skip.bias"}
    with pytest.raises(KeyError):
        ParallelWaveGANVocoder.from_checkpoint({"model": {"generator": missing}}, cfg, device="cpu")
    missing = {k: v for k, v in sd.items() if not k.startswith("upsample_net.conv_in.")}
    with pytest.raises(KeyError):
        ParallelWaveGANVocoder.from_checkpoint({"model": {"generator": missing}}, cfg, device="cpu")
    extra = dict(sd, **{"conv_layers.6.conv.bias": torch.zeros(128)})
    with pytest.raises(ValueError):
        ParallelWaveGANVocoder.from_checkpoint({"model": {"generator": extra}}, cfg, device="cpu")


@pytest.mark.parametrize("change", [
    {"use_causal_conv": True},
    {"upsample_params": {"upsample_scales": [2, 4, 4], "nonlinear_activation": "LeakyReLU"}},
    {"upsample_params": {"upsample_scales": [2, 4, 4], "freq_axis_kernel_size": 3}},
    {"residual_channels": 32},
    {"gate_channels": 256},
    {"skip_channels": 128},
    {"aux_channels": 129},
    {"upsample_params": {"upsample_scales": [2, 4, 8]}},  # prod 64 != hop 32
    {"upsample_params": {"upsample_scales": [32, 1]}},    # beyond the kernel's 16
])
def test_from_checkpoint_refuses_unsupported_options(tmp_path, change):
    from crank_amd.vocoder import ParallelWaveGANVocoder

    g = random_generator(2, **SMALL)
    params = dict(SMALL, **change)
    ck, cfg, _ = _write(tmp_path, g, params, 32, stats=False)
    with pytest.raises(NotImplementedError):
        ParallelWaveGANVocoder.from_checkpoint(ck, cfg, device="cpu")


@pytest.mark.parametrize("scales,window", [([2, 3], 2), ([4, 4], 1), ([2, 4, 4], 0), ([4, 5, 3, 4], 2), ([2, 3, 5], 5),
                                           ([1, 4, 8], 2), ([16, 16], 0), ([2] * 8, 5)])
def test_restated_upsampler_matches_brute_force(scales, window):
    """The restated ConvInUpsampleNetwork (replicate pad, conv_in, nearest stretch + (1, 2s+1) conv per stage with zero
    padding at each stage's edges) against explicit loops, on short inputs where the edges dominate."""
    g = random_generator(3, layers=2, stacks=1, aux_channels=6, aux_context_window=window,
                         upsample_params={"upsample_scales": scales})
    g.remove_weight_norm()
    for T in (1, 2, 5):
        c = torch.randn(T, 6)
        with torch.no_grad():
            got = g.upsample_aux(c).double().numpy()
        kernels = [g.upsample_net.upsample.up_layers[2 * i + 1].weight.detach().numpy() for i in range(len(scales))]
        ref = brute_force_upsample(c.numpy(), g.upsample_net.conv_in.weight.detach().numpy(), kernels, scales, window)
        assert got.shape == ref.shape == (T * int(np.prod(scales)), 6)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), T


def test_pwg_decode_cli_arguments_and_file_names(tmp_path):
    from crank_amd.bin import pwg_decode

    a = pwg_decode.get_parser().parse_args(["--checkpoint", "c.pkl", "--config", "config.yml", "--stats", "stats.h5",
                                            "--featdir", "feats", "--outdir", "wav"])
    assert (a.checkpoint, a.config, a.stats, a.featdir, a.outdir, a.seed) == ("c.pkl", "config.yml", "stats.h5", "feats", "wav", 0)
    assert pwg_decode.get_parser().parse_args(["--checkpoint", "c", "--config", "c", "--stats", "s", "--featdir", "f",
                                               "--outdir", "o", "--seed", "7"]).seed == 7
    with pytest.raises(SystemExit):
        pwg_decode.get_parser().parse_args(["--checkpoint", "c"])
    for n in ("b_utt", "a_utt.x"):
        np.save(tmp_path / f"{n}.npy", np.zeros((3, 80), np.float32))
    (tmp_path / "notes.txt").write_text("")
    files = pwg_decode.feature_files(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["a_utt.x.npy", "b_utt.npy"]
    assert pwg_decode.wav_name("out", files[0]) == os.path.join("out", "a_utt.x_gen.wav")
    pcm = pwg_decode.to_pcm16(np.array([-2.0, -1.0, 0.0, 0.5, 1.0, 3.0]))
    assert pcm.dtype == np.int16 and pcm.tolist() == [-32768, -32768, 0, 16384, 32767, 32767]
