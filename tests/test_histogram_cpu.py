"""The host side of the speaker histograms (crank_amd.histogram, crank_amd.bin.generate_histogram, utils.read_wav): what
needs no GPU.  The header <-> ctypes <-> library comparison of tests/test_oracle_cpu.py covers crk_hist_accumulate."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

from crank_amd.bin import generate_histogram as GH
from crank_amd.histogram import SpeakerHistograms, density_of, edges_of
from crank_amd.utils import read_wav

FS = 16000


def _tone(n, f0=200.0):
    return (8000.0 * np.sin(2 * np.pi * f0 * np.arange(n) / FS)).astype(np.int16)


def _tree(root, layout):
    """{speaker: [file name, ...]} as int16 WAVs under root."""
    for spkr, names in layout.items():
        os.makedirs(os.path.join(root, spkr), exist_ok=True)
        for k, name in enumerate(names):
            wavfile.write(os.path.join(root, spkr, name), FS, _tone(800 + 16 * k))


def test_read_wav_returns_unscaled_float32_and_refuses_stereo(tmp_path):
    x = _tone(1000)
    wavfile.write(str(tmp_path / "a.wav"), FS, x)
    fs, got = read_wav(tmp_path / "a.wav")
    assert fs == FS and got.dtype == np.float32 and got.shape == (1000,)
    assert np.array_equal(got, x.astype(np.float32))  # int16-valued floats: not divided by 32768
    assert np.abs(got).max() > 1000.0
    wavfile.write(str(tmp_path / "st.wav"), FS, np.stack([x, x], 1))
    with pytest.raises(ValueError, match="st.wav"):
        read_wav(tmp_path / "st.wav")


def test_speaker_and_file_discovery_and_the_skip_rule(tmp_path):
    wav_dir, fig_dir = tmp_path / "wav", tmp_path / "fig"
    _tree(str(wav_dir), {"TM1": ["b.wav", "a.wav"], "SF1": ["z.wav"], "SM2": ["q.wav"]})
    (wav_dir / "README.txt").write_text("not a speaker")
    (wav_dir / "SF1" / "notes.txt").write_text("not a wav")
    assert GH.speakers_of(wav_dir) == ["SF1", "SM2", "TM1"]
    assert GH.speakers_of(wav_dir, "TM1") == ["TM1"]
    assert [p.name for p in GH.wav_files(wav_dir, "TM1")] == ["a.wav", "b.wav"]
    assert [p.name for p in GH.wav_files(wav_dir, "SF1")] == ["z.wav"]
    paths = GH.figure_paths(fig_dir, "SF1")
    assert paths["f0"].name == "SF1_f0histogram.png" and paths["npow"].name == "SF1_npowhistogram.png"
    assert paths["npz"].name == "SF1_histogram.npz"
    assert GH.pending(wav_dir, fig_dir) == ["SF1", "SM2", "TM1"]
    fig_dir.mkdir()
    paths["f0"].write_bytes(b"")  # either figure is enough to skip the speaker
    GH.figure_paths(fig_dir, "TM1")["npow"].write_bytes(b"")
    GH.figure_paths(fig_dir, "SM2")["npz"].write_bytes(b"")  # the .npz alone is not
    assert GH.pending(wav_dir, fig_dir) == ["SM2"]
    assert GH.pending(wav_dir, fig_dir, "SF1") == []
    assert GH.pending(wav_dir, fig_dir, "SM2") == ["SM2"]


def test_arguments_are_the_references():
    args = GH.get_parser().parse_args(["--n_jobs", "4", "--spkr", "SF1", "wavs", "figs"])
    assert (args.n_jobs, args.spkr, args.wav_dir, args.figure_dir) == (4, "SF1", "wavs", "figs")
    args = GH.get_parser().parse_args(["wavs", "figs"])
    assert args.spkr is None


@pytest.mark.parametrize("first,last", [(40, 700), (-70, 20)])
def test_density_is_numpys(first, last):
    rng = np.random.default_rng(5)
    x = rng.normal((first + last) / 2.0, (last - first) / 3.0, 5000)
    counts, edges = np.histogram(x, bins=200, range=(first, last))
    want, _ = np.histogram(x, bins=200, range=(first, last), density=True)
    assert np.array_equal(edges_of(first, last, 200), edges)
    assert np.array_equal(density_of(counts, edges), want)
    assert abs(float((density_of(counts, edges) * np.diff(edges)).sum()) - 1.0) < 1e-12


def test_runs_cut_whole_utterances_in_order():
    h = SpeakerHistograms(device="cpu", max_seconds_per_call=10)
    assert h.runs([4, 4, 4, 11, 1, 9, 0.5]) == [(0, 2), (2, 3), (3, 4), (4, 6), (6, 7)]
    assert h.runs([10]) == [(0, 1)] and h.runs([]) == []
    assert SpeakerHistograms(device="cpu", max_seconds_per_call=0.1).runs([1, 2, 3]) == [(0, 1), (1, 2), (2, 3)]


def test_figures_are_written_from_given_counts(tmp_path):
    plt = GH.pyplot()
    assert plt is not None, "matplotlib (Agg) is installed where the tests run"
    rng = np.random.default_rng(6)
    res = {"n_frames": 3000, "n_files": 2}
    for key, (first, last) in (("f0", (40, 700)), ("npow", (-70, 20))):
        res[key] = np.histogram(rng.uniform(first, last, 3000), bins=200, range=(first, last))
    GH.write_speaker(tmp_path / "deep" / "fig", "SF1", res, plt)
    paths = GH.figure_paths(tmp_path / "deep" / "fig", "SF1")
    for key in ("f0", "npow"):
        assert paths[key].read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    z = np.load(str(paths["npz"]))
    assert sorted(z.files) == ["f0_counts", "f0_edges", "n_files", "n_frames", "npow_counts", "npow_edges"]
    assert np.array_equal(z["f0_counts"], res["f0"][0]) and np.array_equal(z["npow_edges"], res["npow"][1])
    assert int(z["n_frames"]) == 3000 and int(z["n_files"]) == 2
    # the patches drawn from counts are those plt.hist draws from the data
    x = rng.uniform(40, 700, 500)
    heights, _, _ = plt.hist(x, bins=200, range=(40, 700), density=True, histtype="stepfilled")
    plt.close()
    counts, edges = np.histogram(x, bins=200, range=(40, 700))
    again, again_edges, _ = plt.hist(edges[:-1], bins=edges, weights=density_of(counts, edges), histtype="stepfilled")
    plt.close()
    assert np.array_equal(again_edges, edges) and np.allclose(again, heights, rtol=1e-12, atol=0)
    # a table without a kept value still gives a figure
    GH.write_figure(plt, np.zeros(200, np.int64), edges, tmp_path / "empty.png", 50, "Fundamental frequency [Hz]")
    assert (tmp_path / "empty.png").stat().st_size > 0


def test_there_is_no_cpu_path():
    h = SpeakerHistograms(device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        h.add({"SF1": [_tone(1600).astype(np.float32)]}, FS)
