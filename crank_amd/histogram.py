"""Per-speaker F0 and frame-power histograms on the device: the reference's "stage 1: initialization"
(crank/bin/generate_histogram.py:31-74,109-146; egs/vaevc/template/run.sh:88-99), whose figures the user reads ``minf0``,
``maxf0`` and ``npow`` of ``conf/spkr.yml`` off.

``extract_f0_and_npow`` analyses every WAV with a wide search range; ``create_histograms`` draws
``plt.hist(np.hstack(f0s), bins=200, range=(40, 700), density=True)`` and the same over (-70, 20) for the frame power.
Here the analysis is ``WorldAnalyzer.analyze_batch`` and ``npow_of_sp_batch`` on ragged batches, and the contours are
reduced where they lie by ``crk_hist_accumulate`` (csrc/histogram_kernels.hip): ``numpy.histogram``'s counts, one row
per speaker.  Only the two count tables and the ``seen`` tallies come back to the host.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from crank_amd import _lib
from crank_amd._lib import check, stream_ptr
from crank_amd._ragged import offsets, require_gpu, size_of

MAX_BINS = 4096  # HG_MAX_BINS


def edges_of(first, last, bins):
    """numpy.histogram's edges of ``bins`` equal bins over (first, last)."""
    return np.linspace(float(first), float(last), int(bins) + 1, endpoint=True, dtype=np.float64)


def density_of(counts, edges):
    """``np.histogram(..., density=True)``: counts / (counts.sum() * diff(edges)), what ``plt.hist(density=True)`` draws;
    divided in numpy's order (by the widths, then by the sum), so the bits are numpy's too."""
    counts = np.asarray(counts)
    return counts / np.diff(np.asarray(edges, np.float64)) / counts.sum()


class HistogramCall:
    """The host and device copies ``crk_hist_accumulate`` takes for one packed batch: utterance offsets and groups.
    ``lens``: values of each utterance in packed order; ``groups``: its group index.  Nothing is checked here that the
    library checks: ``launch`` returns the library's code."""

    def __init__(self, lens, groups, device="cuda"):
        self.device = torch.device(device)
        require_gpu(self.device, "a histogram")
        self.U = len(lens)
        self.start_host = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
        self.group_host = np.ascontiguousarray(np.asarray(groups, np.int32).reshape(-1))
        self.start = offsets(lens, self.device)
        self.group = torch.as_tensor(self.group_host, device=self.device) if self.U else \
            torch.zeros(1, dtype=torch.int32, device=self.device)

    def launch(self, x, G, edges, first, last, bins, counts, seen, U=None):
        """The launch alone (capturable).  x: float64 device vector; edges: float64 device vector of bins + 1;
        counts (G, bins) and seen (G, 3): int64 device tensors, added to.  ``U``: the utterance count handed over, when it is
        not the call's own."""
        for t, dt in ((x, torch.float64), (edges, torch.float64), (counts, torch.int64), (seen, torch.int64)):
            if t.dtype != dt or t.device.type != "cuda" or not t.is_contiguous():
                raise ValueError("x and edges must be contiguous float64, counts and seen contiguous int64 device tensors")
        norm = float(bins) / (float(last) - float(first)) if last != first else float("inf")  # first = last: the library refuses
        return _lib.lib().crk_hist_accumulate(x.data_ptr(), x.numel(), self.start.data_ptr(),
                                              self.start_host.ctypes.data_as(ctypes.c_void_p), self.group.data_ptr(),
                                              self.group_host.ctypes.data_as(ctypes.c_void_p),
                                              self.U if U is None else int(U), int(G), edges.data_ptr(), float(first),
                                              float(last), float(norm), int(bins), counts.data_ptr(), seen.data_ptr(),
                                              stream_ptr())


class Histogram:
    """``G`` rows of ``numpy.histogram(x, bins=bins, range=(first, last))`` kept on the device and added to."""

    def __init__(self, first, last, bins=200, G=1, device="cuda"):
        self.device = torch.device(device)
        require_gpu(self.device, "a histogram")
        self.first, self.last, self.bins = float(first), float(last), int(bins)
        if not 1 <= self.bins <= MAX_BINS:
            raise ValueError(f"{bins} bins: the kernel takes 1 .. {MAX_BINS}")
        if not (np.isfinite(self.first) and np.isfinite(self.last) and self.first < self.last):
            raise ValueError(f"range ({first}, {last}): finite limits with first < last are needed")
        self.edges_host = edges_of(self.first, self.last, self.bins)
        self.edges = torch.as_tensor(self.edges_host, device=self.device)
        self.counts = torch.zeros(int(G), self.bins, dtype=torch.int64, device=self.device)
        self.seen = torch.zeros(int(G), 3, dtype=torch.int64, device=self.device)

    @property
    def G(self):
        return int(self.counts.shape[0])

    def grow(self, G):
        """At least ``G`` rows; the new ones are zero."""
        if G > self.G:
            more = G - self.G
            self.counts = torch.cat([self.counts, self.counts.new_zeros(more, self.bins)])
            self.seen = torch.cat([self.seen, self.seen.new_zeros(more, 3)])

    def launch(self, x, call):
        return call.launch(x, self.G, self.edges, self.first, self.last, self.bins, self.counts, self.seen)


class SpeakerHistograms:
    """What ``generate_histogram.py`` computes for its figures, per speaker: the 200-bin F0 histogram over (40, 700) Hz
    and the 200-bin frame-power histogram over (-70, 20) dB of all the speaker's files.

    ``minf0`` / ``maxf0`` are the analysis search range: what sprocket's ``FeatureExtractor(analyzer="world", fs=fs)`` is
    remembered to default to (unpinned: sprocket is not available to compare with)."""

    def __init__(self, fftl=1024, shiftms=5, minf0=50, maxf0=500, low_cut=70, f0_range=(40, 700), npow_range=(-70, 20),
                 bins=200, device="cuda", max_seconds_per_call=320):
        self.device = torch.device(device)
        self.fftl, self.shiftms, self.minf0, self.maxf0, self.low_cut = fftl, shiftms, minf0, maxf0, low_cut
        self.ranges = {"f0": tuple(f0_range), "npow": tuple(npow_range)}
        self.bins = int(bins)
        if not float(max_seconds_per_call) > 0.0:
            raise ValueError(f"max_seconds_per_call {max_seconds_per_call}: must be positive")
        self.max_seconds = float(max_seconds_per_call)
        self.speakers = {}  # name -> row
        self.n_files = []
        self._analyzers = {}  # fs -> WorldAnalyzer
        self._hists = None

    def _tables(self):
        if self._hists is None:
            self._hists = {k: Histogram(r[0], r[1], self.bins, max(1, len(self.speakers)), self.device)
                           for k, r in self.ranges.items()}
        for h in self._hists.values():
            h.grow(len(self.speakers))
        return self._hists

    def runs(self, seconds):
        """The cut of ``add``: consecutive runs of whole utterances, each at most ``max_seconds_per_call`` seconds of audio
        in total; an utterance longer than that goes alone.  Returns [(begin, end), ...] over the given durations."""
        out, begin, total = [], 0, 0.0
        for i, s in enumerate(seconds):
            if i > begin and total + s > self.max_seconds:
                out.append((begin, i))
                begin, total = i, 0.0
            total += s
        if len(seconds) > begin:
            out.append((begin, len(seconds)))
        return out

    def add(self, waves_by_speaker, fs):
        """Analyse ``{speaker: [waveform, ...]}`` (samples as ``scipy.io.wavfile.read`` returns them: the reference
        analyses them cast to float32 and not rescaled, and so does this) and add the contours to the speakers' tables."""
        from crank_amd.world import HarvestF0, WorldAnalyzer

        require_gpu(self.device, "the speaker histograms")
        spk, raws = [], []
        for name, waves in waves_by_speaker.items():
            for w in waves:
                spk.append(name)
                raws.append(w.detach().reshape(-1).to(torch.float32) if isinstance(w, torch.Tensor)
                            else np.asarray(w, dtype=np.float32).reshape(-1))
        if not raws:
            raise ValueError("no waveform to analyse")
        fs = int(fs)
        if fs not in self._analyzers:
            self._analyzers[fs] = WorldAnalyzer(fs, self.fftl, self.shiftms, self.device)
        wa = self._analyzers[fs]
        if self.shiftms != round(self.shiftms):
            raise ValueError(f"shiftms {self.shiftms}: Harvest takes an integer frame period")
        # Harvest's envelope for the whole corpus, before the first launch
        HarvestF0(fs, int(self.shiftms), self.device).check(raws, [self.minf0] * len(raws), [self.maxf0] * len(raws))
        for name in waves_by_speaker:
            if name not in self.speakers and len(waves_by_speaker[name]):
                self.speakers[name] = len(self.speakers)
                self.n_files.append(0)
        hists = self._tables()
        for begin, end in self.runs([size_of(w) / fs for w in raws]):
            n = end - begin
            f0s, sps = wa.analyze_batch(raws[begin:end], [self.minf0] * n, [self.maxf0] * n, low_cut=self.low_cut)
            npows = wa.npow_of_sp_batch(sps)
            del sps
            lens = [int(f.numel()) for f in f0s]
            groups = [self.speakers[s] for s in spk[begin:end]]
            call = HistogramCall(lens, groups, self.device)
            for key, parts in (("f0", f0s), ("npow", npows)):
                x = torch.cat([p.reshape(-1) for p in parts]).contiguous()
                check(hists[key].launch(x, call), "crk_hist_accumulate")
            for g in groups:
                self.n_files[g] += 1
        return self

    def result(self):
        """{speaker: {"f0": (counts int64 ndarray, edges), "npow": (counts, edges), "n_frames", "n_files"}}: the one
        download."""
        if not self.speakers:
            return {}
        hists = self._tables()
        counts = {k: h.counts.cpu().numpy() for k, h in hists.items()}
        frames = hists["f0"].seen[:, 0].cpu().numpy()
        return {name: {"f0": (counts["f0"][g].copy(), hists["f0"].edges_host.copy()),
                       "npow": (counts["npow"][g].copy(), hists["npow"].edges_host.copy()),
                       "n_frames": int(frames[g]), "n_files": int(self.n_files[g])}
                for name, g in self.speakers.items()}

    def seen(self, which):
        """(G, 3) int64 ndarray of one table: values, values kept in the range, values that are not finite."""
        return self._tables()[which].seen.cpu().numpy()

    def density(self, speaker, which):
        """The heights ``plt.hist(..., density=True)`` draws for one table of one speaker."""
        counts, edges = self.result()[speaker][which]
        return density_of(counts, edges)
