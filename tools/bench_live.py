"""The live conversion loop on one MI355X: milliseconds per push of 1024 samples at 16 kHz / hop 128 for S concurrent
streams of a ``decoder_f0`` model (default generator shapes with ``causal: true``, a Parallel WaveGAN generator of the
published shapes with hop 128), in the steady state of a long voiced signal, two ways in ONE process, alternating push by
push on the same samples:

  live   ``crank_amd.live.LiveConverter.push``: the rows of the two front ends are paired by ``crk_join_push`` on the
         device, de-scaled and normalised by ``crk_feat_renorm``; no count is read back;
  host   the loop INTEGRATION.md section O documented before ``LiveConverter``: the same four public stages, joined by
         Python queues per stream (``n_frames.tolist()`` on both front ends, ``torch.cat`` to grow and shrink the
         queues, padding into fresh tensors, ``voc.normalize(dec * scale + mean)``), converter and vocoder sized at
         ``sl.max_frames + sf.max_frames`` frames.

A push is timed on the host clock from the call to the end of a device synchronise behind it (the host loop's read-backs
are part of what it costs).  Four pushes of five complete an 80 ms F0 block and run Harvest, the fifth does not: the
percentiles show both kinds.  Both loops are given kept buffers of zero noise (the host loop one per chunk width).  Beside them, replayed from a graph: the join's two
launches and the renorm launch alone (HIP events, bursts).  Prints one JSON line per S and writes the table to
profiles/live_bench_mi355x.txt.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FS, HOP, N_FFT, N_MELS, PUSH, N_SPK = 16000, 128, 1024, 80, 1024, 4


def signal(S, n, seed=0):
    """S voiced signals of n samples: eight harmonics of a slowly gliding fundamental plus a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    xs = []
    for s in range(S):
        f0 = rng.uniform(100, 250) * (1 + 0.1 * np.sin(2 * np.pi * rng.uniform(0.3, 1.0) * t))
        ph = 2 * np.pi * np.cumsum(f0) / FS
        y = sum(rng.uniform(0.05, 0.3) * np.sin(h * ph + rng.uniform(0, 6.28)) for h in range(1, 9))
        xs.append(y + 1e-3 * rng.standard_normal(n))
    return torch.from_numpy(np.stack(xs).astype(np.float32)).cuda()


class HostLoop:
    def __init__(self, G, layer, voc, S, scaler, spk_mean, spk_std):
        from crank_amd.stream import StreamingConverter
        from crank_amd.world import StreamingF0

        self.S, self.voc = S, voc
        self.sl = layer.streaming(S, PUSH)
        self.sf = StreamingF0(FS, [70.0] * S, [400.0] * S, spk_mean, spk_std, PUSH, hop_size=HOP,
                              lcf0_scaler=(float(scaler["lcf0"].mean_[0]), float(scaler["lcf0"].scale_[0])))
        K = self.sl.max_frames + self.sf.max_frames
        self.conv, self.sv = StreamingConverter(G, S, K), voc.streaming(S, K)
        self.mean = torch.as_tensor(scaler["mlfb"].mean_, dtype=torch.float32, device="cuda")
        self.scale = torch.as_tensor(scaler["mlfb"].scale_, dtype=torch.float32, device="cuda")
        self.mel_q = [torch.zeros(0, N_MELS, device="cuda") for _ in range(S)]
        self.f0_q = [torch.zeros(0, 2, device="cuda") for _ in range(S)]
        self.noise = {}  # frames -> kept zero noise, as the live loop is given a kept one

    def push(self, x, org, cv, counts, end):
        S, mel_q, f0_q = self.S, self.mel_q, self.f0_q
        ended = torch.tensor(end, device="cuda")
        fr = self.sl.push(x, n_valid=torch.tensor(counts, device="cuda"), end=ended)
        f0 = self.sf.push(x, org, cv, n_valid=counts, end=end)
        nm, nf = fr["n_frames"].tolist(), f0["n_frames"].tolist()
        for s in range(S):
            mel_q[s] = torch.cat([mel_q[s], fr["feats"][s, :nm[s]]])
            f0_q[s] = torch.cat([f0_q[s], torch.cat([f0["lcf0"][s, :nf[s]], f0["uv"][s, :nf[s]]], -1)])
        take = [min(len(m), len(f)) for m, f in zip(mel_q, f0_q)]
        K = max(max(take), 1)
        feats, lcf0, uv = (torch.zeros(S, K, w, device="cuda") for w in (N_MELS, 1, 1))
        for s in range(S):
            k = take[s]
            feats[s, :k], lcf0[s, :k], uv[s, :k] = mel_q[s][:k], f0_q[s][:k, :1], f0_q[s][:k, 1:]
            mel_q[s], f0_q[s] = mel_q[s][k:], f0_q[s][k:]
        n = torch.tensor(take, device="cuda")
        dec = self.conv.push(feats, lcf0, uv, cv.long(), n_valid=n)["decoded"]
        if K not in self.noise:
            self.noise[K] = torch.zeros(S, K * HOP, device="cuda")
        return self.sv.push(self.voc.normalize(dec * self.scale + self.mean), self.noise[K], n_valid=n, end=ended)


def events(fn, warmup, reps, burst):
    """(median, 10th, 90th percentile) of microseconds per call, HIP events around bursts."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / burst)
    return [float(np.percentile(us, q)) for q in (50, 10, 90)]


def launches_alone(lc, S):
    """The join's push and the renorm launch, each replayed from a graph with the steady state's counts (8 new rows on
    both sides, nothing waiting: the state a replay leaves is the state it found)."""
    from crank_amd.live import feat_renorm

    j = lc.join
    a, b = torch.randn(S, j.max_in_a, j.width_a, device="cuda"), torch.randn(S, j.max_in_b, j.width_b, device="cuda")
    n = torch.full((S,), PUSH // HOP, dtype=torch.int32, device="cuda")
    out = j.empty_outputs(S)
    j.reset()
    j.push(a, n, b, n, out=out)
    x, y = torch.randn(S, lc.max_chunk, N_MELS, device="cuda"), torch.empty(S, lc.max_chunk, N_MELS, device="cuda")
    feat_renorm(x, lc._scale, lc._mean, lc._vmean, lc._vscale, n, y)
    torch.cuda.synchronize()
    gj, gr = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gj):
        j.push(a, n, b, n, out=out)
    with torch.cuda.graph(gr):
        feat_renorm(x, lc._scale, lc._mean, lc._vmean, lc._vscale, n, y)
    res = events(gj.replay, 5, 15, 50), events(gr.replay, 5, 15, 50)
    j.reset()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--warmup", type=int, default=20, help="pushes of each loop before the timed ones (the first 480 ms of a "
                    "stream have shorter Harvest windows)")
    ap.add_argument("--reps", type=int, default=100, help="timed pushes of each loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_bench_mi355x.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_live needs the MI355X"
    from bench_voc_stream import random_vocoder
    from crank_amd.live import LiveConverter
    from crank_amd.net.module.mlfb import LogMelFilterBankLayer
    from crank_amd.net.module.vqvae2 import VQVAE2
    from crank_amd.utils import load_yaml

    conf = load_yaml(None, causal=True)
    assert conf["decoder_f0"] and not conf["encoder_f0"]
    torch.manual_seed(0)
    G = VQVAE2(conf, spkr_size=N_SPK).eval()
    rs = np.random.RandomState(0)
    layer = LogMelFilterBankLayer(fs=FS, hop_size=HOP, fft_size=N_FFT, n_mels=N_MELS, fmin=80, fmax=7600, center=True,
                                  scaler=types.SimpleNamespace(mean_=-4.0 + 0.5 * rs.standard_normal(N_MELS),
                                                               var_=rs.uniform(0.5, 1.5, N_MELS)))
    voc = random_vocoder({"upsample_params": {"upsample_scales": [2, 4, 4, 4]}})
    voc.mean = torch.as_tensor(rs.standard_normal(N_MELS), dtype=torch.float32, device="cuda")
    voc.scale = torch.as_tensor(rs.uniform(0.5, 2.0, N_MELS), dtype=torch.float32, device="cuda")
    scaler = {"mlfb": types.SimpleNamespace(mean_=rs.standard_normal(N_MELS), scale_=rs.uniform(0.5, 2.0, N_MELS)),
              "lcf0": types.SimpleNamespace(mean_=np.array([5.0]), scale_=np.array([0.3]))}
    spk_mean, spk_std = np.array([4.9, 5.3, 4.6, 5.1]), np.array([0.21, 0.17, 0.3, 0.25])
    n_push = args.warmup + args.reps
    rows = []
    for S in args.streams:
        lc = LiveConverter(G, layer, voc, S, PUSH, [70.0] * S, [400.0] * S, spk_mean, spk_std, scaler)
        host = HostLoop(G, layer, voc, S, scaler, spk_mean, spk_std)
        x = signal(S, n_push * PUSH)
        org = torch.arange(S, dtype=torch.int32, device="cuda") % N_SPK
        cv = (org + 1) % N_SPK
        out, noise = lc.empty_outputs(S), torch.zeros(S, lc.max_chunk * HOP, device="cuda")
        counts, end = [PUSH] * S, [0] * S
        ms = {"live": [], "host": []}
        frames = 0
        for i in range(n_push):
            chunk = x[:, i * PUSH:(i + 1) * PUSH].contiguous()
            for name in ("live", "host") if i % 2 == 0 else ("host", "live"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "live":
                    lc.push(chunk, org, cv, n_valid=counts, end=end, noise=noise, out=out)
                else:
                    res = host.push(chunk, org, cv, counts, end)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            if i >= args.warmup:
                frames += int(res["n_out"][0]) // HOP
        lc.status()
        host.sf.status()
        assert abs(frames - args.reps * PUSH // HOP) <= lc.max_chunk, "the timed pushes are not the steady state"
        join_us, renorm_us = launches_alone(lc, S)
        pct = lambda v: [round(float(np.percentile(v, q)), 3) for q in (50, 10, 90)]  # noqa: E731
        r = {"metric": "live_push", "streams": S, "samples": PUSH, "fs": FS, "hop": HOP, "reps": args.reps,
             "live_ms_p50_p10_p90": pct(ms["live"]), "host_ms_p50_p10_p90": pct(ms["host"]),
             "host_over_live": round(float(np.median(ms["host"]) / np.median(ms["live"])), 2),
             "real_time_factor": round(float(np.median(ms["live"])) / (PUSH / FS * 1e3), 4),
             "join_us_p50_p10_p90": [round(v, 1) for v in join_us], "renorm_us_p50_p10_p90": [round(v, 1) for v in renorm_us],
             "max_chunk": lc.max_chunk, "host_max_chunk": host.sl.max_frames + host.sf.max_frames,
             "state_bytes": lc.state_bytes, "latency_ms": round(lc.latency_ms, 1)}
        print(json.dumps(r), flush=True)
        rows.append(r)
        del lc, host
    f3 = lambda v: f"{v[0]:8.3f} ({v[1]:.3f} - {v[2]:.3f})"  # noqa: E731
    f1 = lambda v: f"{v[0]:6.1f} ({v[1]:.1f} - {v[2]:.1f})"  # noqa: E731
    lines = [f"LiveConverter.push vs the host loop of four stages and Python queues, alternating in one process: {FS} Hz, hop {HOP}, "
             f"n_fft {N_FFT}, pushes of {PUSH} samples, steady state, zero noise; ms per push incl. a device synchronise, median "
             f"(10th - 90th percentile) of {args.reps} pushes; join / renorm alone: us per graph replay, 15 bursts of 50",
             f"{'S':>3}  {'live ms':>26}  {'host ms':>26}  {'host/live':>9}  {'RTF':>6}  {'join us':>22}  {'renorm us':>22}"]
    for r in rows:
        lines.append(f"{r['streams']:>3}  {f3(r['live_ms_p50_p10_p90']):>26}  {f3(r['host_ms_p50_p10_p90']):>26}  "
                     f"{r['host_over_live']:>9.2f}  {r['real_time_factor']:>6.3f}  {f1(r['join_us_p50_p10_p90']):>22}  "
                     f"{f1(r['renorm_us_p50_p10_p90']):>22}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
