// WORLD waveform synthesis for mel-cepstral models on the device (recipe stage 5 with output_feat_type mcep; gfx950).
//
// Replaces the reference's world2wav (sprocket Synthesizer.synthesis: mod_power, pysptk mc2sp, pyworld
// decode_aperiodicity + synthesize) for a ragged batch of utterances, all in float64.  The oracle is the CPU restatement
// tests/world_synth_ref.py; parity with pyworld / pysptk is unpinned.  Structure:
//  * world_energy_kernel: one wave per (frame, mcep or rmcep): c = freqt(mc, 1024, -alpha) through the precomputed
//    matrix, then SPTK c2ir's recursion h[n] = sum_k k c_k h[n-k] / n with h in LDS and a wave reduction per n; writes
//    sum h^2 (mc2e).  Only with rmcep (power modification).
//  * world_frame_kernel: one thread per (frame, bin): log sp = W . mc' (W = the cosine sum of mc2sp composed with freqt,
//    mc'_0 = mc_0 + log(e_r / e_cv) / 2) and the decoded aperiodicity.
//  * world_timebase_kernel: one workgroup per utterance.  F0 / vuv interpolated in parallel per 2048-sample chunk, the
//    phase accumulated by one thread in sample order (fp contract off: pulse positions are bit-identical to the
//    restatement), fmod, pulse detection and an ordered compaction into the utterance's slots.
//  * world_pulse_kernel: one workgroup per pulse: envelope and ratio, both minimum-phase spectra, the noise spectrum and
//    both inverse transforms in four 1024-point fp64 LDS FFTs (two real sequences per complex transform); writes the
//    pulse's response.
//  * world_ola_kernel: one thread per output sample sums the responses that cover it, in pulse order (no atomics).
// The arithmetic of the first four is csrc/world_frame.h's, one body each, shared with the streaming kernels
// (world_stream_kernels.hip).
#include "../../include/crank_hip.h"
#include "world.h"
#include "world_frame.h"
#include <string.h>

// ---------------------------------------------------------------------------------------------------------- per frame
// mc2e of every frame of mcep (which 0) and rmcep (which 1): e[f * 2 + which].  One wave per item; lane l holds
// k c_k for k = l + 64 j in registers and reads h from its wave's LDS row.
__global__ __launch_bounds__(W_THREADS) void world_energy_kernel(const double* __restrict__ mcep,
                                                                 const double* __restrict__ rmcep, int m1, long long F,
                                                                 const double* __restrict__ at, double* __restrict__ e) {
  __shared__ double hs[W_THREADS / 64][W_IRLEN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * (W_THREADS / 64) + wv;
  if (item >= 2 * F) return;
  const long long f = item >> 1;
  const double* mc = ((item & 1) ? rmcep : mcep) + f * m1;
  double* h = hs[wv];
  const double en = w_energy_row(mc, m1, at, h, lane);
  if (lane == 0) e[item] = en;
}

// sp and decoded ap of every frame: one thread per (frame, bin)
__global__ void world_frame_kernel(const double* __restrict__ mcep, const double* __restrict__ cap, int m1, int bands,
                                   long long F, int fs, const double* __restrict__ wt, const double* __restrict__ e,
                                   double* __restrict__ sp, double* __restrict__ ap) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= F * W_K) return;
  const long long f = idx / W_K;
  const int k = (int)(idx % W_K);
  w_frame_bin(mcep + f * m1, cap + f * bands, m1, bands, fs, k, wt, e ? e + 2 * f : nullptr, sp + idx, ap + idx);
}

// ---------------------------------------------------------------------------------------------------------- time base
struct WTime {
  const double* f0; const long long* foff; const long long* soff;
  int* ppos; double* pshift; unsigned char* pvuv; long long* pcount;
  int fs; double fp;
};

__global__ __launch_bounds__(W_THREADS) void world_timebase_kernel(WTime a) {
#pragma clang fp contract(off)
  __shared__ double ph[W_CHUNK];       // phase increment, then total phase
  __shared__ double wr[W_CHUNK + 1];   // wrapped phase; [0] = the previous chunk's last sample
  __shared__ unsigned char vv[W_CHUNK + 1];
  __shared__ int cnt[W_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long F0 = a.foff[u], S0 = a.soff[u];
  const int T = (int)(a.foff[u + 1] - F0);
  const long long Y = a.soff[u + 1] - S0;
  if (T < 2 || Y < 1) {
    if (tid == 0) a.pcount[u] = 0;
    return;
  }
  const double fsd = (double)a.fs;
  const double* f0 = a.f0 + F0;
  auto row = [&](long long j) { return f0[j]; };
  double total = 0.0;  // thread 0's running phase
  long long base = 0;  // pulses written so far
  for (long long c0 = 0; c0 < Y; c0 += W_CHUNK) {
    const int n = (int)min((long long)W_CHUNK, Y - c0);
    for (int t = tid; t < n; t += W_THREADS) {
      ph[t] = w_phase_increment(c0 + t, T, a.fs, a.fp, row, &vv[t + 1]);
    }
    __syncthreads();
    if (tid == 0) {
      for (int t = 0; t < n; ++t) {
        total = total + ph[t];
        ph[t] = total;
      }
    }
    __syncthreads();
    for (int t = tid; t < n; t += W_THREADS) wr[t + 1] = w_wrap(ph[t]);
    __syncthreads();
    // pulse at sample i = c0 + t - 1 when |wrap[i + 1] - wrap[i]| > pi (t >= 1 in the first chunk)
    const int per = W_CHUNK / W_THREADS, t0 = tid * per, t1 = min(t0 + per, n);
    const int tstart = c0 == 0 ? 1 : 0;
    int mine = 0;
    for (int t = max(t0, tstart); t < t1; ++t) mine += w_is_pulse(wr[t], wr[t + 1]);
    cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int q = 0; q < W_THREADS; ++q) {
        const int c = cnt[q];
        cnt[q] = run;
        run += c;
      }
    }
    __syncthreads();
    long long at = base + cnt[tid];
    for (int t = max(t0, tstart); t < t1; ++t) {
      if (w_is_pulse(wr[t], wr[t + 1])) {
        a.ppos[S0 + at] = (int)(c0 + t - 1);
        a.pshift[S0 + at] = w_pulse_shift(wr[t], wr[t + 1], fsd);
        a.pvuv[S0 + at] = vv[t];
        ++at;
      }
    }
    const int last = cnt[W_THREADS - 1] + (tid == W_THREADS - 1 ? mine : 0);
    __syncthreads();
    if (tid == W_THREADS - 1) cnt[0] = last;  // the chunk's pulse count
    if (tid == 0) {
      wr[0] = wr[n];
      vv[0] = vv[n];
    }
    __syncthreads();
    base += cnt[0];
    __syncthreads();
  }
  if (tid == 0) a.pcount[u] = base;
}

// exclusive scan of the per-utterance pulse counts; poff[n_utts] is the batch's pulse count
__global__ void world_offsets_kernel(const long long* pcount, int n_utts, long long* poff) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long s = 0;
  for (int u = 0; u < n_utts; ++u) {
    poff[u] = s;
    s += pcount[u];
  }
  poff[n_utts] = s;
}

// ---------------------------------------------------------------------------------------------------------- per pulse
struct WPulse {
  const double* sp; const double* ap;
  const long long* foff; const long long* soff; const long long* poff; int n_utts;
  const int* ppos; const double* pshift; const unsigned char* pvuv;
  WPulseTables t;
  double* resp; long long p0;
};

__global__ __launch_bounds__(W_THREADS) void world_pulse_kernel(WPulse a) {
  const long long p = a.p0 + blockIdx.x;
  const int u = w_find(a.poff, a.n_utts, p);
  const long long pu0 = a.poff[u], pu1 = a.poff[u + 1];
  const long long slot = a.soff[u] + (p - pu0);
  const int s = a.ppos[slot];
  const int ns = p + 1 < pu1 ? a.ppos[slot + 1] - s : 0;
  const double shift = a.pshift[slot];
  const double vuv = a.pvuv[slot] ? 1.0 : 0.0;
  const long long nbase = s - a.ppos[a.soff[u]];
  const long long F0 = a.foff[u];
  const int T = (int)(a.foff[u + 1] - F0);
  const double* sp = a.sp + F0 * W_K;
  const double* ap = a.ap + F0 * W_K;
  w_pulse_response(s, T, ns, shift, vuv, nbase, a.t, [&](long long j) { return sp + j * W_K; },
                   [&](long long j) { return ap + j * W_K; }, a.resp + (size_t)blockIdx.x * W_N);
}

// y[g] += the responses of the chunk's pulses that cover sample g, in pulse order
__global__ void world_ola_kernel(const long long* __restrict__ soff, const long long* __restrict__ poff, int n_utts,
                                 long long S, const int* __restrict__ ppos, const double* __restrict__ resp, long long p0,
                                 long long p1, double* __restrict__ y) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= S) return;
  const int u = w_find(soff, n_utts, g);
  const long long i = g - soff[u];
  const long long a0 = max(poff[u], p0), a1 = min(poff[u + 1], p1);
  if (a0 >= a1) return;
  const long long base = soff[u] - poff[u];  // ppos[base + p]: the sample of the utterance's global pulse p
  long long lo = a0, hi = a1;                 // the first pulse with sample >= i - N/2
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (ppos[base + mid] < i - W_N / 2) lo = mid + 1; else hi = mid;
  }
  if (lo >= a1 || ppos[base + lo] > i + W_N / 2 - 1) return;
  double acc = y[g];
  for (long long p = lo; p < a1 && ppos[base + p] <= i + W_N / 2 - 1; ++p) {
    const long long off = ppos[base + p] - W_N / 2 + 1;
    acc = acc + resp[(size_t)(p - p0) * W_N + (i - off)];
  }
  y[g] = acc;
}

// ---------------------------------------------------------------------------------------------------------- host side
// SPTK freqt of the unit vectors: at[i][n] = freqt(e_i, W_IRLEN, -alpha)[n] (n < W_IRLEN; rows 0..N/2 are
// freqt(., N/2, -alpha) too: g_m does not depend on the order)
static void w_freqt_matrix(int m1, double alpha, std::vector<double>& at) {
  at.assign((size_t)m1 * W_IRLEN, 0.0);
  std::vector<double> g, d;
  for (int col = 0; col < m1; ++col) {
    w_freqt_unit(col, m1 - 1, W_IRLEN + 1, -alpha, g, d);
    for (int n = 0; n < W_IRLEN; ++n) at[(size_t)col * W_IRLEN + n] = g[n];
  }
}

extern "C" void* crk_world_create(int fs, int fftl, double shiftms, double alpha, int order1, int bands, int pulse_capacity) {
  if (fftl != W_N || fs < 8000 || fs > 192000 || !(shiftms > 0.0) || !(fabs(alpha) < 1.0) || order1 < 1 ||
      order1 > W_MAX_ORDER1 || bands != w_bands(fs) || bands < 1 || pulse_capacity < 1 || pulse_capacity > (1 << 20))
    return nullptr;
  World* w = new World();
  w->fs = fs; w->m1 = order1; w->bands = bands; w->capacity = pulse_capacity;
  w->shiftms = shiftms; w->fp = shiftms / 1000.0; w->alpha = alpha;
  std::vector<double> at;
  w_freqt_matrix(order1, alpha, at);
  // log sp_k = 2 c0 + 2 sum_{n=1}^{N/2-1} c_n cos(2 pi k n / N) + c_{N/2} cos(pi k), c = at . mc
  std::vector<double> cosn(W_N);
  for (int m = 0; m < W_N; ++m) cosn[m] = cos(2.0 * M_PI * m / W_N);
  std::vector<double> wt((size_t)order1 * W_K, 0.0);
  for (int i = 0; i < order1; ++i)
    for (int k = 0; k < W_K; ++k) {
      double acc = 0.0;
      for (int n = 0; n <= W_N / 2; ++n) {
        const double g = n == W_N / 2 ? 1.0 : 2.0;
        acc += g * cosn[((size_t)k * n) % W_N] * at[(size_t)i * W_IRLEN + n];
      }
      wt[(size_t)i * W_K + k] = acc;
    }
  std::vector<double> dcw(W_N);
  double dc = 0.0;
  for (int i = 0; i < W_N / 2; ++i) {
    dcw[i] = 0.5 - 0.5 * cos(2.0 * M_PI * (i + 1.0) / (1.0 + W_N));
    dcw[W_N - i - 1] = dcw[i];
    dc += dcw[i] * 2.0;
  }
  for (int i = 0; i < W_N / 2; ++i) {
    dcw[i] /= dc;
    dcw[W_N - i - 1] = dcw[i];
  }
  WTables tb;
  const size_t o_at = tb.add(at), o_wt = tb.add(wt), o_tw = tb.add_twiddles(W_N, W_N / 2), o_dc = tb.add(dcw);
  if (!tb.upload(&w->tables)) {
    delete w;
    return nullptr;
  }
  w->at = w->tables + o_at;
  w->wt = w->tables + o_wt;
  w->twc = w->tables + o_tw;
  w->tws = w->twc + W_N / 2;
  w->dcw = w->tables + o_dc;
  return w;
}

extern "C" void crk_world_destroy(void* h) {
  World* w = (World*)h;
  if (!w) return;
  (void)hipFree(w->tables);
  if (w->noise) (void)hipFree(w->noise);
  delete w;
}

// WORLD randn after randn_reseed, max_samples values (one allocation when the table grows; synchronises)
extern "C" int crk_world_reserve(void* h, long long max_samples) {
  World* w = (World*)h;
  if (!w || max_samples < 1 || max_samples > (1LL << 31)) return CRK_ERR_ARG;
  if (max_samples <= w->noise_len) return CRK_OK;
  std::vector<double> v;
  w_randn_table(max_samples, v);
  return w_grow_table(&w->noise, &w->noise_len, max_samples, v.data());
}

struct WWs {
  double *e, *sp, *ap, *pshift, *resp;
  int* ppos; unsigned char* pvuv; long long *pcount, *poff;
  size_t bytes;
};

static WWs w_ws(const World* w, int n_utts, long long F, long long S, unsigned char* base) {
  WWs r;
  WCarve c{base};
  r.e = c.take<double>((size_t)F * 2);
  r.sp = c.take<double>((size_t)F * W_K);
  r.ap = c.take<double>((size_t)F * W_K);
  r.ppos = c.take<int>((size_t)S);
  r.pshift = c.take<double>((size_t)S);
  r.pvuv = c.take<unsigned char>((size_t)S);
  r.pcount = c.take<long long>((size_t)n_utts);
  r.poff = c.take<long long>((size_t)(n_utts + 1));
  r.resp = c.take<double>((size_t)w->capacity * W_N);
  r.bytes = c.bytes;
  return r;
}

extern "C" long long crk_world_workspace_bytes(void* h, int n_utts, long long total_frames, long long total_samples) {
  World* w = (World*)h;
  if (!w || n_utts < 1 || total_frames < 2 || total_samples < 1) return -1;
  return (long long)w_ws(w, n_utts, total_frames, total_samples, nullptr).bytes;
}

static int w_frames(World* w, const double* mcep, const double* rmcep, const double* cap, long long F, double* e,
                    double* sp, double* ap, hipStream_t st) {
  if (rmcep) {
    const long long blocks = (2 * F + W_THREADS / 64 - 1) / (W_THREADS / 64);
    world_energy_kernel<<<dim3((unsigned)blocks), dim3(W_THREADS), 0, st>>>(mcep, rmcep, w->m1, F, w->at, e);
    CRK_CHECK_LAUNCH();
  }
  const long long n = F * W_K;
  world_frame_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(mcep, cap, w->m1, w->bands, F, w->fs,
                                                                             w->wt, rmcep ? e : nullptr, sp, ap);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

static int w_pulses(World* w, const double* f0, const long long* foff, const long long* soff, int n_utts, int* ppos,
                    double* pshift, unsigned char* pvuv, long long* pcount, hipStream_t st) {
  WTime a{f0, foff, soff, ppos, pshift, pvuv, pcount, w->fs, w->fp};
  world_timebase_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, st>>>(a);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_world_frames(void* h, const double* mcep, const double* rmcep, const double* cap, int order1,
                                int bands, long long total_frames, double* sp, double* ap, void* workspace,
                                long long workspace_bytes, void* stream) {
  World* w = (World*)h;
  if (!w || !mcep || !cap || !sp || !ap || total_frames < 1 || !workspace) return CRK_ERR_ARG;
  if (order1 != w->m1 || bands != w->bands) return CRK_ERR_UNSUPPORTED;
  WCarve c{(unsigned char*)workspace};
  double* e = c.take<double>((size_t)total_frames * 2);
  if (workspace_bytes < (long long)c.bytes) return CRK_ERR_ARG;
  return w_frames(w, mcep, rmcep, cap, total_frames, e, sp, ap, (hipStream_t)stream);
}

extern "C" int crk_world_pulses(void* h, const double* f0, const long long* frame_offsets, const long long* sample_offsets,
                                int n_utts, int* pulse_pos, double* pulse_shift, unsigned char* pulse_vuv,
                                long long* pulse_count, void* stream) {
  World* w = (World*)h;
  if (!w || !f0 || !frame_offsets || !sample_offsets || n_utts < 1 || !pulse_pos || !pulse_shift || !pulse_vuv ||
      !pulse_count)
    return CRK_ERR_ARG;
  return w_pulses(w, f0, frame_offsets, sample_offsets, n_utts, pulse_pos, pulse_shift, pulse_vuv, pulse_count,
                  (hipStream_t)stream);
}

extern "C" int crk_world_synthesis(void* h, const double* f0, const double* mcep, const double* rmcep, const double* cap,
                                   int order1, int bands, const long long* frame_offsets, const long long* sample_offsets,
                                   int n_utts, long long total_frames, long long total_samples, long long max_samples,
                                   double* y, long long* n_pulses, void* workspace, long long workspace_bytes,
                                   void* stream) {
  World* w = (World*)h;
  if (!w || !f0 || !mcep || !cap || !frame_offsets || !sample_offsets || !y || !workspace || n_utts < 1 ||
      total_frames < 2 || total_samples < 1 || max_samples < 1 || max_samples > total_samples)
    return CRK_ERR_ARG;
  if (order1 != w->m1 || bands != w->bands) return CRK_ERR_UNSUPPORTED;
  if (max_samples > w->noise_len) return CRK_ERR_ARG;  // crk_world_reserve(max_samples) first
  WWs ws = w_ws(w, n_utts, total_frames, total_samples, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(y, 0, (size_t)total_samples * sizeof(double), st) != hipSuccess) return CRK_ERR_HIP;
  int rc = w_frames(w, mcep, rmcep, cap, total_frames, ws.e, ws.sp, ws.ap, st);
  if (rc) return rc;
  rc = w_pulses(w, f0, frame_offsets, sample_offsets, n_utts, ws.ppos, ws.pshift, ws.pvuv, ws.pcount, st);
  if (rc) return rc;
  world_offsets_kernel<<<1, 1, 0, st>>>(ws.pcount, n_utts, ws.poff);
  CRK_CHECK_LAUNCH();
  // the one device-to-host read of a call: the batch's pulse count sizes the pulse launches
  long long P = 0;
  if (hipMemcpyAsync(&P, ws.poff + n_utts, sizeof(long long), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return CRK_ERR_HIP;
  if (n_pulses) *n_pulses = P;
  for (long long p0 = 0; p0 < P; p0 += w->capacity) {
    const long long np = std::min((long long)w->capacity, P - p0);
    WPulse a{ws.sp, ws.ap, frame_offsets, sample_offsets, ws.poff, n_utts, ws.ppos, ws.pshift, ws.pvuv,
             WPulseTables{w->noise, w->noise_len, w->twc, w->tws, w->dcw, w->fs, w->fp}, ws.resp, p0};
    world_pulse_kernel<<<dim3((unsigned)np), dim3(W_THREADS), 0, st>>>(a);
    CRK_CHECK_LAUNCH();
    world_ola_kernel<<<dim3((unsigned)((total_samples + 255) / 256)), dim3(256), 0, st>>>(
        sample_offsets, ws.poff, n_utts, total_samples, ws.ppos, ws.resp, p0, p0 + np, y);
    CRK_CHECK_LAUNCH();
  }
  return CRK_OK;
}
