// The spectral half of WORLD analysis on the device (gfx950): low-cut filter, CheapTrick spectral envelope, sp2mc and
// normalised power for a ragged batch of waveforms and a GIVEN F0 contour per utterance, all in float64.
//
// Replaces what the reference's evaluate_mcd.py runs on a converted waveform (crank.utils.low_cut_filter, sprocket
// FeatureExtractor.analyze / .mcep / .npow: pyworld cheaptrick, pysptk sp2mc, sprocket spc2npow) except F0 estimation and
// aperiodicity.  The oracle is the CPU restatement tests/world_analysis_ref.py; parity with pyworld / pysptk is unpinned.
// Structure; the arithmetic of a sample and of a frame is in wana_frame.h, one body each, which the
// streaming kernels (wana_stream_kernels.hip) call too:
//  * wana_lowcut_kernel: one thread per output sample, the taps in LDS, float32 in, float64 out, zero history at each
//    utterance's start.
//  * wana_offsets_kernel: one workgroup per utterance: every frame's shape integers (wa_shape) and the exclusive prefix
//    sum of the frames' randn draw counts (2 * half + 1 window draws, then 513).
//  * wana_cheaptrick_kernel: one workgroup per frame.  Window with its three reductions, FFT, power, DC correction,
//    the mirrored cumulative spectrum (summed by one thread in the restatement's order), the two band-edge reads per bin, log, FFT of the even log
//    spectrum, lifter, FFT, exp: three 1024-point fp64 LDS FFTs (signal_common.h) per frame.  Writes sp and / or the
//    liftered cepstrum.  No atomics: a frame's result does not depend on the batch around it.
//  * wana_mcep_kernel: one wave per frame: mcep = A c, A the (order + 1) x 513 freqt matrix folded over the even
//    cepstrum (c0 / 2 included), made once per handle.  c is the liftered cepstrum of the last CheapTrick stage, which
//    is irfft(log sp) up to the rounding of exp and log.
//  * wana_power_kernel / wana_npow_kernel: per-frame power by one wave, then the utterance's mean in a fixed order.
#include "../../include/crank_hip.h"
#include "signal_common.h"
#include "wana.h"
#include "wana_frame.h"

#define WA_TILE 256           // output samples per workgroup of the low-cut kernel

__global__ __launch_bounds__(W_THREADS) void wana_offsets_kernel(const double* __restrict__ f0,
                                                                 const long long* __restrict__ foff, int fs, double shiftms,
                                                                 long long* __restrict__ doff, int* __restrict__ shapes) {
  __shared__ long long cnt[W_THREADS];
  __shared__ long long total;
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long F0 = foff[u], T = foff[u + 1] - F0;
  long long base = 0;
  for (long long c0 = 0; c0 < T; c0 += W_THREADS) {
    const long long i = c0 + tid;
    long long mine = 0;
    if (i < T) {
      const WaShape s = wa_shape(f0[F0 + i], i, fs, shiftms);
      mine = 2 * s.half + 1 + W_K;
      if (shapes) {
        int* o = shapes + (F0 + i) * 4;
        o[0] = s.origin; o[1] = s.half; o[2] = s.dc; o[3] = s.bound;
      }
    }
    cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) {
      long long run = base;
      for (int q = 0; q < W_THREADS; ++q) {
        const long long c = cnt[q];
        cnt[q] = run;
        run += c;
      }
      total = run;
    }
    __syncthreads();
    if (i < T) doff[F0 + i] = cnt[tid];
    base = total;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------- low cut
__global__ __launch_bounds__(WA_TILE) void wana_lowcut_kernel(const float* __restrict__ x, const double* __restrict__ taps,
                                                              int n_taps, const long long* __restrict__ soff, int n_utts,
                                                              long long S, double* __restrict__ y) {
  __shared__ double h[WA_MAX_TAPS];
  for (int k = threadIdx.x; k < n_taps; k += WA_TILE) h[k] = taps[k];
  __syncthreads();
  const long long g = (long long)blockIdx.x * WA_TILE + threadIdx.x;
  if (g >= S) return;
  const int u = w_find(soff, n_utts, g);
  const long long i = g - soff[u];
  const float* xu = x + soff[u];
  y[g] = wa_lowcut_sample(h, n_taps, i, [&](long long q) { return xu[q]; });
}

// ---------------------------------------------------------------------------------------------------------- CheapTrick
struct WaFrame {
  const double* x; const double* f0;
  const long long* foff; const long long* soff; const long long* doff; int n_utts;
  const double* noise; long long noise_len;
  const double* twc; const double* tws;
  double* sp; double* cep;
  int fs; double shiftms;
};

__global__ __launch_bounds__(W_THREADS) void wana_cheaptrick_kernel(WaFrame a) {
  const long long f = blockIdx.x;
  const int u = w_find(a.foff, a.n_utts, f);
  const long long S0 = a.soff[u], xlen = a.soff[u + 1] - S0;
  const double* xs = a.x + S0;
  const WaShape sh = wa_shape(a.f0[f], f - a.foff[u], a.fs, a.shiftms);
  const WaTables t{a.noise, a.noise_len, a.twc, a.tws, a.fs};
  wa_cheaptrick_frame([&](long long idx) { return xs[idx]; }, xlen, sh, a.doff[f], t, a.sp ? a.sp + f * W_K : nullptr,
                      a.cep ? a.cep + f * W_K : nullptr);
}

// mcep[f][m] = sum_k at[m][k] cep[f][k]: one wave per frame, lane l holds cep[l + 64 j]
__global__ __launch_bounds__(W_THREADS) void wana_mcep_kernel(const double* __restrict__ cep, long long F,
                                                              const double* __restrict__ at, int m1,
                                                              double* __restrict__ mc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long f = (long long)blockIdx.x * (W_THREADS / 64) + wv;
  if (f >= F) return;
  wa_mcep_frame(cep + f * W_K, at, m1, lane, [&](int m, double v) { mc[f * m1 + m] = v; });
}

// ---------------------------------------------------------------------------------------------------------- power
__global__ __launch_bounds__(W_THREADS) void wana_power_kernel(const double* __restrict__ sp, long long F,
                                                               double* __restrict__ p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long f = (long long)blockIdx.x * (W_THREADS / 64) + wv;
  if (f >= F) return;
  double acc = 0.0;
  for (int k = lane; k < W_K; k += 64) acc += sp[f * W_K + k] * ((k == 0 || k == W_K - 1) ? 1.0 : 2.0);
  acc = w_wave_sum(acc);
  if (lane == 0) p[f] = acc / W_N;
}

__global__ __launch_bounds__(W_THREADS) void wana_npow_kernel(const double* __restrict__ p,
                                                              const long long* __restrict__ foff,
                                                              double* __restrict__ npow) {
  __shared__ double red[4];
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long F0 = foff[u], T = foff[u + 1] - F0;
  double part = 0.0;
  for (long long i = tid; i < T; i += W_THREADS) part += p[F0 + i];
  const double mean = w_block_sum(part, red) / (double)T;
  for (long long i = tid; i < T; i += W_THREADS) npow[F0 + i] = 10.0 * log10(p[F0 + i] / mean);
}

// ---------------------------------------------------------------------------------------------------------- host side
// at[m][k], k <= N/2: SPTK freqt(., order, alpha) of the even cepstrum c (N values, c[N - k] = c[k], c[0] halved) as a
// matrix on c[0 .. N/2]: column k carries freqt(e_k) + freqt(e_{N-k}) for 0 < k < N/2 and freqt(e_0) / 2 for k = 0.
static void wa_freqt_matrix(int m1, double alpha, std::vector<double>& at) {
  at.assign((size_t)m1 * W_K, 0.0);
  std::vector<double> g, d;
  for (int col = 0; col < W_N; ++col) {
    w_freqt_unit(col, col, m1, alpha, g, d);  // the input is zero above `col`
    const int k = col <= W_N / 2 ? col : W_N - col;
    const double scale = col == 0 ? 0.5 : 1.0;
    for (int m = 0; m < m1; ++m) at[(size_t)m * W_K + k] += scale * g[m];
  }
}

extern "C" void* crk_wana_create(int fs, int fftl, double shiftms, double alpha, int order1) {
  if (fftl != W_N || fs < 8000 || fs > 192000 || !(shiftms > 0.0) || !(fabs(alpha) < 1.0) || order1 < 1 ||
      order1 > WA_MAX_ORDER1)
    return nullptr;
  Wana* w = new Wana();
  w->fs = fs; w->m1 = order1; w->shiftms = shiftms; w->alpha = alpha;
  std::vector<double> at;
  wa_freqt_matrix(order1, alpha, at);
  WTables tb;
  const size_t o_tw = tb.add_twiddles(W_N, W_N / 2), o_at = tb.add(at);
  // D4C at the rates whose two transforms are D4_N points: its twiddles and the Nuttall window of the band slices
  const bool d4 = fs >= D4_FS_MIN && fs <= D4_FS_MAX;
  size_t o_tw2 = 0, o_nut = 0;
  if (d4) {
    w->d4_half = (int)(3000.0 * D4_N / fs);
    w->d4_bands = (int)(fmin(15000.0, fs / 2.0 - 3000.0) / 3000.0);
    const int len = 2 * w->d4_half + 1;
    std::vector<double> nut(len);
    for (int i = 0; i < len; ++i) {
      const double u = i / (len - 1.0);
      nut[i] = 0.355768 - 0.487396 * cos(2.0 * M_PI * u) + 0.144232 * cos(4.0 * M_PI * u) - 0.012604 * cos(6.0 * M_PI * u);
    }
    o_tw2 = tb.add_twiddles(D4_N, D4_N / 2);
    o_nut = tb.add(nut);
  }
  if (!tb.upload(&w->tables)) {
    delete w;
    return nullptr;
  }
  w->twc = w->tables + o_tw;
  w->tws = w->twc + W_N / 2;
  w->at = w->tables + o_at;
  if (d4) {
    w->twc2 = w->tables + o_tw2;
    w->tws2 = w->twc2 + D4_N / 2;
    w->nuttall = w->tables + o_nut;
  }
  return w;
}

extern "C" void crk_wana_destroy(void* h) {
  Wana* w = (Wana*)h;
  if (!w) return;
  (void)hipFree(w->tables);
  if (w->noise) (void)hipFree(w->noise);
  delete w;
}

// WORLD randn after randn_reseed, max_draws values (one allocation when the table grows; synchronises)
extern "C" int crk_wana_reserve(void* h, long long max_draws) {
  Wana* w = (Wana*)h;
  if (!w || max_draws < 1 || max_draws > (1LL << 31)) return CRK_ERR_ARG;
  if (max_draws <= w->noise_len) return CRK_OK;
  std::vector<double> v;
  w_randn_table(max_draws, v);
  return w_grow_table(&w->noise, &w->noise_len, max_draws, v.data());
}

struct WaWs {
  long long* doff; double* cep; double* p;
  size_t bytes;
};

static WaWs wa_ws(long long F, unsigned char* base) {
  WaWs r;
  WCarve c{base};
  r.doff = c.take<long long>((size_t)F);
  r.cep = c.take<double>((size_t)F * W_K);
  r.p = c.take<double>((size_t)F);
  r.bytes = c.bytes;
  return r;
}

extern "C" long long crk_wana_workspace_bytes(int n_utts, long long total_frames, long long total_samples) {
  if (n_utts < 1 || total_frames < 1 || total_frames > (1LL << 31) - 1 || total_samples < 1) return -1;
  return (long long)wa_ws(total_frames, nullptr).bytes;
}

extern "C" int crk_wana_lowcut(void* h, const float* x, const double* taps, int n_taps, const long long* sample_offsets,
                               int n_utts, long long total_samples, double* y, void* stream) {
  Wana* w = (Wana*)h;
  if (!w || !x || !taps || !sample_offsets || !y || n_utts < 1 || total_samples < 1) return CRK_ERR_ARG;
  if (n_taps < 1 || n_taps > WA_MAX_TAPS) return CRK_ERR_UNSUPPORTED;
  const long long blocks = (total_samples + WA_TILE - 1) / WA_TILE;
  if (blocks > (1LL << 31) - 1) return CRK_ERR_UNSUPPORTED;
  wana_lowcut_kernel<<<dim3((unsigned)blocks), dim3(WA_TILE), 0, (hipStream_t)stream>>>(x, taps, n_taps, sample_offsets,
                                                                                        n_utts, total_samples, y);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_wana_lowcut_tile(void) { return WA_TILE; }

extern "C" int crk_wana_frame_shapes(void* h, const double* f0, const long long* frame_offsets, int n_utts,
                                     long long total_frames, int* shapes, long long* draw_offsets, void* stream) {
  Wana* w = (Wana*)h;
  if (!w || !f0 || !frame_offsets || n_utts < 1 || total_frames < 1 || !shapes || !draw_offsets) return CRK_ERR_ARG;
  wana_offsets_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, (hipStream_t)stream>>>(f0, frame_offsets, w->fs, w->shiftms,
                                                                                draw_offsets, shapes);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

static int wa_frames(Wana* w, const double* x, const double* f0, const long long* foff, const long long* soff, int n_utts,
                     long long F, long long S, long long max_draws, double* sp, bool want_cep, void* workspace,
                     long long workspace_bytes, hipStream_t st, WaWs* out) {
  if (!w || !x || !f0 || !foff || !soff || !workspace || n_utts < 1 || F < 1 || F > (1LL << 31) - 1 || S < 1 ||
      max_draws < 1)
    return CRK_ERR_ARG;
  if (max_draws > w->noise_len) return CRK_ERR_ARG;  // crk_wana_reserve(max_draws) first
  WaWs ws = wa_ws(F, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  wana_offsets_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, st>>>(f0, foff, w->fs, w->shiftms, ws.doff, nullptr);
  CRK_CHECK_LAUNCH();
  WaFrame a{x, f0, foff, soff, ws.doff, n_utts, w->noise, w->noise_len, w->twc, w->tws, sp, want_cep ? ws.cep : nullptr,
            w->fs, w->shiftms};
  wana_cheaptrick_kernel<<<dim3((unsigned)F), dim3(W_THREADS), 0, st>>>(a);
  CRK_CHECK_LAUNCH();
  *out = ws;
  return CRK_OK;
}

extern "C" int crk_wana_cheaptrick(void* h, const double* x, const double* f0, const long long* frame_offsets,
                                   const long long* sample_offsets, int n_utts, long long total_frames,
                                   long long total_samples, long long max_draws, double* sp, void* workspace,
                                   long long workspace_bytes, void* stream) {
  if (!sp) return CRK_ERR_ARG;
  WaWs ws;
  return wa_frames((Wana*)h, x, f0, frame_offsets, sample_offsets, n_utts, total_frames, total_samples, max_draws, sp,
                   false, workspace, workspace_bytes, (hipStream_t)stream, &ws);
}

extern "C" int crk_wana_mcep(void* h, const double* x, const double* f0, const long long* frame_offsets,
                             const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                             long long max_draws, int order1, double* mcep, double* sp, void* workspace,
                             long long workspace_bytes, void* stream) {
  Wana* w = (Wana*)h;
  if (!w || !mcep) return CRK_ERR_ARG;
  if (order1 != w->m1) return CRK_ERR_UNSUPPORTED;
  WaWs ws;
  const int rc = wa_frames(w, x, f0, frame_offsets, sample_offsets, n_utts, total_frames, total_samples, max_draws, sp,
                           true, workspace, workspace_bytes, (hipStream_t)stream, &ws);
  if (rc) return rc;
  const long long blocks = (total_frames + W_THREADS / 64 - 1) / (W_THREADS / 64);
  wana_mcep_kernel<<<dim3((unsigned)blocks), dim3(W_THREADS), 0, (hipStream_t)stream>>>(ws.cep, total_frames, w->at,
                                                                                        w->m1, mcep);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_wana_npow(void* h, const double* sp, const long long* frame_offsets, int n_utts, long long total_frames,
                             double* npow, void* workspace, long long workspace_bytes, void* stream) {
  Wana* w = (Wana*)h;
  if (!w || !sp || !frame_offsets || !npow || !workspace || n_utts < 1 || total_frames < 1 ||
      total_frames > (1LL << 31) - 1)
    return CRK_ERR_ARG;
  WaWs ws = wa_ws(total_frames, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  const long long blocks = (total_frames + W_THREADS / 64 - 1) / (W_THREADS / 64);
  wana_power_kernel<<<dim3((unsigned)blocks), dim3(W_THREADS), 0, (hipStream_t)stream>>>(sp, total_frames, ws.p);
  CRK_CHECK_LAUNCH();
  wana_npow_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, (hipStream_t)stream>>>(ws.p, frame_offsets, npow);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
