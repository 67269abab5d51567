// The spectral half of WORLD analysis on the device (gfx950): low-cut filter, CheapTrick spectral envelope, sp2mc and
// normalised power for a ragged batch of waveforms and a GIVEN F0 contour per utterance, all in float64.
//
// Replaces what the reference's evaluate_mcd.py runs on a converted waveform (crank.utils.low_cut_filter, sprocket
// FeatureExtractor.analyze / .mcep / .npow: pyworld cheaptrick, pysptk sp2mc, sprocket spc2npow) except F0 estimation and
// aperiodicity.  The oracle is the CPU restatement tests/world_analysis_ref.py; parity with pyworld / pysptk is unpinned.
// Structure:
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

#define WA_MAX_ORDER1 128
#define WA_MAX_TAPS 256
#define WA_TILE 256           // output samples per workgroup of the low-cut kernel
#define WA_MAX_BOUND 172      // smoothing boundary at F0 = fs / 4
#define WA_DEFAULT_F0 500.0
#define WA_EPS 2.220446049250313e-16
#define WA_NOISE 1e-12
#define WA_Q1 (-0.15)

// ---------------------------------------------------------------------------------------------------------- frame shape
struct WaShape {
  double cur;  // the F0 the frame is analysed at
  int origin, half, dc, bound;
};

// Every integer a frame's shape hangs on, in plain IEEE float64 (no contraction): the restatement's frame_shapes forms
// the same expressions, so both get the same integers also for F0 one ulp either side of a rounding point.  The clamps
// never bind for finite F0 in [0, fs / 4]; they keep a frame with any other F0 inside its LDS arrays.
__device__ WaShape wa_shape(double f0, long long i, int fs, double shiftms) {
#pragma clang fp contract(off)
  const double fsd = (double)fs;
  const double floor_f0 = 3.0 * fsd / (W_N - 3.0);
  WaShape s;
  s.cur = (f0 <= floor_f0 || !(f0 == f0)) ? WA_DEFAULT_F0 : f0;
  const double t = (double)i * shiftms / 1000.0;
  const double o = t * fsd + 0.001;
  s.origin = (int)fmin(o + 0.5, 2147483000.0);
  const double h = 1.5 * fsd / s.cur;
  s.half = (int)fmin(h + 0.5, 1e6);
  s.dc = 2 + (int)fmin(s.cur * W_N / fsd, 1e6);
  const double width = s.cur * 2.0 / 3.0;
  s.bound = (int)fmin(width * W_N / fsd, 1e6) + 1;
  s.half = max(1, min(s.half, W_N / 2 - 1));
  s.dc = max(2, min(s.dc, W_N / 2));
  s.bound = max(1, min(s.bound, WA_MAX_BOUND));
  return s;
}

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
  const int kmax = (int)min((long long)n_taps - 1, i);
  double acc = 0.0;
  for (int k = 0; k <= kmax; ++k) acc = fma(h[k], (double)x[g - k], acc);
  y[g] = acc;
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
#pragma clang fp contract(off)  // x w + noise and wav - w coef round as the restatement's do: on a locally constant signal
                                // the mean removal cancels the signal and what is left is of the size of those roundings
  __shared__ double2 Z[W_N];
  __shared__ double tc[W_N / 2], ts[W_N / 2];
  __shared__ double buf[W_N];      // the window, then the mirrored cumulative spectrum (at most 513 + 2 * 172 values)
  __shared__ double pw[W_K + 7];   // power spectrum, then log spectrum, then liftered cepstrum
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  const int u = w_find(a.foff, a.n_utts, f);
  const long long S0 = a.soff[u], xlen = a.soff[u + 1] - S0;
  const double* xs = a.x + S0;
  const WaShape sh = wa_shape(a.f0[f], f - a.foff[u], a.fs, a.shiftms);
  const long long roff = a.doff[f];
  const double fsd = (double)a.fs, cur = sh.cur;
  const int half = sh.half, n = 2 * half + 1;

  w_stage_twiddles(tc, ts, a.twc, a.tws);
  // the F0-adaptive window, unit energy
  double e = 0.0;
  for (int j = tid; j < n; j += W_THREADS) {
    const double pos = (double)(j - half) / 1.5 / fsd;
    const double w = 0.5 * cos(M_PI * pos * cur) + 0.5;
    buf[j] = w;
    e += w * w;
  }
  const double norm = sqrt(w_block_sum(e, red));
  // windowed waveform (indices clamped to the signal) plus the stream's noise; the window-weighted mean removed
  double wav[4], win[4], s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    wav[r] = 0.0;
    win[r] = 0.0;
    if (j < n) {
      const double w = buf[j] / norm;
      const long long idx = max(0LL, min((long long)sh.origin + (j - half), xlen - 1));
      const double xv = xlen > 0 ? xs[idx] : 0.0;
      const double z = a.noise[min(roff + j, a.noise_len - 1)];
      win[r] = w;
      wav[r] = xv * w + z * WA_NOISE;
      s1 += wav[r];
      s2 += w;
    }
  }
  s1 = w_block_sum(s1, red);
  s2 = w_block_sum(s2, red);
  const double coef = s1 / s2;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    Z[w_brev(j)] = make_double2(j < n ? wav[r] - win[r] * coef : 0.0, 0.0);
  }
  __syncthreads();
  w_fft(Z, tc, ts, -1.0);
  for (int k = tid; k < W_K; k += W_THREADS) pw[k] = Z[k].x * Z[k].x + Z[k].y * Z[k].y;
  __syncthreads();
  // DC correction: the replica mirrored at F0 is added below it (all reads before the first write)
  double rep[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = tid + W_THREADS * r;
    rep[r] = i < sh.dc - 1 ? wa_interp(pw, sh.dc + 1, cur, -(fsd / W_N), (double)i * fsd / W_N) : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = tid + W_THREADS * r;
    if (i < sh.dc - 1) pw[i] += rep[r];
  }
  __syncthreads();
  // linear smoothing of width 2 F0 / 3: mirrored spectrum, its cumulative sum, two reads per bin.  The sum runs in one
  // thread in the restatement's order: a band's level is the difference of two of its values, so a bin far below the
  // frame's total power keeps only the digits both sums round alike (a scan that rounds otherwise was 1e-9 .. 2e-6 off
  // in log sp on harmonic signals, where the two-FFT spread of the restatement is 1e-14 .. 1e-10).
  const int b = sh.bound, len = W_K + 2 * b;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    if (j < len) {
      const int src = j < b ? b - j : (j < W_K - 1 + b ? j - b : (W_K - 1) - (j - (W_K - 1 + b)));
      buf[j] = pw[src] * fsd / W_N;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
#pragma unroll 8
    for (int j = 0; j < len; ++j) {
      run += buf[j];
      buf[j] = run;
    }
  }
  __syncthreads();
  const double width = cur * 2.0 / 3.0;
  const double x0 = -(b - 0.5) * fsd / W_N, dx = fsd / W_N;
  for (int k = tid; k < W_K; k += W_THREADS) {
    const double ax = (double)k / W_N * fsd - width / 2.0;
    const double lo = wa_interp(buf, len, x0, dx, ax), hi = wa_interp(buf, len, x0, dx, ax + width);
    const double z = a.noise[min(roff + n + k, a.noise_len - 1)];
    pw[k] = log((hi - lo) / width + fabs(z) * WA_EPS);
  }
  __syncthreads();
  // cepstrum of the even log spectrum; smoothing and recovery lifters
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    Z[w_brev(j)] = make_double2(pw[j <= W_N / 2 ? j : W_N - j], 0.0);
  }
  __syncthreads();
  w_fft(Z, tc, ts, -1.0);
  double cl[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int k = tid + W_THREADS * r;
    cl[r] = 0.0;
    if (k < W_K) {
      double sm = 1.0, cp = 1.0;
      if (k > 0) {
        const double q = (double)k / fsd;
        sm = sin(M_PI * cur * q) / (M_PI * cur * q);
        cp = (1.0 - 2.0 * WA_Q1) + 2.0 * WA_Q1 * cos(2.0 * M_PI * q * cur);
      }
      cl[r] = Z[k].x * sm * cp / W_N;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int k = tid + W_THREADS * r;
    if (k < W_K) {
      pw[k] = cl[r];
      if (a.cep) a.cep[f * W_K + k] = cl[r];
    }
  }
  if (!a.sp) return;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    Z[w_brev(j)] = make_double2(pw[j <= W_N / 2 ? j : W_N - j], 0.0);
  }
  __syncthreads();
  w_fft(Z, tc, ts, -1.0);
  for (int k = tid; k < W_K; k += W_THREADS) a.sp[f * W_K + k] = exp(Z[k].x);
}

// mcep[f][m] = sum_k at[m][k] cep[f][k]: one wave per frame, lane l holds cep[l + 64 j]
__global__ __launch_bounds__(W_THREADS) void wana_mcep_kernel(const double* __restrict__ cep, long long F,
                                                              const double* __restrict__ at, int m1,
                                                              double* __restrict__ mc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long f = (long long)blockIdx.x * (W_THREADS / 64) + wv;
  if (f >= F) return;
  double c[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int k = lane + 64 * j;
    c[j] = k < W_K ? cep[f * W_K + k] : 0.0;
  }
  for (int m = 0; m < m1; ++m) {
    const double* row = at + (size_t)m * W_K;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = lane + 64 * j;
      if (k < W_K) acc = fma(row[k], c[j], acc);
    }
    acc = w_wave_sum(acc);
    if (lane == 0) mc[f * m1 + m] = acc;
  }
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
