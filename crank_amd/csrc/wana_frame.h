// The per-frame and per-sample arithmetic of the spectral half of WORLD analysis, one body each, shared by the offline
// kernels (world_analysis_kernels.hip: a ragged batch of whole utterances) and the streaming ones
// (wana_stream_kernels.hip: frames of live streams whose samples sit in a ring).  A body takes what a frame hangs on - a
// sample accessor, the frame's F0, its index in the utterance and its offset into the randn stream - so both callers get
// the same bits: the low cut's fma chain, the frame's shape integers, CheapTrick and the freqt fold of the cepstrum.
#pragma once
#include "signal_common.h"
#include "wana.h"

#define WA_MAX_ORDER1 128
#define WA_MAX_TAPS 256
#define WA_MAX_BOUND 172      // smoothing boundary at F0 = fs / 4
#define WA_DEFAULT_F0 500.0
#define WA_EPS 2.220446049250313e-16
#define WA_NOISE 1e-12
#define WA_Q1 (-0.15)
#define WA_MAX_HALF (W_N / 2 - 1)                     // the longest half window
#define WA_MAX_DRAWS (2 * WA_MAX_HALF + 1 + W_K)      // the most randn values one frame draws

// ---------------------------------------------------------------------------------------------------------- low cut
// Output sample p of the causal FIR h (n_taps taps) with zero history before sample 0: the fma chain in tap order.
// sample(q) is the raw signal at q, 0 <= q <= p.
template <class Sample>
__device__ __forceinline__ double wa_lowcut_sample(const double* h, int n_taps, long long p, Sample sample) {
  const int kmax = (int)min((long long)n_taps - 1, p);
  double acc = 0.0;
  for (int k = 0; k <= kmax; ++k) acc = fma(h[k], (double)sample(p - k), acc);
  return acc;
}

// ---------------------------------------------------------------------------------------------------------- frame shape
struct WaShape {
  double cur;  // the F0 the frame is analysed at
  int origin, half, dc, bound;
};

// Every integer a frame's shape hangs on, in plain IEEE float64 (no contraction): the restatement's frame_shapes forms
// the same expressions, so both get the same integers also for F0 one ulp either side of a rounding point.  The clamps
// never bind for finite F0 in [0, fs / 4]; they keep a frame with any other F0 inside its LDS arrays.
__device__ inline WaShape wa_shape(double f0, long long i, int fs, double shiftms) {
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
  s.half = max(1, min(s.half, WA_MAX_HALF));
  s.dc = max(2, min(s.dc, W_N / 2));
  s.bound = max(1, min(s.bound, WA_MAX_BOUND));
  return s;
}

// ---------------------------------------------------------------------------------------------------------- CheapTrick
// What a frame reads besides its samples
struct WaTables {
  const double* noise; long long noise_len;
  const double* twc; const double* tws;
  int fs;
};

// One workgroup (W_THREADS threads), one frame.  Window with its three reductions, FFT, power, DC correction, the
// mirrored cumulative spectrum (summed by one thread in the restatement's order), the two band-edge reads per bin, log,
// FFT of the even log spectrum, lifter, FFT, exp: three 1024-point fp64 LDS FFTs.  xs(idx) is the analysed signal at
// sample idx of xlen (the body clamps idx to 0 .. xlen - 1); roff the frame's offset into the randn table.  Writes the
// 513-value rows sp and / or cep (the liftered cepstrum) where given.
template <class Signal>
__device__ __forceinline__ void wa_cheaptrick_frame(Signal xs, long long xlen, const WaShape sh, long long roff,
                                                    const WaTables a, double* __restrict__ sp, double* __restrict__ cep) {
#pragma clang fp contract(off)  // x w + noise and wav - w coef round as the restatement's do: on a locally constant signal
                                // the mean removal cancels the signal and what is left is of the size of those roundings
  __shared__ double2 Z[W_N];
  __shared__ double tc[W_N / 2], ts[W_N / 2];
  __shared__ double buf[W_N];      // the window, then the mirrored cumulative spectrum (at most 513 + 2 * 172 values)
  __shared__ double pw[W_K + 7];   // power spectrum, then log spectrum, then liftered cepstrum
  __shared__ double red[4];
  const int tid = threadIdx.x;
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
      const double xv = xlen > 0 ? xs(idx) : 0.0;
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
      if (cep) cep[k] = cl[r];
    }
  }
  if (!sp) return;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    Z[w_brev(j)] = make_double2(pw[j <= W_N / 2 ? j : W_N - j], 0.0);
  }
  __syncthreads();
  w_fft(Z, tc, ts, -1.0);
  for (int k = tid; k < W_K; k += W_THREADS) sp[k] = exp(Z[k].x);
}

// ---------------------------------------------------------------------------------------------------------- mcep
// One wave, one frame: mcep[m] = sum_k at[m][k] cep[k], lane l holding cep[l + 64 j]; lane 0 hands coefficient m to
// put(m, value).
template <class Put>
__device__ __forceinline__ void wa_mcep_frame(const double* __restrict__ cep, const double* __restrict__ at, int m1,
                                              int lane, Put put) {
  double c[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int k = lane + 64 * j;
    c[j] = k < W_K ? cep[k] : 0.0;
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
    if (lane == 0) put(m, acc);
  }
}
