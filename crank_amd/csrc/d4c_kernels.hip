// WORLD's D4C aperiodicity and CodeAperiodicity on the device (gfx950), float64, for a ragged batch of waveforms and a
// GIVEN F0 contour per utterance: what sprocket's FeatureExtractor.analyze / .codeap() get from pyworld d4c(threshold
// 0.85, fft_size 1024) and code_aperiodicity.  The oracle is the CPU restatement tests/d4c_ref.py; parity with pyworld is
// unpinned.  Structure:
//  * d4c_offsets_kernel, first use: one workgroup per utterance: every frame's integers (d4_shape) and the exclusive prefix
//    sum of the Love-Train draw counts (2 * half + 1 per voiced frame), the utterance's total kept for the second use.
//  * d4c_lovetrain_kernel: one workgroup per voiced frame: Blackman window of 3 periods at max(f0, 40), one 2048-point
//    FFT, the power summed by one thread in the restatement's order, P[4000 Hz] / P[7900 Hz].
//  * d4c_offsets_kernel, second use: the pass flags (voiced and Love Train above the threshold) and the prefix sum of the
//    general pass's draw counts (3 windows of 2 * half4 + 1) after the utterance's Love-Train draws.  The draw offsets
//    of the general pass depend on the Love-Train result, so they are formed on the device.
//  * d4c_general_kernel: one workgroup per passing frame at max(f0, 47): two centroids (each the two real transforms of
//    x and (n + 1) x packed into one complex FFT, the second part scaled by 2^-11 so that neither drowns the other's
//    rounding), the smoothed power spectrum, the static group delay (three linear smoothings, each cumulative sum by one
//    thread in the restatement's order), then per band: Nuttall-windowed slice, FFT, power, bitonic sort of 2048 values
//    (1025 powers, +inf padding) in LDS, running sum, the band's level in dB.  Six to seven FFTs per frame.
//  * d4c_table_kernel: the 513-bin table and / or the coded bands from the coarse levels.  A coded band reads two bins;
//    without a table it evaluates just those (d4_bin is the one body of a bin's value), so both routes give the same bits.
// LDS: 32 KB for the transform / cumulative sum / sort plus three 1025-value arrays, 57 KB: two workgroups per CU.
// No atomics: a frame's result depends on the batch only through its utterance's draw offsets.
#include "../../include/crank_hip.h"
#include "signal_common.h"
#include "wana.h"

#pragma clang fp contract(off)  // every expression rounds as the restatement's does

#define D4_LOWEST_F0 40.0
#define D4_FLOOR_F0 47.0
#define D4_INTERVAL 3000.0
#define D4_SAFE 1e-12
#define D4_R (D4_N / W_THREADS)  // values per thread of a 2048-point array
#define D4_PAD 1032              // a D4_K array, padded
#define D4_SHAPE_INTS 8
#define D4_BLACKMAN 0
#define D4_HANNING 1

// ---------------------------------------------------------------------------------------------------------- frame shape
struct D4Shape {
  int origin, half_lt, half_gb, oc1, oc2, dc, bh, bf;
};

__device__ __forceinline__ int d4_round(double x) {  // matlab_round, kept inside int
  x = fmax(-2147483000.0, fmin(x, 2147483000.0));
  return x > 0.0 ? (int)(x + 0.5) : (int)(x - 0.5);
}

// The integers of a frame in plain IEEE float64, the expressions of the restatement's frame_shapes.  The clamps never bind
// for finite F0 in [0, fs / 4]; they keep any other frame inside its LDS arrays.  An unvoiced frame has only its origin.
__device__ D4Shape d4_shape(double f0, long long i, int fs, double shiftms) {
  const double fsd = (double)fs;
  const double t = (double)i * shiftms / 1000.0;
  D4Shape s = {};
  s.origin = d4_round(t * fsd + 0.001);
  if (f0 == 0.0) return s;
  const double lt = fmax(f0, D4_LOWEST_F0), gb = fmax(f0, D4_FLOOR_F0);
  s.half_lt = d4_round(3.0 * fsd / lt / 2.0);
  s.half_gb = d4_round(4.0 * fsd / gb / 2.0);
  s.oc1 = d4_round((t - 0.25 / gb) * fsd + 0.001);
  s.oc2 = d4_round((t + 0.25 / gb) * fsd + 0.001);
  s.dc = 2 + (int)fmin(gb * D4_N / fsd, 1e6);
  s.bh = (int)fmin(gb / 2.0 * D4_N / fsd, 1e6) + 1;
  s.bf = (int)fmin(gb * D4_N / fsd, 1e6) + 1;
  s.half_lt = max(1, min(s.half_lt, D4_N / 2 - 1));
  s.half_gb = max(1, min(s.half_gb, D4_N / 2 - 1));
  s.dc = max(2, min(s.dc, D4_N / 2));
  s.bh = max(1, min(s.bh, D4_N / 4 + 1));
  s.bf = max(1, min(s.bf, D4_N / 4 + 1));
  return s;
}

// First use (ap0 null): Love-Train draw offsets, totals[u] = the utterance's Love-Train draws, shapes when asked.
// Second use: pass flags and the general pass's draw offsets, starting at totals[u].
__global__ __launch_bounds__(W_THREADS) void d4c_offsets_kernel(const double* __restrict__ f0,
                                                                const long long* __restrict__ foff, int fs, double shiftms,
                                                                const double* __restrict__ ap0, double threshold,
                                                                long long* __restrict__ totals, long long* __restrict__ off,
                                                                int* __restrict__ pass, int* __restrict__ shapes) {
  __shared__ long long cnt[W_THREADS];
  __shared__ long long total;
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long F0 = foff[u], T = foff[u + 1] - F0;
  long long base = ap0 ? totals[u] : 0;
  for (long long c0 = 0; c0 < T; c0 += W_THREADS) {
    const long long i = c0 + tid;
    long long mine = 0;
    if (i < T) {
      const double f = f0[F0 + i];
      const D4Shape s = d4_shape(f, i, fs, shiftms);
      if (!ap0) {
        mine = f != 0.0 ? 2 * s.half_lt + 1 : 0;
        if (shapes) {
          int* o = shapes + (F0 + i) * D4_SHAPE_INTS;
          o[0] = s.origin; o[1] = s.half_lt; o[2] = s.half_gb; o[3] = s.oc1;
          o[4] = s.oc2; o[5] = s.dc; o[6] = s.bh; o[7] = s.bf;
        }
      } else {
        const int p = f != 0.0 && ap0[F0 + i] > threshold;
        pass[F0 + i] = p;
        mine = p ? 3 * (2 * s.half_gb + 1) : 0;
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
    if (i < T) off[F0 + i] = cnt[tid];
    base = total;
    __syncthreads();
  }
  if (!ap0 && tid == 0) totals[u] = base;
}

// ---------------------------------------------------------------------------------------------------------- windows
struct D4Args {
  const double* x; const double* f0;
  const long long* foff; const long long* soff; int n_utts;
  const double* noise; long long noise_len;
  const double* twc; const double* tws; const double* nuttall;
  const long long* lt_off; const long long* gb_off; const int* pass;
  double* ap0; double* coarse;
  int fs, half_nut, bands; double shiftms;
};

// GetWindowedWaveform: thread tid gets samples tid + 256 r of the 2 * half + 1 (zero beyond): x w + randn 1e-12 with the
// window-weighted mean removed; sample indices clamped to the signal
__device__ void d4_windowed(const double* xs, long long xlen, double fsd, double cur, int origin, int half, int kind,
                            double ratio, const double* noise, long long noff, long long noise_len, double* red,
                            double wav[D4_R]) {
  const int tid = threadIdx.x, n = 2 * half + 1;
  double win[D4_R], s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int r = 0; r < D4_R; ++r) {
    const int j = tid + W_THREADS * r;
    wav[r] = 0.0;
    win[r] = 0.0;
    if (j < n) {
      const double pos = (2.0 * (double)(j - half) / ratio) / fsd;
      const double a = M_PI * pos * cur;
      const double w = kind == D4_HANNING ? 0.5 * cos(a) + 0.5 : 0.42 + 0.5 * cos(a) + 0.08 * cos(a * 2.0);
      const long long idx = max(0LL, min((long long)origin + (j - half), xlen - 1));
      const double xv = xlen > 0 ? xs[idx] : 0.0;
      const double z = noise[max(0LL, min(noff + j, noise_len - 1))];
      win[r] = w;
      wav[r] = xv * w + z * D4_SAFE;
      s1 += wav[r];
      s2 += w;
    }
  }
  s1 = w_block_sum(s1, red);
  s2 = w_block_sum(s2, red);
  const double coef = s1 / s2;
#pragma unroll
  for (int r = 0; r < D4_R; ++r) wav[r] = wav[r] - win[r] * coef;
}

// ---------------------------------------------------------------------------------------------------------- Love Train
__global__ __launch_bounds__(W_THREADS) void d4c_lovetrain_kernel(D4Args a) {
  __shared__ double2 Z[D4_N];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  const double f0 = a.f0[f];
  if (f0 == 0.0) {
    if (tid == 0) a.ap0[f] = 0.0;
    return;
  }
  const int u = w_find(a.foff, a.n_utts, f);
  const long long S0 = a.soff[u], xlen = a.soff[u + 1] - S0;
  const D4Shape sh = d4_shape(f0, f - a.foff[u], a.fs, a.shiftms);
  const double fsd = (double)a.fs;
  double wav[D4_R];
  d4_windowed(a.x + S0, xlen, fsd, fmax(f0, D4_LOWEST_F0), sh.origin, sh.half_lt, D4_BLACKMAN, 3.0, a.noise, a.lt_off[f],
              a.noise_len, red, wav);
#pragma unroll
  for (int r = 0; r < D4_R; ++r) Z[w_brev_n<D4_LOGN>(tid + W_THREADS * r)] = make_double2(wav[r], 0.0);
  __syncthreads();
  w_fft_n<D4_N>(Z, a.twc, a.tws, -1.0);
  if (tid == 0) {
    // bins above fft / 2 (7900 Hz at fs < 15800) count as zero
    const int b0 = (int)ceil(100.0 * D4_N / fsd);
    const int b1 = min((int)ceil(4000.0 * D4_N / fsd), D4_N / 2), b2 = min((int)ceil(7900.0 * D4_N / fsd), D4_N / 2);
    double run = 0.0, at1 = 0.0;
#pragma unroll 8
    for (int k = b0 + 1; k <= b2; ++k) {
      run += Z[k].x * Z[k].x + Z[k].y * Z[k].y;
      if (k == b1) at1 = run;
    }
    a.ap0[f] = at1 / run;
  }
}

// ---------------------------------------------------------------------------------------------------------- general body
// DCCorrection in place: the replica mirrored at F0 is added below it (all reads before the first write)
__device__ void d4_dc_correction(double* p, int dc, double cur, double fsd) {
  const int tid = threadIdx.x;
  double rep[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = tid + W_THREADS * r;
    rep[r] = i < dc - 1 ? wa_interp(p, dc + 1, cur, -(fsd / D4_N), (double)i * fsd / D4_N) : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = tid + W_THREADS * r;
    if (i < dc - 1) p[i] += rep[r];
  }
  __syncthreads();
}

// LinearSmoothing of p (D4_K values) over `width` Hz into q (may be p): the mirrored spectrum, its cumulative sum by one
// thread in the restatement's order (a bin is the difference of two of its values), two reads per bin.  L: 2 b + D4_K values.
__device__ void d4_smooth(const double* p, double* q, double* L, double width, int b, double fsd) {
  const int tid = threadIdx.x, len = D4_K + 2 * b;
  for (int j = tid; j < len; j += W_THREADS) {
    const int src = j < b ? b - j : (j < D4_K - 1 + b ? j - b : (D4_K - 1) - (j - (D4_K - 1 + b)));
    L[j] = p[src] * fsd / D4_N;
  }
  __syncthreads();
  if (tid == 0) {  // blocks of 8 read together, summed in order, written together
    double run = 0.0, v[8];
    int j = 0;
    for (; j + 8 <= len; j += 8) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = L[j + q];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        run += v[q];
        v[q] = run;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) L[j + q] = v[q];
    }
    for (; j < len; ++j) {
      run += L[j];
      L[j] = run;
    }
  }
  __syncthreads();
  const double x0 = -(b - 0.5) * fsd / D4_N, dx = fsd / D4_N;
  for (int k = tid; k < D4_K; k += W_THREADS) {
    const double ax = (double)k / D4_N * fsd - width / 2.0;
    const double lo = wa_interp(L, len, x0, dx, ax), hi = wa_interp(L, len, x0, dx, ax + width);
    q[k] = (hi - lo) / width;
  }
  __syncthreads();
}

// ascending sort of the D4_N values of L
__device__ void d4_sort(double* L) {
  for (int k = 2; k <= D4_N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      // a thread's four pairs: every read before the first write, so that the reads are in flight together
      double x[D4_R / 2], y[D4_R / 2];
#pragma unroll
      for (int r = 0; r < D4_R / 2; ++r) {
        const int t = threadIdx.x + W_THREADS * r, i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        x[r] = L[i];
        y[r] = L[i | j];
      }
#pragma unroll
      for (int r = 0; r < D4_R / 2; ++r) {
        const int t = threadIdx.x + W_THREADS * r, i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const bool swap = (x[r] > y[r]) == ((i & k) == 0);
        L[i] = swap ? y[r] : x[r];
        L[i | j] = swap ? x[r] : y[r];
      }
      __syncthreads();
    }
}

__global__ __launch_bounds__(W_THREADS) void d4c_general_kernel(D4Args a) {
  __shared__ double2 Z[D4_N];  // a transform; as doubles: a cumulative spectrum (at most 2051 values), the sort's 2048
  __shared__ double A[D4_PAD], B[D4_PAD], C[D4_PAD];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  if (!a.pass[f]) return;
  double* L = (double*)Z;
  const int u = w_find(a.foff, a.n_utts, f);
  const long long S0 = a.soff[u], xlen = a.soff[u + 1] - S0;
  const double* xs = a.x + S0;
  const double f0 = a.f0[f], fsd = (double)a.fs, cur = fmax(f0, D4_FLOOR_F0);
  const D4Shape sh = d4_shape(f0, f - a.foff[u], a.fs, a.shiftms);
  const int half = sh.half_gb, n = 2 * half + 1;
  const long long noff = a.gb_off[f];
  double wav[D4_R];

  // static centroid: A = centroid(t - 1 / 4 f0) + centroid(t + 1 / 4 f0), DC-corrected
  for (int c = 0; c < 2; ++c) {
    d4_windowed(xs, xlen, fsd, cur, c ? sh.oc2 : sh.oc1, half, D4_BLACKMAN, 4.0, a.noise, noff + (long long)c * n,
                a.noise_len, red, wav);
    double e = 0.0;
#pragma unroll
    for (int r = 0; r < D4_R; ++r) e += wav[r] * wav[r];
    const double norm = sqrt(w_block_sum(e, red));
#pragma unroll
    for (int r = 0; r < D4_R; ++r) {
      const int j = tid + W_THREADS * r;
      const double v = wav[r] / norm;
      Z[w_brev_n<D4_LOGN>(j)] = make_double2(v, v * (j + 1.0) * (1.0 / D4_N));
    }
    __syncthreads();
    w_fft_n<D4_N>(Z, a.twc, a.tws, -1.0);
    for (int k = tid; k < D4_K; k += W_THREADS) {
      const double2 zk = Z[k], zm = Z[(D4_N - k) & (D4_N - 1)];
      const double xr = (zk.x + zm.x) * 0.5, xi = (zk.y - zm.y) * 0.5;
      const double yr = (zk.y + zm.y) * 0.5 * D4_N, yi = (zm.x - zk.x) * 0.5 * D4_N;
      const double cen = yr * xr + xi * yi;
      A[k] = c ? A[k] + cen : cen;
    }
    __syncthreads();
  }
  d4_dc_correction(A, sh.dc, cur, fsd);

  // smoothed power spectrum: B
  d4_windowed(xs, xlen, fsd, cur, sh.origin, half, D4_HANNING, 4.0, a.noise, noff + 2LL * n, a.noise_len, red, wav);
#pragma unroll
  for (int r = 0; r < D4_R; ++r) Z[w_brev_n<D4_LOGN>(tid + W_THREADS * r)] = make_double2(wav[r], 0.0);
  __syncthreads();
  w_fft_n<D4_N>(Z, a.twc, a.tws, -1.0);
  for (int k = tid; k < D4_K; k += W_THREADS) B[k] = Z[k].x * Z[k].x + Z[k].y * Z[k].y;
  __syncthreads();
  d4_dc_correction(B, sh.dc, cur, fsd);
  d4_smooth(B, B, L, cur, sh.bf, fsd);

  // static group delay: A = smooth(A / B, f0 / 2) minus the same smoothed by f0
  for (int k = tid; k < D4_K; k += W_THREADS) A[k] = A[k] / B[k];
  __syncthreads();
  d4_smooth(A, A, L, cur / 2.0, sh.bh, fsd);
  d4_smooth(A, C, L, cur, sh.bf, fsd);
  for (int k = tid; k < D4_K; k += W_THREADS) A[k] = A[k] - C[k];
  __syncthreads();

  // coarse aperiodicity per band
  const int hw = a.half_nut, wlen = 2 * hw + 1;
  const int boundary = d4_round(D4_N * 8.0 / wlen);
  for (int b = 0; b < a.bands; ++b) {
    const int center = (int)(D4_INTERVAL * (b + 1) * D4_N / fsd);
#pragma unroll
    for (int r = 0; r < D4_R; ++r) {
      const int j = tid + W_THREADS * r, src = center - hw + j;
      const double v = j < wlen && src >= 0 && src < D4_K ? A[src] * a.nuttall[j] : 0.0;
      Z[w_brev_n<D4_LOGN>(j)] = make_double2(v, 0.0);
    }
    __syncthreads();
    w_fft_n<D4_N>(Z, a.twc, a.tws, -1.0);
    double p[D4_R];
#pragma unroll
    for (int r = 0; r < D4_R; ++r) {
      const int k = tid + W_THREADS * r;
      p[r] = k < D4_K ? Z[k].x * Z[k].x + Z[k].y * Z[k].y : INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < D4_R; ++r) L[tid + W_THREADS * r] = p[r];
    __syncthreads();
    d4_sort(L);
    if (tid == 0) {
      const int k1 = max(0, D4_N / 2 - boundary - 1);
      double run = 0.0, v[8];  // the sum up to k1, then on to the total, in blocks of 8 read together
      int k = 0;
      for (; k + 8 <= k1 + 1; k += 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = L[k + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) run += v[q];
      }
      for (; k <= k1; ++k) run += L[k];
      const double at1 = run;
      for (; k + 8 <= D4_N / 2 + 1; k += 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = L[k + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) run += v[q];
      }
      for (; k <= D4_N / 2; ++k) run += L[k];
      const double lvl = 10.0 * log10(at1 / run);
      a.coarse[f * D4_MAX_BANDS + b] = fmin(0.0, lvl + (cur - 100.0) / 50.0);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------- table, coding
// bin k of the fftl / 2 + 1 = 513 table: interp1 of the knots (0, -60), (3000 b, coarse_b), (fs / 2, -1e-12), 10^(. / 20)
__device__ double d4_bin(const double* coarse, int pass, int bands, double fsd, int k) {
  if (!pass) return 1.0 - D4_SAFE;
  const double xi = (double)k * fsd / W_N;
  int j = 0;
  while (j < bands && D4_INTERVAL * (j + 1) <= xi) ++j;  // the last knot at or below xi, at most the one before last
  const double xj = D4_INTERVAL * j, xn = j == bands ? fsd / 2.0 : D4_INTERVAL * (j + 1);
  const double yj = j == 0 ? -60.0 : coarse[j - 1], yn = j == bands ? -D4_SAFE : coarse[j];
  const double s = (xi - xj) / (xn - xj);
  return pow(10.0, (yj + s * (yn - yj)) / 20.0);
}

// ap [F][513] and / or cap [F][bands]; table: a given ap to code (then coarse and pass are not read)
__global__ __launch_bounds__(W_THREADS) void d4c_table_kernel(const double* __restrict__ coarse, const int* __restrict__ pass,
                                                              const double* __restrict__ table, int bands, int fs,
                                                              double* __restrict__ ap, double* __restrict__ cap) {
  const long long f = blockIdx.x;
  const int tid = threadIdx.x;
  const double fsd = (double)fs;
  double co[D4_MAX_BANDS] = {0.0, 0.0, 0.0};
  int ps = 0;
  if (!table) {
    ps = pass[f];
    if (ps)
      for (int b = 0; b < bands; ++b) co[b] = coarse[f * D4_MAX_BANDS + b];
  }
  if (ap)
    for (int k = tid; k < W_K; k += W_THREADS) ap[f * W_K + k] = d4_bin(co, ps, bands, fsd, k);
  if (cap && tid < bands) {
    const double xk = D4_INTERVAL * (tid + 1.0);
    int j = max(0, min((int)(xk * W_N / fsd), W_K - 2));  // the last bin at or below the knot, at most the one before last
    while (j + 1 <= W_K - 2 && (double)(j + 1) * fsd / W_N <= xk) ++j;
    while (j > 0 && (double)j * fsd / W_N > xk) --j;
    const double xj = (double)j * fsd / W_N, xn = (double)(j + 1) * fsd / W_N;
    const double aj = table ? table[f * W_K + j] : d4_bin(co, ps, bands, fsd, j);
    const double an = table ? table[f * W_K + j + 1] : d4_bin(co, ps, bands, fsd, j + 1);
    const double yj = 20.0 * log10(aj), yn = 20.0 * log10(an);
    const double s = (xk - xj) / (xn - xj);
    cap[f * bands + tid] = yj + s * (yn - yj);
  }
}

// ---------------------------------------------------------------------------------------------------------- host side
struct D4Ws {
  long long *lt_off, *gb_off, *totals;
  int* pass;
  double *ap0, *coarse;
  size_t bytes;
};

static D4Ws d4_ws(int n_utts, long long F, unsigned char* base) {
  D4Ws r;
  WCarve c{base};
  r.lt_off = c.take<long long>((size_t)F);
  r.gb_off = c.take<long long>((size_t)F);
  r.totals = c.take<long long>((size_t)n_utts);
  r.pass = c.take<int>((size_t)F);
  r.ap0 = c.take<double>((size_t)F);
  r.coarse = c.take<double>((size_t)F * D4_MAX_BANDS);
  r.bytes = c.bytes;
  return r;
}

extern "C" long long crk_wana_d4c_workspace_bytes(int n_utts, long long total_frames) {
  if (n_utts < 1 || total_frames < 1 || total_frames > (1LL << 31) - 1) return -1;
  return (long long)d4_ws(n_utts, total_frames, nullptr).bytes;
}

extern "C" int crk_wana_d4c_draws_per_frame(void* h) {
  Wana* w = (Wana*)h;
  if (!w || !w->twc2) return -1;
  const double fsd = (double)w->fs;
  return (2 * (int)(1.5 * fsd / D4_LOWEST_F0 + 0.5) + 1) + 3 * (2 * (int)(2.0 * fsd / D4_FLOOR_F0 + 0.5) + 1);
}

// the launches up to the pass flags; lt_off / gb_off / pass default to the workspace's
static int d4_front(Wana* w, const double* x, const double* f0, const long long* foff, const long long* soff, int n_utts,
                    long long F, long long S, long long max_draws, double threshold, void* workspace,
                    long long workspace_bytes, hipStream_t st, int* shapes, long long* lt_off, long long* gb_off, int* pass,
                    D4Args* out, D4Ws* wsout) {
  if (!w || !x || !f0 || !foff || !soff || !workspace || n_utts < 1 || F < 1 || F > (1LL << 31) - 1 || S < 1 ||
      max_draws < 1 || !(threshold == threshold))
    return CRK_ERR_ARG;
  if (!w->twc2) return CRK_ERR_UNSUPPORTED;           // fs outside D4_FS_MIN .. D4_FS_MAX
  if (max_draws > w->noise_len) return CRK_ERR_ARG;  // crk_wana_reserve(max_draws) first
  D4Ws ws = d4_ws(n_utts, F, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  if (lt_off) ws.lt_off = lt_off;
  if (gb_off) ws.gb_off = gb_off;
  if (pass) ws.pass = pass;
  d4c_offsets_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, st>>>(f0, foff, w->fs, w->shiftms, nullptr, threshold, ws.totals,
                                                               ws.lt_off, nullptr, shapes);
  CRK_CHECK_LAUNCH();
  // a table that covers max_draws covers every index the kernels form when max_draws bounds the utterances' draws
  D4Args a{x, f0, foff, soff, n_utts, w->noise, min(w->noise_len, max_draws), w->twc2, w->tws2, w->nuttall, ws.lt_off,
           ws.gb_off, ws.pass, ws.ap0, ws.coarse, w->fs, w->d4_half, w->d4_bands, w->shiftms};
  d4c_lovetrain_kernel<<<dim3((unsigned)F), dim3(W_THREADS), 0, st>>>(a);
  CRK_CHECK_LAUNCH();
  d4c_offsets_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, st>>>(f0, foff, w->fs, w->shiftms, ws.ap0, threshold, ws.totals,
                                                               ws.gb_off, ws.pass, nullptr);
  CRK_CHECK_LAUNCH();
  *out = a;
  *wsout = ws;
  return CRK_OK;
}

extern "C" int crk_wana_d4c(void* h, const double* x, const double* f0, const long long* frame_offsets,
                            const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                            long long max_draws, double threshold, double* ap, double* cap, void* workspace,
                            long long workspace_bytes, void* stream) {
  Wana* w = (Wana*)h;
  if (!ap && !cap) return CRK_ERR_ARG;
  if (w && cap && w->twc2 && w->d4_bands < 1) return CRK_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  D4Args a;
  D4Ws ws;
  const int rc = d4_front(w, x, f0, frame_offsets, sample_offsets, n_utts, total_frames, total_samples, max_draws,
                          threshold, workspace, workspace_bytes, st, nullptr, nullptr, nullptr, nullptr, &a, &ws);
  if (rc) return rc;
  d4c_general_kernel<<<dim3((unsigned)total_frames), dim3(W_THREADS), 0, st>>>(a);
  CRK_CHECK_LAUNCH();
  d4c_table_kernel<<<dim3((unsigned)total_frames), dim3(W_THREADS), 0, st>>>(ws.coarse, ws.pass, nullptr, w->d4_bands, w->fs,
                                                                             ap, cap);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_wana_d4c_code(void* h, const double* ap, long long total_frames, double* cap, void* stream) {
  Wana* w = (Wana*)h;
  if (!w || !ap || !cap || total_frames < 1 || total_frames > (1LL << 31) - 1) return CRK_ERR_ARG;
  const int bands = (int)(fmin(15000.0, w->fs / 2.0 - 3000.0) / 3000.0);
  if (bands < 1 || bands > D4_MAX_BANDS) return CRK_ERR_UNSUPPORTED;
  d4c_table_kernel<<<dim3((unsigned)total_frames), dim3(W_THREADS), 0, (hipStream_t)stream>>>(nullptr, nullptr, ap, bands,
                                                                                              w->fs, nullptr, cap);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_wana_d4c_frame_shapes(void* h, const double* x, const double* f0, const long long* frame_offsets,
                                         const long long* sample_offsets, int n_utts, long long total_frames,
                                         long long total_samples, long long max_draws, double threshold, int* shapes,
                                         int* pass, long long* lt_offsets, long long* gb_offsets, void* workspace,
                                         long long workspace_bytes, void* stream) {
  if (!shapes || !pass || !lt_offsets || !gb_offsets) return CRK_ERR_ARG;
  D4Args a;
  D4Ws ws;
  return d4_front((Wana*)h, x, f0, frame_offsets, sample_offsets, n_utts, total_frames, total_samples, max_draws, threshold,
                  workspace, workspace_bytes, (hipStream_t)stream, shapes, lt_offsets, gb_offsets, pass, &a, &ws);
}
