// What the float64 signal families outside the training step share (WORLD synthesis world_kernels.hip, WORLD analysis
// world_analysis_kernels.hip, Griffin-Lim griffin_lim_kernels.hip, Harvest f0_kernels.hip).  Device side: the 1024-point
// FFT in LDS with its twiddle staging, the deterministic workgroup sum and the offset search.  Host side: WORLD's randn
// stream, SPTK freqt of a unit vector, a handle's block of host-made tables, a grow-only device table and the carving of a
// caller's workspace.
#pragma once
#include "runtime.h"
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

#define W_N 1024
#define W_K (W_N / 2 + 1)
#define W_LOGN 10
#define W_THREADS 256


static size_t w_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------- device
__device__ __forceinline__ double w_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// deterministic workgroup sum (W_THREADS threads): wave sums, then the four partials in order
__device__ double w_block_sum(double v, double* red) {
  v = w_wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// largest u < n with off[u * stride] <= v
__device__ __forceinline__ int w_find(const long long* off, int n, long long v, int stride = 1) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[(size_t)mid * stride] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int LOGN> __device__ __forceinline__ int w_brev_n(int n) { return (int)(__brev((unsigned)n) >> (32 - LOGN)); }
__device__ __forceinline__ int w_brev(int n) { return w_brev_n<W_LOGN>(n); }

// a handle's twiddle table (WTables::add_twiddles(W_N, W_N / 2)) into the workgroup's LDS; no barrier
__device__ __forceinline__ void w_stage_twiddles(double* tc, double* ts, const double* twc, const double* tws) {
  for (int m = threadIdx.x; m < W_N / 2; m += W_THREADS) { tc[m] = twc[m]; ts[m] = tws[m]; }
}

// in-place radix-2 DIT FFT of N points in LDS, input in bit-reversed order; sign -1 forward, +1 inverse (unnormalised);
// twc / tws: cos, sin of 2 pi m / N for m < N / 2, in LDS or in global memory
template <int N> __device__ void w_fft_n(double2* x, const double* twc, const double* tws, double sign) {
  for (int half = 1; half < N; half <<= 1) {
    const int stride = N / (2 * half);
    for (int b = threadIdx.x; b < N / 2; b += W_THREADS) {
      const int pos = b & (half - 1);
      const int i = ((b - pos) << 1) + pos, j = i + half;
      const double c = twc[pos * stride], s = sign * tws[pos * stride];
      const double2 xj = x[j], xi = x[i];
      const double tr = c * xj.x - s * xj.y, ti = c * xj.y + s * xj.x;
      x[j] = make_double2(xi.x - tr, xi.y - ti);
      x[i] = make_double2(xi.x + tr, xi.y + ti);
    }
    __syncthreads();
  }
}

// the W_N-point transform, twiddles staged by w_stage_twiddles
__device__ void w_fft(double2* x, const double* twc, const double* tws, double sign) { w_fft_n<W_N>(x, twc, tws, sign); }

// ---------------------------------------------------------------------------------------------------------- host
// WORLD randn after randn_reseed: the first n values of the stream
static inline void w_randn_table(long long n, std::vector<double>& v) {
  v.resize(n);
  uint32_t x = 123456789u, y = 362436069u, z = 521288629u, w = 88675123u;
  for (long long i = 0; i < n; ++i) {
    uint32_t acc = 0;
    for (int r = 0; r < 12; ++r) {
      const uint32_t t = x ^ (x << 11);
      x = y; y = z; z = w;
      w = (w ^ (w >> 19)) ^ (t ^ (t >> 8));
      acc += w >> 4;
    }
    v[i] = acc / 268435456.0 - 6.0;
  }
}

// g[0 .. n) = SPTK freqt(e_col, n - 1, a) fed the input's samples top .. 0 (the state is still zero above col, so a caller
// may start at top = col); d is scratch
static inline void w_freqt_unit(int col, int top, int n, double a, std::vector<double>& g, std::vector<double>& d) {
  const double b = 1.0 - a * a;
  g.assign(n, 0.0);
  for (int i = top; i >= 0; --i) {
    d = g;
    g[0] = (i == col ? 1.0 : 0.0) + a * d[0];
    if (n > 1) g[1] = b * d[0] + a * d[1];
    for (int m = 2; m < n; ++m) g[m] = d[m - 1] + a * (d[m] - g[m - 1]);
  }
}

// The host tables of a handle, laid end to end and uploaded as one device block; add* return the element offset.
struct WTables {
  std::vector<double> host;
  size_t add(const std::vector<double>& v) {
    host.insert(host.end(), v.begin(), v.end());
    return host.size() - v.size();
  }
  size_t add_twiddles(int n, int count) {  // cos, then sin, of 2 pi m / n for m < count
    for (int m = 0; m < count; ++m) host.push_back(cos(2.0 * M_PI * m / n));
    for (int m = 0; m < count; ++m) host.push_back(sin(2.0 * M_PI * m / n));
    return host.size() - 2 * (size_t)count;
  }
  bool upload(double** dev) const {  // one counted allocation; nothing is left allocated on failure
    if (hipMalloc(dev, host.size() * sizeof(double)) != hipSuccess) return false;
    crk_count_alloc_();
    if (hipMemcpy(*dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess) return true;
    (void)hipFree(*dev);
    return false;
  }
};

// Grow-only device table: a new block of n doubles (filled from `host` when given) replaces *dev only once it is complete.
// One counted allocation per call; synchronises when it copies.
static inline int w_grow_table(double** dev, long long* len, long long n, const double* host) {
  double* d = nullptr;
  if (hipMalloc(&d, (size_t)n * sizeof(double)) != hipSuccess) return CRK_ERR_HIP;
  crk_count_alloc_();
  if (host && hipMemcpy(d, host, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return CRK_ERR_HIP;
  }
  if (*dev) (void)hipFree(*dev);
  *dev = d;
  *len = n;
  return CRK_OK;
}

// Cuts a caller's workspace into arrays at 256-byte steps; with base null it only measures.
struct WCarve {
  unsigned char* base;
  size_t bytes = 0;
  template <typename T> T* take(size_t count) {
    T* p = base ? (T*)(base + bytes) : nullptr;
    bytes += w_align(count * sizeof(T));
    return p;
  }
};
