// What the WORLD synthesis kernels (world_kernels.hip) and the WORLD analysis kernels (world_analysis_kernels.hip) share:
// the 1024-point fp64 FFT in LDS, the deterministic workgroup sum and the offset search.
#pragma once
#include <stddef.h>

#define W_N 1024
#define W_K (W_N / 2 + 1)
#define W_LOGN 10
#define W_THREADS 256

static size_t w_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------- helpers
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

__device__ __forceinline__ int w_find(const long long* off, int n, long long v) {  // largest u with off[u] <= v
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int w_brev(int n) { return (int)(__brev((unsigned)n) >> (32 - W_LOGN)); }

// in-place radix-2 DIT FFT of W_N points in LDS, input in bit-reversed order; sign -1 forward, +1 inverse (unnormalised)
__device__ void w_fft(double2* x, const double* twc, const double* tws, double sign) {
  for (int half = 1; half < W_N; half <<= 1) {
    const int stride = W_N / (2 * half);
    for (int b = threadIdx.x; b < W_N / 2; b += W_THREADS) {
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
