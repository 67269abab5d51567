// Per-speaker histograms of contours packed in HBM (gfx950): the reduction of the recipe's "stage 1: initialization",
// crank/bin/generate_histogram.py:31-74,109-146, which draws plt.hist(np.hstack(f0s), bins=200, range=(40, 700)) and the
// same over (-70, 20) for the frame power of every speaker.  plt.hist is numpy.histogram; its counts are restated here.
//
// numpy.histogram(x, bins, range=(first, last)) with equal bins keeps first <= x <= last (a NaN or an infinity is never
// kept), forms i = int((x - first) * norm) with norm = bins / (last - first), moves i == bins down by one, and then
// corrects i by one step against the edges np.linspace(first, last, bins + 1): down when x < edges[i], up when
// x >= edges[i + 1] and i is not the last bin.  The result is the bin whose edges hold x, the last edge closed; the
// truncated index alone is not (it is off by one for values on or next to an edge).  All of it is float64, contraction is
// off for this file, and the edges are the caller's array, so the comparisons are numpy's own.
//
// Counts are integers: LDS 32-bit adds within a tile, 64-bit global adds across tiles.  Integer addition commutes, so the
// tables do not depend on the launch shape, the order of the utterances, the load width or on how a call is split.
#include "common.h"
#include "../../include/crank_hip.h"

#include <cmath>

#pragma clang fp contract(off)

#define HG_THREADS 256
#define HG_PER_THREAD 16
#define HG_TILE (HG_THREADS * HG_PER_THREAD)  // values of one workgroup pass: far below what a 32-bit counter holds
#define HG_MAX_BINS 4096

typedef __attribute__((ext_vector_type(2))) double f64x2;

// LDS of one workgroup: the edges (bins + 1 doubles), then the table (bins counters) and the three `seen` counters.
static inline size_t hist_lds_bytes(int bins) { return (size_t)(bins + 1) * 8 + (size_t)(bins + 3) * 4; }

// numpy's bin of a kept value (first <= x <= last); `edge` is the LDS copy of the edges
__device__ __forceinline__ int hist_bin(double x, const double* edge, double first, double norm, int bins) {
  int i = (int)((x - first) * norm);
  i = min(max(i, 0), bins - 1);  // numpy's "index == bins" step; the rest of the clamp only keeps a bad norm in the table
  if (i > 0 && x < edge[i])
    --i;
  else if (i != bins - 1 && x >= edge[i + 1])
    ++i;
  return i;
}

// Workgroup (u, t): utterance u, its values [t * HG_TILE, +HG_TILE), then every gridDim.y-th tile after that.  Each
// thread fetches its 16 values first (eight 16-byte loads when the tile starts on a 16-byte boundary, sixteen 8-byte
// loads otherwise), then bins them with LDS adds; the non-zero bins go to the group's row with 64-bit global adds.
__global__ __launch_bounds__(HG_THREADS) void hist_accumulate_kernel(const double* __restrict__ x, long long N,
                                                                     const long long* __restrict__ utt_start,
                                                                     const int* __restrict__ utt_group, int G,
                                                                     const double* __restrict__ edges, double first,
                                                                     double last, double norm, int bins,
                                                                     unsigned long long* __restrict__ counts,
                                                                     unsigned long long* __restrict__ seen) {
  extern __shared__ double hist_lds[];
  double* edge = hist_lds;
  unsigned* table = (unsigned*)(hist_lds + bins + 1);
  unsigned* tally = table + bins;  // kept, not finite
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long s0 = utt_start[u], s1 = utt_start[u + 1];
  const int g = utt_group[u];
  // the host checked its copies of the offsets and the groups; this guards the device's
  if (s0 < 0 || s1 <= s0 || s1 > N || g < 0 || g >= G) return;
  const long long len = s1 - s0;
  if ((long long)blockIdx.y * HG_TILE >= len) return;

  for (int b = tid; b <= bins; b += HG_THREADS) edge[b] = edges[b];
  for (long long t0 = (long long)blockIdx.y * HG_TILE; t0 < len; t0 += (long long)gridDim.y * HG_TILE) {
    for (int b = tid; b < bins + 2; b += HG_THREADS) table[b] = 0u;  // the table and the two tallies behind it
    __syncthreads();
    const double* p = x + s0 + t0;
    const int n = (int)min((long long)HG_TILE, len - t0);
    double v[HG_PER_THREAD];
    bool have[HG_PER_THREAD];
    if ((((uintptr_t)p) & 15) == 0) {
#pragma unroll
      for (int k = 0; k < HG_PER_THREAD / 2; ++k) {
        const int i = 2 * (k * HG_THREADS + tid);
        have[2 * k] = i < n, have[2 * k + 1] = i + 1 < n;
        if (have[2 * k + 1]) {
          const f64x2 q = *(const f64x2*)(p + i);
          v[2 * k] = q.x, v[2 * k + 1] = q.y;
        } else {
          v[2 * k] = have[2 * k] ? p[i] : 0.0, v[2 * k + 1] = 0.0;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < HG_PER_THREAD; ++k) {
        const int i = k * HG_THREADS + tid;
        have[k] = i < n;
        v[k] = have[k] ? p[i] : 0.0;
      }
    }
    unsigned kept = 0, odd = 0;
#pragma unroll
    for (int k = 0; k < HG_PER_THREAD; ++k) {
      if (!have[k]) continue;
      const double xv = v[k];
      if (xv >= first && xv <= last) {  // false for a NaN
        atomicAdd(&table[hist_bin(xv, edge, first, norm, bins)], 1u);
        ++kept;
      } else if (!isfinite(xv)) {
        ++odd;
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      kept += __shfl_xor(kept, s);
      odd += __shfl_xor(odd, s);
    }
    if ((tid & 63) == 0) {
      if (kept) atomicAdd(&tally[0], kept);
      if (odd) atomicAdd(&tally[1], odd);
    }
    __syncthreads();
    unsigned long long* row = counts + (long long)g * bins;
    for (int b = tid; b < bins; b += HG_THREADS) {
      const unsigned c = table[b];
      if (c) atomicAdd(&row[b], (unsigned long long)c);
    }
    if (tid == 0) {
      atomicAdd(&seen[3LL * g], (unsigned long long)n);
      if (tally[0]) atomicAdd(&seen[3LL * g + 1], (unsigned long long)tally[0]);
      if (tally[1]) atomicAdd(&seen[3LL * g + 2], (unsigned long long)tally[1]);
    }
    __syncthreads();  // the table is cleared again for the next tile
  }
}

extern "C" int crk_hist_accumulate(const double* x, long long N, const long long* utt_start,
                                   const long long* utt_start_host, const int* utt_group, const int* utt_group_host, int U,
                                   int G, const double* edges, double first, double last, double norm, int bins,
                                   long long* counts, long long* seen, void* stream) {
  if (!x || !utt_start || !utt_start_host || !utt_group || !utt_group_host || !edges || !counts || !seen) return CRK_ERR_ARG;
  if (U < 1 || G < 1 || N < 1 || bins < 1 || bins > HG_MAX_BINS) return CRK_ERR_ARG;
  if (!std::isfinite(first) || !std::isfinite(last) || !(first < last) || !(norm > 0.0)) return CRK_ERR_ARG;
  if (((uintptr_t)x & 7) != 0 || utt_start_host[0] < 0 || utt_start_host[U] > N) return CRK_ERR_ARG;
  long long longest = 0;
  for (int u = 0; u < U; ++u) {
    const long long len = utt_start_host[u + 1] - utt_start_host[u];
    if (len <= 0) return CRK_ERR_ARG;  // an empty utterance
    if (utt_group_host[u] < 0 || utt_group_host[u] >= G) return CRK_ERR_ARG;
    longest = len > longest ? len : longest;
  }
  const long long tiles = (longest + HG_TILE - 1) / HG_TILE;
  const unsigned gy = (unsigned)(tiles < 65535 ? tiles : 65535);
  if ((long long)U * gy * HG_THREADS > 0xffffffffLL) return CRK_ERR_ARG;
  hipLaunchKernelGGL(hist_accumulate_kernel, dim3((unsigned)U, gy), dim3(HG_THREADS), hist_lds_bytes(bins),
                     (hipStream_t)stream, x, N, utt_start, utt_group, G, edges, first, last, norm, bins,
                     (unsigned long long*)counts, (unsigned long long*)seen);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
