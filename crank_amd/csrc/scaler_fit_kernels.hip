// Fitting the recipe's StandardScalers over a corpus packed in HBM (gfx950): stage 2 of the recipe,
// crank/bin/extract_statistics.py, which calls sklearn's StandardScaler.partial_fit once per utterance in file order.
//
// sklearn's partial_fit (sklearn/utils/extmath.py, _incremental_mean_and_var) is two things: the moments of the new
// block alone - sum, then the corrected two-pass sum of squares around T = sum / n - and a Chan / Golub / LeVeque merge
// of those with the running statistics.  Both are float64.  The merge is a handful of scalar operations per utterance
// whose bits depend on their order, so it is restated operation for operation (crk_scaler_merge; contraction is off for
// this file).  The moments are sums over the utterance's frames, where only the summation order is free: a fixed
// order that depends on the utterance's length and the window's width alone (crk_scaler_moments).
#include "common.h"
#include "../../include/crank_hip.h"

#include <cmath>

#pragma clang fp contract(off)

#define SF_THREADS 256
#define SF_TILE 64  // columns of one workgroup: 16 threads of 4 columns
#define SF_ALIGN 256

struct ScalerWs {
  long long status, n, sum, m2, total;  // byte offsets
};

static bool scaler_ws(int U, int D, ScalerWs* w) {
  if (U < 1 || D < 1) return false;
  const long long tiles = (D + SF_TILE - 1) / SF_TILE;
  auto up = [](long long b) { return (b + SF_ALIGN - 1) / SF_ALIGN * SF_ALIGN; };
  w->status = 0;
  w->n = up((long long)U * tiles * 4);
  w->sum = w->n + up((long long)U * 8);
  w->m2 = w->sum + up((long long)U * D * 8);
  w->total = w->m2 + up((long long)U * D * 8);
  return true;
}

extern "C" long long crk_scaler_workspace_bytes(int U, int D) {
  ScalerWs w;
  return scaler_ws(U, D, &w) ? w.total : -1;
}

// Sum over the row lanes of a workgroup, lane 0 first: cell (rl, cg) of `red` holds lane rl's four columns of column
// group cg.  A fixed tree, so the result depends on the lane count alone.
__device__ __forceinline__ void lane_tree(double (*red)[4], int rl, int cg, int CG, int RL) {
  for (int s = RL >> 1; s >= 1; s >>= 1) {
    __syncthreads();
    if (rl < s) {
      double* a = red[rl * CG + cg];
      const double* b = red[(rl + s) * CG + cg];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = a[j] + b[j];
    }
  }
  __syncthreads();
}

// One workgroup: utterance blockIdx.x, columns [64 * blockIdx.y, +64) of the window.  Thread (rl, cg) owns columns
// 4 cg .. 4 cg + 3 of the tile and frames rl, rl + RL, ... of the utterance, which it adds up one after the other; the
// lanes are then added by the tree above.  VEC only changes how the four floats are fetched, never the order.
template <bool VEC>
__global__ __launch_bounds__(SF_THREADS) void scaler_moments_kernel(const float* __restrict__ x, int ld, int col0, int D,
                                                                   long long F_total,
                                                                   const long long* __restrict__ utt_start,
                                                                   int* __restrict__ status, long long* __restrict__ n_out,
                                                                   double* __restrict__ sum_out,
                                                                   double* __restrict__ m2_out) {
  __shared__ double red[SF_THREADS][4];
  __shared__ double red2[SF_THREADS][4];
  const int u = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
  const int c_tile = tile * SF_TILE;
  const int W = min(SF_TILE, D - c_tile);
  const int quads = (W + 3) >> 2;
  int CG = 1;
  while (CG < quads) CG <<= 1;
  const int RL = SF_THREADS / CG;
  const int cg = tid % CG, rl = tid / CG;
  const int c = c_tile + 4 * cg;                 // first of this thread's columns, in the window
  const int nc = max(0, min(4, D - c));          // how many of them exist
  const long long s0 = utt_start[u], s1 = utt_start[u + 1];
  const int cell = u * gridDim.y + tile;
  if (s0 < 0 || s1 <= s0 || s1 > F_total) {      // the host checked its copy of the offsets; this guards the device's
    if (tid == 0) status[cell] = 2;
    return;
  }
  const long long len = s1 - s0;
  const float* base = x + s0 * (long long)ld + col0 + c;

  auto fetch = [&](long long r, double* v) {
    const float* p = base + r * (long long)ld;
    if (VEC) {
      const f32x4 q = *(const f32x4*)p;
      v[0] = (double)q.x, v[1] = (double)q.y, v[2] = (double)q.z, v[3] = (double)q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < nc ? (double)p[j] : 0.0;
    }
  };

  // ---- pass 1: sum
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (nc > 0) {
    long long r = rl;
    for (; r + 3LL * RL < len; r += 4LL * RL) {  // four loads in flight, added in frame order
      double v0[4], v1[4], v2[4], v3[4];
      fetch(r, v0), fetch(r + RL, v1), fetch(r + 2LL * RL, v2), fetch(r + 3LL * RL, v3);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = (((acc[j] + v0[j]) + v1[j]) + v2[j]) + v3[j];
    }
    for (; r < len; r += RL) {
      double v[4];
      fetch(r, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = acc[j] + v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[tid][j] = acc[j];
  lane_tree(red, rl, cg, CG, RL);
  double sum[4], T[4];
  const double n = (double)len;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sum[j] = red[cg][j];
    T[j] = sum[j] / n;
  }
  __syncthreads();

  // ---- pass 2: corr = sum (x - T), sq = sum (x - T)^2; the utterance comes from cache this time
  double corr[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
  if (nc > 0) {
    long long r = rl;
    for (; r + 3LL * RL < len; r += 4LL * RL) {
      double v[4][4];
      fetch(r, v[0]), fetch(r + RL, v[1]), fetch(r + 2LL * RL, v[2]), fetch(r + 3LL * RL, v[3]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = v[k][j] - T[j];
          corr[j] = corr[j] + d;
          sq[j] = sq[j] + d * d;
        }
    }
    for (; r < len; r += RL) {
      double v[4];
      fetch(r, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = v[j] - T[j];
        corr[j] = corr[j] + d;
        sq[j] = sq[j] + d * d;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[tid][j] = corr[j], red2[tid][j] = sq[j];
  lane_tree(red, rl, cg, CG, RL);
  lane_tree(red2, rl, cg, CG, RL);

  if (rl == 0) {
    bool finite = true;
    for (int j = 0; j < nc; ++j) {
      const double cr = red[cg][j];
      sum_out[(long long)u * D + c + j] = sum[j];
      m2_out[(long long)u * D + c + j] = red2[cg][j] - cr * cr / n;
      // a float64 sum of float32 values cannot overflow: it is finite exactly when every value is
      finite = finite && isfinite(sum[j]);
    }
    red[cg][0] = finite ? 0.0 : 1.0;
  }
  __syncthreads();
  if (tid == 0) {
    bool bad = false;
    for (int g = 0; g < quads; ++g) bad = bad || red[g][0] != 0.0;
    status[cell] = bad ? 1 : 0;
    if (tile == 0) n_out[u] = len;
  }
}

extern "C" int crk_scaler_moments(const float* x, int ld, int col0, int D, long long F_total, const long long* utt_start,
                                  const long long* utt_start_host, int U, void* workspace, long long workspace_bytes,
                                  void* stream) {
  ScalerWs w;
  if (!x || !utt_start || !utt_start_host || !workspace || !scaler_ws(U, D, &w)) return CRK_ERR_ARG;
  if (col0 < 0 || ld < col0 + D || F_total < 1 || workspace_bytes < w.total) return CRK_ERR_ARG;
  if (((uintptr_t)workspace & 7) != 0 || utt_start_host[0] < 0 || utt_start_host[U] > F_total) return CRK_ERR_ARG;
  for (int u = 0; u < U; ++u)
    if (utt_start_host[u + 1] <= utt_start_host[u]) return CRK_ERR_ARG;  // an empty utterance
  const int tiles = (D + SF_TILE - 1) / SF_TILE;
  if (tiles > 65535 || (long long)U * tiles > 0x7fffffffLL) return CRK_ERR_ARG;
  char* ws = (char*)workspace;
  int* status = (int*)(ws + w.status);
  long long* n = (long long*)(ws + w.n);
  double *sum = (double*)(ws + w.sum), *m2 = (double*)(ws + w.m2);
  const bool vec = ((ld | col0 | D) & 3) == 0 && ((uintptr_t)x & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(scaler_moments_kernel<true>, dim3(U, tiles), dim3(SF_THREADS), 0, (hipStream_t)stream, x, ld, col0, D,
                       F_total, utt_start, status, n, sum, m2);
  else
    hipLaunchKernelGGL(scaler_moments_kernel<false>, dim3(U, tiles), dim3(SF_THREADS), 0, (hipStream_t)stream, x, ld, col0,
                       D, F_total, utt_start, status, n, sum, m2);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

// sklearn's update, one thread per (group, column), the group's utterances in the order given.  Every line is the
// numpy expression of _incremental_mean_and_var with the same operands in the same order; the integer counts enter the
// arithmetic as float64, as numpy promotes them.
__global__ __launch_bounds__(64) void scaler_merge_kernel(const long long* __restrict__ n_in, const double* __restrict__ sum_in,
                                                         const double* __restrict__ m2_in, int U, int D,
                                                         const long long* __restrict__ group_start,
                                                         const int* __restrict__ group_utts, int G,
                                                         double* __restrict__ mean_out, double* __restrict__ var_out,
                                                         long long* __restrict__ count_out) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= (long long)G * D) return;
  const int g = (int)(i / D), d = (int)(i - (long long)g * D);
  double mean = 0.0, var = 0.0;
  long long count = 0;
  for (long long k = group_start[g]; k < group_start[g + 1]; ++k) {
    const int u = group_utts[k];
    if (u < 0 || u >= U) continue;  // the host checked its copy
    const long long new_count = n_in[u];
    const double new_sum = sum_in[(long long)u * D + d];
    const double new_m2 = m2_in[(long long)u * D + d];
    const double last_sum = mean * (double)count;
    const long long updated_count = count + new_count;
    const double updated_mean = (last_sum + new_sum) / (double)updated_count;
    const double last_m2 = var * (double)count;
    double updated_m2;
    if (count == 0) {
      updated_m2 = new_m2;
    } else {
      const double r = (double)count / (double)new_count;
      const double t = last_sum / r - new_sum;
      updated_m2 = (last_m2 + new_m2) + (r / (double)updated_count) * (t * t);
    }
    mean = updated_mean;
    var = updated_m2 / (double)updated_count;
    count = updated_count;
  }
  mean_out[i] = mean;
  var_out[i] = var;
  if (d == 0) count_out[g] = count;
}

extern "C" int crk_scaler_merge(const void* workspace, long long workspace_bytes, int U, int D, const long long* group_start,
                                const int* group_utts, const long long* group_start_host, const int* group_utts_host, int G,
                                double* mean, double* var, long long* count, void* stream) {
  ScalerWs w;
  if (!workspace || !group_start || !group_utts || !group_start_host || !group_utts_host || !mean || !var || !count)
    return CRK_ERR_ARG;
  if (!scaler_ws(U, D, &w) || G < 1 || workspace_bytes < w.total || ((uintptr_t)workspace & 7) != 0) return CRK_ERR_ARG;
  if (group_start_host[0] != 0) return CRK_ERR_ARG;
  for (int g = 0; g < G; ++g)
    if (group_start_host[g + 1] <= group_start_host[g]) return CRK_ERR_ARG;  // an empty group
  for (long long k = 0; k < group_start_host[G]; ++k)
    if (group_utts_host[k] < 0 || group_utts_host[k] >= U) return CRK_ERR_ARG;
  const char* ws = (const char*)workspace;
  const long long total = (long long)G * D;
  if ((total + 63) / 64 > 0x7fffffffLL) return CRK_ERR_ARG;
  hipLaunchKernelGGL(scaler_merge_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                     (const long long*)(ws + w.n), (const double*)(ws + w.sum), (const double*)(ws + w.m2), U, D, group_start,
                     group_utts, G, mean, var, count);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
