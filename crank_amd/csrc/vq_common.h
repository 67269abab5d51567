// The codebook search's arithmetic, one device body per piece (vq_kernels.hip: the four search kernels and the exact
// re-scoring of the split-f16 one; stream_kernels.hip: st_vq).  A search returns, per row x, the lowest index k that attains
// the smallest
//   dist_k = (w2_k - 2 x.w_k) + x2,   w2_k = sum_d w_kd^2,  x2 = sum_d x_d^2
// with w2 and x2 as d-ordered chains of SEPARATELY ROUNDED squares, x.w_k as a d-ordered chain of fused multiply-adds, and
// code 0 for a row no code of which has a distance that compares (NaN rows).  Every rounding is written out here, so the
// compiler's contraction - which depends on the code around an expression - cannot make two kernels disagree on a near tie.
#pragma once

// One term of a squared norm, acc + e * e with the product rounded on its own (NOT an fma).  Left to the compiler the same
// source line became v_pk_mul + v_add in one kernel and v_fmac in another (and a mix of the two inside one loop), one ulp apart,
// which is enough to send a near tie to the other code.
__device__ __forceinline__ float vq_sq_acc(float acc, float e) {
#pragma clang fp contract(off)
  const float sq = e * e;
  return acc + sq;
}
// a row in memory whose address the caller knows to be a multiple of 16 bytes (the bodies below index rows by element)
__device__ __forceinline__ const float* vq_row16(const float* p) { return static_cast<const float*>(__builtin_assume_aligned(p, 16)); }
// squared norm of a row of D values (registers, or memory the caller declares 16-byte aligned), d ascending
template <int D>
__device__ __forceinline__ float vq_norm(const float* v) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < D; d++) s = vq_sq_acc(s, v[d]);
  return s;
}
// the dot product x.w: one fused multiply-add per d, d ascending from 0 (what v_mfma_f32_32x32x2_f32 forms per output element)
__device__ __forceinline__ float vq_dot_step(float x, float w, float dot) { return __builtin_fmaf(x, w, dot); }
template <int D>
__device__ __forceinline__ float vq_dot(const float* x, const float* w) {
  float dot = 0.f;
#pragma unroll
  for (int d = 0; d < D; d++) dot = vq_dot_step(x[d], w[d], dot);
  return dot;
}
// two roundings after the dot product, the association torch evaluates the reference's expression in (2 * dot is exact: the
// fma rounds like the subtraction, and differs from it only where 2 * dot alone would overflow)
__device__ __forceinline__ float vq_dist(float w2, float dot, float x2) { return __builtin_fmaf(-2.f, dot, w2) + x2; }
// (distance, then index): does candidate (d, i) go before (bd, bi)?  The rule wherever two partial results meet; a scan that
// visits its codes in ascending order keeps the first index with a strict `d < bd` alone.
__device__ __forceinline__ bool vq_better(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }
// A row whose distances never compared (all NaN) ends with the scan's start value or a padding code: torch.argmin would pick
// a NaN slot, the kernels pin code 0.
__device__ __forceinline__ int vq_pin(int bi, int K) { return bi >= K ? 0 : bi; }
// straight-through value x + (e - x), two roundings like the reference
__device__ __forceinline__ float vq_st(float x, float e) { return x + (e - x); }
__device__ __forceinline__ float4 vq_st4(float4 x, float4 e) {
  return make_float4(vq_st(x.x, e.x), vq_st(x.y, e.y), vq_st(x.z, e.z), vq_st(x.w, e.w));
}
// four channels of the commitment sum (x - e)^2: each square rounded on its own, added in channel order
__device__ __forceinline__ float vq_commit_acc(float csum, float4 x, float4 e) {
  return vq_sq_acc(vq_sq_acc(vq_sq_acc(vq_sq_acc(csum, x.x - e.x), x.y - e.y), x.z - e.z), x.w - e.w);
}
// the workgroup's {sum, count} -> cpart[2 * block]: xor butterfly inside a wave, the nw waves in order through red[2 * nw]
__device__ __forceinline__ void vq_commit_reduce(float csum, float ccnt, float* red, int nw, float* cpart) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { csum += __shfl_xor(csum, o, 64); ccnt += __shfl_xor(ccnt, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = csum; red[nw + (threadIdx.x >> 6)] = ccnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = red[0], c = red[nw];
#pragma unroll
    for (int w = 1; w < nw; w++) { a += red[w]; c += red[nw + w]; }
    cpart[2 * blockIdx.x] = a; cpart[2 * blockIdx.x + 1] = c;
  }
}
