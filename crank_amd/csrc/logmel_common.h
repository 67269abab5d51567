// The register transform bodies the log-mel kernels share (mlfb_kernels.hip: the offline n_fft = 1024 kernel;
// logmel_stream_kernels.hip: the streaming one): complex arithmetic on (re, im) pairs and the in-register DFT-16.
#pragma once
#include "common.h"

struct lm_c { float re, im; };
__device__ __forceinline__ lm_c lm_add(lm_c a, lm_c b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ lm_c lm_sub(lm_c a, lm_c b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ lm_c lm_mul(lm_c a, lm_c b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ lm_c lm_mnegi(lm_c a) { return {a.im, -a.re}; }   // x (-i)
__device__ __forceinline__ lm_c lm_mposi(lm_c a) { return {-a.im, a.re}; }   // x (+i)
// forward DFT-4 (W_4 = -i) of (x0, x1, x2, x3) -> (y0, y1, y2, y3)
#define LM_DFT4(x0, x1, x2, x3, y0, y1, y2, y3)                                  \
  {                                                                              \
    const lm_c s02_ = lm_add(x0, x2), d02_ = lm_sub(x0, x2), s13_ = lm_add(x1, x3), d13_ = lm_sub(x1, x3); \
    y0 = lm_add(s02_, s13_); y1 = lm_add(d02_, lm_mnegi(d13_)); y2 = lm_sub(s02_, s13_); y3 = lm_add(d02_, lm_mposi(d13_)); \
  }
// in-register forward DFT-16, natural order in and out: n = 4 a + b, k = c + 4 d
__device__ __forceinline__ void lm_fft16(lm_c (&v)[16]) {
  lm_c y[16];
#pragma unroll
  for (int b = 0; b < 4; b++) LM_DFT4(v[b], v[4 + b], v[8 + b], v[12 + b], y[b], y[4 + b], y[8 + b], y[12 + b])  // y[4 c + b]
  // x W_16^(b c): (cos, -sin) of 2 pi b c / 16
  const lm_c w1 = {0.92387953251128674f, -0.38268343236508977f}, w2 = {0.70710678118654752f, -0.70710678118654752f};
  const lm_c w3 = {0.38268343236508977f, -0.92387953251128674f}, w6 = {-0.70710678118654752f, -0.70710678118654752f};
  const lm_c w9 = {-0.92387953251128674f, 0.38268343236508977f};
  y[4 + 1] = lm_mul(y[4 + 1], w1); y[4 + 2] = lm_mul(y[4 + 2], w2); y[4 + 3] = lm_mul(y[4 + 3], w3);
  y[8 + 1] = lm_mul(y[8 + 1], w2); y[8 + 2] = lm_mnegi(y[8 + 2]);    y[8 + 3] = lm_mul(y[8 + 3], w6);
  y[12 + 1] = lm_mul(y[12 + 1], w3); y[12 + 2] = lm_mul(y[12 + 2], w6); y[12 + 3] = lm_mul(y[12 + 3], w9);
#pragma unroll
  for (int c = 0; c < 4; c++) LM_DFT4(y[4 * c], y[4 * c + 1], y[4 * c + 2], y[4 * c + 3], v[c], v[c + 4], v[c + 8], v[c + 12])
}
