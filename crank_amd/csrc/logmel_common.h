// What a log-mel cell is, once, for the four log-mel kernels (mlfb_kernels.hip: logmel_kernel and logmel_wave_kernel, the
// offline call; logmel_stream_kernels.hip: ls_frame_kernel and ls_frame1024_kernel, the streaming push):
//   sizes        LM_MAX_FFT, LM_MAX_MELS, LM_WTAB, LM_ZS, LM_MAG
//   host         lm_log2n, lm_log_eps
//   framing      lm_reflect: torch.stft's mirror rule (what is inside the signal and where it is loaded from is the caller's)
//   transforms   lm_c and its arithmetic, lm_fft16 (in-register DFT-16), lm_transpose16 (16 x 16 inside a row of 16 lanes),
//                lm_radix2_magnitudes (the radix-2 stages in LDS and the one-sided magnitudes)
//   projection   lm_run_dot2: a filter's run of bins against the two frames of a wave, weights from a packed table or the basis
//   cell         lm_log_clamped, lm_standardised: clamp and log10, standardisation
// The kernels keep their framing and staging, their twiddle tables, the two 1024-point decompositions with the separation of
// their spectra, and how a filter's run of bins is found.  Also kept where they were, each with its reason beside it: the
// one-frame projection loop of the two radix-2 kernels and ls_frame_kernel's cell, and the streaming kernel's loop over a
// run read from the basis.
#pragma once
#include "common.h"
#include <math.h>

#define LM_MAX_FFT 2048   // the radix-2 kernels' LDS arrays
#define LM_MAX_MELS 256   // filters: the per-filter LDS tables, one filter per thread of a workgroup
#define LM_WTAB 2048      // floats of the n_fft = 1024 kernels' LDS table of packed filter weights
#define LM_ZS 1088        // complex slots per wave: 4 rows x 16 x 17 (padded transposes) >= 1024 (the spectrum, or two of 512)
#define LM_MAG 520        // floats of a frame's magnitude strip (513 bins at n_fft = 1024)

inline int lm_log2n(int n_fft) {
  int log2n = 0;
  while ((1 << log2n) < n_fft) log2n++;
  return log2n;
}
// The value of every clamped cell, rounded from double on the host: the device's log10f(1e-10f) is -10.000001f, one ulp
// below the correctly rounded -10.0f that torch.log10 returns for the reference's clamp.  Cells above eps are untouched.
inline float lm_log_eps(float eps) { return (float)log10((double)eps); }

// torch.stft / librosa center=True, pad_mode="reflect": n_fft / 2 mirrored samples either side, the edge not repeated.
// pos: a position of the padded signal minus n_fft / 2; n: the signal's length.
__device__ __forceinline__ long long lm_reflect(long long pos, long long n) {
  pos = pos < 0 ? -pos : pos;
  return pos >= n ? 2 * (n - 1) - pos : pos;
}

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
// 16 x 16 transpose inside a row of 16 lanes: register k of lane q <-> register q of lane k.  row: the row's 16 x 17
// complex slots of LDS (row stride 17 complex: conflict-free 8-byte accesses); q: the lane inside its row.
__device__ __forceinline__ void lm_transpose16(lm_c (&v)[16], lm_c* row, int q) {
#pragma unroll
  for (int k1 = 0; k1 < 16; k1++) row[k1 * 17 + q] = v[k1];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
  for (int qq = 0; qq < 16; qq++) v[qq] = row[q * 17 + qq];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// A 256-thread workgroup's radix-2 complex FFT in LDS, then the one-sided magnitudes: re, im hold the n_fft points in
// bit-reversed order and twr, twi stage st's twiddles at [2^st, 2^(st+1)) (consecutive lanes, consecutive words), all
// written by the caller, which has met at a barrier since.  On return re[k] = |X[k]|, k = 0 .. n_fft / 2, behind a barrier.
__device__ __forceinline__ void lm_radix2_magnitudes(float* re, float* im, const float* twr, const float* twi, int n_fft,
                                                     int log2n, int tid) {
  for (int st = 0; st < log2n; st++) {
    const int half = 1 << st;
    for (int bf = tid; bf < n_fft / 2; bf += 256) {
      const int grp = bf >> st, pos = bf & (half - 1);
      const int i0 = (grp << (st + 1)) + pos, i1 = i0 + half;
      const float wr = twr[half + pos], wi = twi[half + pos];
      const float xr = re[i1] * wr - im[i1] * wi;
      const float xi = re[i1] * wi + im[i1] * wr;
      const float ar = re[i0], ai = im[i0];
      re[i0] = ar + xr; im[i0] = ai + xi;
      re[i1] = ar - xr; im[i1] = ai - xi;
    }
    __syncthreads();
  }
  const int n_bins = n_fft / 2 + 1;
  for (int k = tid; k < n_bins; k += 256) re[k] = sqrtf(re[k] * re[k] + im[k] * im[k]);
  __syncthreads();
}

// A filter against the two frames of a wave over its nonzero run of bins: bins k0, k0 + step, ... below hi, bin k's weight
// at w[k * stride] - stride 1 and w = table + offset - lo for a run packed into the LDS table, stride n_mels and
// w = basis + m for one read from the basis.  (The products with the zero weights outside the run add exact zeros to a
// non-negative sum: skipping them leaves every output bit unchanged.)
__device__ __forceinline__ void lm_run_dot2(const float* mag_a, const float* mag_b, const float* w, long stride, int k0, int hi,
                                            int step, float& sa, float& sb) {
  for (int k = k0; k < hi; k += step) {
    const float wk = w[k * stride];
    sa += mag_a[k] * wk;
    sb += mag_b[k] * wk;
  }
}

// A cell from its mel energy: clamp at eps (log_eps: lm_log_eps) and log10, then where the layer has a scaler the filter's
// standardisation.  Two functions, the test for the scaler between them at the call: a kernel that finishes the two
// frames of a wave takes that branch once and its two divisions overlap (one function per cell, branch and loads inside:
// + 1.2 % on a streaming push of 256 x 8192 samples, profiles/logmel_one_body_ab.txt).
__device__ __forceinline__ float lm_log_clamped(float acc, float eps, float log_eps) { return acc > eps ? log10f(acc) : log_eps; }
__device__ __forceinline__ float lm_standardised(float v, float mean_m, float std_m) { return (v - mean_m) / std_m; }
