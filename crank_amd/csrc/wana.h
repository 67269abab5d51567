// What the two WORLD analysis families on one crk_wana handle share (world_analysis_kernels.hip: low cut, CheapTrick,
// sp2mc, npow; d4c_kernels.hip: D4C aperiodicity and its coding): the handle and the equally spaced interpolation.
#pragma once
#include "signal_common.h"

#define D4_N 2048  // both of D4C's transforms at the supported rates
#define D4_K (D4_N / 2 + 1)
#define D4_LOGN 11
#define D4_MAX_BANDS 3
#define D4_FS_MIN 13640
#define D4_FS_MAX 24052

struct Wana {
  int fs, m1;
  double shiftms, alpha;
  double* tables;  // one device block: tw cos [W_N/2], tw sin [W_N/2], at [m1][W_K]; with D4C: tw2 cos, sin [D4_N/2], nuttall
  const double *twc, *tws, *at;
  double* noise;
  long long noise_len;
  // D4C (null / 0 outside D4_FS_MIN .. D4_FS_MAX)
  const double *twc2, *tws2, *nuttall;
  int d4_half, d4_bands;  // half length of the Nuttall window; coded bands
};

// linear interpolation on the knots x0 + j dx (j < len) by index arithmetic; zero slope from the last knot on.  No
// contraction: y0 + (y1 - y0) * s fused rounds once where the restatement rounds twice, which on a cumulative spectrum
// moves a bin 1e5 below the frame's peak by 1e-11 in the rare case where the two differ (seen in 3 of 54 frames).
__device__ __forceinline__ double wa_interp(const double* y, int len, double x0, double dx, double xi) {
#pragma clang fp contract(off)
  const double fr = (xi - x0) / dx;
  const int base = max(0, min((int)fr, len - 1));
  const double y0 = y[base], y1 = base + 1 < len ? y[base + 1] : y0;
  return y0 + (y1 - y0) * (fr - base);
}
