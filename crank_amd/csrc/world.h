// The WORLD synthesis handle (world_kernels.hip) as the streaming synthesis (world_stream_kernels.hip) reads it.
#pragma once
#include <math.h>

struct World {
  int fs, m1, bands, capacity;
  double shiftms, fp, alpha;
  double* tables;  // one device block: at [m1][W_IRLEN], wt [m1][W_K], tw cos [W_N/2], tw sin [W_N/2], dc [W_N]
  const double *at, *wt, *twc, *tws, *dcw;
  double* noise;
  long long noise_len;
};

static int w_bands(int fs) { return (int)(fmin(15000.0, fs / 2.0 - 3000.0) / 3000.0); }
