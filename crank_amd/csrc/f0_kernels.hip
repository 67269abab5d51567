// Harvest F0 estimation on the device (gfx950), float64, for a ragged batch of utterances with a search range each.
//
// Replaces pyworld.harvest as sprocket's FeatureExtractor.analyze calls it (crank/feature/feature.py:75-88,
// crank/bin/evaluate_mcd.py:26-42).  The definition is the CPU restatement tests/harvest_ref.py; parity with pyworld is
// unpinned.  The caller (crank_amd/world.py HarvestF0) forms every integer of the batch's layout on
// the host and passes it in two device tables, so no kernel re-derives a size the buffers were cut by:
//   utt  [n_utts][F0_U] int64: sample offset, samples, decimated offset, decimated samples, 1 ms frame offset, 1 ms frames,
//                              channel offset, channels, raw-table offset, output offset, output frames, unused
//   chan [channels][4] int64:  half filter length h, event offset, event capacity per stream, utterance
// with range [n_utts][2] = (floor, ceil) = (0.9 minf0, 1.1 maxf0) and chan_bf [channels] the centre frequencies.
// Kernels, in the order crk_f0_harvest chains them:
//  * f0_decimate_kernel   one workgroup per utterance: zero-phase order-3 Chebyshev-I low-pass as two sequential
//                         recurrences (thread 0, chunks staged through LDS by the whole workgroup), every r-th sample, mean
//                         removed in a fixed order.
//  * f0_events_kernel     the hot path.  One workgroup per (utterance, channel) walks the decimated signal in tiles of 1024
//                         samples: taps (symmetric, h + 1 values) and tile plus halo in LDS, a direct FIR, then the four
//                         zero-crossing streams found from the filtered tile in LDS and appended in time order (a
//                         workgroup scan of the per-thread counts; no atomics).  The filtered signal never reaches HBM.
//  * f0_raw_kernel        one workgroup per 1 ms frame, one thread per channel: four interpolations by binary search into the
//                         streams, the limits, then thread 0 finds the runs of >= 10 channels.
//  * f0_overlap_kernel    one thread per (frame, slot).
//  * f0_refine_kernel     one wave per frame, the live slots one after the other: the <= 6 bins of both windowed spectra
//                         as direct sums, twiddles from a table indexed by (k j) mod N in integers.
//  * f0_reliable_kernel   one thread per (frame, slot).
//  * f0_contour_kernel    one wave per utterance: sequential along frames, the lanes share every scan.
//  * f0_subsample_kernel, f0_continuous_kernel.
// No atomics anywhere; every sum has a fixed order, so two calls give the same bits and a batch equals its rows alone.
#include "../../include/crank_hip.h"
#include "signal_common.h"

#define F0_U 12
#define F0_MAX_CH 192
#define F0_MAX_H 672
#define F0_TILE 1024
#define F0_NC 16
#define F0_NS (7 * F0_NC)
#define F0_NTW 8192
#define F0_DCHUNK 2048
#define F0_PAD 9
#define F0_SPAD 300
enum { U_S0, U_N, U_D0, U_ND, U_T0, U_T1, U_C0, U_NCH, U_R0, U_O0, U_TO };

struct F0Coef { double b[4], a[4]; };

struct F0 {
  int fs, r, shift;
  double fs_d;
  F0Coef cb;
  double* tw;  // cos [F0_NTW], sin [F0_NTW]
  double* events;
  long long events_len;
};

// ---------------------------------------------------------------------------------------------------------- decimation
__device__ __forceinline__ void f0_iir3_chunk(double* buf, int len, const F0Coef& cb, double* st) {
#pragma clang fp contract(off)
  double x1 = st[0], x2 = st[1], x3 = st[2], y1 = st[3], y2 = st[4], y3 = st[5];
  for (int j = 0; j < len; ++j) {
    const double x0 = buf[j];
    const double v = cb.b[0] * x0 + cb.b[1] * x1 + cb.b[2] * x2 + cb.b[3] * x3 - cb.a[1] * y1 - cb.a[2] * y2 - cb.a[3] * y3;
    buf[j] = v;
    x3 = x2; x2 = x1; x1 = x0;
    y3 = y2; y2 = y1; y1 = v;
  }
  st[0] = x1; st[1] = x2; st[2] = x3; st[3] = y1; st[4] = y2; st[5] = y3;
}

__global__ __launch_bounds__(W_THREADS) void f0_decimate_kernel(const double* __restrict__ x,
                                                                const long long* __restrict__ utt, int r, F0Coef cb,
                                                                double* __restrict__ tmp, double* __restrict__ yd) {
#pragma clang fp contract(off)
  __shared__ double buf[F0_DCHUNK];
  __shared__ double red[4];
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long* d = utt + (size_t)u * F0_U;
  const long long n = d[U_N], nd = d[U_ND];
  const double* xs = x + d[U_S0];
  double* out = yd + d[U_D0];
  if (r == 1) {
    for (long long i = tid; i < n; i += W_THREADS) out[i] = xs[i];
  } else {
    double* tp = tmp + d[U_S0] + 2LL * F0_PAD * u;
    const long long np = n + 2 * F0_PAD;
    double st[6] = {0, 0, 0, 0, 0, 0};
    for (long long c0 = 0; c0 < np; c0 += F0_DCHUNK) {
      const int len = (int)min((long long)F0_DCHUNK, np - c0);
      for (int j = tid; j < len; j += W_THREADS) {
        const long long i = c0 + j;
        double v;
        if (i < F0_PAD) v = 2 * xs[0] - xs[F0_PAD - i];
        else if (i < n + F0_PAD) v = xs[i - F0_PAD];
        else v = 2 * xs[n - 1] - xs[n - 2 - (i - (n + F0_PAD))];
        buf[j] = v;
      }
      __syncthreads();
      if (tid == 0) f0_iir3_chunk(buf, len, cb, st);
      __syncthreads();
      for (int j = tid; j < len; j += W_THREADS) tp[c0 + j] = buf[j];
      __syncthreads();
    }
    for (int q = 0; q < 6; ++q) st[q] = 0.0;
    for (long long c0 = 0; c0 < np; c0 += F0_DCHUNK) {
      const int len = (int)min((long long)F0_DCHUNK, np - c0);
      for (int j = tid; j < len; j += W_THREADS) buf[j] = tp[np - 1 - (c0 + j)];
      __syncthreads();
      if (tid == 0) f0_iir3_chunk(buf, len, cb, st);
      __syncthreads();
      for (int j = tid; j < len; j += W_THREADS) {
        const long long k = np - 1 - (c0 + j) - F0_PAD;
        if (k >= 0 && k < n && k % r == 0) out[k / r] = buf[j];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  double part = 0.0;
  for (long long i = tid; i < nd; i += W_THREADS) part += out[i];
  const double mean = w_block_sum(part, red) / (double)nd;
  for (long long i = tid; i < nd; i += W_THREADS) out[i] -= mean;
}

// ---------------------------------------------------------------------------------------------------------- band-pass, events
__global__ __launch_bounds__(W_THREADS) void f0_events_kernel(const double* __restrict__ yd,
                                                              const long long* __restrict__ utt,
                                                              const double* __restrict__ chan_bf,
                                                              const long long* __restrict__ chan, double fs_d,
                                                              double* __restrict__ events, int* __restrict__ counts,
                                                              int* __restrict__ status) {
  __shared__ double taps[F0_MAX_H + 1];
  __shared__ double sig[F0_TILE + 2 * F0_MAX_H + 2];
  __shared__ double s[F0_TILE + 2];
  __shared__ unsigned long long wtot[4];
  __shared__ double wpk[4];
  const long long c = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long* ci = chan + c * 4;
  const int h = max(1, min((int)ci[0], F0_MAX_H));
  const long long ev_off = ci[1];
  const int cap = (int)ci[2], u = (int)ci[3];
  const double bf = chan_bf[c];
  const long long nd = utt[(size_t)u * F0_U + U_ND];
  const double* y = yd + utt[(size_t)u * F0_U + U_D0];
  for (int k = tid; k <= h; k += W_THREADS) {
    const double p = (double)(k + h) / (2.0 * h);
    const double w = 0.355768 - 0.487396 * cos(2.0 * M_PI * p) + 0.144232 * cos(4.0 * M_PI * p) -
                     0.012604 * cos(6.0 * M_PI * p);
    taps[k] = w * cos(2.0 * M_PI * bf * k / fs_d);
  }
  // a filtered value within 1e-10 of the input's peak times h of zero is rounding residue (digital silence, a nulled
  // constant), not signal: it is taken as exactly zero, and so is such a first difference
  double pk = 0.0;
  for (long long i = tid; i < nd; i += W_THREADS) pk = fmax(pk, fabs(y[i]));
  for (int o = 32; o > 0; o >>= 1) pk = fmax(pk, __shfl_xor(pk, o));
  if (lane == 0) wpk[wv] = pk;
  __syncthreads();
  const double gate = 1e-10 * fmax(fmax(wpk[0], wpk[1]), fmax(wpk[2], wpk[3])) * (double)h;
  int base[4] = {0, 0, 0, 0};
  bool over = false;
  for (long long t0 = 0; t0 < nd; t0 += F0_TILE) {
    __syncthreads();
    for (int j = tid; j < F0_TILE + 2 + 2 * h; j += W_THREADS) {
      const long long g = t0 - h + j;
      sig[j] = (g >= 0 && g < nd) ? y[g] : 0.0;
    }
    __syncthreads();
    {
      const double* p0 = sig + h + tid;
      double acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = taps[0] * p0[W_THREADS * q];
      for (int k = 1; k <= h; ++k) {
        const double w = taps[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(w, p0[W_THREADS * q - k] + p0[W_THREADS * q + k], acc[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) s[tid + W_THREADS * q] = fabs(acc[q]) <= gate ? 0.0 : acc[q];
      if (tid < 2) {
        const double* p1 = sig + h + F0_TILE + tid;
        double a = taps[0] * p1[0];
        for (int k = 1; k <= h; ++k) a = fma(taps[k], p1[-k] + p1[k], a);
        s[F0_TILE + tid] = fabs(a) <= gate ? 0.0 : a;
      }
    }
    __syncthreads();
    // the four streams of this thread's 4 consecutive positions, in time order
    double ev[4][4];
    int n_ev[4] = {0, 0, 0, 0};
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = 4 * tid + q;
        const long long g = t0 + p;
        const double a = s[p], b = s[p + 1], e = s[p + 2];
        if (g + 1 <= nd - 1) {
          if (a > 0.0 && b <= 0.0) ev[0][n_ev[0]++] = (double)g + a / (a - b);
          if (a < 0.0 && b >= 0.0) ev[1][n_ev[1]++] = (double)g + a / (a - b);
        }
        if (g + 2 <= nd - 1) {
          double da = b - a, db = e - b;
          da = fabs(da) <= gate ? 0.0 : da;
          db = fabs(db) <= gate ? 0.0 : db;
          if (da > 0.0 && db <= 0.0) ev[2][n_ev[2]++] = (double)g + da / (da - db);
          if (da < 0.0 && db >= 0.0) ev[3][n_ev[3]++] = (double)g + da / (da - db);
        }
      }
    }
    const unsigned long long mine = (unsigned long long)n_ev[0] | ((unsigned long long)n_ev[1] << 16) |
                                    ((unsigned long long)n_ev[2] << 32) | ((unsigned long long)n_ev[3] << 48);
    unsigned long long inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int q = 0; q < 4; ++q) {
      if (q < wv) before += wtot[q];
      total += wtot[q];
    }
    const unsigned long long excl = before + inc - mine;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int at = base[st] + (int)((excl >> (16 * st)) & 0xffff);
      double* dst = events + ev_off + (long long)st * cap;
      for (int q = 0; q < n_ev[st]; ++q) {
        if (at + q < cap) dst[at + q] = ev[st][q]; else over = true;
      }
      base[st] += (int)((total >> (16 * st)) & 0xffff);
    }
  }
  if (over) status[u] = 1;
  if (tid == 0)
    for (int st = 0; st < 4; ++st) counts[c * 4 + st] = min(base[st], cap);
}

// ---------------------------------------------------------------------------------------------------------- candidates
// every run of at least 10 non-empty channels (first and last channel forced empty) gives its mean
__device__ void f0_runs(const double* col, long long stride, int n_ch, double* out) {
#pragma clang fp contract(off)
  int k = 0, c = 1;
  while (c < n_ch - 1) {
    if (col[c * stride] == 0.0) { ++c; continue; }
    int e = c;
    double acc = 0.0;
    while (e < n_ch - 1 && col[e * stride] != 0.0) { acc += col[e * stride]; ++e; }
    if (e - c >= 10 && k < F0_NC) out[k++] = acc / (double)(e - c);
    c = e;
  }
  for (; k < F0_NC; ++k) out[k] = 0.0;
}

__global__ __launch_bounds__(F0_MAX_CH) void f0_raw_kernel(const double* __restrict__ events,
                                                           const int* __restrict__ counts,
                                                           const long long* __restrict__ utt,
                                                           const double* __restrict__ range,
                                                           const double* __restrict__ chan_bf,
                                                           const long long* __restrict__ chan, int n_utts, double fs_d,
                                                           double* __restrict__ raw, double* __restrict__ official) {
#pragma clang fp contract(off)
  __shared__ double col[F0_MAX_CH];
  const long long fg = blockIdx.x;
  const int u = w_find(utt + U_T0, n_utts, fg, F0_U), c = threadIdx.x;
  const long long* d = utt + (size_t)u * F0_U;
  const long long i = fg - d[U_T0], T1 = d[U_T1];
  const int n_ch = (int)min((long long)F0_MAX_CH, d[U_NCH]);
  const double floor_f = range[2 * u], ceil_f = range[2 * u + 1];
  double val = 0.0;
  if (c < n_ch) {
    const long long cg = d[U_C0] + c;
    const double bf = chan_bf[cg], t = (double)i / 1000.0;
    const long long ev_off = chan[cg * 4 + 1];
    const int cap = (int)chan[cg * 4 + 2];
    bool ok = true;
    double v[4] = {0, 0, 0, 0};
    for (int st = 0; st < 4 && ok; ++st) {
      const int ne = counts[cg * 4 + st];
      if (ne < 3) { ok = false; break; }
      const double* e = events + ev_off + (long long)st * cap;
      int lo = 0, hi = ne - 3;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((e[mid] + e[mid + 1]) / 2.0 / fs_d <= t) lo = mid; else hi = mid - 1;
      }
      const double e0 = e[lo], e1 = e[lo + 1], e2 = e[lo + 2];
      const double x0 = (e0 + e1) / 2.0 / fs_d, x1 = (e1 + e2) / 2.0 / fs_d;
      const double y0 = fs_d / (e1 - e0), y1 = fs_d / (e2 - e1);
      const double sl = (t - x0) / (x1 - x0);
      v[st] = y0 + sl * (y1 - y0);
    }
    if (ok) {
      const double a = (((v[0] + v[1]) + v[2]) + v[3]) / 4.0;
      if (a >= 0.9 * bf && a <= 1.1 * bf && a >= floor_f && a <= ceil_f) val = a;
    }
    if (raw) raw[d[U_R0] + (long long)c * T1 + i] = val;
  }
  col[c] = val;
  __syncthreads();
  if (c == 0 && official) f0_runs(col, 1, n_ch, official + fg * F0_NC);
}

__global__ __launch_bounds__(W_THREADS) void f0_official_kernel(const double* __restrict__ raw,
                                                                const long long* __restrict__ utt, int n_utts, long long F,
                                                                double* __restrict__ official) {
  const long long fg = (long long)blockIdx.x * W_THREADS + threadIdx.x;
  if (fg >= F) return;
  const int u = w_find(utt + U_T0, n_utts, fg, F0_U);
  const long long* d = utt + (size_t)u * F0_U;
  f0_runs(raw + d[U_R0] + (fg - d[U_T0]), d[U_T1], (int)min((long long)F0_MAX_CH, d[U_NCH]), official + fg * F0_NC);
}

__global__ __launch_bounds__(W_THREADS) void f0_overlap_kernel(const double* __restrict__ official,
                                                               const long long* __restrict__ utt, int n_utts, long long F,
                                                               double* __restrict__ cands) {
  const long long g = (long long)blockIdx.x * W_THREADS + threadIdx.x;
  if (g >= F * F0_NS) return;
  const long long fg = g / F0_NS;
  const int slot = (int)(g - fg * F0_NS), b = slot / F0_NC, j = slot - b * F0_NC;
  const int u = w_find(utt + U_T0, n_utts, fg, F0_U);
  const long long t0 = utt[(size_t)u * F0_U + U_T0], T1 = utt[(size_t)u * F0_U + U_T1];
  const long long src = fg - t0 + (b == 0 ? 0 : (b <= 3 ? -b : b - 3));
  cands[g] = (src >= 0 && src < T1) ? official[(t0 + src) * F0_NC + j] : 0.0;
}

// ---------------------------------------------------------------------------------------------------------- refinement
__global__ __launch_bounds__(64) void f0_refine_kernel(const double* __restrict__ x, const double* __restrict__ cands,
                                                       const long long* __restrict__ utt, const double* __restrict__ range,
                                                       int n_utts, int fs, const double* __restrict__ twc,
                                                       const double* __restrict__ tws, double* __restrict__ refined,
                                                       double* __restrict__ scores) {
#pragma clang fp contract(off)
  const long long fg = blockIdx.x;
  const int u = w_find(utt + U_T0, n_utts, fg, F0_U), lane = threadIdx.x;
  const long long* d = utt + (size_t)u * F0_U;
  const double* xs = x + d[U_S0];
  const long long n_s = d[U_N];
  const double floor_f = range[2 * u], ceil_f = range[2 * u + 1];
  const double fsd = (double)fs, t = (double)(fg - d[U_T0]) / 1000.0;
  for (int slot = 0; slot < F0_NS; ++slot) {
    const double f = cands[fg * F0_NS + slot];
    double r_out = 0.0, s_out = 0.0;
    const double hd = f > 0.0 ? 1.5 * fsd / f + 1.0 : 0.0;
    if (hd >= 2.0 && hd < 1048576.0) {
      const int half = (int)hd, n = 2 * half + 1;
      const int N = 1 << (2 + (31 - __clz(n)));
      const int nh = min((int)(fsd / 2.0 / f), 6);
      if (N <= F0_NTW && nh >= 1) {
        // every loop over the harmonics is unrolled to 6 and guarded: the accumulators stay in registers
        int km[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) km[m] = (int)floor(f * N / fsd * (double)(m + 1) + 0.5);
        const double T = (double)n / fsd;
        const int tstep = F0_NTW / N;
        double acc[6][4];
#pragma unroll
        for (int m = 0; m < 6; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0.0;
        for (int b0 = -1; b0 < n; b0 += 62) {
          const int j = b0 + lane;
          double wj = 0.0, xv = 0.0;
          if (j >= 0 && j < n) {
            const long long idx = (long long)floor((t + (double)(j - half) / fsd) * fsd + 0.001 + 0.5);
            const double tt = (double)idx / fsd - t;
            wj = 0.42 + 0.5 * cos(2.0 * M_PI * tt / T) + 0.08 * cos(4.0 * M_PI * tt / T);
            xv = xs[max(0LL, min(idx, n_s - 1))];
          }
          const double wm = __shfl_up(wj, 1), wp = __shfl_down(wj, 1);
          if (lane >= 1 && lane <= 62 && j < n) {
            const double dj = j == 0 ? -wp / 2.0 : (j == n - 1 ? wm / 2.0 : -(wp - wm) / 2.0);
            const double a = xv * wj, bb = xv * dj;
#pragma unroll
            for (int m = 0; m < 6; ++m) {
              if (m >= nh) break;
              const int p = ((km[m] * j) & (N - 1)) * tstep;  // k j < 2^26: k <= 0.66 N, j < N / 2
              const double cs = twc[p], sn = tws[p];
              acc[m][0] = fma(a, cs, acc[m][0]);
              acc[m][1] = fma(-a, sn, acc[m][1]);
              acc[m][2] = fma(bb, cs, acc[m][2]);
              acc[m][3] = fma(-bb, sn, acc[m][3]);
            }
          }
        }
        double num = 0.0, den = 0.0, dev = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) {
          if (m >= nh) break;
          const double mr = w_wave_sum(acc[m][0]), mi = w_wave_sum(acc[m][1]);
          const double dr = w_wave_sum(acc[m][2]), di = w_wave_sum(acc[m][3]);
          const double power = mr * mr + mi * mi;
          const double inst = (double)km[m] * fsd / (double)N + (mr * di - mi * dr) / power * fsd / (2.0 * M_PI);
          const double amp = sqrt(power);
          num += amp * inst;
          den += amp * (double)(m + 1);
          dev += fabs(inst / (double)(m + 1) - f);
        }
        const double ref = num / den, score = 1.0 / (1e-12 + dev / (double)nh / f);
        if (ref >= floor_f && ref <= ceil_f && score >= 2.5) { r_out = ref; s_out = score; }
      }
    }
    if (lane == 0) {
      refined[fg * F0_NS + slot] = r_out;
      scores[fg * F0_NS + slot] = s_out;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- contour
__global__ __launch_bounds__(W_THREADS) void f0_reliable_kernel(const double* __restrict__ cands,
                                                                const double* __restrict__ scores,
                                                                const long long* __restrict__ utt, int n_utts, long long F,
                                                                double* __restrict__ oc, double* __restrict__ os) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * W_THREADS + threadIdx.x;
  if (g >= F * F0_NS) return;
  const long long fg = g / F0_NS;
  double f = cands[g], sc = scores[g];
  if (f != 0.0) {
    const int u = w_find(utt + U_T0, n_utts, fg, F0_U);
    const long long i = fg - utt[(size_t)u * F0_U + U_T0], T1 = utt[(size_t)u * F0_U + U_T1];
    if (i >= 1 && i <= T1 - 2) {
      double e = 1.0e300;
      const double* ra = cands + (fg - 1) * F0_NS;
      const double* rb = cands + (fg + 1) * F0_NS;
      for (int q = 0; q < F0_NS; ++q) e = fmin(e, fmin(fabs(f - ra[q]) / f, fabs(f - rb[q]) / f));
      if (e > 0.05) f = sc = 0.0;
    }
  }
  oc[g] = f;
  os[g] = sc;
}

// inclusive (start, end) of every voiced run of f[0 .. T), first and last frame taken as unvoiced; returns the run count
__device__ int f0_bounds(const double* f, int T, int* bl, int lane) {
  int count = 0;
  for (int b0 = 0; b0 < T - 1; b0 += 64) {
    const int i = b0 + lane;
    bool flag = false;
    if (i < T - 1) {
      const bool v0 = i > 0 && f[i] != 0.0, v1 = i + 1 < T - 1 && f[i + 1] != 0.0;
      flag = v0 != v1;
    }
    const unsigned long long mask = __ballot(flag);
    if (flag) {
      const int pos = count + __popcll(mask & ((1ULL << lane) - 1ULL));
      bl[pos] = (pos & 1) ? i : i + 1;
    }
    count += __popcll(mask);
  }
  __syncthreads();
  return count / 2;
}

// SelectBestF0 shared by the wave: the slot nearest to prev within `allowed`, the later slot on a tie; 0 when none
__device__ double f0_select(double prev, const double* row, int lane) {
#pragma clang fp contract(off)
  double be = 2.0, bc = 0.0;
  int bq = -1;
  for (int q = lane; q < F0_NS; q += 64) {
    const double c = row[q], e = fabs(prev - c) / prev;
    if (e <= 0.18 && (e < be || (e == be && q > bq))) { be = e; bc = c; bq = q; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double oe = __shfl_xor(be, o), oc = __shfl_xor(bc, o);
    const int oq = __shfl_xor(bq, o);
    if (oe < be || (oe == be && oq > bq)) { be = oe; bc = oc; bq = oq; }
  }
  return bc;
}

__device__ __forceinline__ double f0_search_score(double f, const double* row, const double* srow) {
  double best = 0.0;
  for (int q = 0; q < F0_NS; ++q)
    if (row[q] == f && srow[q] > best) best = srow[q];
  return best;
}

struct F0Contour {
  const double* cands; const double* scores;  // after f0_reliable_kernel
  const long long* utt;
  double *base, *step, *ext, *merged, *pad;  // [F] each; pad [n_utts][64][F0_SPAD]
  int* bl;                                   // [F + 2 n_utts]
  double* out;                               // [F]
};

__global__ __launch_bounds__(64) void f0_contour_kernel(F0Contour a) {
#pragma clang fp contract(off)
  const int u = blockIdx.x, lane = threadIdx.x;
  const long long t0 = a.utt[(size_t)u * F0_U + U_T0];
  const int T = (int)a.utt[(size_t)u * F0_U + U_T1];
  const double* cc = a.cands + t0 * F0_NS;
  const double* ss = a.scores + t0 * F0_NS;
  double *base = a.base + t0, *step = a.step + t0, *ext = a.ext + t0, *merged = a.merged + t0, *out = a.out + t0;
  int* bl = a.bl + t0 + 2LL * u;
  // the best-scored candidate of every frame
  for (int i = lane; i < T; i += 64) {
    double best = 0.0, bv = 0.0;
    for (int q = 0; q < F0_NS; ++q) {
      const double sc = ss[(long long)i * F0_NS + q];
      if (sc > best) { best = sc; bv = cc[(long long)i * F0_NS + q]; }
    }
    base[i] = bv;
    merged[i] = 0.0;
    out[i] = 0.0;
  }
  __syncthreads();
  // frames that jump from both the previous value and its linear prediction go
  for (int i = lane; i < T; i += 64) {
    double v = 0.0;
    if (i >= 2 && base[i] != 0.0) {
      const double ref = base[i - 1] * 2 - base[i - 2];
      const bool jump = fabs((base[i] - ref) / ref) > 0.008 && fabs((base[i] - base[i - 1]) / base[i - 1]) > 0.008;
      v = jump ? 0.0 : base[i];
    }
    step[i] = v;
  }
  __syncthreads();
  int nr = f0_bounds(step, T, bl, lane);
  for (int p = lane; p < nr; p += 64) {
    const int s0 = bl[2 * p], e0 = bl[2 * p + 1];
    if (e0 - s0 + 1 < 6)
      for (int i = s0; i <= e0; ++i) step[i] = 0.0;
  }
  __syncthreads();
  nr = f0_bounds(step, T, bl, lane);
  // extend every run through the candidate table, keep the long ones, merge by score
  int cs = -1, ce = -1;
  for (int p = 0; p < nr; ++p) {
    const int s0 = bl[2 * p], e0 = bl[2 * p + 1];
    for (int i = s0 + lane; i <= e0; i += 64) ext[i] = step[i];
    int na = s0, nb = e0;
    double prev = step[e0];
    for (int i = e0 + 1; i <= min(T - 2, e0 + 100); ++i) {
      const double v = f0_select(prev, cc + (long long)i * F0_NS, lane);
      if (v == 0.0) break;
      if (lane == 0) ext[i] = v;
      prev = v;
      nb = i;
    }
    prev = step[s0];
    for (int i = s0 - 1; i >= max(1, s0 - 100); --i) {
      const double v = f0_select(prev, cc + (long long)i * F0_NS, lane);
      if (v == 0.0) break;
      if (lane == 0) ext[i] = v;
      prev = v;
      na = i;
    }
    __syncthreads();
    double part = 0.0;
    for (int i = na + lane; i <= nb; i += 64) part += ext[i];
    const double mean = w_wave_sum(part) / (double)(nb - na + 1);
    if ((double)(nb - na + 1) > 2200.0 / mean) {
      if (ce < 0 || na > ce) {
        for (int i = na + lane; i <= nb; i += 64) merged[i] = ext[i];
        cs = na; ce = nb;
      } else if (cs <= na && ce >= nb) {
      } else {
        double s1 = 0.0, s2 = 0.0;
        for (int i = na + lane; i <= ce; i += 64) {
          s1 += f0_search_score(merged[i], cc + (long long)i * F0_NS, ss + (long long)i * F0_NS);
          s2 += f0_search_score(i <= nb ? ext[i] : 0.0, cc + (long long)i * F0_NS, ss + (long long)i * F0_NS);
        }
        s1 = w_wave_sum(s1);
        s2 = w_wave_sum(s2);
        if (s1 > s2) {
          for (int i = ce + 1 + lane; i <= nb; i += 64) merged[i] = ext[i];
        } else {
          for (int i = na + lane; i <= nb; i += 64) merged[i] = ext[i];
        }
        ce = nb;
      }
    }
    __syncthreads();
  }
  // short gaps are bridged linearly
  nr = f0_bounds(merged, T, bl, lane);
  for (int i = lane; i < T; i += 64) step[i] = merged[i];
  __syncthreads();
  for (int p = lane; p + 1 < nr; p += 64) {
    const int e0 = bl[2 * p + 1], s1 = bl[2 * p + 2];
    if (s1 - e0 - 1 < 9)
      for (int j = e0 + 1; j < s1; ++j)
        step[j] = merged[e0] + (merged[s1] - merged[e0]) * (double)(j - e0) / (double)(s1 - e0);
  }
  __syncthreads();
  // zero-phase second-order low-pass over each voiced run, one lane per run
  nr = f0_bounds(step, T, bl, lane);
  double* pad = a.pad + ((size_t)u * 64 + lane) * F0_SPAD;
  const double B0 = 0.0078202080334971724, A1 = -1.7347257688092754, A2 = 0.76600660094326412;
  for (int p = lane; p < nr; p += 64) {
    const int s0 = bl[2 * p], e0 = bl[2 * p + 1];
    double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0;
    for (int q = 0; q < 2 * F0_SPAD + (e0 - s0 + 1); ++q) {
      const int i = s0 + q - F0_SPAD;
      const double x0 = step[max(s0, min(i, e0))];
      const double o = B0 * x0 + 2.0 * B0 * x1 + B0 * x2 - A1 * y1 - A2 * y2;
      if (i >= s0 && i <= e0) out[i] = o;
      else if (i > e0) pad[i - e0 - 1] = o;
      x2 = x1; x1 = x0; y2 = y1; y1 = o;
    }
    x1 = x2 = y1 = y2 = 0.0;
    for (int q = 0; q < F0_SPAD + (e0 - s0 + 1); ++q) {
      const int i = e0 + F0_SPAD - q;
      const double x0 = i > e0 ? pad[i - e0 - 1] : out[i];
      const double o = B0 * x0 + 2.0 * B0 * x1 + B0 * x2 - A1 * y1 - A2 * y2;
      if (i <= e0) out[i] = o;
      x2 = x1; x1 = x0; y2 = y1; y1 = o;
    }
  }
}

__global__ __launch_bounds__(W_THREADS) void f0_subsample_kernel(const double* __restrict__ f1,
                                                                 const long long* __restrict__ utt, int n_utts, int shift,
                                                                 long long total_out, double* __restrict__ f0) {
  const long long g = (long long)blockIdx.x * W_THREADS + threadIdx.x;
  if (g >= total_out) return;
  const int u = w_find(utt + U_O0, n_utts, g, F0_U);
  const long long* d = utt + (size_t)u * F0_U;
  f0[g] = f1[d[U_T0] + min((g - d[U_O0]) * shift, d[U_T1] - 1)];
}

// ---------------------------------------------------------------------------------------------------------- continuous F0
__global__ __launch_bounds__(W_THREADS) void f0_continuous_kernel(const double* __restrict__ f0,
                                                                  const long long* __restrict__ foff, float* __restrict__ uv,
                                                                  double* __restrict__ filled, double* __restrict__ cf0,
                                                                  double* __restrict__ lf0, double* __restrict__ lcf0,
                                                                  int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ int first[W_THREADS], last[W_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const long long F0 = foff[u];
  const int T = (int)(foff[u + 1] - F0);
  const double* f = f0 + F0;
  int lo = T, hi = -1;
  for (int i = tid; i < T; i += W_THREADS)
    if (f[i] != 0.0) { lo = min(lo, i); hi = max(hi, i); }
  first[tid] = lo;
  last[tid] = hi;
  __syncthreads();
  for (int o = W_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { first[tid] = min(first[tid], first[tid + o]); last[tid] = max(last[tid], last[tid + o]); }
    __syncthreads();
  }
  const int si = first[0], ei = last[0];
  if (ei < 0) {
    if (tid == 0) status[u] = 1;
    return;
  }
  if (tid == 0) status[u] = 0;
  const double fs0 = f[si], fe0 = f[ei];
  for (int i = tid; i < T; i += W_THREADS) {
    uv[F0 + i] = f[i] != 0.0 ? 1.f : 0.f;
    const double v = i < si ? fs0 : (i >= ei ? fe0 : f[i]);
    filled[F0 + i] = v;
    lf0[F0 + i] = log(v + 1e-10);
  }
  __syncthreads();
  const double* g = filled + F0;
  for (int i = tid; i < T; i += W_THREADS) {
    double c = g[i];
    if (c == 0.0) {  // between two voiced frames (the ends are filled): numpy.interp's slope * (x - x_lo) + y_lo
      int b = i + 1, a0 = i - 1;
      while (b < T - 1 && g[b] == 0.0) ++b;
      while (a0 > 0 && g[a0] == 0.0) --a0;
      c = (g[b] - g[a0]) / (double)(b - a0) * (double)(i - a0) + g[a0];
    }
    cf0[F0 + i] = c;
    lcf0[F0 + i] = log(c);
  }
}

// ---------------------------------------------------------------------------------------------------------- host side
extern "C" void* crk_f0_create(int fs, int shiftms, const double* cheby) {
  if (fs < 8000 || fs > 48000 || shiftms < 1 || shiftms > 1000 || !cheby) return nullptr;
  F0* h = new F0();
  h->fs = fs;
  h->shift = shiftms;
  h->r = (int)fmin(12.0, fmax(1.0, floor(fs / 8000.0 + 0.5)));
  h->fs_d = (double)fs / h->r;
  for (int i = 0; i < 4; ++i) { h->cb.b[i] = cheby[i]; h->cb.a[i] = cheby[4 + i]; }
  WTables tb;
  tb.add_twiddles(F0_NTW, F0_NTW);  // the full circle
  if (!tb.upload(&h->tw)) {
    delete h;
    return nullptr;
  }
  return h;
}

extern "C" void crk_f0_destroy(void* p) {
  F0* h = (F0*)p;
  if (!h) return;
  (void)hipFree(h->tw);
  if (h->events) (void)hipFree(h->events);
  delete h;
}

extern "C" int crk_f0_reserve(void* p, long long total_events) {
  F0* h = (F0*)p;
  if (!h || total_events < 1 || total_events > (1LL << 36)) return CRK_ERR_ARG;
  if (total_events <= h->events_len) return CRK_OK;
  return w_grow_table(&h->events, &h->events_len, total_events, nullptr);  // the kernels fill it
}

struct F0Ws {
  double *tmp, *yd, *official, *ta, *tb, *tc, *td, *te, *base, *step, *ext, *merged, *f1, *pad;
  int *bl, *counts;
  size_t bytes;
};

static F0Ws f0_ws(int n_utts, long long S, long long F, long long C, unsigned char* base) {
  F0Ws r;
  WCarve c{base};
  r.tmp = c.take<double>((size_t)(S + 2LL * F0_PAD * n_utts));
  r.yd = c.take<double>((size_t)S);
  r.official = c.take<double>((size_t)F * F0_NC);
  r.ta = c.take<double>((size_t)F * F0_NS);
  r.tb = c.take<double>((size_t)F * F0_NS);
  r.tc = c.take<double>((size_t)F * F0_NS);
  r.td = c.take<double>((size_t)F * F0_NS);
  r.te = c.take<double>((size_t)F * F0_NS);
  r.base = c.take<double>((size_t)F);
  r.step = c.take<double>((size_t)F);
  r.ext = c.take<double>((size_t)F);
  r.merged = c.take<double>((size_t)F);
  r.f1 = c.take<double>((size_t)F);
  r.pad = c.take<double>((size_t)n_utts * 64 * F0_SPAD);
  r.bl = c.take<int>((size_t)(F + 2LL * n_utts));
  r.counts = c.take<int>((size_t)C * 4);
  r.bytes = c.bytes;
  return r;
}

static bool f0_shape_ok(int n_utts, long long S, long long F, long long C) {
  return n_utts >= 1 && S >= 1 && F >= 1 && C >= 1 && S < (1LL << 40) && F * F0_NS < (1LL << 31) * W_THREADS &&
         F <= (1LL << 31) - 1 && C <= (1LL << 31) - 1 && C <= (long long)n_utts * F0_MAX_CH;
}

extern "C" long long crk_f0_workspace_bytes(int n_utts, long long total_samples, long long total_frames,
                                            long long total_channels) {
  if (!f0_shape_ok(n_utts, total_samples, total_frames, total_channels)) return -1;
  return (long long)f0_ws(n_utts, total_samples, total_frames, total_channels, nullptr).bytes;
}

static unsigned f0_blocks(long long n) { return (unsigned)((n + W_THREADS - 1) / W_THREADS); }

extern "C" int crk_f0_decimate(void* p, const double* x, const long long* utt, int n_utts, long long total_samples,
                               double* yd, void* workspace, long long workspace_bytes, void* stream) {
  F0* h = (F0*)p;
  if (!h || !x || !utt || !yd || !workspace || n_utts < 1 || total_samples < 1) return CRK_ERR_ARG;
  WCarve c{(unsigned char*)workspace};
  double* tmp = c.take<double>((size_t)(total_samples + 2LL * F0_PAD * n_utts));
  if (workspace_bytes < (long long)c.bytes) return CRK_ERR_ARG;
  f0_decimate_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, (hipStream_t)stream>>>(x, utt, h->r, h->cb, tmp, yd);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

static int f0_raw(F0* h, const double* yd, const long long* utt, const double* range, const double* chan_bf,
                  const long long* chan, int n_utts, long long C, long long F, long long E, double* raw, double* official,
                  int* counts, int* status, hipStream_t st) {
  if (E < 1 || E > h->events_len) return CRK_ERR_ARG;  // crk_f0_reserve(total_events) first
  if (hipMemsetAsync(status, 0, (size_t)n_utts * sizeof(int), st) != hipSuccess) return CRK_ERR_HIP;
  f0_events_kernel<<<dim3((unsigned)C), dim3(W_THREADS), 0, st>>>(yd, utt, chan_bf, chan, h->fs_d, h->events, counts, status);
  CRK_CHECK_LAUNCH();
  f0_raw_kernel<<<dim3((unsigned)F), dim3(F0_MAX_CH), 0, st>>>(h->events, counts, utt, range, chan_bf, chan, n_utts,
                                                              h->fs_d, raw, official);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_f0_raw_candidates(void* p, const double* yd, const long long* utt, const double* range,
                                     const double* chan_bf, const long long* chan, int n_utts, long long total_channels,
                                     long long total_frames, long long total_events, double* raw, int* status,
                                     void* workspace, long long workspace_bytes, void* stream) {
  F0* h = (F0*)p;
  if (!h || !yd || !utt || !range || !chan_bf || !chan || !raw || !status || !workspace ||
      !f0_shape_ok(n_utts, 1, total_frames, total_channels))
    return CRK_ERR_ARG;
  WCarve c{(unsigned char*)workspace};
  int* counts = c.take<int>((size_t)total_channels * 4);
  if (workspace_bytes < (long long)c.bytes) return CRK_ERR_ARG;
  return f0_raw(h, yd, utt, range, chan_bf, chan, n_utts, total_channels, total_frames, total_events, raw, nullptr,
                counts, status, (hipStream_t)stream);
}

extern "C" int crk_f0_candidates(void* p, const double* raw, const long long* utt, int n_utts, long long total_frames,
                                 double* cands, void* workspace, long long workspace_bytes, void* stream) {
  F0* h = (F0*)p;
  if (!h || !raw || !utt || !cands || !workspace || !f0_shape_ok(n_utts, 1, total_frames, 1)) return CRK_ERR_ARG;
  WCarve c{(unsigned char*)workspace};
  double* official = c.take<double>((size_t)total_frames * F0_NC);
  if (workspace_bytes < (long long)c.bytes) return CRK_ERR_ARG;
  f0_official_kernel<<<dim3(f0_blocks(total_frames)), dim3(W_THREADS), 0, (hipStream_t)stream>>>(raw, utt, n_utts,
                                                                                               total_frames, official);
  CRK_CHECK_LAUNCH();
  f0_overlap_kernel<<<dim3(f0_blocks(total_frames * F0_NS)), dim3(W_THREADS), 0, (hipStream_t)stream>>>(
      official, utt, n_utts, total_frames, cands);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_f0_refine(void* p, const double* x, const double* cands, const long long* utt, const double* range,
                             int n_utts, long long total_frames, double* refined, double* scores, void* stream) {
  F0* h = (F0*)p;
  if (!h || !x || !cands || !utt || !range || !refined || !scores || !f0_shape_ok(n_utts, 1, total_frames, 1))
    return CRK_ERR_ARG;
  f0_refine_kernel<<<dim3((unsigned)total_frames), dim3(64), 0, (hipStream_t)stream>>>(
      x, cands, utt, range, n_utts, h->fs, h->tw, h->tw + F0_NTW, refined, scores);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

static int f0_contour(const double* refined, const double* scores, const long long* utt, int n_utts, long long F,
                      double* f1, const F0Ws& ws, hipStream_t st) {
  f0_reliable_kernel<<<dim3(f0_blocks(F * F0_NS)), dim3(W_THREADS), 0, st>>>(refined, scores, utt, n_utts, F, ws.td, ws.te);
  CRK_CHECK_LAUNCH();
  F0Contour a{ws.td, ws.te, utt, ws.base, ws.step, ws.ext, ws.merged, ws.pad, ws.bl, f1};
  f0_contour_kernel<<<dim3(n_utts), dim3(64), 0, st>>>(a);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_f0_contour(void* p, const double* refined, const double* scores, const long long* utt, int n_utts,
                              long long total_frames, double* f0_1ms, void* workspace, long long workspace_bytes,
                              void* stream) {
  F0* h = (F0*)p;
  if (!h || !refined || !scores || !utt || !f0_1ms || !workspace || !f0_shape_ok(n_utts, 1, total_frames, 1))
    return CRK_ERR_ARG;
  const F0Ws ws = f0_ws(n_utts, 1, total_frames, 1, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  return f0_contour(refined, scores, utt, n_utts, total_frames, f0_1ms, ws, (hipStream_t)stream);
}

extern "C" int crk_f0_harvest(void* p, const double* x, const long long* utt, const double* range, const double* chan_bf,
                              const long long* chan, int n_utts, long long total_samples, long long total_channels,
                              long long total_frames, long long total_events, long long total_out, double* f0, int* status,
                              void* workspace, long long workspace_bytes, void* stream) {
  F0* h = (F0*)p;
  if (!h || !x || !utt || !range || !chan_bf || !chan || !f0 || !status || !workspace || total_out < 1 ||
      !f0_shape_ok(n_utts, total_samples, total_frames, total_channels))
    return CRK_ERR_ARG;
  const F0Ws ws = f0_ws(n_utts, total_samples, total_frames, total_channels, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long F = total_frames;
  f0_decimate_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, st>>>(x, utt, h->r, h->cb, ws.tmp, ws.yd);
  CRK_CHECK_LAUNCH();
  int rc = f0_raw(h, ws.yd, utt, range, chan_bf, chan, n_utts, total_channels, F, total_events, nullptr, ws.official,
                  ws.counts, status, st);
  if (rc) return rc;
  f0_overlap_kernel<<<dim3(f0_blocks(F * F0_NS)), dim3(W_THREADS), 0, st>>>(ws.official, utt, n_utts, F, ws.ta);
  CRK_CHECK_LAUNCH();
  f0_refine_kernel<<<dim3((unsigned)F), dim3(64), 0, st>>>(x, ws.ta, utt, range, n_utts, h->fs, h->tw, h->tw + F0_NTW,
                                                          ws.tb, ws.tc);
  CRK_CHECK_LAUNCH();
  rc = f0_contour(ws.tb, ws.tc, utt, n_utts, F, ws.f1, ws, st);
  if (rc) return rc;
  f0_subsample_kernel<<<dim3(f0_blocks(total_out)), dim3(W_THREADS), 0, st>>>(ws.f1, utt, n_utts, h->shift, total_out, f0);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_f0_continuous(const double* f0, const long long* frame_offsets, int n_utts, long long total_frames,
                                 float* uv, double* f0_filled, double* cf0, double* lf0, double* lcf0, int* status,
                                 void* stream) {
  if (!f0 || !frame_offsets || !uv || !f0_filled || !cf0 || !lf0 || !lcf0 || !status || n_utts < 1 || total_frames < 1 ||
      total_frames > (1LL << 31) - 1)
    return CRK_ERR_ARG;
  f0_continuous_kernel<<<dim3(n_utts), dim3(W_THREADS), 0, (hipStream_t)stream>>>(f0, frame_offsets, uv, f0_filled, cf0,
                                                                                 lf0, lcf0, status);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
