// Streaming log-mel front end (gfx950): samples in, the frames that have become computable out, for many concurrent
// streams.  The framing is crk_logmel_fwd's - centred with torch.stft's reflect rule at both ends
// (the offline extraction) or uncentred (the on-the-fly layer) - and so are the clamp, log10, the host-rounded log_eps
// and the optional standardisation.
//
// Per stream the handle keeps a RING of the last n_fft samples, addressed by absolute sample index (pos & (n_fft - 1)),
// and two 64-bit counts: samples received and frames emitted in the current utterance.  Nothing else is needed:
//   * a frame that was not computable before this push starts less than n_fft samples before the old end of the signal
//     (uncentred: t hop + n_fft > n0; centred: t hop + n_fft / 2 > n0), so what it reads below n0 is in the ring;
//   * the left mirror (pos < 0 -> -pos, at most n_fft / 2) is needed only by frames with t hop < n_fft / 2, which are
//     not yet computable only while n0 < n_fft: the ring still holds the signal from sample 0;
//   * the right mirror (at the end flag, taken at the final count n1) reaches back to n1 - n_fft / 2 - 1 at the most.
// So the frame kernel reads positions below the old count from the ring and positions at or above it from the push's own
// input.  tests/logmel_stream_ref.py restates the machine in float64 and asserts the bound for every read.
//
// A push is two launches whatever S, C, n_valid and end are: ls_frame_kernel over a fixed grid of (frames a push of C
// samples can emit at the most, S) whose surplus workgroups leave at once, then ls_commit_kernel (one workgroup per
// stream), which appends the new samples to the ring, advances or resets the counts and writes n_frames.  Both derive
// the ready count from the same old counts; the stream orders them, no workgroup waits on another.
//
// A frame is transformed ALONE - by one 256-thread workgroup as a radix-2 complex FFT of z = frame + i 0 in LDS
// (ls_frame_kernel), or for n_fft = 1024 by half a wave as a real transform through a 512-point complex one
// (ls_frame1024_kernel) - with twiddles, padded window, the filters' runs of bins and their packed weights from tables the
// handle made at create time.  A frame's bits therefore depend on its own n_fft samples and the configuration alone -
// not on the cut, S, the stream's row or the frames beside it (the offline n_fft = 1024 kernel pairs neighbouring frames
// in one complex transform; this one must not).
#include "runtime.h"
#include "logmel_common.h"

#include "../../include/crank_hip.h"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <vector>

#define LS_MIN_FFT 256
#define LS_THREADS 256  // (lm_radix2_magnitudes is written for a workgroup of 256)

struct LsGeom {
  int n_fft, log2n, hop, n_mels, center, scaler, max_frames;
  float eps, log_eps;
  long long* counts;      // [S][2]: samples received, frames emitted
  float* ring;            // [S][n_fft]
  const float2* tw;       // stage st's twiddles at [2^st, 2^(st+1)), as logmel_kernel lays them out
  const float2* tw1024;   // exp(-2 pi i m / 1024), m = 0 .. 1023 (the n_fft = 1024 kernel)
  const float* wnd;       // the window zero-padded to n_fft around its centre
  const float* mel;       // [n_bins][n_mels]
  const int *mel_lo, *mel_hi;  // each filter's nonzero run of bins [lo, hi); (n_bins, 0) for an all-zero filter
  const float* wtab;      // the runs' weights packed side by side, LM_WTAB floats at the most (the n_fft = 1024 kernel's LDS table)
  const int* mel_off;     // where a filter's run starts in wtab; -1: no room, its weights are read from mel
  int wtab_n;             // floats of wtab in use
  const float *mean, *stdv;
};

// Frames of an utterance that exist once n samples of it have arrived (end: the utterance is over at n).
__host__ __device__ inline long long ls_ready(int n_fft, int hop, int center, long long n, int end) {
  if (center) {
    const int h = n_fft / 2;
    if (n <= h) return 0;  // reflect padding needs more than h samples: the offline call refuses such an utterance
    return end ? 1 + n / hop : (n - h) / hop + 1;
  }
  return n < n_fft ? 0 : (n - n_fft) / hop + 1;
}
// The most frames one push of at most M samples emits, over all histories and with the end flag.  Centred: from n0 = h
// (nothing emitted yet) an ended push of M samples emits 1 + (h + M) / hop; later histories emit ceil((h + M) / hop) at the
// most.  Uncentred: floor((a + M) / hop) - floor(a / hop) <= ceil(M / hop), reached from n0 = n_fft - 1.
static long long ls_max_frames(int n_fft, int hop, int center, long long M) {
  if (center) return 1 + (n_fft / 2 + M) / hop;
  return (M + hop - 1) / hop;
}

__device__ __forceinline__ void ls_push_range(const LsGeom& g, int s, const int* n_valid, const int* end, int C, long long& n0,
                                              long long& f0, int& nv, int& e, long long& f1) {
  n0 = g.counts[2 * s];
  f0 = g.counts[2 * s + 1];
  nv = n_valid ? n_valid[s] : C;
  nv = nv < 0 ? 0 : (nv > C ? C : nv);
  e = end ? (end[s] != 0) : 0;
  f1 = ls_ready(g.n_fft, g.hop, g.center, n0 + nv, e);
  if (f1 < f0) f1 = f0;
  if (f1 - f0 > g.max_frames) f1 = f0 + g.max_frames;  // (cannot happen: ls_max_frames is exact)
}

__global__ __launch_bounds__(LS_THREADS) void ls_frame_kernel(LsGeom g, const float* __restrict__ x, int ldx,
                                                              const int* __restrict__ n_valid, const int* __restrict__ end,
                                                              int C, float* __restrict__ out, int ldo) {
  __shared__ float re[LM_MAX_FFT], im[LM_MAX_FFT];
  __shared__ float twr[LM_MAX_FFT], twi[LM_MAX_FFT];
  const int tid = threadIdx.x, s = blockIdx.y;
  long long n0, f0, f1;
  int nv, e;
  ls_push_range(g, s, n_valid, end, C, n0, f0, nv, e, f1);
  if ((long long)blockIdx.x >= f1 - f0) return;  // (workgroup-uniform)
  const long long t = f0 + blockIdx.x, n1 = n0 + nv;
  const int n_fft = g.n_fft, mask = n_fft - 1;
  const float* ring = g.ring + (long)s * n_fft;
  const float* src = x + (long)s * ldx;
  for (int j = tid; j < n_fft; j += LS_THREADS) {
    long long pos = t * g.hop + j;
    if (g.center) pos = lm_reflect(pos - n_fft / 2, n1);  // (the right mirror is taken at the final count)
    float v = 0.f;
    if (pos >= 0 && pos < n1) v = pos < n0 ? ring[(int)(pos & mask)] : src[pos - n0];
    const int r = (int)(__brev((unsigned)j) >> (32 - g.log2n));
    re[r] = v * g.wnd[j];
    im[r] = 0.f;
    const float2 w = g.tw[j];
    twr[j] = w.x; twi[j] = w.y;
  }
  __syncthreads();
  lm_radix2_magnitudes(re, im, twr, twi, n_fft, g.log2n, tid);
  for (int m = tid; m < g.n_mels; m += LS_THREADS) {
    // The projection and the cell as logmel_kernel writes them, not through shared bodies: this serial loop of L2 reads is
    // most of a workgroup's time at n_fft 2048, and with either part behind a function of logmel_common.h a push of
    // 256 x 8192 samples measured 1.9 % slower, from code that differs in its scheduling only
    // (profiles/logmel_one_body_ab.txt).
    float acc = 0.f;
    const int k_hi = g.mel_hi[m];
    for (int k = g.mel_lo[m]; k < k_hi; k++) acc += re[k] * g.mel[(long)k * g.n_mels + m];
    float v = acc > g.eps ? log10f(acc) : g.log_eps;  // (lm_log_clamped, lm_standardised)
    if (g.scaler) v = (v - g.mean[m]) / g.stdv[m];
    out[((long)s * g.max_frames + blockIdx.x) * ldo + m] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// n_fft = 1024 (every recipe of the reference): HALF a wave transforms one frame, as a real transform through a 512-point
// complex one, 16 points per lane in registers; a wave holds two frames side by side and no value of one enters the
// other's arithmetic.  With z[m] = xw[2 m] + i xw[2 m + 1] (xw: the windowed frame), l the lane inside the half:
//   lane l holds z[32 j + l], j = 0 .. 15                             -> DFT-16 over j in registers            (k1)
//   x W_512^(k1 l); DFT-2 over lane bit 4 as one exchange                                                       (r)
//   x W_32^(q r), q = l & 15; 16 x 16 transpose inside each row of 16 lanes through LDS; DFT-16 over q         (s)
//   -> register s of lane l holds Z[(l & 15) + 16 r + 32 s];
//   X[k] = (Z[k] + conj Z[512 - k]) / 2 - (i / 2) W_1024^k (Z[k] - conj Z[512 - k]), k = 0 .. 512 (Z[512] = Z[0]).
// The waves of a workgroup meet at one barrier, behind the transform: in front of it the workgroup copies the filters'
// packed runs of weights (made at create time) into LDS, under the transforms' own loads.  Magnitudes go to a per-wave
// LDS strip; the mel projection reads each filter's run of bins, both frames of the wave per lane.
// One wave: the magnitudes of frame t (lanes 0 .. 31) and t + 1 (lanes 32 .. 63) of the stream into mag[0] and mag[1];
// live: this half's frame exists (a half without one transforms zeros).  zw: the wave's LM_ZS complex slots.
__device__ __forceinline__ void ls_magnitudes1024(const LsGeom& g, long long t, bool live, long long n0, long long n1,
                                                  const float* __restrict__ ring, const float* __restrict__ src, int lane,
                                                  lm_c* zw, float (*mag)[LM_MAG]) {
  constexpr int N = 1024, NH = 512, NB = 513;
  const int hw = lane >> 5, l = lane & 31, q = lane & 15, r = (lane >> 4) & 1;
  const lm_c* tw = reinterpret_cast<const lm_c*>(g.tw1024);
  // Every load below is issued whatever the position turns out to be (a position outside the signal reads ring[0] and is
  // replaced by 0 afterwards): 32 independent loads in flight per lane, not 32 round trips behind 32 branches.
  const long long base = t * g.hop - (g.center ? N / 2 : 0);
  auto sample = [&](int n) -> float {
    long long pos = base + n;
    if (g.center) pos = lm_reflect(pos, n1);  // (the right mirror is taken at the final count)
    const bool ok = live && pos >= 0 && pos < n1;
    const float* p = !ok ? ring : (pos < n0 ? ring + (int)(pos & (N - 1)) : src + (pos - n0));
    const float val = *p;
    return ok ? val : 0.f;
  };
  lm_c v[16], wk[17];
  const float2* wnd2 = reinterpret_cast<const float2*>(g.wnd) + l;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int n = 64 * j + 2 * l;
    const float2 w = wnd2[32 * j];  // window taps n, n + 1
    v[j] = {sample(n) * w.x, sample(n + 1) * w.y};
  }
#pragma unroll
  for (int i = 0; i < 17; i++) wk[i] = tw[l + 32 * i < NB ? l + 32 * i : 0];  // W_1024^k of this lane's bins, requested now
  lm_fft16(v);  // over j -> k1
  const lm_c twb = tw[32 * q * r];  // W_32^(q r)
#pragma unroll
  for (int k1 = 0; k1 < 16; k1++) {
    lm_c u = lm_mul(v[k1], tw[2 * k1 * l]);  // W_512^(k1 l)
    const lm_c o = {__shfl_xor(u.re, 16, 64), __shfl_xor(u.im, 16, 64)};
    u = r ? lm_sub(o, u) : lm_add(u, o);     // C[r] = B[p = 0] + (-1)^r B[p = 1]
    v[k1] = lm_mul(u, twb);
  }
  lm_transpose16(v, zw + (lane >> 4) * (16 * 17), q);
  lm_fft16(v);  // over q -> s
  lm_c* zh = zw + hw * NH;
#pragma unroll
  for (int sx = 0; sx < 16; sx++) zh[q + 16 * r + 32 * sx] = v[sx];  // Z[k1 + 16 k2], k2 = r + 2 s
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
  for (int i = 0; i < 17; i++) {
    const int k = l + 32 * i;
    if (k < NB) {
      const lm_c z = zh[k & (NH - 1)], y = zh[(NH - k) & (NH - 1)], w = wk[i];
      const float ar = z.re + y.re, ai = z.im - y.im, br = z.re - y.re, bi = z.im + y.im;
      const float xr = ar + (bi * w.re + br * w.im), xi = ai + (bi * w.im - br * w.re);
      mag[hw][k] = 0.5f * sqrtf(xr * xr + xi * xi);
    }
  }
}

__global__ __launch_bounds__(LS_THREADS) void ls_frame1024_kernel(LsGeom g, const float* __restrict__ x, int ldx,
                                                                  const int* __restrict__ n_valid,
                                                                  const int* __restrict__ end, int C,
                                                                  float* __restrict__ out, int ldo) {
  __shared__ lm_c zb[4][LM_ZS];
  __shared__ float mag[4][2][LM_MAG];
  __shared__ float wtab[LM_WTAB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y;
  long long n0, f0, f1;
  int nv, e;
  ls_push_range(g, s, n_valid, end, C, n0, f0, nv, e, f1);
  const long long cnt = f1 - f0;
  if ((long long)blockIdx.x * 8 >= cnt) return;  // (workgroup-uniform: a surplus workgroup leaves at once)
  for (int i = tid; i < g.wtab_n; i += LS_THREADS) wtab[i] = g.wtab[i];
  const long long ja = ((long long)blockIdx.x * 4 + wave) * 2;  // this wave's frames of the push: ja (lanes 0 .. 31), ja + 1
  const bool active = ja < cnt;                                 // (wave-uniform)
  if (active)
    ls_magnitudes1024(g, f0 + ja + (lane >> 5), ja + (lane >> 5) < cnt, n0, n0 + nv, g.ring + (long)s * 1024,
                      x + (long)s * ldx, lane, zb[wave], mag[wave]);
  __syncthreads();  // the weight table is in LDS, this wave's magnitudes are in its strip
  if (!active) return;
  // Mel projection, 64 filters a pass, both frames per lane.  A last pass of at most 32 (16) filters - the recipe's 80 leave
  // 16, its widest - gives each filter 2 (4) neighbouring lanes, which take every 2nd (4th) bin of its run and are summed
  // pairwise: the split is a function of n_mels alone, so it is the same for every frame of a handle.
  const bool two = ja + 1 < cnt;
  for (int m0 = 0; m0 < g.n_mels; m0 += 64) {
    const int rem = g.n_mels - m0;                         // (wave-uniform)
    const int gsh = rem <= 16 ? 2 : (rem <= 32 ? 1 : 0);   // 1 << gsh lanes per filter
    const int m = m0 + (lane >> gsh), part = lane & ((1 << gsh) - 1);
    const bool mine = m < g.n_mels;
    float sa = 0.f, sb = 0.f;
    if (mine) {
      const int lo = g.mel_lo[m], hi = g.mel_hi[m], off = g.mel_off[m];
      if (off >= 0) lm_run_dot2(mag[wave][0], mag[wave][1], wtab + off - lo, 1, lo + part, hi, 1 << gsh, sa, sb);
      else {  // a filter the table had no room for: its weights are read from the basis itself, four loads in flight.
        // Not lm_run_dot2: the rounding below is what the compiler first made of this loop unrolled by four (the leading
        // steps % 4 fused, then groups of four whose products are rounded before they are added), and such a filter's
        // cells have had these bits since; written out, they no longer depend on the code around the loop.
        const float* wp = g.mel + m;
        const int step = 1 << gsh;
        int k = lo + part;
        for (int i = k < hi ? ((hi - k + step - 1) >> gsh) & 3 : 0; i > 0; i--, k += step) {
          const float w = wp[(long)k * g.n_mels];
          sa = fmaf(mag[wave][0][k], w, sa);
          sb = fmaf(mag[wave][1][k], w, sb);
        }
#pragma unroll 4
        for (; k < hi; k += step) {
#pragma clang fp contract(off)
          const float w = wp[(long)k * g.n_mels];
          sa += mag[wave][0][k] * w;
          sb += mag[wave][1][k] * w;
        }
      }
    }
    if (gsh >= 1) { sa += __shfl_xor(sa, 1, 64); sb += __shfl_xor(sb, 1, 64); }
    if (gsh >= 2) { sa += __shfl_xor(sa, 2, 64); sb += __shfl_xor(sb, 2, 64); }
    if (mine && part == 0) {
      float va = lm_log_clamped(sa, g.eps, g.log_eps), vb = lm_log_clamped(sb, g.eps, g.log_eps);
      if (g.scaler) { va = lm_standardised(va, g.mean[m], g.stdv[m]); vb = lm_standardised(vb, g.mean[m], g.stdv[m]); }
      out[((long)s * g.max_frames + ja) * ldo + m] = va;
      if (two) out[((long)s * g.max_frames + ja + 1) * ldo + m] = vb;
    }
  }
}

__global__ __launch_bounds__(LS_THREADS) void ls_commit_kernel(LsGeom g, const float* __restrict__ x, int ldx,
                                                               const int* __restrict__ n_valid, const int* __restrict__ end,
                                                               int C, int* __restrict__ n_frames) {
  const int tid = threadIdx.x, s = blockIdx.x;
  long long n0, f0, f1;
  int nv, e;
  ls_push_range(g, s, n_valid, end, C, n0, f0, nv, e, f1);
  __syncthreads();  // every thread holds the old counts before thread 0 replaces them
  const int keep = nv < g.n_fft ? nv : g.n_fft;  // the last n_fft samples of the push are all the ring can hold
  float* ring = g.ring + (long)s * g.n_fft;
  const float* src = x + (long)s * ldx;
  for (int i = nv - keep + tid; i < nv; i += LS_THREADS) ring[(int)((n0 + i) & (g.n_fft - 1))] = src[i];
  if (tid == 0) {
    g.counts[2 * s] = e ? 0 : n0 + nv;
    g.counts[2 * s + 1] = e ? 0 : f1;
    n_frames[s] = (int)(f1 - f0);
  }
}

struct LogMelStream {
  LsGeom g;
  int S, max_samples;
  char* block;
  size_t bytes;
};

static size_t ls_align(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" int crk_logmel_stream_create(int n_fft, int hop, int win_length, const float* window, const float* mel_basis,
                                        int n_mels, float eps, const float* mean, const float* stdv, int center,
                                        int n_streams, int max_samples, void** handle) {
  if (!window || !mel_basis || !handle || n_fft < LS_MIN_FFT || n_fft > LM_MAX_FFT || (n_fft & (n_fft - 1)) ||
      win_length < 1 || win_length > n_fft || hop < 1 || n_mels < 1 || n_mels > LM_MAX_MELS || n_streams < 1 || max_samples < 1 ||
      (mean == nullptr) != (stdv == nullptr))
    return CRK_ERR_ARG;
  const long long mf = ls_max_frames(n_fft, hop, center != 0, max_samples);
  if (n_streams > 65535 || mf > INT_MAX) return CRK_ERR_UNSUPPORTED;  // a grid's y and x extents
  const int n_bins = n_fft / 2 + 1;
  // window, basis and statistics may live on either side: they are staged on the host, where the tables are made
  std::vector<float> w(win_length), fb((size_t)n_bins * n_mels), mu(n_mels, 0.f), sd(n_mels, 1.f);
  bool ok = hipMemcpy(w.data(), window, w.size() * 4, hipMemcpyDefault) == hipSuccess &&
            hipMemcpy(fb.data(), mel_basis, fb.size() * 4, hipMemcpyDefault) == hipSuccess;
  if (ok && mean)
    ok = hipMemcpy(mu.data(), mean, mu.size() * 4, hipMemcpyDefault) == hipSuccess &&
         hipMemcpy(sd.data(), stdv, sd.size() * 4, hipMemcpyDefault) == hipSuccess;
  if (!ok) return CRK_ERR_HIP;
  const int log2n = lm_log2n(n_fft);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += ls_align(bytes); return at; };
  const size_t o_counts = take((size_t)n_streams * 16), o_ring = take((size_t)n_streams * n_fft * 4);
  const size_t o_tables = o;
  const size_t o_tw = take((size_t)n_fft * 8), o_tw1024 = take(1024 * 8), o_wnd = take((size_t)n_fft * 4),
               o_mel = take(fb.size() * 4);
  const size_t o_lo = take((size_t)n_mels * 4), o_hi = take((size_t)n_mels * 4), o_mu = take((size_t)n_mels * 4),
               o_sd = take((size_t)n_mels * 4), o_wtab = take(LM_WTAB * 4), o_off = take((size_t)n_mels * 4);
  std::vector<char> host(o - o_tables, 0);
  auto at = [&](size_t off) { return host.data() + (off - o_tables); };
  float* tw = reinterpret_cast<float*>(at(o_tw));
  for (int i = 1; i < n_fft; i++) {  // exp(-2 pi i k / n_fft), k = pos (n_fft / 2 >> st), at index 2^st + pos; rounded from double
    int st = 0;
    while ((2 << st) <= i) st++;
    const int k = (i - (1 << st)) * ((n_fft >> 1) >> st);
    const double a = -2.0 * M_PI * (double)k / (double)n_fft;
    tw[2 * i] = (float)cos(a);
    tw[2 * i + 1] = (float)sin(a);
  }
  float* tw2 = reinterpret_cast<float*>(at(o_tw1024));
  for (int m = 0; m < 1024; m++) {
    const double a = -2.0 * M_PI * (double)m / 1024.0;
    tw2[2 * m] = (float)cos(a);
    tw2[2 * m + 1] = (float)sin(a);
  }
  float* wn = reinterpret_cast<float*>(at(o_wnd));
  const int lpad = (n_fft - win_length) / 2;
  for (int j = 0; j < win_length; j++) wn[lpad + j] = w[j];
  memcpy(at(o_mel), fb.data(), fb.size() * 4);
  int* lo = reinterpret_cast<int*>(at(o_lo));
  int* hi = reinterpret_cast<int*>(at(o_hi));
  for (int m = 0; m < n_mels; m++) {
    lo[m] = n_bins; hi[m] = 0;
    for (int k = 0; k < n_bins; k++)
      if (fb[(size_t)k * n_mels + m] != 0.f) { lo[m] = lo[m] < k ? lo[m] : k; hi[m] = k + 1; }
  }
  float* wt = reinterpret_cast<float*>(at(o_wtab));
  int* off = reinterpret_cast<int*>(at(o_off));
  int wtab_n = 0;
  for (int m = 0; m < n_mels; m++) {  // filters in order while their runs fit; one that does not fit is read from the basis
    const int len = hi[m] > lo[m] ? hi[m] - lo[m] : 0;
    off[m] = wtab_n + len <= LM_WTAB ? wtab_n : -1;
    if (off[m] < 0) continue;
    for (int k = 0; k < len; k++) wt[wtab_n + k] = fb[(size_t)(lo[m] + k) * n_mels + m];
    wtab_n += len;
  }
  memcpy(at(o_mu), mu.data(), mu.size() * 4);
  memcpy(at(o_sd), sd.data(), sd.size() * 4);

  LogMelStream* h = new LogMelStream();
  h->S = n_streams; h->max_samples = max_samples; h->bytes = o;
  if (hipMalloc(&h->block, h->bytes) != hipSuccess) { delete h; return CRK_ERR_HIP; }
  crk_count_alloc_();
  if (hipMemset(h->block, 0, o_tables) != hipSuccess ||
      hipMemcpy(h->block + o_tables, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(h->block);
    delete h;
    return CRK_ERR_HIP;
  }
  LsGeom& g = h->g;
  g.n_fft = n_fft; g.log2n = log2n; g.hop = hop; g.n_mels = n_mels; g.center = center != 0; g.scaler = mean != nullptr;
  g.max_frames = (int)mf;
  g.eps = eps;
  g.log_eps = lm_log_eps(eps);
  g.counts = reinterpret_cast<long long*>(h->block + o_counts);
  g.ring = reinterpret_cast<float*>(h->block + o_ring);
  g.tw = reinterpret_cast<const float2*>(h->block + o_tw);
  g.tw1024 = reinterpret_cast<const float2*>(h->block + o_tw1024);
  g.wnd = reinterpret_cast<const float*>(h->block + o_wnd);
  g.mel = reinterpret_cast<const float*>(h->block + o_mel);
  g.mel_lo = reinterpret_cast<const int*>(h->block + o_lo);
  g.mel_hi = reinterpret_cast<const int*>(h->block + o_hi);
  g.wtab = reinterpret_cast<const float*>(h->block + o_wtab);
  g.mel_off = reinterpret_cast<const int*>(h->block + o_off);
  g.wtab_n = wtab_n;
  g.mean = reinterpret_cast<const float*>(h->block + o_mu);
  g.stdv = reinterpret_cast<const float*>(h->block + o_sd);
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_logmel_stream_destroy(void* st) {
  LogMelStream* h = static_cast<LogMelStream*>(st);
  if (!h) return;
  (void)hipFree(h->block);
  delete h;
}

extern "C" long long crk_logmel_stream_state_bytes(void* st) {
  const LogMelStream* h = static_cast<const LogMelStream*>(st);
  return h ? (long long)h->bytes : -1;
}

extern "C" int crk_logmel_stream_max_frames(void* st) {
  const LogMelStream* h = static_cast<const LogMelStream*>(st);
  return h ? h->g.max_frames : -1;
}

extern "C" int crk_logmel_stream_reset(void* st, const int* stream_ids, int n, void* stream) {
  LogMelStream* h = static_cast<LogMelStream*>(st);
  if (!h) return CRK_ERR_ARG;
  return crk_zero_stream_rows(h->g.counts, 16, h->S, stream_ids, n, (hipStream_t)stream);  // a stream's two 64-bit counts
}

extern "C" int crk_logmel_stream_push(void* st, const float* x, int ldx, const int* n_valid, const int* end, int S, int C,
                                      float* out, int ldo, int* n_frames, void* stream) {
  LogMelStream* h = static_cast<LogMelStream*>(st);
  if (!h || !out || !n_frames || S < 1 || C < 0 || (C > 0 && !x) || ldx < C || ldo < h->g.n_mels) return CRK_ERR_ARG;
  if (S > h->S || C > h->max_samples) return CRK_ERR_UNSUPPORTED;
  const LsGeom& g = h->g;
  hipStream_t q = (hipStream_t)stream;
  long long fr = ls_max_frames(g.n_fft, g.hop, g.center, C);  // <= g.max_frames: C <= max_samples
  if (fr < 1) fr = 1;
  if (g.n_fft == 1024)  // eight frames per workgroup: two per wave
    ls_frame1024_kernel<<<dim3((unsigned)((fr + 7) / 8), S), LS_THREADS, 0, q>>>(g, x, ldx, n_valid, end, C, out, ldo);
  else
    ls_frame_kernel<<<dim3((unsigned)fr, S), LS_THREADS, 0, q>>>(g, x, ldx, n_valid, end, C, out, ldo);
  CRK_CHECK_LAUNCH();
  ls_commit_kernel<<<S, LS_THREADS, 0, q>>>(g, x, ldx, n_valid, end, C, n_frames);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
