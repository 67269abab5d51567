// Streaming F0 conditioning (gfx950): samples in, the lcf0 / uv rows a decoder_f0 model's streaming conversion takes out,
// for many concurrent streams.  Harvest's contour rules reach arbitrarily far along a voiced run,
// so it is not streamed bit for bit: it is run, by the kernels of f0_kernels.hip unchanged (crk_f0_harvest through a
// handle with a frame period of 1 ms), on a bounded window around each BLOCK of 1 ms frames.
//
// The grid is in whole milliseconds and in integers (FsGrid; tests/f0_stream_ref.py restates it with sets):
//   block j = the stream's 1 ms frames [j block, (j + 1) block), ready once the stream holds ((j + 1) block + ahead) ms;
//   its window = the signal over [max(j block - back, 0) ms, ((j + 1) block + ahead) ms), truncated - not filled - at the
//   stream's start and, at the end flag, at the last sample;
//   output frame t sits at 1 ms frame t shiftms, or (2000 t hop + fs) / (2 fs): the 1 ms frame nearest t hop samples.
//
// Per stream the handle keeps a RING of raw fp32 samples addressed by absolute position (pos & mask), two 64-bit counts
// (samples received, blocks emitted), the carry (the last continuous F0 emitted) and a sticky flag word.  A window that
// was not ready before this push starts less than back + block + ahead ms before the old count, and the low cut reaches
// n_taps - 1 samples further back: what a window reads below the old count is in the ring, the rest in the push's own
// input.  The low cut is the causal FIR of crank.utils.low_cut_filter with zero history at the stream's start, each
// sample by wana_lowcut_kernel's fma chain in its tap order, so a window equals the same slice of the whole signal's
// filter output bit for bit.
//
// The HOST keeps the same two counts (it knows how many samples it pushed), so it knows which streams are ready and how
// long their windows are: crk_f0_stream_plan tells the caller, who brings Harvest's layout tables for each ROUND (the
// streams that have a j-th block ready in this push).  A push runs, per round, fs_window_kernel, crk_f0_harvest and
// fs_finish_kernel, then fs_commit_kernel; a push with no ready block is the commit alone.  Nothing is read back.
#include "runtime.h"
#include "wana_frame.h"

#include "../../include/crank_hip.h"
#include <limits.h>
#include <vector>

#define FS_THREADS 256
#define FS_MAX_TAPS 256
#define FS_MIN_SAMPLES 64  // Harvest's shortest signal
#define FS_FLAG_EVENTS 1   // a Harvest event stream overflowed in one of the stream's windows
#define FS_FLAG_LAYOUT 2   // a round's tables did not fit the device's counts (the window was zeroed, nothing emitted)

struct FsGrid {
  int fs, back, ahead, block, shift, hop;  // ms; shift > 0: the shiftms grid, else the hop grid
  long long Bs, As;                        // block and ahead in samples
};

struct FsState {
  long long n, b;  // samples received, blocks emitted in the current utterance
  double carry;    // the last cf0 emitted
  int has_carry, flags;
};

#define FS_HD __host__ __device__ inline

FS_HD long long fs_min(long long a, long long b) { return a < b ? a : b; }
FS_HD long long fs_max(long long a, long long b) { return a > b ? a : b; }
// the 1 ms frame of output frame t
FS_HD long long fs_idx(const FsGrid& g, long long t) {
  return g.shift ? t * g.shift : (2000LL * t * g.hop + g.fs) / (2LL * g.fs);
}
// the first output frame at or after 1 ms frame m
FS_HD long long fs_tlo(const FsGrid& g, long long m) {
  if (m <= 0) return 0;
  if (g.shift) return (m + g.shift - 1) / g.shift;
  const long long d = 2000LL * g.hop;
  return (2LL * g.fs * m - g.fs + d - 1) / d;
}
// the offline frame count of n samples
FS_HD long long fs_frames(const FsGrid& g, long long n) {
  return g.shift ? 1000LL * n / ((long long)g.fs * g.shift) + 1 : 1 + n / g.hop;
}
// blocks that exist once n samples have arrived (e: the utterance is over at n)
FS_HD long long fs_blocks(const FsGrid& g, long long n, int e) {
  if (e) return n < FS_MIN_SAMPLES ? 0 : (1000LL * n / g.fs) / g.block + 1;
  return n < g.As + g.Bs ? 0 : (n - g.As) / g.Bs;
}
// block j's window: first 1 ms frame, first sample, samples
FS_HD void fs_window(const FsGrid& g, long long j, long long n1, int e, long long& a_ms, long long& a, long long& L) {
  a_ms = fs_max(j * g.block - g.back, 0);
  a = a_ms * g.fs / 1000;
  long long hi = (j + 1) * g.Bs + g.As;
  if (e) hi = fs_min(hi, n1);
  L = hi - a;
}
// The output frames block j's window of T1 1 ms frames holds, [wlo, whi), and those the block emits, [elo, ehi); base: the
// first frame this push emits (block b0's first).  At the end the frames are those below the offline count T, their 1 ms
// index clamped to the last 1 ms frame M - 1; a window the end did not truncate holds what it would have held had the
// stream gone on, so that the cut cannot matter.
FS_HD void fs_spans(const FsGrid& g, long long b0, long long j, long long a_ms, long long T1, long long n1, int e,
                    long long& base, long long& wlo, long long& whi, long long& elo, long long& ehi) {
  const long long T = e ? fs_frames(g, n1) : LLONG_MAX, M = 1000LL * n1 / g.fs + 1;
  base = fs_min(fs_tlo(g, b0 * g.block), T);
  wlo = fs_min(fs_tlo(g, a_ms), T);
  whi = (e && (j + 1) * g.Bs + g.As > n1) ? T : fs_tlo(g, a_ms + T1);  // T: the end truncated the window
  elo = fs_min(fs_tlo(g, j * g.block), T);
  ehi = (e && (j + 1) * g.block >= M) ? T : fs_min(fs_tlo(g, (j + 1) * g.block), T);
}

struct FsGeom {
  FsGrid grid;
  int n_taps, ring_n, max_frames, gmax;
  FsState* state;      // [S]
  float* ring;         // [S][ring_n]
  const double* taps;  // [n_taps]; n_taps = 0: no low cut
  double* gbuf;        // [S][gmax]: a window's contour at its output frames
};

__device__ __forceinline__ void fs_push_range(const FsGeom& g, int s, const int* n_valid, const int* end, int C,
                                              long long& n0, long long& b0, int& nv, int& e, long long& b1) {
  n0 = g.state[s].n;
  b0 = g.state[s].b;
  nv = n_valid ? n_valid[s] : C;
  nv = nv < 0 ? 0 : (nv > C ? C : nv);
  e = end ? (end[s] != 0) : 0;
  b1 = fs_max(b0, fs_blocks(g.grid, n0 + nv, e));
}

// The windows of one round's ready streams, float64, laid out as the round's Harvest tables have them (utt: sample offset
// and samples in columns 0 and 1): sample p of the stream from the ring below the old count, from the push above it.
__global__ __launch_bounds__(FS_THREADS) void fs_window_kernel(FsGeom g, const float* __restrict__ x, int ldx,
                                                               const int* __restrict__ n_valid, const int* __restrict__ end,
                                                               int C, int round, const int* __restrict__ ids,
                                                               const long long* __restrict__ utt, double* __restrict__ xwin) {
  __shared__ double h[FS_MAX_TAPS];
  for (int k = threadIdx.x; k < g.n_taps; k += FS_THREADS) h[k] = g.taps[k];
  __syncthreads();
  const int u = blockIdx.y, s = ids[u];
  long long n0, b0, b1, a_ms, a, L;
  int nv, e;
  fs_push_range(g, s, n_valid, end, C, n0, b0, nv, e, b1);
  const long long j = b0 + round, off = utt[(size_t)u * 12], Lt = utt[(size_t)u * 12 + 1];
  fs_window(g.grid, j, n0 + nv, e, a_ms, a, L);
  const long long i = (long long)blockIdx.x * FS_THREADS + threadIdx.x;
  if (i >= Lt) return;
  if (j >= b1 || L != Lt) {  // (cannot happen while the host's counts are the device's)
    xwin[off + i] = 0.0;
    if (i == 0) g.state[s].flags |= FS_FLAG_LAYOUT;
    return;
  }
  const float* ring = g.ring + (size_t)s * g.ring_n;
  const float* src = x + (size_t)s * ldx;
  const int mask = g.ring_n - 1;
  const long long p = a + i;
  auto sample = [&](long long q) -> double { return (double)(q < n0 ? ring[(int)(q & mask)] : src[q - n0]); };
  if (g.n_taps == 0) {
    xwin[off + i] = sample(p);
    return;
  }
  xwin[off + i] = wa_lowcut_sample(h, g.n_taps, p, sample);  // (wana_lowcut_kernel's chain)
}

struct FsFinish {
  const int* ids;
  const long long* utt;
  const double* f1;      // the round's 1 ms contours at the tables' frame offsets
  const int* hstatus;    // Harvest's status per ready stream
  const int *org, *cv;
  const double *spk_mean, *spk_std;
  int n_spk, has_scaler;
  double g_mean, g_scale;
  float *lcf0, *uv;
  double *raw, *cv_f0;   // optional
};

// One workgroup per ready stream: the window's contour at its output frames, convert_continuos_f0 of it (or the carry
// where it has no voiced frame), convert_f0 org -> cv, the global scaler; float64, rounded once.  Only the block's frames
// are written, behind what the push's earlier rounds wrote.
__global__ __launch_bounds__(FS_THREADS) void fs_finish_kernel(FsGeom g, const int* __restrict__ n_valid,
                                                               const int* __restrict__ end, int C, int round, FsFinish a) {
#pragma clang fp contract(off)
  __shared__ int first[FS_THREADS], last[FS_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x, s = a.ids[u];
  long long n0, b0, b1, a_ms, as, L, base, wlo, whi, elo, ehi;
  int nv, e;
  fs_push_range(g, s, n_valid, end, C, n0, b0, nv, e, b1);
  const long long j = b0 + round, T1 = a.utt[(size_t)u * 12 + 5];
  fs_window(g.grid, j, n0 + nv, e, a_ms, as, L);
  if (j >= b1 || L != a.utt[(size_t)u * 12 + 1]) return;  // (fs_window_kernel set the flag)
  fs_spans(g.grid, b0, j, a_ms, T1, n0 + nv, e, base, wlo, whi, elo, ehi);
  const int G = (int)fs_min(fs_max(whi - wlo, 0), g.gmax);
  const double* f1 = a.f1 + a.utt[(size_t)u * 12 + 4];
  double* gb = g.gbuf + (size_t)s * g.gmax;
  int lo = G, hi = -1;
  for (int i = tid; i < G; i += FS_THREADS) {
    const long long li = fs_min(fs_max(fs_idx(g.grid, wlo + i) - a_ms, 0), T1 - 1);
    const double v = f1[li];
    gb[i] = v;
    if (v != 0.0) { lo = min(lo, i); hi = max(hi, i); }
  }
  first[tid] = lo;
  last[tid] = hi;
  const int n_spk = a.n_spk;
  const int o = min(max(a.org[s], 0), n_spk - 1), c = min(max(a.cv[s], 0), n_spk - 1);
  const double carry = g.state[s].has_carry ? g.state[s].carry : exp(a.spk_mean[o]);
  __syncthreads();  // the contour is in gbuf; every thread holds the old carry
  for (int w = FS_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) { first[tid] = min(first[tid], first[tid + w]); last[tid] = max(last[tid], last[tid + w]); }
    __syncthreads();
  }
  const int si = first[0], ei = last[0];
  const double m_org = a.spk_mean[o], s_org = a.spk_std[o], m_cv = a.spk_mean[c], s_cv = a.spk_std[c];
  const int i0 = (int)(elo - wlo), i1 = (int)fs_min(ehi - wlo, G);
  for (int i = i0 + tid; i < i1; i += FS_THREADS) {
    const long long k = elo - base + (i - i0);
    if (i < 0 || k < 0 || k >= g.max_frames) continue;  // (cannot happen: max_frames is exact)
    const double v = gb[i];
    double cf = carry;
    if (ei >= 0) {
      cf = i < si ? gb[si] : (i >= ei ? gb[ei] : v);
      if (cf == 0.0) {  // between two voiced frames: numpy.interp's slope * (x - x_lo) + y_lo, as f0_continuous_kernel
        int q = i + 1, p = i - 1;
        while (gb[q] == 0.0) ++q;  // (stops at ei at the latest)
        while (gb[p] == 0.0) --p;  // (stops at si)
        cf = (gb[q] - gb[p]) / (double)(q - p) * (double)(i - p) + gb[p];
      }
    }
    const float voiced = (ei >= 0 && v != 0.0) ? 1.f : 0.f;
    const double cvv = (log(cf) - m_org) / s_org * s_cv + m_cv;  // convert_f0, left to right like the numpy expression
    const size_t at = (size_t)s * g.max_frames + k;
    a.lcf0[at] = (float)(a.has_scaler ? (cvv - a.g_mean) / a.g_scale : cvv);
    a.uv[at] = voiced;
    if (a.raw) a.raw[at] = v;
    if (a.cv_f0) a.cv_f0[at] = exp(cvv) * (double)voiced;
    if (i == i1 - 1) {
      g.state[s].carry = cf;
      g.state[s].has_carry = 1;
    }
  }
  if (tid == 0 && a.hstatus[u]) g.state[s].flags |= FS_FLAG_EVENTS;
}

// One workgroup per stream: appends the push to the ring, advances or resets the counts, writes n_frames.
__global__ __launch_bounds__(FS_THREADS) void fs_commit_kernel(FsGeom g, const float* __restrict__ x, int ldx,
                                                               const int* __restrict__ n_valid, const int* __restrict__ end,
                                                               int C, int* __restrict__ n_frames) {
  const int tid = threadIdx.x, s = blockIdx.x;
  long long n0, b0, b1;
  int nv, e;
  fs_push_range(g, s, n_valid, end, C, n0, b0, nv, e, b1);
  __syncthreads();  // every thread holds the old counts before thread 0 replaces them
  const int keep = nv < g.ring_n ? nv : g.ring_n;
  float* ring = g.ring + (size_t)s * g.ring_n;
  const float* src = x + (size_t)s * ldx;
  for (int i = nv - keep + tid; i < nv; i += FS_THREADS) ring[(int)((n0 + i) & (g.ring_n - 1))] = src[i];
  if (tid == 0) {
    const long long n1 = n0 + nv, T = e ? fs_frames(g.grid, n1) : LLONG_MAX;
    const long long f0 = fs_min(fs_tlo(g.grid, b0 * g.grid.block), T);
    const long long f1 = b1 == b0 ? f0 : (e ? T : fs_tlo(g.grid, b1 * g.grid.block));
    n_frames[s] = (int)fs_min(f1 - f0, g.max_frames);
    g.state[s].n = e ? 0 : n1;
    g.state[s].b = e ? 0 : b1;
    if (e) g.state[s].has_carry = 0;
  }
}

struct F0Stream {
  FsGeom g;
  int S, max_samples, max_rounds;
  long long wmax;       // samples of the longest window
  long long fmax;       // its 1 ms frames
  char* block;
  size_t bytes;
  double *xwin, *f1;    // [S][wmax], [S][fmax]: a round's windows and 1 ms contours
  int* hstatus;         // [S]
  std::vector<long long> n, b;  // the host's counts
};

static size_t fs_align(size_t b) { return (b + 255) & ~(size_t)255; }

static long long fs_gcd(long long a, long long b) {
  while (b) { const long long t = a % b; a = b; b = t; }
  return a;
}

// The most frames one push of at most Cmax samples emits, over all histories and with the end flag.  An ended push emits
// T(n1) - tlo(b0 block), most from the count just below block b0's readiness, n0 = (b0 + 1) Bs + As - 1.  With
// b0 Bs = q shift_samples + r the count of the shiftms grid is largest at r = 0, b0 = 0.  On the hop grid tlo(b0 block) is
// q + (2000 r > fs) for b0 Bs = q hop + r, so the largest count has the largest residue r <= fs / 2000 that multiples of
// Bs reach modulo hop.  tests/f0_stream_ref.py finds the same by trying every history.
static long long fs_max_frames(const FsGrid& g, long long Cmax) {
  const long long K = g.As + g.Bs - 1 + Cmax;
  if (g.shift) return 1000LL * K / ((long long)g.fs * g.shift) + 1;
  const long long d = fs_gcd(g.Bs, g.hop);
  return 1 + (K + (g.fs / 2000) / d * d) / g.hop;
}

static bool fs_whole(int ms, int fs) { return ((long long)ms * fs) % 1000 == 0; }

extern "C" int crk_f0_stream_create(int fs, int back_ms, int ahead_ms, int block_ms, int shiftms, int hop_size,
                                    const double* taps, int n_taps, int n_streams, int max_samples, void** handle) {
  if (!handle || fs < 8000 || fs > 48000 || back_ms < 1 || ahead_ms < 1 || block_ms < 1 || back_ms > 10000 ||
      ahead_ms > 10000 || block_ms > 10000 || !fs_whole(back_ms, fs) || !fs_whole(ahead_ms, fs) || !fs_whole(block_ms, fs) ||
      (shiftms > 0) == (hop_size > 0) || shiftms < 0 || hop_size < 0 || shiftms > 1000 || hop_size > 65536 ||
      (hop_size > 0 && 1000LL * hop_size < fs) || n_taps < 0 || n_taps > FS_MAX_TAPS || (n_taps > 0 && !taps) ||
      n_streams < 1 || max_samples < 1)
    return CRK_ERR_ARG;
  FsGrid gr{fs, back_ms, ahead_ms, block_ms, shiftms, hop_size, (long long)block_ms * fs / 1000,
            (long long)ahead_ms * fs / 1000};
  const long long back_s = (long long)back_ms * fs / 1000;
  // every window Harvest is given holds its 64 samples: a later block's holds min(back, block) ms at the least
  if (gr.Bs < FS_MIN_SAMPLES || back_s < FS_MIN_SAMPLES) return CRK_ERR_ARG;
  const long long wmax = back_s + gr.Bs + gr.As, w_ms = (long long)back_ms + block_ms + ahead_ms;
  const long long mf = fs_max_frames(gr, max_samples);
  if (n_streams > 65535 || mf > INT_MAX || max_samples > (1 << 28)) return CRK_ERR_UNSUPPORTED;
  long long ring_n = 1;
  while (ring_n < wmax + (n_taps > 0 ? n_taps - 1 : 0) + max_samples) ring_n <<= 1;
  // output frames a window of w_ms + 1 1 ms frames holds, and one for each end
  const long long gmax = (shiftms ? (w_ms + 1) / shiftms : (w_ms + 1) * fs / (1000LL * hop_size)) + 2;

  F0Stream* h = new F0Stream();
  h->S = n_streams; h->max_samples = max_samples; h->wmax = wmax; h->fmax = w_ms + 1;
  h->max_rounds = (int)((1000LL * (gr.As + gr.Bs - 1 + max_samples) / fs) / block_ms + 1);
  h->n.assign(n_streams, 0);
  h->b.assign(n_streams, 0);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += fs_align(bytes); return at; };
  const size_t o_state = take((size_t)n_streams * sizeof(FsState)), o_ring = take((size_t)n_streams * ring_n * 4),
               o_taps = take((size_t)FS_MAX_TAPS * 8), o_gbuf = take((size_t)n_streams * gmax * 8),
               o_xwin = take((size_t)n_streams * wmax * 8), o_f1 = take((size_t)n_streams * h->fmax * 8),
               o_hst = take((size_t)n_streams * 4);
  h->bytes = o;
  if (hipMalloc(&h->block, h->bytes) != hipSuccess) { delete h; return CRK_ERR_HIP; }
  crk_count_alloc_();
  bool ok = hipMemset(h->block, 0, h->bytes) == hipSuccess;
  if (ok && n_taps > 0) ok = hipMemcpy(h->block + o_taps, taps, (size_t)n_taps * 8, hipMemcpyDefault) == hipSuccess;
  if (!ok || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(h->block);
    delete h;
    return CRK_ERR_HIP;
  }
  FsGeom& g = h->g;
  g.grid = gr;
  g.n_taps = n_taps; g.ring_n = (int)ring_n; g.max_frames = (int)mf; g.gmax = (int)gmax;
  g.state = reinterpret_cast<FsState*>(h->block + o_state);
  g.ring = reinterpret_cast<float*>(h->block + o_ring);
  g.taps = reinterpret_cast<const double*>(h->block + o_taps);
  g.gbuf = reinterpret_cast<double*>(h->block + o_gbuf);
  h->xwin = reinterpret_cast<double*>(h->block + o_xwin);
  h->f1 = reinterpret_cast<double*>(h->block + o_f1);
  h->hstatus = reinterpret_cast<int*>(h->block + o_hst);
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_f0_stream_destroy(void* st) {
  F0Stream* h = static_cast<F0Stream*>(st);
  if (!h) return;
  (void)hipFree(h->block);
  delete h;
}

extern "C" long long crk_f0_stream_state_bytes(void* st) {
  const F0Stream* h = static_cast<const F0Stream*>(st);
  return h ? (long long)h->bytes : -1;
}

extern "C" int crk_f0_stream_max_frames(void* st) {
  const F0Stream* h = static_cast<const F0Stream*>(st);
  return h ? h->g.max_frames : -1;
}

extern "C" int crk_f0_stream_max_rounds(void* st) {
  const F0Stream* h = static_cast<const F0Stream*>(st);
  return h ? h->max_rounds : -1;
}

extern "C" int crk_f0_stream_reset(void* st, const int* stream_ids, int n, void* stream) {
  F0Stream* h = static_cast<F0Stream*>(st);
  if (!h) return CRK_ERR_ARG;
  const int rc = crk_zero_stream_rows(h->g.state, sizeof(FsState), h->S, stream_ids, n, (hipStream_t)stream);
  if (rc != CRK_OK) return rc;
  // the host's copy of the counts
  if (!stream_ids) {
    h->n.assign(h->S, 0);
    h->b.assign(h->S, 0);
  }
  for (int i = 0; stream_ids && i < n; ++i) h->n[stream_ids[i]] = h->b[stream_ids[i]] = 0;
  return CRK_OK;
}

// The sizes of a push, judged before anything else.
static int fs_check_sizes(const F0Stream* h, const int* n_valid, int S, int C, int ldx) {
  if (!h || S < 1 || C < 0 || ldx < C) return CRK_ERR_ARG;
  if (S > h->S || C > h->max_samples) return CRK_ERR_UNSUPPORTED;
  if (n_valid)
    for (int s = 0; s < S; ++s)
      if (n_valid[s] < 0 || n_valid[s] > C) return CRK_ERR_ARG;
  return CRK_OK;
}

struct FsPlan {
  std::vector<std::vector<int>> ids;         // per round the ready streams, ascending
  std::vector<std::vector<long long>> lens;  // and their windows' samples
  std::vector<long long> n1, b1;             // per stream the counts after the push
};

static FsPlan fs_plan(const F0Stream* h, const int* n_valid, const int* end, int S, int C) {
  FsPlan p;
  p.n1.resize(S);
  p.b1.resize(S);
  for (int s = 0; s < S; ++s) {
    const int e = end ? (end[s] != 0) : 0;
    const long long n1 = h->n[s] + (n_valid ? n_valid[s] : C), b0 = h->b[s];
    const long long b1 = fs_max(b0, fs_blocks(h->g.grid, n1, e));
    for (long long j = b0; j < b1; ++j) {
      const size_t r = (size_t)(j - b0);
      if (p.ids.size() <= r) { p.ids.emplace_back(); p.lens.emplace_back(); }
      long long a_ms, a, L;
      fs_window(h->g.grid, j, n1, e, a_ms, a, L);
      p.ids[r].push_back(s);
      p.lens[r].push_back(L);
    }
    p.n1[s] = e ? 0 : n1;
    p.b1[s] = e ? 0 : b1;
  }
  return p;
}

extern "C" int crk_f0_stream_plan(void* st, const int* n_valid, const int* end, int S, int C, int* n_rounds, int* round_n,
                                  int* ids, long long* lens) {
  const F0Stream* h = static_cast<const F0Stream*>(st);
  const int rc = fs_check_sizes(h, n_valid, S, C, C);
  if (rc) return rc;
  if (!n_rounds || !round_n || !ids || !lens) return CRK_ERR_ARG;
  const FsPlan p = fs_plan(h, n_valid, end, S, C);
  if ((int)p.ids.size() > h->max_rounds) return CRK_ERR_UNSUPPORTED;  // (cannot happen: max_rounds is exact)
  *n_rounds = (int)p.ids.size();
  for (size_t r = 0; r < p.ids.size(); ++r) {
    round_n[r] = (int)p.ids[r].size();
    for (size_t i = 0; i < p.ids[r].size(); ++i) {
      ids[r * S + i] = p.ids[r][i];
      lens[r * S + i] = p.lens[r][i];
    }
  }
  return CRK_OK;
}

extern "C" int crk_f0_stream_push(void* st, void* f0h, const float* x, int ldx, const int* n_valid, const int* end,
                                  const int* n_valid_dev, const int* end_dev, int S, int C,
                                  const crk_f0_stream_round* rounds, int n_rounds, const int* org_spk, const int* cv_spk,
                                  const double* spk_lcf0_mean, const double* spk_lcf0_std, int n_spk, double lcf0_mean,
                                  double lcf0_scale, int has_lcf0_scaler, float* lcf0, float* uv, int* n_frames, double* raw,
                                  double* cv_f0, void* workspace, long long workspace_bytes, void* stream) {
  F0Stream* h = static_cast<F0Stream*>(st);
  int rc = fs_check_sizes(h, n_valid, S, C, ldx);
  if (rc) return rc;
  if (n_rounds < 0 || n_spk < 1 || (n_rounds > 0 && !rounds)) return CRK_ERR_ARG;
  const FsPlan p = fs_plan(h, n_valid, end, S, C);
  if ((int)p.ids.size() != n_rounds) return CRK_ERR_ARG;
  for (int r = 0; r < n_rounds; ++r) {  // the caller's tables are for this plan's windows
    long long tot = 0, frames = 0;
    for (size_t i = 0; i < p.lens[r].size(); ++i) {
      tot += p.lens[r][i];
      frames += 1000LL * p.lens[r][i] / h->g.grid.fs + 1;
    }
    const crk_f0_stream_round& t = rounds[r];
    if (t.n_ready != (int)p.ids[r].size() || t.total_samples != tot || t.total_frames != frames || !t.ids || !t.utt ||
        !t.range || !t.chan_bf || !t.chan)
      return CRK_ERR_ARG;
  }
  if ((C > 0 && !x) || !lcf0 || !uv || !n_frames || !org_spk || !cv_spk || !spk_lcf0_mean || !spk_lcf0_std ||
      (n_valid == nullptr) != (n_valid_dev == nullptr) || (end == nullptr) != (end_dev == nullptr) ||
      (n_rounds > 0 && (!f0h || !workspace)))
    return CRK_ERR_ARG;
  const FsGeom& g = h->g;
  hipStream_t q = (hipStream_t)stream;
  for (int r = 0; r < n_rounds; ++r) {
    const crk_f0_stream_round& t = rounds[r];
    long long lmax = 0;
    for (long long L : p.lens[r]) lmax = fs_max(lmax, L);
    fs_window_kernel<<<dim3((unsigned)((lmax + FS_THREADS - 1) / FS_THREADS), t.n_ready), FS_THREADS, 0, q>>>(
        g, x, ldx, n_valid_dev, end_dev, C, r, t.ids, t.utt, h->xwin);
    CRK_CHECK_LAUNCH();
    rc = crk_f0_harvest(f0h, h->xwin, t.utt, t.range, t.chan_bf, t.chan, t.n_ready, t.total_samples, t.total_channels,
                        t.total_frames, t.total_events, t.total_frames, h->f1, h->hstatus, workspace, workspace_bytes, stream);
    if (rc) return rc;
    FsFinish a{t.ids, t.utt, h->f1, h->hstatus, org_spk, cv_spk, spk_lcf0_mean, spk_lcf0_std, n_spk, has_lcf0_scaler != 0,
               lcf0_mean, lcf0_scale, lcf0, uv, raw, cv_f0};
    fs_finish_kernel<<<t.n_ready, FS_THREADS, 0, q>>>(g, n_valid_dev, end_dev, C, r, a);
    CRK_CHECK_LAUNCH();
  }
  fs_commit_kernel<<<S, FS_THREADS, 0, q>>>(g, x, ldx, n_valid_dev, end_dev, C, n_frames);
  CRK_CHECK_LAUNCH();
  for (int s = 0; s < S; ++s) { h->n[s] = p.n1[s]; h->b[s] = p.b1[s]; }
  return CRK_OK;
}

extern "C" int crk_f0_stream_status(void* st, int* flags, void* stream) {
  F0Stream* h = static_cast<F0Stream*>(st);
  if (!h || !flags) return CRK_ERR_ARG;
  std::vector<FsState> host(h->S);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
      hipMemcpy(host.data(), h->g.state, host.size() * sizeof(FsState), hipMemcpyDeviceToHost) != hipSuccess)
    return CRK_ERR_HIP;
  for (int s = 0; s < h->S; ++s) flags[s] = host[s].flags;
  return CRK_OK;
}
