// Streaming WORLD synthesis (gfx950): F0, mel-cepstrum and coded-aperiodicity rows of many concurrent streams in, the
// samples WorldSynthesizer.synthesis_batch would write for the whole utterance out, bit for bit under any cut (DESIGN.md
// section 6p; the definition in sets is tests/wsyn_stream_ref.py).  The offline synthesis touches an utterance through
// little, and each piece is carried per stream:
//   * a queue of the frame rows still open to a pulse or to the time base (F0, sp and ap row of frame k at k % qcap);
//   * the time base's running float64 phase, the previous sample's wrapped phase and vuv, and the 64-bit counts;
//   * the utterance's first pulse (the origin of the randn offsets) and the one pending pulse - found, but not added
//     before its successor gives its noise size;
//   * a power-of-two float64 ring of the samples a pulse can still reach, addressed by absolute position.
// After a push with R rows the time base has run over every sample whose frame is at most R - 2 (its next row is there);
// a pulse at i is found when sample i + 1 has its phase and added when the next pulse is found; sample i leaves once
// i + 511 < B, B the pending pulse or else the last sample with a phase.  An end push runs the front to y_length(R) with
// the clamp and the extrapolated knot, adds the last pulse with noise size 0, emits everything and resets the stream.
//
// A push is five launches (six with rmcep) whose grids depend on the handle and S alone: ys_commit_kernel,
// [ys_energy_kernel,] ys_frame_kernel, ys_timebase_kernel (time base and plan), ys_pulse_kernel over (max_pulses, S) with
// early exit and ys_ola_kernel, one thread per ring sample.  The arithmetic is world_frame.h's, the bodies the offline
// kernels run; the ring receives the adds of world_ola_kernel in the same (pulse) order from the same 0.0.  Nothing is
// allocated, synchronised or read back, so a push can be captured in a graph.  No atomics.
#include "../../include/crank_hip.h"
#include "world.h"
#include "world_frame.h"
#include <limits.h>

#define YS_THREADS 256
#define YS_LO (W_N / 2 - 1)  // a pulse at s covers s - YS_LO .. s + YS_HI
#define YS_HI (W_N / 2)

#define YS_FLAG_RING 1     // a push needed more of the sample ring than ring_capacity: adds past it were lost
#define YS_FLAG_QUEUE 2    // the row queue overflowed: the newest rows were dropped
#define YS_FLAG_NOISE 4    // a pulse's noise offset passed the reserved randn table (the kernel's clamp applied)
#define YS_FLAG_SHORT 8    // an end push on a stream holding one row: dropped, nothing leaves
#define YS_FLAG_F0 16      // an F0 row not finite, negative or above f0_ceil: synthesised as unvoiced
#define YS_FLAG_PULSES 32  // a push found more pulses than max_pulses: the last ones were lost
#define YS_FLAG_OUT 64     // more samples were ready than max_out: the rest were lost

struct YsState {
  long long rows, row_lo;   // rows received in this utterance; the oldest row still held
  long long n, emitted;     // samples with a phase; samples that have left
  long long pend_pos, pos0; // the pending pulse; the utterance's first pulse
  double total, wr_prev, pend_shift;
  int vv_prev, pend_vuv, has_pend, has_pos0, flags, pad;
};

struct YsPlan {
  long long row0;           // the first row this push appended
  long long rows, row_lo;   // the rows held while this push's pulses run: [row_lo, rows)
  long long e0;             // the absolute position of the ring's oldest sample
  long long pos0;
  int n_new, n_list, n_add, n_emit, end, pad;
};

struct YsGeom {
  int fs, m1, bands, qcap, ring_n, ring_cap, max_pulses, max_out, max_rows_in, power_mod;
  double fp, shiftms, f0_ceil;
  YsState* state;  // [S]
  YsPlan* plan;    // [S]
  double* f0q;     // [S][qcap]
  double* spq;     // [S][qcap][W_K]
  double* apq;     // [S][qcap][W_K]
  double* e;       // [S][max_rows_in][2]
  double* ring;    // [S][ring_n]
  long long* lpos; // [S][max_pulses + 1]: the pending pulse, then the pulses this push found
  double* lshift;
  int* lvuv;
  double* resp;    // [S][max_pulses][W_N]
};

// ---------------------------------------------------------------------------------------------------------- commit
// One workgroup per stream: sanitise and append the F0 rows the queue has room for, advance the row count.
__global__ __launch_bounds__(YS_THREADS) void ys_commit_kernel(YsGeom g, const double* __restrict__ f0,
                                                               const int* __restrict__ n_rows, int R,
                                                               int* __restrict__ n_dropped) {
  const int tid = threadIdx.x, s = blockIdx.x;
  const long long rows0 = g.state[s].rows, lo = g.state[s].row_lo;
  int nr = n_rows ? n_rows[s] : R;
  nr = max(0, min(nr, R));
  const long long room = (long long)g.qcap - (rows0 - lo);
  const int keep = (int)max(0LL, min((long long)nr, room));
  __syncthreads();  // every thread holds the old counts before thread 0 replaces them
  double* queue = g.f0q + (size_t)s * g.qcap;
  int bad = 0;
  for (int r = tid; r < keep; r += YS_THREADS) {
    double v = f0[(size_t)s * R + r];
    if (!(v >= 0.0) || !(v <= g.f0_ceil)) {  // (NaN fails both)
      v = 0.0;
      bad = 1;
    }
    queue[(int)((rows0 + r) % g.qcap)] = v;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    g.plan[s].row0 = rows0;
    g.plan[s].n_new = keep;
    g.state[s].rows = rows0 + keep;
    g.state[s].flags |= (bad ? YS_FLAG_F0 : 0) | (keep < nr ? YS_FLAG_QUEUE : 0);
    n_dropped[s] = nr - keep;
  }
}

// mc2e of the appended rows of mcep (which 0) and rmcep (which 1): one wave per item
__global__ __launch_bounds__(W_THREADS) void ys_energy_kernel(YsGeom g, const double* __restrict__ mcep,
                                                              const double* __restrict__ rmcep, int R,
                                                              const double* __restrict__ at) {
  __shared__ double hs[W_THREADS / 64][W_IRLEN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, s = blockIdx.y;
  const int item = blockIdx.x * (W_THREADS / 64) + wv;
  if (item >= 2 * g.plan[s].n_new) return;
  const int r = item >> 1;
  const double* mc = ((item & 1) ? rmcep : mcep) + ((size_t)s * R + r) * g.m1;
  const double en = w_energy_row(mc, g.m1, at, hs[wv], lane);
  if (lane == 0) g.e[((size_t)s * g.max_rows_in + r) * 2 + (item & 1)] = en;
}

// sp and decoded ap of the appended rows into the queue: one thread per (row, bin)
__global__ void ys_frame_kernel(YsGeom g, const double* __restrict__ mcep, const double* __restrict__ cap, int R,
                                const double* __restrict__ wt) {
  const int s = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = idx / W_K, k = idx % W_K;
  if (r >= g.plan[s].n_new) return;
  const size_t slot = (size_t)s * g.qcap + (size_t)((g.plan[s].row0 + r) % g.qcap);
  const size_t in = (size_t)s * R + r;
  w_frame_bin(mcep + in * g.m1, cap + in * g.bands, g.m1, g.bands, g.fs, k, wt,
              g.power_mod ? g.e + ((size_t)s * g.max_rows_in + r) * 2 : nullptr, g.spq + slot * W_K + k,
              g.apq + slot * W_K + k);
}

// ---------------------------------------------------------------------------------------------------------- time base
// One workgroup per stream: world_timebase_kernel's chunks over the samples that became ready (parallel interpolation, one
// thread's serial sum from the carried total, ordered compaction into the push's pulse list behind the pending pulse),
// then thread 0 closes the plan: the pulses to add, the new pending pulse, the emit range, the flags, the carry.
__global__ __launch_bounds__(YS_THREADS) void ys_timebase_kernel(YsGeom g, const int* __restrict__ end,
                                                                 long long noise_len, int* __restrict__ n_samples,
                                                                 int* __restrict__ n_dropped) {
#pragma clang fp contract(off)
  __shared__ double ph[W_CHUNK];      // phase increment, then total phase
  __shared__ double wr[W_CHUNK + 1];  // wrapped phase; [0] = the previous sample's
  __shared__ unsigned char vv[W_CHUNK + 1];
  __shared__ int cnt[YS_THREADS];
  const int tid = threadIdx.x, s = blockIdx.x;
  const YsState st = g.state[s];
  const int e = end ? (end[s] != 0) : 0;
  const long long T = st.rows;
  YsPlan* plan = g.plan + s;
  __syncthreads();  // every thread holds the old state
  if (e && T < 2) {  // nothing to run; one row cannot be synthesised (offline refuses T < 2)
    if (tid == 0) {
      plan->rows = T; plan->row_lo = st.row_lo; plan->e0 = st.emitted; plan->pos0 = 0;
      plan->n_list = plan->n_add = plan->n_emit = 0; plan->end = 1;
      n_samples[s] = 0;
      n_dropped[s] += (int)T;
      YsState z = {};
      z.flags = st.flags | (T > 0 ? YS_FLAG_SHORT : 0);
      g.state[s] = z;
    }
    return;
  }
  const double fsd = (double)g.fs, fp = g.fp;
  const double* queue = g.f0q + (size_t)s * g.qcap;
  auto row = [&](long long j) { return queue[(int)(max(j, 0LL) % g.qcap)]; };
  // the front: every sample whose frame is at most T - 2, or at an end the utterance's y_length
  long long n1 = 0;
  if (e) {
    n1 = (long long)((double)T * g.shiftms * fsd / 1000.0);
  } else if (T >= 2) {
    n1 = max(0LL, (long long)ceil((double)(T - 1) * fp * fsd));
    while (n1 > 0 && w_frame_of(n1 - 1, T, fsd, fp) >= T - 1) --n1;
    while (w_frame_of(n1, T, fsd, fp) < T - 1) ++n1;
  }
  n1 = max(n1, st.n);
  const int cap_list = g.max_pulses + 1;
  long long* lpos = g.lpos + (size_t)s * cap_list;
  double* lshift = g.lshift + (size_t)s * cap_list;
  int* lvuv = g.lvuv + (size_t)s * cap_list;
  if (tid == 0) {
    wr[0] = st.wr_prev;
    vv[0] = (unsigned char)st.vv_prev;
    if (st.has_pend) { lpos[0] = st.pend_pos; lshift[0] = st.pend_shift; lvuv[0] = st.pend_vuv; }
  }
  double total = st.total;            // thread 0's running phase
  long long base = st.has_pend ? 1 : 0;  // list entries so far
  __syncthreads();
  for (long long c0 = st.n; c0 < n1; c0 += W_CHUNK) {
    const int n = (int)min((long long)W_CHUNK, n1 - c0);
    for (int t = tid; t < n; t += YS_THREADS) ph[t] = w_phase_increment(c0 + t, T, g.fs, fp, row, &vv[t + 1]);
    __syncthreads();
    if (tid == 0) {
      for (int t = 0; t < n; ++t) {
        total = total + ph[t];
        ph[t] = total;
      }
    }
    __syncthreads();
    for (int t = tid; t < n; t += YS_THREADS) wr[t + 1] = w_wrap(ph[t]);
    __syncthreads();
    // pulse at sample i = c0 + t - 1 when the wrapped phase jumps between i and i + 1 (no pair before sample 0)
    const int per = W_CHUNK / YS_THREADS, t0 = tid * per, t1 = min(t0 + per, n);
    const int tstart = c0 == 0 ? 1 : 0;
    int mine = 0;
    for (int t = max(t0, tstart); t < t1; ++t) mine += w_is_pulse(wr[t], wr[t + 1]);
    cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int q = 0; q < YS_THREADS; ++q) {
        const int c = cnt[q];
        cnt[q] = run;
        run += c;
      }
    }
    __syncthreads();
    long long at = base + cnt[tid];
    for (int t = max(t0, tstart); t < t1; ++t) {
      if (w_is_pulse(wr[t], wr[t + 1])) {
        if (at < cap_list) {
          lpos[at] = c0 + t - 1;
          lshift[at] = w_pulse_shift(wr[t], wr[t + 1], fsd);
          lvuv[at] = vv[t];
        }
        ++at;
      }
    }
    const int last = cnt[YS_THREADS - 1] + (tid == YS_THREADS - 1 ? mine : 0);
    __syncthreads();
    if (tid == YS_THREADS - 1) cnt[0] = last;  // the chunk's pulse count
    if (tid == 0) {
      wr[0] = wr[n];
      vv[0] = vv[n];
    }
    __syncthreads();
    base += cnt[0];
    __syncthreads();
  }
  // ---- the plan
  const int L = (int)min(base, (long long)cap_list);
  const int n_add = e ? min(L, g.max_pulses) : max(L - 1, 0);
  const long long pos0 = st.has_pos0 ? st.pos0 : (L > 0 ? lpos[0] : 0);
  int over = 0;  // a pulse whose noise reaches past the table
  for (int k = tid; k < n_add; k += YS_THREADS) {
    const long long ns = k + 1 < L ? lpos[k + 1] - lpos[k] : 0;
    if (ns > 0 && lpos[k] - pos0 + min(ns, (long long)W_N) > noise_len) over = 1;
  }
  over = __syncthreads_or(over);
  if (tid != 0) return;
  int flags = st.flags | (over ? YS_FLAG_NOISE : 0) | (base > cap_list || (e && L > g.max_pulses) ? YS_FLAG_PULSES : 0);
  const bool pend = !e && L >= 1;
  const long long B = pend ? lpos[L - 1] : n1 - 1;
  const long long E0 = st.emitted;
  long long E1 = e ? n1 : max(E0, min(n1, B - YS_LO));
  if ((e ? n1 - E0 : n1 + YS_HI - 1 - E0) > g.ring_cap) flags |= YS_FLAG_RING;
  if (E1 - E0 > g.max_out) {
    flags |= YS_FLAG_OUT;
    E1 = E0 + g.max_out;
  }
  E1 = min(E1, E0 + g.ring_n);
  const double q = (double)max(B, 0LL) / fsd / fp;
  plan->rows = T; plan->row_lo = st.row_lo; plan->e0 = E0; plan->pos0 = pos0;
  plan->n_list = L; plan->n_add = n_add; plan->n_emit = (int)(E1 - E0); plan->end = e;
  n_samples[s] = (int)(E1 - E0);
  YsState z = {};
  z.flags = flags;
  if (!e) {
    z.rows = T;
    z.row_lo = max(0LL, min(T - 2, (long long)floor(q)));
    z.n = n1; z.emitted = E1;
    z.total = total; z.wr_prev = wr[0]; z.vv_prev = vv[0];
    z.has_pos0 = st.has_pos0 || L > 0; z.pos0 = pos0;
    z.has_pend = pend;
    if (pend) { z.pend_pos = lpos[L - 1]; z.pend_shift = lshift[L - 1]; z.pend_vuv = lvuv[L - 1]; }
  }
  g.state[s] = z;
}

// ---------------------------------------------------------------------------------------------------------- pulses
__global__ __launch_bounds__(W_THREADS) void ys_pulse_kernel(YsGeom g, WPulseTables t) {
  const int k = blockIdx.x, s = blockIdx.y;
  const YsPlan p = g.plan[s];
  if (k >= p.n_add) return;
  const int cap_list = g.max_pulses + 1;
  const long long* lpos = g.lpos + (size_t)s * cap_list;
  const long long pos = lpos[k];
  const int ns = k + 1 < p.n_list ? (int)min(lpos[k + 1] - pos, (long long)INT_MAX) : 0;
  const double* spq = g.spq + (size_t)s * g.qcap * W_K;
  const double* apq = g.apq + (size_t)s * g.qcap * W_K;
  auto slot = [&](long long j) { return (size_t)(max(p.row_lo, min(j, p.rows - 1)) % g.qcap) * W_K; };
  w_pulse_response(pos, p.rows, ns, g.lshift[(size_t)s * cap_list + k], g.lvuv[(size_t)s * cap_list + k] ? 1.0 : 0.0,
                   pos - p.pos0, t, [&](long long j) { return spq + slot(j); }, [&](long long j) { return apq + slot(j); },
                   g.resp + ((size_t)s * g.max_pulses + k) * W_N);
}

// One thread per ring sample: the responses of this push's pulses that cover it, added in pulse order; the samples that
// leave go to y and their slots return to 0.0 (every slot at an end).
__global__ void ys_ola_kernel(YsGeom g, double* __restrict__ y, int clip) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (r >= g.ring_n) return;
  const YsPlan p = g.plan[s];
  const long long i = p.e0 + ((r - p.e0) & (long long)(g.ring_n - 1));
  const long long* lpos = g.lpos + (size_t)s * (g.max_pulses + 1);
  const double* resp = g.resp + (size_t)s * g.max_pulses * W_N;
  double* slot = g.ring + (size_t)s * g.ring_n + r;
  double acc = *slot;
  int lo = 0, hi = p.n_add;  // the first pulse with sample >= i - N/2
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lpos[mid] < i - YS_HI) lo = mid + 1; else hi = mid;
  }
  for (int k = lo; k < p.n_add && lpos[k] <= i + YS_LO; ++k) acc = acc + resp[(size_t)k * W_N + (i - (lpos[k] - YS_LO))];
  if (i - p.e0 < p.n_emit) {
    y[(size_t)s * g.max_out + (i - p.e0)] = clip ? fmax(-1.0, fmin(1.0, acc)) : acc;
    acc = 0.0;
  }
  *slot = p.end ? 0.0 : acc;
}

// ---------------------------------------------------------------------------------------------------------- host side
struct WsynStream {
  YsGeom g;
  World* w;
  int S;
  long long noise;  // the randn values reserved at creation
  char* block;
  size_t bytes;
};

extern "C" int crk_wsyn_stream_create(void* world, int n_streams, int max_rows_in, int row_capacity, int ring_capacity,
                                      int max_pulses, int max_out, double f0_ceil, int power_mod,
                                      long long max_utt_samples, void** handle) {
  World* w = (World*)world;
  if (!w || !handle || n_streams < 1 || max_rows_in < 1 || row_capacity < 2 || ring_capacity < W_N || max_pulses < 1 ||
      max_out < 1 || !(f0_ceil > 0.0) || !(f0_ceil <= w->fs / 4.0) || max_utt_samples < 1)
    return CRK_ERR_ARG;
  if (n_streams > 65535 || max_rows_in > 4096 || row_capacity > 65536 || ring_capacity > (1 << 24) || max_pulses > 65535 ||
      max_out > (1 << 24) || max_utt_samples > (1LL << 31) || !(w->fp * w->fs >= 2.0))
    return CRK_ERR_UNSUPPORTED;
  const int rc = crk_world_reserve(w, max_utt_samples);
  if (rc) return rc;
  long long ring_n = 1;
  while (ring_n < ring_capacity) ring_n <<= 1;
  WsynStream* h = new WsynStream();
  h->w = w; h->S = n_streams; h->noise = max_utt_samples;
  const size_t S = (size_t)n_streams, Q = (size_t)row_capacity, P = (size_t)max_pulses;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += w_align(bytes); return at; };
  const size_t o_state = take(S * sizeof(YsState)), o_ring = take(S * ring_n * 8), o_plan = take(S * sizeof(YsPlan)),
               o_f0 = take(S * Q * 8), o_sp = take(S * Q * W_K * 8), o_ap = take(S * Q * W_K * 8),
               o_e = take(S * (size_t)max_rows_in * 16), o_pos = take(S * (P + 1) * 8), o_shift = take(S * (P + 1) * 8),
               o_vuv = take(S * (P + 1) * 4), o_resp = take(S * P * W_N * 8);
  h->bytes = o;
  if (hipMalloc(&h->block, h->bytes) != hipSuccess) { delete h; return CRK_ERR_HIP; }
  crk_count_alloc_();
  if (hipMemset(h->block, 0, h->bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(h->block);
    delete h;
    return CRK_ERR_HIP;
  }
  YsGeom& g = h->g;
  g.fs = w->fs; g.m1 = w->m1; g.bands = w->bands; g.qcap = row_capacity; g.ring_n = (int)ring_n; g.ring_cap = ring_capacity;
  g.max_pulses = max_pulses; g.max_out = max_out; g.max_rows_in = max_rows_in; g.power_mod = power_mod ? 1 : 0;
  g.fp = w->fp; g.shiftms = w->shiftms; g.f0_ceil = f0_ceil;
  g.state = reinterpret_cast<YsState*>(h->block + o_state);
  g.ring = reinterpret_cast<double*>(h->block + o_ring);
  g.plan = reinterpret_cast<YsPlan*>(h->block + o_plan);
  g.f0q = reinterpret_cast<double*>(h->block + o_f0);
  g.spq = reinterpret_cast<double*>(h->block + o_sp);
  g.apq = reinterpret_cast<double*>(h->block + o_ap);
  g.e = reinterpret_cast<double*>(h->block + o_e);
  g.lpos = reinterpret_cast<long long*>(h->block + o_pos);
  g.lshift = reinterpret_cast<double*>(h->block + o_shift);
  g.lvuv = reinterpret_cast<int*>(h->block + o_vuv);
  g.resp = reinterpret_cast<double*>(h->block + o_resp);
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_wsyn_stream_destroy(void* st) {
  WsynStream* h = static_cast<WsynStream*>(st);
  if (!h) return;
  (void)hipFree(h->block);
  delete h;
}

extern "C" long long crk_wsyn_stream_state_bytes(void* st) {
  const WsynStream* h = static_cast<const WsynStream*>(st);
  return h ? (long long)h->bytes : -1;
}

extern "C" int crk_wsyn_stream_max_out(void* st) {
  const WsynStream* h = static_cast<const WsynStream*>(st);
  return h ? h->g.max_out : -1;
}

extern "C" int crk_wsyn_stream_reset(void* st, const int* stream_ids, int n, void* stream) {
  WsynStream* h = static_cast<WsynStream*>(st);
  if (!h) return CRK_ERR_ARG;
  const int rc = crk_zero_stream_rows(h->g.state, sizeof(YsState), h->S, stream_ids, n, (hipStream_t)stream);
  return rc != CRK_OK ? rc
                      : crk_zero_stream_rows(h->g.ring, (size_t)h->g.ring_n * 8, h->S, stream_ids, n, (hipStream_t)stream);
}

extern "C" int crk_wsyn_stream_push(void* st, const double* f0, const double* mcep, const double* codeap,
                                    const double* rmcep, const int* n_rows, int R, const int* end, int S, int clip,
                                    double* y, int* n_samples, int* n_dropped, void* stream) {
  WsynStream* h = static_cast<WsynStream*>(st);
  if (!h || S < 1 || R < 0) return CRK_ERR_ARG;
  if (S > h->S || R > h->g.max_rows_in) return CRK_ERR_UNSUPPORTED;
  if ((R > 0 && (!f0 || !mcep || !codeap)) || !y || !n_samples || !n_dropped) return CRK_ERR_ARG;
  if ((h->g.power_mod && R > 0 && !rmcep) || (!h->g.power_mod && rmcep)) return CRK_ERR_ARG;
  if (h->w->noise_len < h->noise) return CRK_ERR_ARG;  // (cannot happen: the table only grows)
  const YsGeom& g = h->g;
  const World* w = h->w;
  hipStream_t q = (hipStream_t)stream;
  ys_commit_kernel<<<S, YS_THREADS, 0, q>>>(g, f0, n_rows, R, n_dropped);
  CRK_CHECK_LAUNCH();
  if (g.power_mod) {
    const int waves = W_THREADS / 64;
    ys_energy_kernel<<<dim3((2 * g.max_rows_in + waves - 1) / waves, S), W_THREADS, 0, q>>>(g, mcep, rmcep, R, w->at);
    CRK_CHECK_LAUNCH();
  }
  ys_frame_kernel<<<dim3((g.max_rows_in * W_K + 255) / 256, S), 256, 0, q>>>(g, mcep, codeap, R, w->wt);
  CRK_CHECK_LAUNCH();
  ys_timebase_kernel<<<S, YS_THREADS, 0, q>>>(g, end, h->noise, n_samples, n_dropped);
  CRK_CHECK_LAUNCH();
  ys_pulse_kernel<<<dim3(g.max_pulses, S), W_THREADS, 0, q>>>(
      g, WPulseTables{w->noise, h->noise, w->twc, w->tws, w->dcw, w->fs, w->fp});
  CRK_CHECK_LAUNCH();
  ys_ola_kernel<<<dim3((g.ring_n + 255) / 256, S), 256, 0, q>>>(g, y, clip);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_wsyn_stream_status(void* st, int* flags, void* stream) {
  WsynStream* h = static_cast<WsynStream*>(st);
  if (!h || !flags) return CRK_ERR_ARG;
  std::vector<YsState> host(h->S);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
      hipMemcpy(host.data(), h->g.state, host.size() * sizeof(YsState), hipMemcpyDeviceToHost) != hipSuccess)
    return CRK_ERR_HIP;
  for (int s = 0; s < h->S; ++s) flags[s] = host[s].flags;
  return CRK_OK;
}
