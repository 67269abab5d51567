// Streaming CheapTrick and mel-cepstrum analysis (gfx950): samples and F0 rows of many concurrent streams in, the frames
// WorldAnalyzer.mcep_batch would write for the whole utterance out, bit for bit (the definition in
// sets is tests/wana_stream_ref.py).  CheapTrick touches an utterance through four things only - the samples within 511
// of the frame's origin, the frame's F0, its index and its offset into the randn stream - and each is carried per stream:
//   * the analysed signal y (the low cut of the stream by wana_lowcut_kernel's fma chain, or (double)x) in a power-of-two
//     float64 ring addressed by absolute position, each sample filtered once by the push that brings it; the last raw
//     samples the filter reaches back to beside it;
//   * a queue of the F0 rows that have arrived and whose frames have not left (row k of an utterance is frame k);
//   * 64-bit counts (samples, rows, frames that left) and the draw offset of the next frame.
// Frame i leaves in the first push after which its row has arrived and n >= origin_i + 512 (an F0-independent bound: the
// clamp of `half` plus one), or in the push that carries the end flag, where windows clamp at the final length as the
// offline kernel clamps to xlen - 1 and the stream returns to its start state.
//
// A push is four launches whose grids depend on the handle alone: ws_commit_kernel (filter and append the samples, append
// the rows, advance the counts), ws_plan_kernel (per stream the frames that leave, their draw offsets from the carry, the
// flags and the new carry), ws_cheaptrick_kernel over (max_frames, S) with early exit and ws_mcep_kernel.  The frame
// arithmetic is wana_frame.h's, the bodies the offline kernels run.  Nothing is allocated, synchronised or read back, so
// a push can be captured in a graph.  No atomics: a frame depends on its stream only through the carried counts.
#include "../../include/crank_hip.h"
#include "wana_stream.h"
#include <limits.h>

// ---------------------------------------------------------------------------------------------------------- commit
// One workgroup per stream.
__global__ __launch_bounds__(WS_THREADS) void ws_commit_kernel(WsGeom g, const float* __restrict__ x, int ldx,
                                                               const int* __restrict__ n_valid, int C,
                                                               const double* __restrict__ f0, int ldf,
                                                               const int* __restrict__ n_f0, int R,
                                                               int* __restrict__ n_dropped) {
  __shared__ double h[WA_MAX_TAPS];
  const int tid = threadIdx.x, s = blockIdx.x;
  for (int k = tid; k < g.n_taps; k += WS_THREADS) h[k] = g.taps[k];
  const long long n0 = g.state[s].n, rows0 = g.state[s].rows, em = g.state[s].emitted;
  int nv = n_valid ? n_valid[s] : C, nf = n_f0 ? n_f0[s] : R;
  nv = max(0, min(nv, C));
  nf = max(0, min(nf, R));
  __syncthreads();  // the taps are staged; every thread holds the old counts before thread 0 replaces them
  double* ring = g.ring + (size_t)s * g.ring_n;
  float* hist = g.hist + (size_t)s * WS_HIST;
  const float* src = x + (size_t)s * ldx;
  const int mask = g.ring_n - 1;
  auto sample = [&](long long q) -> float { return q < n0 ? hist[(int)(q & (WS_HIST - 1))] : src[q - n0]; };
  for (int i = tid; i < nv; i += WS_THREADS) {
    const long long p = n0 + i;
    ring[(int)(p & mask)] = g.n_taps ? wa_lowcut_sample(h, g.n_taps, p, sample) : (double)src[i];
  }
  __syncthreads();  // the filter has read the old history
  for (int i = max(0, nv - WS_HIST) + tid; i < nv; i += WS_THREADS) hist[(int)((n0 + i) & (WS_HIST - 1))] = src[i];
  // the rows: what the queue has room for
  const long long room = (long long)g.qcap - (rows0 - em);
  const int keep = (int)max(0LL, min((long long)nf, room));
  double* queue = g.queue + (size_t)s * g.qcap;
  const double top = (double)g.fs / 4.0;
  int bad = 0;
  for (int r = tid; r < keep; r += WS_THREADS) {
    double v = f0[(size_t)s * ldf + r];
    if (!(v >= 0.0) || !(v <= top)) {  // (NaN fails both)
      v = 0.0;
      bad = 1;
    }
    queue[(int)((rows0 + r) % g.qcap)] = v;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    g.state[s].n = n0 + nv;
    g.state[s].rows = rows0 + keep;
    g.state[s].flags |= (bad ? WS_FLAG_F0 : 0) | (keep < nf ? WS_FLAG_QUEUE : 0);
    n_dropped[s] = nf - keep;
  }
}

// ---------------------------------------------------------------------------------------------------------- plan
// One workgroup per stream: the waiting frames that leave in this push, in order, with their draw offsets.
__global__ __launch_bounds__(WS_THREADS) void ws_plan_kernel(WsGeom g, const int* __restrict__ end, long long noise_len,
                                                             int* __restrict__ n_frames, int* __restrict__ first_out,
                                                             int* __restrict__ n_dropped) {
#pragma clang fp contract(off)
  __shared__ double s_f0[WS_THREADS];
  __shared__ long long s_start[WS_THREADS];
  __shared__ int s_cnt[WS_THREADS];  // the frame's draws; 0: the frame stays (and every later one)
  __shared__ long long carry[2];     // the running draw offset, the frames that left
  __shared__ int tally[4];           // slots written, frames dropped, flags, stop
  const int tid = threadIdx.x, s = blockIdx.x;
  const long long n = g.state[s].n, rows = g.state[s].rows, em = g.state[s].emitted;
  const int e = end ? (end[s] != 0) : 0;
  const double* queue = g.queue + (size_t)s * g.qcap;
  WsSlot* slots = g.slots + (size_t)s * g.qcap;
  if (tid == 0) {
    carry[0] = g.state[s].doff;
    carry[1] = 0;
    tally[0] = tally[1] = tally[2] = tally[3] = 0;
  }
  __syncthreads();
  for (long long c0 = em; c0 < rows; c0 += WS_THREADS) {
    const long long k = c0 + tid;
    int cnt = 0;
    if (k < rows) {
      const double f = queue[(int)(k % g.qcap)];
      const WaShape sh = wa_shape(f, k, g.fs, g.shiftms);
      const bool leaves = e ? (n > 0 && !((double)k * g.shift > (double)n + g.shift)) : (n >= (long long)sh.origin + WS_REACH + 1);
      if (leaves) cnt = 2 * sh.half + 1 + W_K;
      s_f0[tid] = f;
      s_start[tid] = max(0LL, (long long)sh.origin - sh.half);
    }
    s_cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
      long long run = carry[0], left = carry[1];
      int j = tally[0], dropped = tally[1], flags = tally[2], stop = 0;
      const int m = (int)min((long long)WS_THREADS, rows - c0);
      for (int q = 0; q < m; ++q) {
        if (s_cnt[q] == 0) { stop = 1; break; }
        if (run + s_cnt[q] > noise_len) flags |= WS_FLAG_DRAWS;
        if (s_start[q] < n - g.ring_cap) {
          flags |= WS_FLAG_RING;
          ++dropped;
        } else if (j < g.qcap) {  // (always: no more frames wait than the queue holds)
          slots[j].f0 = s_f0[q];
          slots[j].index = c0 + q;
          slots[j].doff = run;
          ++j;
        }
        run += s_cnt[q];
        ++left;
      }
      carry[0] = run; carry[1] = left;
      tally[0] = j; tally[1] = dropped; tally[2] = flags; tally[3] = stop;
    }
    __syncthreads();
    if (tally[3]) break;
  }
  if (tid == 0) {
    int dropped = tally[1], flags = tally[2];
    const long long past = rows - em - carry[1];  // rows whose frames did not leave
    if (e && past > 0) {
      flags |= WS_FLAG_PAST_END;
      dropped += (int)min(past, (long long)INT_MAX / 2);
    }
    g.plan[s].n_len = n;
    g.plan[s].n_emit = tally[0];
    n_frames[s] = tally[0];
    first_out[s] = g.first;
    n_dropped[s] += dropped;
    g.state[s].flags |= flags;
    g.state[s].n = e ? 0 : n;
    g.state[s].rows = e ? 0 : rows;
    g.state[s].emitted = e ? 0 : em + carry[1];
    g.state[s].doff = e ? 0 : carry[0];
  }
}

// ---------------------------------------------------------------------------------------------------------- frames
__global__ __launch_bounds__(W_THREADS) void ws_cheaptrick_kernel(WsGeom g, WaTables t, double* __restrict__ sp) {
  const int j = blockIdx.x, s = blockIdx.y;
  if (j >= g.plan[s].n_emit) return;
  const size_t row = (size_t)s * g.qcap + j;
  const WsSlot slot = g.slots[row];
  const double* ring = g.ring + (size_t)s * g.ring_n;
  const int mask = g.ring_n - 1;
  const WaShape sh = wa_shape(slot.f0, slot.index, g.fs, g.shiftms);
  wa_cheaptrick_frame([&](long long idx) { return ring[(int)(idx & mask)]; }, g.plan[s].n_len, sh, slot.doff, t,
                      sp ? sp + row * W_K : nullptr, g.cep + row * W_K);
}

// One wave per frame: mcep, and the rows a generator takes - column m >= first as (mcep - mean) / scale where a scaler is
// given, float64, rounded once.
__global__ __launch_bounds__(W_THREADS) void ws_mcep_kernel(WsGeom g, const double* __restrict__ at,
                                                            const double* __restrict__ mean,
                                                            const double* __restrict__ scale, double* __restrict__ mc,
                                                            float* __restrict__ feats) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * (W_THREADS / 64) + wv, s = blockIdx.y;
  if (j >= g.plan[s].n_emit) return;
  const size_t row = (size_t)s * g.qcap + j;
  const int m1 = g.m1, first = g.first, width = m1 - first;
  wa_mcep_frame(g.cep + row * W_K, at, m1, lane, [&](int m, double v) {
    mc[row * m1 + m] = v;
    if (m >= first) feats[row * width + (m - first)] = (float)(mean ? (v - mean[m]) / scale[m] : v);
  });
}

// ---------------------------------------------------------------------------------------------------------- host side
struct WanaStream {
  WsGeom g;
  Wana* w;
  int S, max_samples, max_f0_in;
  long long draws;  // the randn values reserved at creation
  char* block;
  size_t bytes;
};

extern "C" int crk_wana_stream_create(void* wana, const double* taps, int n_taps, int n_streams, int max_samples,
                                      int max_f0_in, int f0_capacity, int ring_capacity, int max_utt_frames,
                                      int use_mcep_0th, void** handle) {
  Wana* w = (Wana*)wana;
  if (!w || !handle || n_taps < 0 || n_taps > WS_HIST - 1 || (n_taps > 0 && !taps) || n_streams < 1 || max_samples < 1 ||
      max_f0_in < 1 || f0_capacity < 1 || ring_capacity < max_samples || max_utt_frames < 1)
    return CRK_ERR_ARG;
  if (n_streams > 65535 || f0_capacity > WS_MAX_QUEUE || max_f0_in > WS_MAX_QUEUE || ring_capacity > (1 << 26) ||
      (long long)max_utt_frames * WA_MAX_DRAWS > (1LL << 31) || (use_mcep_0th == 0 && w->m1 < 2))
    return CRK_ERR_UNSUPPORTED;
  const long long draws = (long long)max_utt_frames * WA_MAX_DRAWS;
  const int rc = crk_wana_reserve(w, draws);
  if (rc) return rc;
  long long ring_n = 1;
  while (ring_n < ring_capacity) ring_n <<= 1;
  WanaStream* h = new WanaStream();
  h->w = w; h->S = n_streams; h->max_samples = max_samples; h->max_f0_in = max_f0_in; h->draws = draws;
  const size_t S = (size_t)n_streams, Q = (size_t)f0_capacity;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += w_align(bytes); return at; };
  const size_t o_state = take(S * sizeof(WsState)), o_ring = take(S * ring_n * 8), o_hist = take(S * WS_HIST * 4),
               o_queue = take(S * Q * 8), o_taps = take((size_t)WA_MAX_TAPS * 8), o_plan = take(S * sizeof(WsPlan)),
               o_slots = take(S * Q * sizeof(WsSlot)), o_cep = take(S * Q * W_K * 8);
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
  WsGeom& g = h->g;
  g.fs = w->fs; g.n_taps = n_taps; g.ring_n = (int)ring_n; g.ring_cap = ring_capacity; g.qcap = f0_capacity;
  g.m1 = w->m1; g.first = use_mcep_0th ? 0 : 1;
  g.shiftms = w->shiftms;
  g.shift = w->shiftms / 1000.0 * w->fs;
  g.state = reinterpret_cast<WsState*>(h->block + o_state);
  g.ring = reinterpret_cast<double*>(h->block + o_ring);
  g.hist = reinterpret_cast<float*>(h->block + o_hist);
  g.queue = reinterpret_cast<double*>(h->block + o_queue);
  g.taps = reinterpret_cast<const double*>(h->block + o_taps);
  g.plan = reinterpret_cast<WsPlan*>(h->block + o_plan);
  g.slots = reinterpret_cast<WsSlot*>(h->block + o_slots);
  g.cep = reinterpret_cast<double*>(h->block + o_cep);
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_wana_stream_destroy(void* st) {
  WanaStream* h = static_cast<WanaStream*>(st);
  if (!h) return;
  (void)hipFree(h->block);
  delete h;
}

extern "C" long long crk_wana_stream_state_bytes(void* st) {
  const WanaStream* h = static_cast<const WanaStream*>(st);
  return h ? (long long)h->bytes : -1;
}

extern "C" int crk_wana_stream_max_frames(void* st) {
  const WanaStream* h = static_cast<const WanaStream*>(st);
  return h ? h->g.qcap : -1;
}

extern "C" int crk_wana_stream_reset(void* st, const int* stream_ids, int n, void* stream) {
  WanaStream* h = static_cast<WanaStream*>(st);
  if (!h) return CRK_ERR_ARG;
  return crk_zero_stream_rows(h->g.state, sizeof(WsState), h->S, stream_ids, n, (hipStream_t)stream);
}

extern "C" int crk_wana_stream_push(void* st, const float* x, int ldx, const int* n_valid, int C, const double* f0, int ldf,
                                    const int* n_f0, int R, const int* end, int S, const double* mean, const double* scale,
                                    double* mcep, double* sp, float* feats, int* n_frames, int* first, int* n_dropped,
                                    void* stream) {
  WanaStream* h = static_cast<WanaStream*>(st);
  if (!h || S < 1 || C < 0 || R < 0 || ldx < C || ldf < R) return CRK_ERR_ARG;
  if (S > h->S || C > h->max_samples || R > h->max_f0_in) return CRK_ERR_UNSUPPORTED;
  if ((C > 0 && !x) || (R > 0 && !f0) || (mean == nullptr) != (scale == nullptr) || !mcep || !feats || !n_frames ||
      !first || !n_dropped)
    return CRK_ERR_ARG;
  if (h->w->noise_len < h->draws) return CRK_ERR_ARG;  // (cannot happen: the table only grows)
  const WsGeom& g = h->g;
  hipStream_t q = (hipStream_t)stream;
  ws_commit_kernel<<<S, WS_THREADS, 0, q>>>(g, x, ldx, n_valid, C, f0, ldf, n_f0, R, n_dropped);
  CRK_CHECK_LAUNCH();
  ws_plan_kernel<<<S, WS_THREADS, 0, q>>>(g, end, h->draws, n_frames, first, n_dropped);
  CRK_CHECK_LAUNCH();
  const WaTables t{h->w->noise, h->draws, h->w->twc, h->w->tws, g.fs};
  ws_cheaptrick_kernel<<<dim3(g.qcap, S), W_THREADS, 0, q>>>(g, t, sp);
  CRK_CHECK_LAUNCH();
  ws_mcep_kernel<<<dim3((g.qcap + W_THREADS / 64 - 1) / (W_THREADS / 64), S), W_THREADS, 0, q>>>(g, h->w->at, mean, scale,
                                                                                              mcep, feats);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_wana_stream_status(void* st, int* flags, void* stream) {
  WanaStream* h = static_cast<WanaStream*>(st);
  if (!h || !flags) return CRK_ERR_ARG;
  std::vector<WsState> host(h->S);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
      hipMemcpy(host.data(), h->g.state, host.size() * sizeof(WsState), hipMemcpyDeviceToHost) != hipSuccess)
    return CRK_ERR_HIP;
  for (int s = 0; s < h->S; ++s) flags[s] = host[s].flags;
  return CRK_OK;
}
