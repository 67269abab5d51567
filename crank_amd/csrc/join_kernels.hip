// Device-side frame join and the live loop's back-half affine (gfx950).
//
// crk_join_*: two inputs of rows (A: width_a floats, B: width_b floats) arrive per stream at different delays - for the
// live loop the log-mel frames and the [lcf0, uv] rows of StreamingF0 - and leave as pairs: output row j of a push is
// pair first + j of the utterance, on both outputs.  Per stream the handle keeps a ring of waiting rows per side, the two
// waiting counts and `first` (join_kernels.h).  Nothing is read back and nothing is allocated by a push.
//
// A push is two launches whatever the counts are:
//   join_emit_kernel    grid (ceil(max_frames / JN_ROWS), S): READS the state, the rings and the new rows and writes the
//                       output rows below take; a workgroup whose rows lie at or past take returns at once.
//   join_commit_kernel  grid (S): one workgroup per stream derives the same plan from the same old state, stores the new
//                       rows that have to wait into the rings, and only then (behind a barrier) thread 0 replaces the
//                       state and writes n_out / first_out / n_dropped.
// The emit launch writes no state and no ring, the commit launch is the only writer of either and has one workgroup
// per stream, and the stream orders the two: no workgroup can see a state that another one has half replaced.
//
// A side's ring has cap + max_in slots for at most cap waiting rows; waiting row i sits in slot (head + i) % slots.  The
// rows read by a push sit at offsets [0, a0) from head, a0 <= cap; the rows it stores sit at offsets [a0, a0 + n),
// n <= max_in: all below cap + max_in, so a slot read in a push and a slot written in it are never the same one, and rows
// that stay waiting are not moved at all (head advances by take).
//
// Rows move as 16-byte vectors where width, strides and bases are multiples of 16 bytes (the mel rows), else float by float.
//
// crk_feat_renorm: out = ((x * scale + mean) - vmean) / vscale on the rows below a DEVICE count, four separately rounded
// fp32 operations - the bits of torch's voc.normalize(dec * scale + mean).
#include "runtime.h"
#include "join_kernels.h"

#include "../../include/crank_hip.h"
#include <limits.h>
#include <stdint.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

#define JN_THREADS 256
#define JN_ROWS 8  // output rows of both sides per workgroup of the emit launch

struct JoinGeom {
  JoinSide A, B;
  int max_frames;
  JoinState* state;  // [S]
  float *ring_a, *ring_b;  // [S][slots][width]
};

// Copies `rows` rows of `width` floats: row r from src(r) to dst(r).  VEC: as float4.
template <bool VEC, typename Src, typename Dst>
__device__ __forceinline__ void jn_move(int rows, int width, int tid, Src src, Dst dst) {
  const int units = VEC ? width >> 2 : width;
  for (int i = tid; i < rows * units; i += JN_THREADS) {
    const int r = i / units, c = i - r * units;
    if (VEC) reinterpret_cast<float4*>(dst(r))[c] = reinterpret_cast<const float4*>(src(r))[c];
    else dst(r)[c] = src(r)[c];
  }
}

// Output rows [j0, j1) of one side: waiting rows first (oldest first), then the push's new rows.
template <bool VEC>
__device__ __forceinline__ void jn_emit_side(const JoinSide& sd, const float* ring, int head, int w0, const float* in, int ld,
                                             float* out, int ldo, int j0, int j1, int tid) {
  jn_move<VEC>(j1 - j0, sd.width, tid,
               [&](int r) -> const float* {
                 const int j = j0 + r;
                 return j < w0 ? ring + (size_t)((head + j) % sd.slots) * sd.width : in + (size_t)(j - w0) * ld;
               },
               [&](int r) -> float* { return out + (size_t)(j0 + r) * ldo; });
}

__global__ __launch_bounds__(JN_THREADS) void join_emit_kernel(JoinGeom g, const float* __restrict__ a, int lda,
                                                               const int* __restrict__ n_a, const float* __restrict__ b, int ldb,
                                                               const int* __restrict__ n_b, const int* __restrict__ end,
                                                               float* __restrict__ out_a, int ldoa, float* __restrict__ out_b,
                                                               int ldob, int C_out, int vec_a, int vec_b) {
  const int s = blockIdx.y, tid = threadIdx.x;
  const JoinState st = g.state[s];
  const JoinPlan p = join_plan(st, g.A, g.B, n_a[s], n_b[s], end ? end[s] : 0);
  const int j0 = blockIdx.x * JN_ROWS;
  if (j0 >= p.take) return;  // (workgroup-uniform: nothing of this stream's pairs lies here)
  const int j1 = min(j0 + JN_ROWS, p.take);
  const float* ra = g.ring_a + (size_t)s * g.A.slots * g.A.width;
  const float* rb = g.ring_b + (size_t)s * g.B.slots * g.B.width;
  const float* ia = a + (size_t)s * g.A.max_in * lda;
  const float* ib = b + (size_t)s * g.B.max_in * ldb;
  float* oa = out_a + (size_t)s * C_out * ldoa;
  float* ob = out_b + (size_t)s * C_out * ldob;
  if (vec_a) jn_emit_side<true>(g.A, ra, st.head_a, p.a0, ia, lda, oa, ldoa, j0, j1, tid);
  else jn_emit_side<false>(g.A, ra, st.head_a, p.a0, ia, lda, oa, ldoa, j0, j1, tid);
  if (vec_b) jn_emit_side<true>(g.B, rb, st.head_b, p.b0, ib, ldb, ob, ldob, j0, j1, tid);
  else jn_emit_side<false>(g.B, rb, st.head_b, p.b0, ib, ldb, ob, ldob, j0, j1, tid);
}

// New rows [skip, skip + keep) of one side's input into its ring, behind the w0 rows that waited.
template <bool VEC>
__device__ __forceinline__ void jn_store_side(const JoinSide& sd, float* ring, int head, int w0, const float* in, int ld,
                                              int skip, int keep, int tid) {
  jn_move<VEC>(keep, sd.width, tid, [&](int r) -> const float* { return in + (size_t)(skip + r) * ld; },
               [&](int r) -> float* { return ring + (size_t)((head + w0 + skip + r) % sd.slots) * sd.width; });
}

__global__ __launch_bounds__(JN_THREADS) void join_commit_kernel(JoinGeom g, const float* __restrict__ a, int lda,
                                                                 const int* __restrict__ n_a, const float* __restrict__ b,
                                                                 int ldb, const int* __restrict__ n_b,
                                                                 const int* __restrict__ end, int* __restrict__ n_out,
                                                                 int* __restrict__ first_out, int* __restrict__ n_dropped,
                                                                 int vec_a, int vec_b) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const JoinState st = g.state[s];
  const JoinPlan p = join_plan(st, g.A, g.B, n_a[s], n_b[s], end ? end[s] : 0);
  __syncthreads();  // every thread holds the old state before thread 0 replaces it
  if (p.keep_a > 0) {
    float* ra = g.ring_a + (size_t)s * g.A.slots * g.A.width;
    const float* ia = a + (size_t)s * g.A.max_in * lda;
    if (vec_a) jn_store_side<true>(g.A, ra, st.head_a, p.a0, ia, lda, p.skip_a, p.keep_a, tid);
    else jn_store_side<false>(g.A, ra, st.head_a, p.a0, ia, lda, p.skip_a, p.keep_a, tid);
  }
  if (p.keep_b > 0) {
    float* rb = g.ring_b + (size_t)s * g.B.slots * g.B.width;
    const float* ib = b + (size_t)s * g.B.max_in * ldb;
    if (vec_b) jn_store_side<true>(g.B, rb, st.head_b, p.b0, ib, ldb, p.skip_b, p.keep_b, tid);
    else jn_store_side<false>(g.B, rb, st.head_b, p.b0, ib, ldb, p.skip_b, p.keep_b, tid);
  }
  if (tid == 0) {
    g.state[s] = join_next(st, g.A, g.B, p);
    n_out[s] = p.take;
    first_out[s] = st.first;
    n_dropped[s] = p.dropped;
  }
}

struct FrameJoin {
  JoinGeom g;
  int S;
  char* block;
  size_t bytes, state_bytes;
};

static size_t jn_align(size_t b) { return (b + 255) & ~(size_t)255; }
static bool jn_vec_ok(int width, std::initializer_list<int> strides, std::initializer_list<const void*> bases) {
  if (width & 3) return false;
  for (int ld : strides)
    if (ld & 3) return false;
  for (const void* p : bases)
    if ((uintptr_t)p & 15) return false;
  return true;
}

extern "C" int crk_join_create(int n_streams, int width_a, int width_b, int max_in_a, int max_in_b, int cap_a, int cap_b,
                               void** handle) {
  if (!handle || n_streams < 1 || width_a < 1 || width_b < 1 || max_in_a < 1 || max_in_b < 1 || cap_a < 0 || cap_b < 0)
    return CRK_ERR_ARG;
  const long long lim = 1 << 20;  // rows and floats per row: keeps every index of a stream's block inside an int
  if (n_streams > 65535 || width_a > lim || width_b > lim || max_in_a > lim || max_in_b > lim || cap_a > lim || cap_b > lim ||
      (long long)(cap_a + max_in_a) * width_a > INT_MAX || (long long)(cap_b + max_in_b) * width_b > INT_MAX)
    return CRK_ERR_UNSUPPORTED;
  FrameJoin* h = new FrameJoin();
  JoinGeom& g = h->g;
  // a side that keeps nothing needs no ring: slots = 0 and its ring is never indexed (w0 = 0, keep = 0)
  g.A = JoinSide{width_a, max_in_a, cap_a, cap_a ? cap_a + max_in_a : 0};
  g.B = JoinSide{width_b, max_in_b, cap_b, cap_b ? cap_b + max_in_b : 0};
  g.max_frames = (int)std::min<long long>(cap_a + max_in_a, cap_b + max_in_b);
  h->S = n_streams;
  h->state_bytes = (size_t)n_streams * sizeof(JoinState);
  const size_t o_a = jn_align(h->state_bytes);
  const size_t o_b = o_a + jn_align((size_t)n_streams * g.A.slots * width_a * 4);
  h->bytes = o_b + jn_align((size_t)n_streams * g.B.slots * width_b * 4);
  if (hipMalloc(&h->block, h->bytes) != hipSuccess) { delete h; return CRK_ERR_HIP; }
  crk_count_alloc_();
  if (hipMemset(h->block, 0, h->bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(h->block);
    delete h;
    return CRK_ERR_HIP;
  }
  g.state = reinterpret_cast<JoinState*>(h->block);
  g.ring_a = reinterpret_cast<float*>(h->block + o_a);
  g.ring_b = reinterpret_cast<float*>(h->block + o_b);
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_join_destroy(void* st) {
  FrameJoin* h = static_cast<FrameJoin*>(st);
  if (!h) return;
  (void)hipFree(h->block);
  delete h;
}

extern "C" long long crk_join_state_bytes(void* st) {
  const FrameJoin* h = static_cast<const FrameJoin*>(st);
  return h ? (long long)h->bytes : -1;
}

extern "C" int crk_join_max_frames(void* st) {
  const FrameJoin* h = static_cast<const FrameJoin*>(st);
  return h ? h->g.max_frames : -1;
}

extern "C" int crk_join_reset(void* st, const int* stream_ids, int n, void* stream) {
  FrameJoin* h = static_cast<FrameJoin*>(st);
  if (!h) return CRK_ERR_ARG;
  return crk_zero_stream_rows(h->g.state, sizeof(JoinState), h->S, stream_ids, n, (hipStream_t)stream);
}

extern "C" int crk_join_push(void* st, const float* a, int lda, const int* n_a, const float* b, int ldb, const int* n_b,
                             const int* end, int S, float* out_a, int ldoa, float* out_b, int ldob, int C_out, int* n_out,
                             int* first_out, int* n_dropped, void* stream) {
  FrameJoin* h = static_cast<FrameJoin*>(st);
  if (!h || !a || !n_a || !b || !n_b || !out_a || !out_b || !n_out || !first_out || !n_dropped || S < 1) return CRK_ERR_ARG;
  const JoinGeom& g = h->g;
  if (lda < g.A.width || ldb < g.B.width || ldoa < g.A.width || ldob < g.B.width || C_out < g.max_frames) return CRK_ERR_ARG;
  if (S > h->S) return CRK_ERR_UNSUPPORTED;
  if ((long long)g.A.max_in * lda > INT_MAX || (long long)g.B.max_in * ldb > INT_MAX || (long long)C_out * ldoa > INT_MAX ||
      (long long)C_out * ldob > INT_MAX)
    return CRK_ERR_UNSUPPORTED;
  hipStream_t q = (hipStream_t)stream;
  const int vec_a = jn_vec_ok(g.A.width, {lda, ldoa}, {a, out_a, g.ring_a});
  const int vec_b = jn_vec_ok(g.B.width, {ldb, ldob}, {b, out_b, g.ring_b});
  join_emit_kernel<<<dim3((g.max_frames + JN_ROWS - 1) / JN_ROWS, S), JN_THREADS, 0, q>>>(
      g, a, lda, n_a, b, ldb, n_b, end, out_a, ldoa, out_b, ldob, C_out, vec_a, vec_b);
  CRK_CHECK_LAUNCH();
  join_commit_kernel<<<S, JN_THREADS, 0, q>>>(g, a, lda, n_a, b, ldb, n_b, end, n_out, first_out, n_dropped, vec_a, vec_b);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_join_status(void* st, int* flags, void* stream) {
  FrameJoin* h = static_cast<FrameJoin*>(st);
  if (!h || !flags) return CRK_ERR_ARG;
  std::vector<JoinState> host(h->S);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
      hipMemcpy(host.data(), h->g.state, host.size() * sizeof(JoinState), hipMemcpyDeviceToHost) != hipSuccess)
    return CRK_ERR_HIP;
  for (int s = 0; s < h->S; ++s) flags[s] = host[s].overflow;
  return CRK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JN_THREADS) void feat_renorm_kernel(const float* __restrict__ x, int ldx,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ vmean,
                                                                 const float* __restrict__ vscale,
                                                                 const int* __restrict__ n_valid, int C, int width,
                                                                 float* __restrict__ out, int ldo) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const int nv = join_clamp(n_valid[s], C);
  const int i = blockIdx.x * JN_THREADS + threadIdx.x;
  if (i >= nv * width) return;  // (a workgroup past the stream's rows returns at once)
  const int j = i / width, c = i - j * width;
  const float v = x[((size_t)s * C + j) * ldx + c];
  const float d = v * scale[c];
  const float e = d + mean[c];
  const float f = e - vmean[c];
  out[((size_t)s * C + j) * ldo + c] = f / vscale[c];
}

extern "C" int crk_feat_renorm(const float* x, int ldx, const float* scale, const float* mean, const float* vmean,
                               const float* vscale, const int* n_valid, int S, int C, int width, float* out, int ldo,
                               void* stream) {
  if (!x || !scale || !mean || !vmean || !vscale || !n_valid || !out || S < 1 || C < 1 || width < 1 || ldx < width ||
      ldo < width)
    return CRK_ERR_ARG;
  if (S > 65535 || (long long)C * width > INT_MAX || (long long)C * ldx > INT_MAX || (long long)C * ldo > INT_MAX)
    return CRK_ERR_UNSUPPORTED;
  feat_renorm_kernel<<<dim3((C * width + JN_THREADS - 1) / JN_THREADS, S), JN_THREADS, 0, (hipStream_t)stream>>>(
      x, ldx, scale, mean, vmean, vscale, n_valid, C, width, out, ldo);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
