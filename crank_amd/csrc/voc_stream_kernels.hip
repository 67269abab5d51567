// Streaming Parallel WaveGAN vocoding (gfx950): the generator of vocoder_kernels.hip for chunks of new frames of many
// concurrent streams, every layer's history kept on the device.
//
// The published generator is not causal, so a stream runs at a fixed look-ahead LA = win + ceil((D + A) / H) frames
// (D: sum of the layers' dilations, A: forward reach of the upsampling network in samples, H: hop).  Every stage of the
// generator - conv_in, each upsampling stage, each residual layer - owns a FRONTIER: the position up to which its output
// exists.  A frontier is a function of the frames T the stream has received in its utterance and of whether the
// utterance has ended, so the only carried position is T; a push moves every frontier from its value at T0 to its value
// at T1 = T0 + n_valid (at the utterance's end: to the end), and a stage computes exactly the positions in between:
//   conv_in        frames  [max(0, T - win)]                  (T at the end)
//   stage i        samples [max(0, (P_i - 1) s_i)]            P_i: frontier of its input  (T r_{i+1} at the end)
//   layer l        samples [max(0, Pc - (d_0 + .. + d_l))]    Pc: frontier of the conditioning  (T H at the end)
//   last layer     samples [max(0, T - LA) H]                 what the push emits
// Operands live in per-stream rings indexed by (position mod capacity); what is inside the utterance is decided by
// position - [0, E) with E unknown (no right edge in reach) until the end flag - never by a carried zero, so a reset is
// T = 0 and nothing else.  The arithmetic is the offline kernels' own (voc_common.h), one launch per stage over all
// streams: 2 + 1 + n_scales + layers launches per push whatever S, C, n_valid and end are; grids cover the worst case
// and a workgroup past its stream's range exits before it touches LDS.
#include "runtime.h"
#include "voc_common.h"
#include "../../include/crank_hip.h"
#include <limits.h>
#include <math.h>
#include <vector>


#define VS_MAX_SAMPLES 0x3fffffff  // an utterance's samples: positions and position + dilation stay inside int

// geometry and ring layout, by value in every kernel's arguments; offsets in bytes from a stream's state
struct VsGeom {
  int scales[VOC_MAX_SCALES];
  int n_scales, win, hop, la, aux, auxp;
  int cap_c, cap_u[VOC_MAX_SCALES], cap_cond, cap_noise, cap_skip;
  size_t per_stream, o_c, o_u[VOC_MAX_SCALES], o_chi, o_clo, o_noise, o_skip;
};
struct VsPlan { int t0, t1, end, pad; };  // a stream's push: frames before / after it, end flag

// ---- frontiers ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int vs_frames(const VsGeom& g, int T, bool e) { return e ? T : max(0, T - g.win); }
// frontier of stage i's input at its own rate (i = 0: conv_in's output, i = n_scales: the conditioning)
__device__ __forceinline__ int vs_stage(const VsGeom& g, int T, bool e, int i) {
  int p = vs_frames(g, T, e), rate = 1;
  for (int j = 0; j < i; ++j) {
    rate *= g.scales[j];
    p = e ? T * rate : max(0, (p - 1) * g.scales[j]);
  }
  return p;
}
// frontier of the residual stream sd dilations behind the conditioning
__device__ __forceinline__ int vs_x(const VsGeom& g, int T, bool e, int sd) {
  return e ? T * g.hop : max(0, vs_stage(g, T, e, g.n_scales) - sd);
}
__device__ __forceinline__ int vs_emit(const VsGeom& g, int T, bool e) { return e ? T * g.hop : max(0, T - g.la) * g.hop; }

__device__ __forceinline__ size_t vs_mod(long long pos, int cap) { return (size_t)((unsigned long long)pos % (unsigned)cap); }

// ---- kernels --------------------------------------------------------------------------------------------------------
__global__ void vs_begin_kernel(VsGeom g, int S, int C, const int* __restrict__ n_valid, const int* __restrict__ end,
                                int* __restrict__ t_in, VsPlan* __restrict__ plan, int* __restrict__ n_out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int t0 = t_in[s];
  int nv = n_valid ? min(max(n_valid[s], 0), C) : C;
  nv = min(nv, max(VS_MAX_SAMPLES / g.hop - t0, 0));
  const bool e = end && end[s] != 0;
  const int t1 = t0 + nv;
  plan[s] = VsPlan{t0, t1, e ? 1 : 0, 0};
  n_out[s] = vs_emit(g, t1, e) - vs_emit(g, t0, false);
  t_in[s] = e ? 0 : t1;
}

// the push's valid frames and noise into their rings
__global__ void vs_stage_in_kernel(VsGeom g, int C, const float* __restrict__ c, const float* __restrict__ noise,
                                   const VsPlan* __restrict__ plan, unsigned char* __restrict__ state) {
  const int s = blockIdx.y;
  const VsPlan p = plan[s];
  const int nv = p.t1 - p.t0, nn = C * g.hop, nc = C * g.aux;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned char* base = state + (size_t)s * g.per_stream;
  if (idx < nn) {
    if (idx < nv * g.hop)
      reinterpret_cast<float*>(base + g.o_noise)[vs_mod((long long)p.t0 * g.hop + idx, g.cap_noise)] = noise[(size_t)s * nn + idx];
  } else if (idx < nn + nc) {
    const int j = idx - nn, f = j / g.aux, a = j % g.aux;
    if (f < nv)
      reinterpret_cast<float*>(base + g.o_c)[vs_mod(p.t0 + f, g.cap_c) * g.aux + a] = c[((size_t)s * C + f) * g.aux + a];
  }
}

__global__ void vs_conv_in_kernel(VsGeom g, const float* __restrict__ w, const VsPlan* __restrict__ plan,
                                  unsigned char* __restrict__ state) {
  const int s = blockIdx.y;
  const VsPlan p = plan[s];
  const int lo = vs_frames(g, p.t0, false), hi = vs_frames(g, p.t1, p.end);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int f = lo + idx / g.aux, o = idx % g.aux;
  if (f >= hi) return;
  unsigned char* base = state + (size_t)s * g.per_stream;
  const float* cring = reinterpret_cast<const float*>(base + g.o_c);
  float* out = reinterpret_cast<float*>(base + g.o_u[0]);
  const int e = p.end ? p.t1 : INT_MAX;  // no right edge in reach before the end flag
  out[vs_mod(f, g.cap_u[0]) * g.aux + o] =
      voc_conv_in_value([&](int fr) { return cring + vs_mod(fr, g.cap_c) * g.aux; }, w, f, o, 0, e, g.aux, g.win);
}

// upsampling stage i; the last one writes the conditioning's bf16 hi and lo rings [cap][auxp] (zeros in the padding channels)
__global__ void vs_upsample_kernel(VsGeom g, int i, const float* __restrict__ w, const VsPlan* __restrict__ plan,
                                   unsigned char* __restrict__ state) {
  const int s = blockIdx.y;
  const VsPlan p = plan[s];
  const bool last = i + 1 == g.n_scales;
  const int ld = last ? g.auxp : g.aux;
  const int lo = vs_stage(g, p.t0, false, i + 1), hi = vs_stage(g, p.t1, p.end, i + 1);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = lo + idx / ld, ch = idx % ld;
  if (t >= hi) return;
  unsigned char* base = state + (size_t)s * g.per_stream;
  uint16_t* chi = reinterpret_cast<uint16_t*>(base + g.o_chi);
  uint16_t* clo = reinterpret_cast<uint16_t*>(base + g.o_clo);
  const size_t cpos = vs_mod(t, g.cap_cond) * g.auxp + ch;
  if (ch >= g.aux) {
    chi[cpos] = 0;
    clo[cpos] = 0;
    return;
  }
  long long rate_out = 1;
  for (int j = 0; j <= i; ++j) rate_out *= g.scales[j];
  const long long E = p.end ? p.t1 * rate_out : LLONG_MAX;
  const float* in = reinterpret_cast<const float*>(base + g.o_u[i]);
  const int cap_in = g.cap_u[i], aux = g.aux;
  const float acc = voc_upsample_value([&](long long j) { return in[vs_mod(j, cap_in) * aux + ch]; }, w, g.scales[i], t, 0, E);
  if (last)
    voc_cond_store(acc, chi + cpos, clo + cpos);
  else
    reinterpret_cast<float*>(base + g.o_u[i + 1])[vs_mod(t, g.cap_u[i + 1]) * aux + ch] = acc;
}

struct VsLayerArgs {
  VocLayerW w;
  VsGeom g;
  const VsPlan* plan;
  unsigned char* state;
  float* wave;
  size_t o_xin, o_xout;
  int cap_xin, cap_xout, sd_out, dil, wave_ld;
};

// where a stream's samples live: rings by position mod capacity; the utterance is [0, ue)
struct VsRingLoc {
  const float* noise_; const float* xin_; float* xout_; float* skip_; const uint16_t* chi_; const uint16_t* clo_; float* y_;
  int cap_noise, cap_xin, cap_xout, cap_skip, cap_cond, auxp, y0, ue;
  __device__ __forceinline__ bool inside(int m) const { return m >= 0 && m < ue; }
  __device__ __forceinline__ float noise(int m) const { return noise_[vs_mod(m, cap_noise)]; }
  __device__ __forceinline__ const float* xin(int m) const { return xin_ + vs_mod(m, cap_xin) * VOC_RES; }
  __device__ __forceinline__ float* xout(int n) const { return xout_ + vs_mod(n, cap_xout) * VOC_RES; }
  __device__ __forceinline__ float* skip(int n) const { return skip_ + vs_mod(n, cap_skip) * VOC_RES; }
  __device__ __forceinline__ const uint16_t* chi(int n) const { return chi_ + vs_mod(n, cap_cond) * auxp; }
  __device__ __forceinline__ const uint16_t* clo(int n) const { return clo_ + vs_mod(n, cap_cond) * auxp; }
  __device__ __forceinline__ float* y(int n) const { return y_ + (n - y0); }
};

// grid (worst-case tiles of a stream / VOC_WAVES, streams): a wave's tile is 32 samples from the layer's old frontier
template <bool P, bool FIRST, bool LAST>
__global__ __launch_bounds__(64 * VOC_WAVES) void vs_layer_kernel(VsLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vs_lds[];
  const int s = blockIdx.y;
  const VsPlan p = a.plan[s];
  const int lo = LAST ? vs_emit(a.g, p.t0, false) : vs_x(a.g, p.t0, false, a.sd_out);
  const int hi = LAST ? vs_emit(a.g, p.t1, p.end) : vs_x(a.g, p.t1, p.end, a.sd_out);
  const int first = lo + blockIdx.x * (32 * VOC_WAVES);
  if (first >= hi) return;  // the whole workgroup: nothing of this stream here
  voc_layer_fill_lds(a.w, vs_lds);
  __syncthreads();
  const int lane = threadIdx.x & 63, r = lane & 31, wave = threadIdx.x >> 6;
  const int n0 = first + wave * 32;
  if (n0 >= hi) return;
  const int n = n0 + r;
  unsigned char* base = a.state + (size_t)s * a.g.per_stream;
  VsRingLoc loc;
  loc.noise_ = reinterpret_cast<const float*>(base + a.g.o_noise);
  loc.xin_ = reinterpret_cast<const float*>(base + a.o_xin);
  loc.xout_ = reinterpret_cast<float*>(base + a.o_xout);
  loc.skip_ = reinterpret_cast<float*>(base + a.g.o_skip);
  loc.chi_ = reinterpret_cast<const uint16_t*>(base + a.g.o_chi);
  loc.clo_ = reinterpret_cast<const uint16_t*>(base + a.g.o_clo);
  loc.y_ = a.wave + (size_t)s * a.wave_ld;
  loc.cap_noise = a.g.cap_noise; loc.cap_xin = a.cap_xin; loc.cap_xout = a.cap_xout; loc.cap_skip = a.g.cap_skip;
  loc.cap_cond = a.g.cap_cond; loc.auxp = a.g.auxp; loc.y0 = lo;
  loc.ue = p.end ? p.t1 * a.g.hop : INT_MAX;  // no right edge in reach before the end flag
  {
    const VocLayerW& aw = a.w; const bool valid = n < hi; const int dil = a.dil; const unsigned char* lds = vs_lds;
#include "voc_layer_tile.inc"
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct VocStream {
  const Voc* v;
  int S, C;
  VsGeom g;
  unsigned char* block;  // the one device allocation: [t_in S][plan S][state S x per_stream]
  size_t bytes;
  int* t_in;
  VsPlan* plan;
  unsigned char* state;
  std::vector<size_t> o_x;   // ring of layer l's input, l = 1 .. layers - 1
  std::vector<int> cap_x, sd;  // sd[l] = d_0 + .. + d_{l-1}
  long long up_rate[VOC_MAX_SCALES], up_a[VOC_MAX_SCALES];  // stage i's output rate and what it and the stages before it hold back
};

template <bool P, bool FIRST, bool LAST>
static void* vs_layer_fn() { return (void*)vs_layer_kernel<P, FIRST, LAST>; }
static void* vs_pick(bool p, bool first, bool last) {
  if (p) {
    if (first) return last ? vs_layer_fn<true, true, true>() : vs_layer_fn<true, true, false>();
    return last ? vs_layer_fn<true, false, true>() : vs_layer_fn<true, false, false>();
  }
  if (first) return last ? vs_layer_fn<false, true, true>() : vs_layer_fn<false, true, false>();
  return last ? vs_layer_fn<false, false, true>() : vs_layer_fn<false, false, false>();
}

static size_t vs_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the look-ahead and every ring of one stream; false where a capacity leaves int
static bool vs_layout(const Voc* v, int C, VocStream* h) {
  VsGeom& g = h->g;
  const long long H = v->hop, win = v->win;
  g.n_scales = v->n_scales; g.win = v->win; g.hop = v->hop; g.aux = v->aux; g.auxp = v->auxp;
  for (int i = 0; i < VOC_MAX_SCALES; ++i) g.scales[i] = i < v->n_scales ? v->scales[i] : 1;
  const int lps = v->layers / v->stacks;
  h->sd.assign(v->layers + 1, 0);
  long long D = 0;
  for (int l = 0; l < v->layers; ++l) {
    h->sd[l] = (int)D;
    D += 1LL << (l % lps);
    if (D > VS_MAX_SAMPLES) return false;
  }
  h->sd[v->layers] = (int)D;
  // a[i]: what the stages in front of stage i hold back, in samples of stage i's input rate; A = a[n_scales]
  long long a[VOC_MAX_SCALES + 1], rate[VOC_MAX_SCALES + 1];
  a[0] = 0; rate[0] = 1;
  for (int i = 0; i < v->n_scales; ++i) {
    rate[i + 1] = rate[i] * v->scales[i];
    a[i + 1] = (a[i] + 1) * v->scales[i];
  }
  const long long A = a[v->n_scales];
  const long long la = win + (D + A + H - 1) / H;
  if ((C + la + 1) * H + D > VS_MAX_SAMPLES) return false;
  g.la = (int)la;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += vs_align(bytes); return at; };
  // live spans: [oldest position a reader of this push touches, newest position its writer reaches)
  g.cap_c = (int)(C + 2 * win);
  g.o_c = take((size_t)g.cap_c * v->aux * 4);
  for (int i = 0; i < v->n_scales; ++i) {
    g.cap_u[i] = (int)((C + win) * rate[i] + a[i] + 2);
    g.o_u[i] = take((size_t)g.cap_u[i] * v->aux * 4);
    h->up_rate[i] = rate[i + 1];
    h->up_a[i] = a[i + 1];
  }
  for (int i = v->n_scales; i < VOC_MAX_SCALES; ++i) { g.cap_u[i] = 1; g.o_u[i] = 0; h->up_rate[i] = h->up_a[i] = 0; }
  g.cap_cond = (int)((C + la) * H);
  g.o_chi = take((size_t)g.cap_cond * v->auxp * 2);
  g.o_clo = take((size_t)g.cap_cond * v->auxp * 2);
  g.cap_noise = (int)((C + win + 1) * H + A + 2);
  g.o_noise = take((size_t)g.cap_noise * 4);
  g.cap_skip = (int)((C + la) * H);
  g.o_skip = take((size_t)g.cap_skip * VOC_RES * 4);
  h->o_x.assign(v->layers, 0);
  h->cap_x.assign(v->layers, 1);
  for (int l = 1; l < v->layers; ++l) {
    // x_l: written up to X_l, read from X_{l+1} - d_l; the end push writes win H + A + sd[l] further than an ordinary one
    const long long d = 1LL << (l % lps);
    h->cap_x[l] = (int)((C + win + 1) * H + A + h->sd[l] + 2 * d);
    h->o_x[l] = take((size_t)h->cap_x[l] * VOC_RES * 4);
  }
  g.per_stream = o;
  return true;
}

extern "C" int crk_voc_stream_create(void* voc, int n_streams, int max_chunk, void** handle) {
  const Voc* v = static_cast<const Voc*>(voc);
  if (!v || !handle || n_streams < 1 || max_chunk < 1) return CRK_ERR_ARG;
  if (n_streams > 65535) return CRK_ERR_UNSUPPORTED;  // a grid's y extent
  VocStream* h = new VocStream();
  h->v = v; h->S = n_streams; h->C = max_chunk;
  if (!vs_layout(v, max_chunk, h)) { delete h; return CRK_ERR_UNSUPPORTED; }
  const size_t meta = vs_align((size_t)n_streams * 4) + vs_align((size_t)n_streams * sizeof(VsPlan));
  h->bytes = meta + h->g.per_stream * (size_t)n_streams;
  if (hipMalloc(&h->block, h->bytes) != hipSuccess) { delete h; return CRK_ERR_HIP; }
  crk_count_alloc_();
  const size_t lds = voc_lds_bytes(v);
  bool ok = hipMemset(h->block, 0, h->bytes) == hipSuccess;
  for (int i = 0; ok && i < 8; ++i)
    ok = hipFuncSetAttribute(vs_pick(i & 1, i & 2, i & 4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
  if (!ok) {
    (void)hipFree(h->block);
    delete h;
    return CRK_ERR_HIP;
  }
  h->t_in = reinterpret_cast<int*>(h->block);
  h->plan = reinterpret_cast<VsPlan*>(h->block + vs_align((size_t)n_streams * 4));
  h->state = h->block + meta;
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_voc_stream_destroy(void* st) {
  VocStream* h = static_cast<VocStream*>(st);
  if (!h) return;
  (void)hipFree(h->block);
  delete h;
}

extern "C" long long crk_voc_stream_state_bytes(void* st) {
  const VocStream* h = static_cast<const VocStream*>(st);
  return h ? (long long)h->bytes : -1;
}

extern "C" int crk_voc_stream_lookahead(void* st) {
  const VocStream* h = static_cast<const VocStream*>(st);
  return h ? h->g.la : -1;
}

extern "C" int crk_voc_stream_reset(void* st, const int* stream_ids, int n, void* stream) {
  VocStream* h = static_cast<VocStream*>(st);
  if (!h) return CRK_ERR_ARG;
  return crk_zero_stream_rows(h->t_in, 4, h->S, stream_ids, n, (hipStream_t)stream);
}

extern "C" int crk_voc_stream_push(void* st, const float* c, const float* noise, const int* n_valid, const int* end, int S,
                                   int C, float* wave, int* n_out, int flags, void* stream) {
  VocStream* h = static_cast<VocStream*>(st);
  if (!h || !c || !noise || !wave || !n_out || S < 1 || S > h->S || C < 1 || C > h->C) return CRK_ERR_ARG;
  const Voc* v = h->v;
  const VsGeom& g = h->g;
  hipStream_t q = (hipStream_t)stream;
  const bool P = (flags & CRK_FLAG_PRECISE) != 0;
  const int T = 256;
  vs_begin_kernel<<<(S + T - 1) / T, T, 0, q>>>(g, S, C, n_valid, end, h->t_in, h->plan, n_out);
  CRK_CHECK_LAUNCH();
  vs_stage_in_kernel<<<dim3((C * (g.hop + g.aux) + T - 1) / T, S), T, 0, q>>>(g, C, c, noise, h->plan, h->state);
  CRK_CHECK_LAUNCH();
  vs_conv_in_kernel<<<dim3(((C + g.win) * g.aux + T - 1) / T, S), T, 0, q>>>(g, v->conv_in, h->plan, h->state);
  CRK_CHECK_LAUNCH();
  for (int i = 0; i < g.n_scales; ++i) {
    // outputs of stage i in a push of C frames: at most (C + win) r_{i+1} + a_{i+1} (the end push)
    const long long n_max = (C + g.win) * h->up_rate[i] + h->up_a[i];
    const long long nt = n_max * (i + 1 == g.n_scales ? g.auxp : g.aux);
    vs_upsample_kernel<<<dim3((unsigned)((nt + T - 1) / T), S), T, 0, q>>>(g, i, v->up[i], h->plan, h->state);
    CRK_CHECK_LAUNCH();
  }
  const int span = (C + g.la) * g.hop;  // most samples one layer computes for one stream in one push
  const dim3 grid((span + 32 * VOC_WAVES - 1) / (32 * VOC_WAVES), S);
  const size_t lds = voc_lds_bytes(v);
  const int lps = v->layers / v->stacks;
  for (int l = 0; l < v->layers; ++l) {
    VsLayerArgs a;
    a.w = voc_layer_weights(v, l);
    a.g = g;
    a.plan = h->plan; a.state = h->state; a.wave = wave;
    a.o_xin = h->o_x[l]; a.cap_xin = h->cap_x[l];
    const bool last = l + 1 == v->layers;
    a.o_xout = last ? 0 : h->o_x[l + 1];
    a.cap_xout = last ? 1 : h->cap_x[l + 1];
    a.sd_out = h->sd[l + 1];
    a.dil = 1 << (l % lps);
    a.wave_ld = span;
    void* fn = vs_pick(P, l == 0, last);
    void* args[] = {&a};
    if (hipLaunchKernel(fn, grid, dim3(64 * VOC_WAVES), args, lds, q) != hipSuccess) return CRK_ERR_HIP;
    CRK_CHECK_LAUNCH();
  }
  return CRK_OK;
}
