// Parallel WaveGAN vocoder inference on the device (recipe stage 6; gfx950).
//
// Replaces `parallel-wavegan-decode` (egs/vaevc/template/run.sh:217-226): the forward pass of the published
// ParallelWaveGANGenerator.inference(c, x) for a ragged batch of utterances, forward only - no autograd, no saved planes.
//
// Structure (DESIGN.md section "Parallel WaveGAN vocoder"):
//  * aux path, fp32, frame rate then each upsampling rate: voc_conv_in_kernel (replicate pad + conv_in, one thread per
//    frame x channel), then one voc_upsample_kernel per upsample scale (nearest stretch x s + the shared (1, 2s+1) kernel
//    with zero padding at each utterance's edges of that stage, one thread per sample x channel).  The last stage writes
//    the upsampled conditioning as bf16 hi (+ lo residual) planes [N][auxp], auxp = aux rounded up to 16 (zero padded).
//  * residual stack: one launch per layer (voc_layer_kernel).  One wave owns 32 consecutive samples; the gate conv is
//    D[128 gate ch][32 samples] = W[128][3*64 + auxp] . [x(n-d); x(n); x(n+d); c_up(n)] on the 32x32x16 bf16 MFMA with
//    fp32 accumulation (zero taps outside the sample's utterance), then tanh * sigmoid in registers, and the gate output
//    feeds the out / skip 1x1 convs straight from the accumulator registers (its rows are the next product's k index).
//    The residual stream x is fp32 [N][64] ping-ponged between two planes, the skip sum fp32 [N][64] read-modified-written.
//    The first layer computes first_conv (1 -> 64) from the noise on the fly; the last folds the tail (x sqrt(1/L),
//    ReLU, 1x1 64 -> 64, ReLU, 1x1 64 -> 1) into its epilogue and writes the waveform.
//  * weights (weight norm folded by the caller) are laid out once by crk_voc_create as MFMA A fragments: one 16-byte
//    bf16x8 per lane and k-step.  A workgroup copies the layer's hi fragments into LDS once and then walks sample tiles;
//    CRK_FLAG_PRECISE adds the lo fragments (read from L2) and the split operands: hi.hi + hi.lo + lo.hi per product.
//  * the arithmetic of all three kernels lives in voc_common.h and voc_layer_tile.inc, one body per piece, shared with the
//    streaming kernels (voc_stream_kernels.hip); the kernels here say where a position's operands are in the flat planes
//    of a ragged batch.
#include "runtime.h"
#include "voc_common.h"
#include "../../include/crank_hip.h"
#include <math.h>
#include <string.h>
#include <vector>


struct VocLayerArgs {
  VocLayerW w;
  const float* xin; float* xout; float* skip;
  const float* noise;
  const uint16_t* chi; const uint16_t* clo;
  float* y;
  const long long* foff; int n_utts, hop, N, dil;
};

// the utterance u of frame f: largest u with off[u] <= f
__device__ __forceinline__ int voc_find_utt(const long long* off, int n_utts, long long f) {
  int lo = 0, hi = n_utts - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= f) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void voc_conv_in_kernel(const float* __restrict__ c, const float* __restrict__ w, const long long* __restrict__ off,
                                   int n_utts, int F, int aux, int win, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)F * aux) return;
  const int f = (int)(idx / aux), o = (int)(idx % aux);
  const int u = voc_find_utt(off, n_utts, f);
  const int s = (int)off[u], e = (int)off[u + 1];
  out[idx] = voc_conv_in_value([&](int fr) { return c + (size_t)fr * aux; }, w, f, o, s, e, aux, win);
}

// One upsampling stage (voc_common.h: voc_upsample_value); in_rate / in_rate * s samples per frame before / after the
// stage.  The last stage writes bf16 hi / lo planes [n][auxp] (zeros in the padding channels) and, when `out` is given,
// fp32 [n][aux].
__global__ void voc_upsample_kernel(const float* __restrict__ in, int in_rate, int s, const float* __restrict__ w,
                                    const long long* __restrict__ off, int n_utts, long long n_out, int aux, int auxp,
                                    float* __restrict__ out, uint16_t* __restrict__ ohi, uint16_t* __restrict__ olo) {
  const int ld = ohi ? auxp : aux;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_out * ld) return;
  const long long t = idx / ld;
  const int ch = (int)(idx % ld);
  if (ch >= aux) {
    ohi[idx] = 0;
    if (olo) olo[idx] = 0;
    return;
  }
  const long long out_rate = (long long)in_rate * s;
  const int u = voc_find_utt(off, n_utts, t / out_rate);
  const long long S = off[u] * out_rate, E = off[u + 1] * out_rate, Sin = off[u] * in_rate;
  const float acc = voc_upsample_value([&](long long j) { return in[(Sin + j) * aux + ch]; }, w, s, t, S, E);
  if (out) out[t * aux + ch] = acc;
  if (ohi) voc_cond_store(acc, ohi + idx, olo ? olo + idx : nullptr);
}

// where the offline kernel's samples live: flat planes over the ragged batch, utterance [us, ue) of the lane's sample
struct VocFlatLoc {
  const VocLayerArgs& a;
  int us, ue;
  __device__ __forceinline__ bool inside(int m) const { return m >= us && m < ue; }
  __device__ __forceinline__ float noise(int m) const { return a.noise[m]; }
  __device__ __forceinline__ const float* xin(int m) const { return a.xin + (size_t)m * VOC_RES; }
  __device__ __forceinline__ float* xout(int n) const { return a.xout + (size_t)n * VOC_RES; }
  __device__ __forceinline__ float* skip(int n) const { return a.skip + (size_t)n * VOC_RES; }
  __device__ __forceinline__ const uint16_t* chi(int n) const { return a.chi + (size_t)n * a.w.auxp; }
  __device__ __forceinline__ const uint16_t* clo(int n) const { return a.clo + (size_t)n * a.w.auxp; }
  __device__ __forceinline__ float* y(int n) const { return a.y + n; }
};

template <bool P, bool FIRST, bool LAST>
__global__ __launch_bounds__(64 * VOC_WAVES) void voc_layer_kernel(VocLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char voc_lds[];
  voc_layer_fill_lds(a.w, voc_lds);
  __syncthreads();
  const int lane = threadIdx.x & 63, r = lane & 31;
  const int wave = threadIdx.x >> 6;
  const int ntiles = (a.N + 31) >> 5;
  for (int tile = blockIdx.x * VOC_WAVES + wave; tile < ntiles; tile += gridDim.x * VOC_WAVES) {
    const int n = tile * 32 + r;
    const bool valid = n < a.N;
    int us = 0, ue = 0;
    if (valid) {
      const int u = voc_find_utt(a.foff, a.n_utts, n / a.hop);
      us = (int)a.foff[u] * a.hop;
      ue = (int)a.foff[u + 1] * a.hop;
    }
    {
      const VocLayerW& aw = a.w; const VocFlatLoc loc{a, us, ue}; const int dil = a.dil; const unsigned char* lds = voc_lds;
#include "voc_layer_tile.inc"
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------

static size_t voc_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct VocWs {
  float *cin, *upa, *upb, *x0, *x1, *skip;
  uint16_t *chi, *clo;
  size_t bytes;
};

static VocWs voc_ws(const Voc* v, long long F, unsigned char* base) {
  VocWs w;
  const long long N = F * v->hop;
  long long inter = 0, cum = 1;
  for (int i = 0; i + 1 < v->n_scales; ++i) {
    cum *= v->scales[i];
    inter = cum > inter ? cum : inter;
  }
  size_t o = 0;
  auto take = [&](size_t bytes) { unsigned char* p = base ? base + o : nullptr; o += voc_align(bytes); return p; };
  w.cin = (float*)take((size_t)F * v->aux * 4);
  w.upa = (float*)take((size_t)F * inter * v->aux * 4);
  w.upb = (float*)take((size_t)F * inter * v->aux * 4);
  w.chi = (uint16_t*)take((size_t)N * v->auxp * 2);
  w.clo = (uint16_t*)take((size_t)N * v->auxp * 2);
  w.x0 = (float*)take((size_t)N * VOC_RES * 4);
  w.x1 = (float*)take((size_t)N * VOC_RES * 4);
  w.skip = (float*)take((size_t)N * VOC_RES * 4);
  w.bytes = o;
  return w;
}

template <bool P, bool FIRST, bool LAST>
static void* voc_layer_fn() { return (void*)voc_layer_kernel<P, FIRST, LAST>; }

static void* voc_pick(bool p, bool first, bool last) {
  if (p) {
    if (first) return last ? voc_layer_fn<true, true, true>() : voc_layer_fn<true, true, false>();
    return last ? voc_layer_fn<true, false, true>() : voc_layer_fn<true, false, false>();
  }
  if (first) return last ? voc_layer_fn<false, true, true>() : voc_layer_fn<false, true, false>();
  return last ? voc_layer_fn<false, false, true>() : voc_layer_fn<false, false, false>();
}

// A fragments: element j of lane (r, h) of k-step q is A[row r][k(q, h, j)]
static void voc_put(std::vector<uint16_t>& hi, std::vector<uint16_t>& lo, size_t unit, int lane, int j, float w) {
  uint32_t b;
  memcpy(&b, &w, 4);
  const uint32_t rb = b + 0x7fffu + ((b >> 16) & 1u);  // round to nearest even (weights are finite)
  const uint16_t hb = (uint16_t)(rb >> 16);
  const uint32_t hf = (uint32_t)hb << 16;
  float hv;
  memcpy(&hv, &hf, 4);
  const float res = w - hv;
  memcpy(&b, &res, 4);
  const uint32_t rl = b + 0x7fffu + ((b >> 16) & 1u);
  hi[unit * VOC_FRAG + lane * 8 + j] = hb;
  lo[unit * VOC_FRAG + lane * 8 + j] = (uint16_t)(rl >> 16);
}
// k index of element j, lane half h, k-step (mt, s) of an operand taken from accumulator registers 8s..8s+7 of tile mt
static int voc_acc_k(int ks, int h, int j) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }

extern "C" void* crk_voc_create(int layers, int stacks, int aux_ch, int aux_window, const int* scales, int n_scales,
                                const float* params) {
  if (layers < 1 || stacks < 1 || layers % stacks || aux_ch < 1 || aux_ch > VOC_MAX_AUX || aux_window < 0 ||
      n_scales < 1 || n_scales > VOC_MAX_SCALES || !scales || !params)
    return nullptr;
  if (layers / stacks > 30) return nullptr;  // dilation 2^29 at most
  Voc* v = new Voc();
  v->layers = layers; v->stacks = stacks; v->aux = aux_ch; v->auxp = round_up(aux_ch, 16); v->win = aux_window;
  v->n_scales = n_scales; v->hop = 1;
  for (int i = 0; i < n_scales; ++i) {
    if (scales[i] < 1 || scales[i] > VOC_MAX_SCALE) { delete v; return nullptr; }
    v->scales[i] = scales[i];
    v->hop *= scales[i];
  }
  v->kq = 12 + v->auxp / 16;
  const int K = 2 * aux_window + 1, A = aux_ch, kq = v->kq;
  // host parameter block (crank_hip.h: crk_voc_create)
  const float* p = params;
  const float* first = p; p += 2 * VOC_RES;
  const float* conv_in = p; p += (size_t)A * A * K;
  const float* up[VOC_MAX_SCALES];
  for (int i = 0; i < n_scales; ++i) { up[i] = p; p += 2 * scales[i] + 1; }
  const float* lay = p;
  const size_t per_layer = (size_t)VOC_GATE * VOC_RES * 3 + VOC_GATE + (size_t)VOC_GATE * A + 2 * ((size_t)VOC_RES * VOC_RES + VOC_RES);
  p += per_layer * layers;
  const float* t1w = p; p += VOC_RES * VOC_RES;
  const float* t1b = p; p += VOC_RES;
  const float* t2w = p; p += VOC_RES;
  const float* t2b = p;

  // fp32 block: first, conv_in, up taps, gate bias, os bias, tail
  std::vector<float> f32;
  auto fput = [&](const float* s, size_t n) { size_t at = f32.size(); f32.insert(f32.end(), s, s + n); return at; };
  const size_t o_first = fput(first, 2 * VOC_RES);
  const size_t o_cin = fput(conv_in, (size_t)A * A * K);
  size_t o_up[VOC_MAX_SCALES];
  for (int i = 0; i < n_scales; ++i) o_up[i] = fput(up[i], 2 * scales[i] + 1);
  const size_t o_gb = f32.size(); f32.resize(o_gb + (size_t)layers * VOC_GATE);
  const size_t o_ob = f32.size(); f32.resize(o_ob + (size_t)layers * VOC_GATE);
  const size_t o_tail = f32.size(); f32.resize(o_tail + 2 * VOC_RES + 4);
  const size_t gate_units = (size_t)4 * kq, os_units = 16;
  std::vector<uint16_t> ghi(layers * gate_units * VOC_FRAG), glo(ghi.size());
  std::vector<uint16_t> ohi(layers * os_units * VOC_FRAG), olo(ohi.size());
  std::vector<uint16_t> thi(8 * VOC_FRAG), tlo(thi.size());
  for (int l = 0; l < layers; ++l) {
    const float* L = lay + per_layer * l;
    const float* cw = L;                                  // conv.weight [128][64][3]
    const float* cb = cw + VOC_GATE * VOC_RES * 3;        // conv.bias [128]
    const float* aw = cb + VOC_GATE;                      // conv1x1_aux.weight [128][aux]
    const float* ow = aw + (size_t)VOC_GATE * A;          // conv1x1_out.weight [64][64]
    const float* ob = ow + VOC_RES * VOC_RES;             // conv1x1_out.bias
    const float* sw = ob + VOC_RES;                       // conv1x1_skip.weight
    const float* sb = sw + VOC_RES * VOC_RES;             // conv1x1_skip.bias
    for (int c = 0; c < VOC_GATE; ++c) f32[o_gb + l * VOC_GATE + c] = cb[c];
    for (int c = 0; c < VOC_RES; ++c) {
      f32[o_ob + l * VOC_GATE + c] = ob[c];
      f32[o_ob + l * VOC_GATE + VOC_RES + c] = sb[c];
    }
    for (int t = 0; t < 4; ++t)
      for (int q = 0; q < kq; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int row = 32 * t + (lane & 31), h = lane >> 5;
            float w;
            if (q < 12) {
              const int tap = q / 4, ci = (q % 4) * 16 + 8 * h + j;
              w = cw[((size_t)row * VOC_RES + ci) * 3 + tap];
            } else {
              const int ca = (q - 12) * 16 + 8 * h + j;
              w = ca < A ? aw[(size_t)row * A + ca] : 0.f;
            }
            voc_put(ghi, glo, l * gate_units + t * kq + q, lane, j, w);
          }
    for (int t = 0; t < 4; ++t)
      for (int ks = 0; ks < 4; ++ks)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int row = 32 * (t & 1) + (lane & 31);
            const float* W = t < 2 ? ow : sw;
            voc_put(ohi, olo, l * os_units + t * 4 + ks, lane, j, W[row * VOC_RES + voc_acc_k(ks, lane >> 5, j)]);
          }
  }
  for (int t = 0; t < 2; ++t)
    for (int ks = 0; ks < 4; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int row = 32 * t + (lane & 31);
          voc_put(thi, tlo, t * 4 + ks, lane, j, t1w[row * VOC_RES + voc_acc_k(ks, lane >> 5, j)]);
        }
  for (int c = 0; c < VOC_RES; ++c) {
    f32[o_tail + c] = t1b[c];
    f32[o_tail + VOC_RES + c] = t2w[c];
  }
  f32[o_tail + 2 * VOC_RES] = t2b[0];

  // one device block: [bf16 fragments][fp32]
  size_t off = 0;
  auto place = [&](size_t bytes) { size_t at = off; off += voc_align(bytes); return at; };
  const size_t b_ghi = place(ghi.size() * 2), b_glo = place(glo.size() * 2), b_ohi = place(ohi.size() * 2),
               b_olo = place(olo.size() * 2), b_thi = place(thi.size() * 2), b_tlo = place(tlo.size() * 2),
               b_f32 = place(f32.size() * 4);
  std::vector<unsigned char> host(off, 0);
  memcpy(&host[b_ghi], ghi.data(), ghi.size() * 2);
  memcpy(&host[b_glo], glo.data(), glo.size() * 2);
  memcpy(&host[b_ohi], ohi.data(), ohi.size() * 2);
  memcpy(&host[b_olo], olo.data(), olo.size() * 2);
  memcpy(&host[b_thi], thi.data(), thi.size() * 2);
  memcpy(&host[b_tlo], tlo.data(), tlo.size() * 2);
  memcpy(&host[b_f32], f32.data(), f32.size() * 4);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v->n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipMalloc(&v->block, off) != hipSuccess) {
    delete v;
    return nullptr;
  }
  crk_count_alloc_();
  if (hipMemcpy(v->block, host.data(), off, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(v->block);
    delete v;
    return nullptr;
  }
  const size_t lds = voc_lds_bytes(v);
  for (int i = 0; i < 8; ++i)
    if (hipFuncSetAttribute(voc_pick(i & 1, i & 2, i & 4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipFree(v->block);
      delete v;
      return nullptr;
    }
  const float* F32 = reinterpret_cast<const float*>(v->block + b_f32);
  v->first = F32 + o_first;
  v->conv_in = F32 + o_cin;
  for (int i = 0; i < n_scales; ++i) v->up[i] = F32 + o_up[i];
  v->gate_b = F32 + o_gb;
  v->os_b = F32 + o_ob;
  v->tail = F32 + o_tail;
  v->gate_hi = reinterpret_cast<const uint16_t*>(v->block + b_ghi);
  v->gate_lo = reinterpret_cast<const uint16_t*>(v->block + b_glo);
  v->os_hi = reinterpret_cast<const uint16_t*>(v->block + b_ohi);
  v->os_lo = reinterpret_cast<const uint16_t*>(v->block + b_olo);
  v->t1_hi = reinterpret_cast<const uint16_t*>(v->block + b_thi);
  v->t1_lo = reinterpret_cast<const uint16_t*>(v->block + b_tlo);
  return v;
}

extern "C" void crk_voc_destroy(void* voc) {
  Voc* v = static_cast<Voc*>(voc);
  if (!v) return;
  (void)hipFree(v->block);
  delete v;
}

extern "C" long long crk_voc_workspace_bytes(void* voc, int n_utts, int total_frames) {
  const Voc* v = static_cast<const Voc*>(voc);
  if (!v || n_utts < 1 || total_frames < 1) return -1;
  return (long long)voc_ws(v, total_frames, nullptr).bytes;
}

// the aux path: conv_in and every upsampling stage; the last stage into (fp32 out) and / or (chi, clo)
static int voc_aux(const Voc* v, const float* c, const long long* off, int n_utts, int F, const VocWs& w, float* out,
                   uint16_t* chi, uint16_t* clo, hipStream_t st) {
  const int T = 256;
  const long long nin = (long long)F * v->aux;
  voc_conv_in_kernel<<<(unsigned)((nin + T - 1) / T), T, 0, st>>>(c, v->conv_in, off, n_utts, F, v->aux, v->win, w.cin);
  CRK_CHECK_LAUNCH();
  const float* src = w.cin;
  int rate = 1;
  for (int i = 0; i < v->n_scales; ++i) {
    const bool last = i + 1 == v->n_scales;
    float* dst = last ? out : (i & 1 ? w.upb : w.upa);
    const long long n_out = (long long)F * rate * v->scales[i];
    const long long nt = n_out * (last && chi ? v->auxp : v->aux);
    voc_upsample_kernel<<<(unsigned)((nt + T - 1) / T), T, 0, st>>>(src, rate, v->scales[i], v->up[i], off, n_utts, n_out,
                                                                   v->aux, v->auxp, dst, last ? chi : nullptr,
                                                                   last ? clo : nullptr);
    CRK_CHECK_LAUNCH();
    src = dst;
    rate *= v->scales[i];
  }
  return CRK_OK;
}

static int voc_check(const Voc* v, const void* c, const long long* off, int n_utts, int F, const void* ws, long long ws_bytes) {
  if (!v || !c || !off || n_utts < 1 || F < 1 || !ws) return CRK_ERR_ARG;
  if ((long long)F * v->hop > 0x7fffffffLL / VOC_RES) return CRK_ERR_UNSUPPORTED;
  if (ws_bytes < (long long)voc_ws(v, F, nullptr).bytes) return CRK_ERR_ARG;
  return CRK_OK;
}

extern "C" int crk_voc_upsample(void* voc, const float* c, const long long* frame_offsets, int n_utts, int total_frames,
                                float* out, void* workspace, long long workspace_bytes, void* stream) {
  const Voc* v = static_cast<const Voc*>(voc);
  int rc = voc_check(v, c, frame_offsets, n_utts, total_frames, workspace, workspace_bytes);
  if (rc) return rc;
  if (!out) return CRK_ERR_ARG;
  const VocWs w = voc_ws(v, total_frames, static_cast<unsigned char*>(workspace));
  return voc_aux(v, c, frame_offsets, n_utts, total_frames, w, out, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int crk_voc_forward(void* voc, const float* c, const long long* frame_offsets, int n_utts, int total_frames,
                               const float* noise, float* out, void* workspace, long long workspace_bytes, int flags,
                               void* stream) {
  const Voc* v = static_cast<const Voc*>(voc);
  int rc = voc_check(v, c, frame_offsets, n_utts, total_frames, workspace, workspace_bytes);
  if (rc) return rc;
  if (!noise || !out) return CRK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool P = (flags & CRK_FLAG_PRECISE) != 0;
  const VocWs w = voc_ws(v, total_frames, static_cast<unsigned char*>(workspace));
  rc = voc_aux(v, c, frame_offsets, n_utts, total_frames, w, nullptr, w.chi, P ? w.clo : nullptr, st);
  if (rc) return rc;
  const int N = total_frames * v->hop;
  const int ntiles = (N + 31) / 32;
  int grid = (ntiles + VOC_WAVES - 1) / VOC_WAVES;
  if (grid > v->n_cu) grid = v->n_cu;
  const size_t lds = voc_lds_bytes(v);
  const int lps = v->layers / v->stacks;
  float* xb[2] = {w.x0, w.x1};
  for (int l = 0; l < v->layers; ++l) {
    VocLayerArgs a;
    a.xin = l ? xb[(l - 1) & 1] : nullptr;
    a.xout = xb[l & 1];
    a.skip = w.skip;
    a.w = voc_layer_weights(v, l);
    a.noise = noise;
    a.chi = w.chi; a.clo = w.clo;
    a.y = out;
    a.foff = frame_offsets; a.n_utts = n_utts; a.hop = v->hop; a.N = N;
    a.dil = 1 << (l % lps);
    void* fn = voc_pick(P, l == 0, l + 1 == v->layers);
    void* args[] = {&a};
    if (hipLaunchKernel(fn, dim3(grid), dim3(64 * VOC_WAVES), args, lds, st) != hipSuccess) return CRK_ERR_HIP;
    CRK_CHECK_LAUNCH();
  }
  return CRK_OK;
}
