// The Parallel WaveGAN generator's arithmetic, one device body per piece (vocoder_kernels.hip: the offline kernels over a
// ragged batch; voc_stream_kernels.hip: the streaming kernels over per-stream rings).  A body computes one output - a
// conv_in value, an upsampled value, the 32 samples of a layer tile (voc_layer_tile.inc) - and asks a caller-supplied
// accessor where an operand lives and whether a position is inside the utterance; the kernels differ in nothing else.  In a layer tile a
// sample is one MFMA column: its value depends neither on its tile nor on its neighbours in the tile, and its skip sum is
// read-modified-written once per layer, so any kernel that presents the same operands gets the same bits.
#pragma once
#include "common.h"

#define VOC_RES 64
#define VOC_GATE 128
#define VOC_MAX_AUX 128
#define VOC_MAX_SCALES 8
#define VOC_MAX_SCALE 16
#define VOC_WAVES 8
#define VOC_FRAG 512  // bf16 elements of one A fragment set: 64 lanes x 8

struct Voc {
  int layers, stacks, aux, auxp, win, n_scales, hop, kq, n_cu;
  int scales[VOC_MAX_SCALES];
  unsigned char* block;  // the one device allocation of the handle
  const float* first;    // w[64], b[64]
  const float* conv_in;  // [aux][aux][2 win + 1]
  const float* up[VOC_MAX_SCALES];
  const uint16_t *gate_hi, *gate_lo;  // per layer [4 tiles][kq][64 lanes][8]
  const float* gate_b;                // per layer [128]
  const uint16_t *os_hi, *os_lo;      // per layer [4 tiles: out 0-1, skip 2-3][4 k-steps][64][8]
  const float* os_b;                  // per layer [128]: out bias 64, skip bias 64
  const uint16_t *t1_hi, *t1_lo;      // [2][4][64][8]
  const float* tail;                  // b1[64], w2[64], b2
};

// one layer's weights as the tile body reads them
struct VocLayerW {
  const float* first;
  const uint16_t* gw_hi; const uint16_t* gw_lo; const float* gb;
  const uint16_t* ow_hi; const uint16_t* ow_lo; const float* ob;
  const uint16_t* tw_hi; const uint16_t* tw_lo; const float* tail;
  float skip_scale;
  int auxp, kq;
};

static inline size_t voc_lds_bytes(const Voc* v) { return (size_t)(4 * v->kq + 16) * 64 * 16; }

static inline VocLayerW voc_layer_weights(const Voc* v, int l) {
  VocLayerW a;
  a.first = v->first;
  a.gw_hi = v->gate_hi + (size_t)l * 4 * v->kq * VOC_FRAG;
  a.gw_lo = v->gate_lo + (size_t)l * 4 * v->kq * VOC_FRAG;
  a.gb = v->gate_b + (size_t)l * VOC_GATE;
  a.ow_hi = v->os_hi + (size_t)l * 16 * VOC_FRAG;
  a.ow_lo = v->os_lo + (size_t)l * 16 * VOC_FRAG;
  a.ob = v->os_b + (size_t)l * VOC_GATE;
  a.tw_hi = v->t1_hi; a.tw_lo = v->t1_lo; a.tail = v->tail;
  a.skip_scale = sqrtf(1.f / (float)v->layers);
  a.auxp = v->auxp;
  a.kq = v->kq;
  return a;
}

// conv_in at frame f, output channel o, of an utterance of frames [s, e): ReplicationPad1d(win) + Conv1d.  frame(fr) is
// the row of aux inputs of frame fr.
template <class Frame>
__device__ __forceinline__ float voc_conv_in_value(const Frame& frame, const float* __restrict__ w, int f, int o, int s, int e,
                                                   int aux, int win) {
  const int K = 2 * win + 1;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    const int fr = min(max(f - win + k, s), e - 1);  // ReplicationPad1d(aux_context_window)
    const float* cr = frame(fr);
    const float* wr = w + (size_t)o * aux * K + k;
    for (int i = 0; i < aux; ++i) acc = fmaf(wr[(size_t)i * K], cr[i], acc);
  }
  return acc;
}

// One upsampling stage at output sample t of an utterance whose output samples are [S, E):
// out[t] = sum_k w[k] * stretch(in)[t + k - s], stretch(in)[t'] = in[(t' - S) / s] inside the utterance and 0 outside it
// (the Conv2d's zero padding (0, s) at the stage's edges).  in(j) is the stage's input sample j of the utterance.
template <class In>
__device__ __forceinline__ float voc_upsample_value(const In& in, const float* __restrict__ w, int s, long long t, long long S,
                                                    long long E) {
  float acc = 0.f;
  for (int k = 0; k <= 2 * s; ++k) {
    const long long tt = t + k - s;
    if (tt >= S && tt < E) acc = fmaf(w[k], in((tt - S) / s), acc);
  }
  return acc;
}
// the last stage's value as the layers read it: bf16 hi and the bf16 of the residual
__device__ __forceinline__ void voc_cond_store(float acc, uint16_t* hi, uint16_t* lo) {
  const __bf16 hb = (__bf16)acc;
  *hi = __builtin_bit_cast(uint16_t, hb);
  if (lo) *lo = f2bf(acc - (float)hb);
}

__device__ __forceinline__ bf16x8 voc_pack8(const float* v) {
  uint4 u = make_uint4(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7]));
  return __builtin_bit_cast(bf16x8, u);
}
// hi = bf16(v), lo = bf16(v - hi)
template <bool P>
__device__ __forceinline__ void voc_split8(const float* v, bf16x8& hi, bf16x8& lo) {
  hi = voc_pack8(v);
  if (P) {
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = v[j] - (float)hi[j];
    lo = voc_pack8(r);
  }
}
template <bool P>
__device__ __forceinline__ f32x16 voc_mma(f32x16 acc, bf16x8 ah, const uint16_t* al_ptr, bf16x8 bh, bf16x8 bl) {
  acc = mfma_bf16(ah, bh, acc);
  if (P) {
    const bf16x8 al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(al_ptr));
    acc = mfma_bf16(ah, bl, acc);
    acc = mfma_bf16(al, bh, acc);
  }
  return acc;
}
__device__ __forceinline__ float voc_sigmoid(float v) { return 1.f / (1.f + __expf(-v)); }
__device__ __forceinline__ float voc_tanh(float v) { return 1.f - 2.f / (__expf(2.f * v) + 1.f); }

// the workgroup's copy of a layer's hi fragments (gate, then out / skip) into LDS; the caller synchronises
__device__ __forceinline__ void voc_layer_fill_lds(const VocLayerW& a, unsigned char* lds) {
  const int gate_units = 4 * a.kq * 64, os_units = 16 * 64;  // 16-byte fragments
  uint4* l4 = reinterpret_cast<uint4*>(lds);
  const uint4* g4 = reinterpret_cast<const uint4*>(a.gw_hi);
  const uint4* o4 = reinterpret_cast<const uint4*>(a.ow_hi);
  for (int i = threadIdx.x; i < gate_units; i += blockDim.x) l4[i] = g4[i];
  for (int i = threadIdx.x; i < os_units; i += blockDim.x) l4[gate_units + i] = o4[i];
}

// The layer's tile body itself is voc_layer_tile.inc, included as text by the two layer kernels.
