// What the streaming-conversion kernel families share (stream_kernels.hip: causal generators; stream_la_kernels.hip:
// non-causal generators followed at a fixed look-ahead): the tile geometry, the tables of effective fp32 weights, the
// device bodies every multiply-add, gate, residual / skip term and codebook search of both families is made of - and the
// lines around them that are the same in both: the LDS carve, the input-tile load, the speaker's conditioning value, a
// layer's conv + aux into the gate tile, a stack's last two convs - and the host handle StHandle with the functions both
// families' entry points are made of (declared at the end, defined once in stream_kernels.hip; the ones that fill a
// kernel's parameter block are templates on it, StP or LaP, which stay as their kernels take them).  What differs stays
// with its family: the net and tile bodies (residual, skip, history and rings) and the kernels.  An output element is
// bias + one chain of fmaf over (tap, input channel) in ascending order whatever thread, tile or chunk computes it;
// contraction is off for every file that includes this one.
#pragma once
#include <math.h>
#include <string.h>

#include <vector>

#include "runtime.h"
#include "vq_common.h"
#include "../../include/crank_hip.h"

#pragma clang fp contract(off)

#define ST_THREADS 256
#define ST_TILE 64      // frames resident in LDS
#define ST_HALO 64      // largest (k - 1) * dilation of a layer
#define ST_LD 128       // row stride (floats) of the io / conditioning / gate tiles
#define ST_MAX_STACKS 3
#define ST_MAX_CHUNK 65536

enum { ST_ROLE_FIRST = 0, ST_ROLE_CONV = 1, ST_ROLE_AUX = 2, ST_ROLE_OUT = 3, ST_ROLE_SKIP = 4, ST_ROLE_LAST1 = 5, ST_ROLE_LAST2 = 6 };

// offsets: w_* into the prepared table, b_* into the model's parameter block (-1: no bias), state_off into a stream's state
struct StLayer { long long w_conv, w_aux, w_os, b_conv, b_out, b_skip, state_off; int dil, halo; };
struct StNet {
  long long w_first, w_last1, w_last2, b_first, b_last1, b_last2;
  int in_ch, in_pad, out_ch, aux_ch, aux_pad, k, L, layer0;
  float skip_scale;
};
// one conv of the prepare pass: rows [row0, row0 + cout) of the launch; element (r, ci, j) of weight_v goes to
// table[w_off + (j * cin_pad + ci) * ld + col0 + r]
struct StPrep { long long off_g, off_v, w_off; int row0, cout, cin, cin_pad, k, ld, col0; };


static inline int st_pad4(int c) { return (c + 3) & ~3; }
static inline size_t st_lds_bytes() {
  return sizeof(float) * ((size_t)(ST_HALO + ST_TILE) * 64 + 3 * (size_t)ST_TILE * ST_LD + (size_t)ST_TILE * 64 + 10 * ST_TILE);
}


// ------------------------------------------------------------------------------------------------------------ dense
// out(f, co) for f < nv, co < cout: the fmaf chain over taps j = 0 .. taps-1 and input channels ci = 0 .. cin_pad-1 of
// W[j][ci][co] * in[f - (taps - 1 - j) * dil][ci], started at 0, handed to epi(f, co, sum).  A thread owns one output channel
// and FT consecutive frames; rows past nv inside its run are computed from whatever the tile holds and dropped.  `in` points
// at frame 0's row; rows in front of it are the layer's history.  No barrier inside.
template <int FT, class Epi>
__device__ __forceinline__ void st_dense(const float* __restrict__ W, int cout, int cin_pad, int taps, int dil, const float* in,
                                         int ldi, int nv, Epi epi) {
  const int slots = cout <= 16 ? 16 : (cout <= 32 ? 32 : (cout <= 64 ? 64 : 128));
  const int groups = ST_THREADS / slots;
  const int co = threadIdx.x & (slots - 1), grp = threadIdx.x / slots;
  if (co >= cout) return;
  for (int f0 = grp * FT; f0 < nv; f0 += groups * FT) {
    float acc[FT];
#pragma unroll
    for (int i = 0; i < FT; i++) acc[i] = 0.f;
    for (int j = 0; j < taps; j++) {
      const float* inj = in + (f0 - (taps - 1 - j) * dil) * ldi;
      const float* wj = W + (size_t)j * cin_pad * cout + co;
#pragma unroll 2
      for (int ci = 0; ci < cin_pad; ci += 4) {
        const float w0 = wj[(size_t)ci * cout], w1 = wj[(size_t)(ci + 1) * cout], w2 = wj[(size_t)(ci + 2) * cout],
                    w3 = wj[(size_t)(ci + 3) * cout];
#pragma unroll
        for (int i = 0; i < FT; i++) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(inj + i * ldi + ci);
          acc[i] = fmaf(w0, xv[0], acc[i]);
          acc[i] = fmaf(w1, xv[1], acc[i]);
          acc[i] = fmaf(w2, xv[2], acc[i]);
          acc[i] = fmaf(w3, xv[3], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FT; i++)
      if (f0 + i < nv) epi(f0 + i, co, acc[i]);
  }
}

struct StLds { float *xw, *g, *skip, *cond, *io, *red_d, *x2s; int *red_i, *idxs; };

// The tiles of a workgroup in its st_lds_bytes() of dynamic LDS.
__device__ __forceinline__ StLds st_carve(float* lds) {
  StLds m;
  m.xw = lds;
  m.g = m.xw + (ST_HALO + ST_TILE) * 64;
  m.skip = m.g + ST_TILE * ST_LD;
  m.cond = m.skip + ST_TILE * 64;
  m.io = m.cond + ST_TILE * ST_LD;
  m.red_d = m.io + ST_TILE * ST_LD;
  m.red_i = reinterpret_cast<int*>(m.red_d + 4 * ST_TILE);
  m.x2s = m.red_d + 8 * ST_TILE;
  m.idxs = reinterpret_cast<int*>(m.red_d + 9 * ST_TILE);
  return m;
}

// Rows [r0, r0 + nv) of the caller's features into m.io, zero in the padded channels and in a row f without an input
// frame (has(f) false: the look-ahead's flush).  P: StP / LaP.
template <class P, class Has>
__device__ __forceinline__ void st_load_input(const P& p, long long r0, int nv, const StLds& m, Has has) {
  const int ip = p.enc[0].in_pad, ic = p.enc[0].in_ch;
  for (int i = threadIdx.x; i < nv * ip; i += ST_THREADS) {
    const int f = i / ip, c = i - f * ip;
    m.io[f * ST_LD + c] = (c < ic && has(f)) ? p.x[(r0 + f) * p.ldx + c] : 0.f;
  }
}

// Column e of the conditioning of speaker spk (held to the table by the caller): one-hot, or the embedding's row in the
// parameter block par.  (References, like st_last's skip: the callers' own expressions, evaluated where they stood.)
template <class P, class I>
__device__ __forceinline__ float st_spk_value(const P& p, const float* const& par, const I& spk, const int& e) {
  return p.spk_onehot ? (e == (int)spk ? 1.f : 0.f) : par[p.spk_off + (long long)spk * p.spk_dim + e];
}

// z = tanh(a) * sigmoid(b) of the gate rows g = [a | b] (64 + 64 columns), written over a.  No barrier inside.
__device__ __forceinline__ void st_gate(float* g, int nv) {
  for (int i = threadIdx.x; i < nv * 64; i += ST_THREADS) {
    const int f = i >> 6, c = i & 63;
    const float a = g[f * ST_LD + c], b = g[f * ST_LD + 64 + c];
    g[f * ST_LD + c] = tanhf(a) * (1.f / (1.f + expf(-b)));
  }
}

// The two halves of the [out | skip] 1x1 of z (column co of 128, a its fmaf chain): the layer's residual output
// (out + x) * sqrt(.5) for co < 64 on the layer's input value *x of the same frame, stored to *out (the causal kernel
// updates in place: out == x), and the term the skip sum takes.
__device__ __forceinline__ void st_residual(float* out, const float* P, long long b_out, int co, float a, const float* x) {
  *out = (((b_out >= 0 ? P[b_out + co] : 0.f) + a) + *x) * 0.70710678118654752440f;
}
__device__ __forceinline__ float st_skip_term(const float* P, long long b_skip, int co, float a) {
  return (b_skip >= 0 ? P[b_skip + co - 64] : 0.f) + a;
}

// A stack's tail on the rows g = relu(skip sum * skip_scale): relu(last1) into skip, last2 into m.io.  Ends on a barrier.
// skip is m.skip, by reference: the causal net hands over the copy it made on entry, the look-ahead net m.skip itself,
// which its out-of-line form then loads where it is used - what each did before this body was shared.
template <int FT>
__device__ __forceinline__ void st_last(const float* W, const float* P, const StNet& n, float* g, float* const& skip, int nv,
                                        const StLds& m) {
  st_dense<FT>(W + n.w_last1, 64, 64, 1, 1, g, ST_LD, nv,
               [&](int f, int co, float a) { skip[f * 64 + co] = fmaxf(P[n.b_last1 + co] + a, 0.f); });
  __syncthreads();
  st_dense<FT>(W + n.w_last2, n.out_ch, 64, 1, 1, skip, 64, nv,
               [&](int f, int co, float a) { m.io[f * ST_LD + co] = P[n.b_last2 + co] + a; });
  __syncthreads();
}

// Nearest code of the nv rows xs (row stride ST_LD) in cb [K][D]: a thread owns a code (its row in registers), the frames
// pass by as LDS broadcasts, a wave meets per frame under the (distance, then index) order, the four waves through LDS.
template <int D>
__device__ void st_vq(const float* __restrict__ cb, int K, const float* xs, int nv, const StLds& m) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < nv) m.x2s[tid] = vq_norm<D>(vq_row16(xs + tid * ST_LD));
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += ST_THREADS) {
    const int k = k0 + tid;
    const bool live = k < K;
    float w[D];
    const float* wp = cb + (size_t)(live ? k : 0) * D;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(wp + d);
      w[d] = v[0]; w[d + 1] = v[1]; w[d + 2] = v[2]; w[d + 3] = v[3];
    }
    const float w2 = vq_norm<D>(w);
    for (int f = 0; f < nv; f++) {
      const float dist = vq_dist(w2, vq_dot<D>(vq_row16(xs + f * ST_LD), w), m.x2s[f]);
      const bool ok = live && dist < INFINITY;  // (a NaN or an infinite distance never wins: the row then takes code 0)
      float bd = ok ? dist : INFINITY;
      int bi = ok ? k : 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (vq_better(od, oi, bd, bi)) { bd = od; bi = oi; }
      }
      if (lane == 0) {
        const int slot = wave * ST_TILE + f;
        if (k0 == 0 || vq_better(bd, bi, m.red_d[slot], m.red_i[slot])) { m.red_d[slot] = bd; m.red_i[slot] = bi; }
      }
    }
  }
  __syncthreads();
  if (tid < nv) {
    float bd = m.red_d[tid];
    int bi = m.red_i[tid];
    for (int wv = 1; wv < ST_THREADS / 64; wv++) {
      const float od = m.red_d[wv * ST_TILE + tid];
      const int oi = m.red_i[wv * ST_TILE + tid];
      if (vq_better(od, oi, bd, bi)) { bd = od; bi = oi; }
    }
    m.idxs[tid] = vq_pin(bi, K);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------ host
// The tables a handle of either family builds from the model's stack handles, and what a handle of either family holds
// beside its kernel's parameter block.  stream_kernels.hip defines the functions that are no templates.
struct StTables {
  std::vector<StLayer> layers;
  std::vector<StPrep> preps;
  long long wt_floats = 0, state_floats = 0;
  int rows = 0;
};
struct StHandle : StTables {
  int S = 0, Cmax = 0;
  float *wt = nullptr, *state = nullptr;
  StLayer* d_layers = nullptr;
  StPrep* d_preps = nullptr;
  bool prepared = false;
};
int st_malloc(void** q, size_t bytes);
// the conv table of one stack (crk_net_conv_info) as this family's tables; CRK_ERR_UNSUPPORTED for what the kernels do not take
int st_add_net(StTables* h, void* net, long long base, int in_ch, int out_ch, int aux_ch, StNet* out);
// stream_prepare_kernel on `rows` output rows: the effective weights of every conv of `preps` into the table wt
int st_prepare_launch(const StPrep* d_preps, int nprep, int rows, const float* params, float* wt, void* stream);

// create: arguments and shapes (causal: what the family takes); the last decoder's input and conditioning widths
int st_check_desc(const crk_stream_desc* d, void* const* enc_nets, void* const* dec_nets, void** handle, bool causal, int* qsum,
                  int* d_aux);
// create: the model fields of p and the tables of every stack, encoders and decoders in the kernels' layer order
template <class P>
int st_fill_model(StTables* h, P& p, const crk_stream_desc& d, void* const* enc_nets, void* const* dec_nets, int qsum, int d_aux) {
  memset(&p, 0, sizeof(p));
  p.nst = d.n_stacks; p.enc_f0 = d.enc_f0 ? 1 : 0; p.dec_f0 = d.dec_f0 ? 2 : 0; p.spk_dim = d.spk_dim;
  p.spk_onehot = d.spk_onehot ? 1 : 0; p.n_spk = d.n_spk; p.spk_off = d.spk_off;
  int rc = CRK_OK;
  for (int n = 0; n < d.n_stacks && rc == CRK_OK; n++) {
    p.emb_dim[n] = d.emb_dim[n]; p.emb_size[n] = d.emb_size[n]; p.cb_off[n] = d.cb_off[n];
    rc = st_add_net(h, enc_nets[n], d.enc_base[n], n == 0 ? d.in_ch : d.emb_dim[n - 1], d.emb_dim[n],
                    n == 0 && d.enc_f0 ? 2 : 0, &p.enc[n]);
    if (rc == CRK_OK)
      rc = st_add_net(h, dec_nets[n], d.dec_base[n], n == 0 ? qsum : d.emb_dim[n], n == 0 ? d.out_ch : d.emb_dim[n - 1],
                      n == 0 ? d_aux : 0, &p.dec[n]);
  }
  p.state_stride = h->state_floats;
  return rc;
}
// reserve: the arguments; on the first call the zeroed weight table and the layer and prep tables on the device.  (The
// caller raises the dynamic-LDS limit, crk_raise_lds per reserve: it belongs to the current device's copy of a kernel.)
int st_reserve_tables(StHandle* h, int S, int C_max);
// reserve: a new zeroed buffer for more streams (every stream starts over); *q is null where it fails
int st_zeroed(void** q, size_t bytes);
template <class P>
int st_prepare(StHandle* h, P& p, const float* params, void* stream) {
  if (!h || !params || !h->wt) return CRK_ERR_ARG;
  const int rc = st_prepare_launch(h->d_preps, (int)h->preps.size(), h->rows, params, h->wt, stream);
  if (rc != CRK_OK) return rc;
  p.params = params;
  h->prepared = true;
  return CRK_OK;
}
void st_free_tables(StHandle* h);  // wt, state, d_layers, d_preps
// push: the checks both families make, then the per-push fields of p (a copy of the handle's block) and its tables
template <class P>
int st_push_args(const StHandle* h, P& p, const float* x, int ldx, const float* dec_cond, int ldd, const float* enc_cond, int lde,
                 const long long* spk, const int* n_valid, int S, int C, float* decoded, long long* const* qidx,
                 float* const* encoded) {
  if (S < 1 || S > h->S || C < 1 || C > h->Cmax) return CRK_ERR_UNSUPPORTED;
  if (!h->prepared || !x || !spk || !decoded || !qidx || !encoded || ldx < p.enc[0].in_ch) return CRK_ERR_ARG;
  if ((p.dec_f0 && (!dec_cond || ldd < 2)) || (p.enc_f0 && (!enc_cond || lde < 2))) return CRK_ERR_ARG;
  for (int n = 0; n < p.nst; n++) {
    if (!qidx[n] || !encoded[n]) return CRK_ERR_ARG;
    p.qidx[n] = qidx[n]; p.encoded[n] = encoded[n];
  }
  p.layers = h->d_layers; p.wt = h->wt; p.state = h->state;
  p.x = x; p.ldx = ldx; p.dcond = dec_cond; p.ldd = ldd; p.econd = enc_cond; p.lde = lde; p.spk = spk; p.n_valid = n_valid;
  p.C = C; p.decoded = decoded;
  return CRK_OK;
}
