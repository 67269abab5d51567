// Streaming conversion for causal generators (gfx950): ONE launch runs the whole generator forward of
// crank/net/module/vqvae2.py:160-190 - encoders, "enc[n] + dec", codebook search and lookup, decoders, the last decoder on
// cat[q_top .. q_0] with its conditioning - for a chunk of new frames of S independent streams, carrying each dilated
// convolution's history between launches.
//
// Decomposition.  With use_causal_conv no frame needs a later one and no stream another stream's data, so workgroup s owns
// stream s: it walks every layer of every stack with the chunk's activations in LDS (tiles of ST_TILE frames; a longer push
// is a loop over tiles inside the launch, the state handing one tile's history to the next).  No grid-wide synchronisation.
//
// State.  Residual layer l of a stack keeps the last halo_l = (k - 1) * dil_l frames of ITS INPUT, per stream, zero at
// reset - the left zero padding of the reference's causal convolution (ResidualBlock: padding = (k-1)*dil, output cut to
// the input's length).  One buffer [stream][layer][frame][64 channels]; a push reads a layer's rows in front of the tile's
// frames and writes back the last halo_l rows of (old state | the n_valid new frames): a push shorter than the halo shifts.
//
// Arithmetic: fp32 throughout, every multiply-add an explicit fmaf, contraction off for the rest of the file.  An output
// element is bias + one chain of fmaf over (tap, input channel) in ascending order whatever thread, tile or chunk computes
// it, so a frame's result does not depend on where it sits in a chunk or how long the chunk is, bit for bit.  Weight norm is
// applied once per parameter version by stream_prepare_kernel into a table of effective fp32 weights laid out
// [tap][input channel (padded to 4)][output channel]: a thread owns an output channel, its weight loads are coalesced and
// the frame rows are LDS broadcasts.  (The nets' own prepared tables hold bf16 hi / lo planes in MFMA fragment order: not
// what an fp32 chain reads.)  The codebook search is built from the device bodies of vq_common.h - the ones every search
// kernel of vq_kernels.hip is built from: norms, dot product, distance, (distance, then index) order, NaN pin and
// straight-through value - so the indices are crk_vq_forward's on the same rows by construction.
//
// Host side.  This file defines, once, what the entry points of this family and of stream_la_kernels.hip are made of and
// stream_common.h declares: the table builder, the descriptor check, the first reserve's tables, the zeroed per-stream
// buffer, the prepare launch, the common frees.  crk_stream_* at the end is that plus StP and the launch.
#include "stream_common.h"

struct StP {
  StNet enc[ST_MAX_STACKS], dec[ST_MAX_STACKS];
  int nst, emb_dim[ST_MAX_STACKS], emb_size[ST_MAX_STACKS];
  long long cb_off[ST_MAX_STACKS], spk_off, state_stride;
  int enc_f0, dec_f0, spk_dim, spk_onehot, n_spk;
  const StLayer* layers;
  const float* wt;
  const float* params;
  float* state;
  const float* x; int ldx;
  const float* dcond; int ldd;
  const float* econd; int lde;
  const long long* spk;
  const int* n_valid;
  int C;
  float* decoded;
  long long* qidx[ST_MAX_STACKS];
  float* encoded[ST_MAX_STACKS];
};


// ------------------------------------------------------------------------------------------------------------ prepare
// One wave per output row: ||v|| from lane-strided partial sums met in a fixed order, w = v * (g / ||v||) as
// torch._weight_norm forms it, stored transposed.  The padded input channels of the table stay zero from the reserve.
__global__ __launch_bounds__(64) void stream_prepare_kernel(const StPrep* __restrict__ preps, int nprep,
                                                            const float* __restrict__ params, float* __restrict__ wt) {
  const int row = blockIdx.x, lane = threadIdx.x;
  int c = 0;
  while (c + 1 < nprep && preps[c + 1].row0 <= row) c++;
  const StPrep q = preps[c];
  const int r = row - q.row0;
  if (r >= q.cout) return;
  const int n = q.cin * q.k;
  const float* v = params + q.off_v + (long long)r * n;
  float ss = 0.f;
  for (int i = lane; i < n; i += 64) ss = fmaf(v[i], v[i], ss);
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float scale = params[q.off_g + r] / sqrtf(ss);
  for (int i = lane; i < n; i += 64) {
    const int ci = i / q.k, j = i - ci * q.k;
    wt[q.w_off + ((long long)j * q.cin_pad + ci) * q.ld + q.col0 + r] = v[i] * scale;
  }
}


// One PWG generator stack (oracle/pwg.py ParallelWaveGANGenerator.forward, use_causal_conv) on nv frames: `in` (row stride
// ST_LD, n.in_pad columns) -> m.io (n.out_ch columns).  cond: the conditioning rows (n.aux_pad columns) when n.aux_ch > 0.
template <int FT>
__device__ void st_net(const StP& p, const StNet& n, int s, const float* in, int nv, const StLds& m) {
  const float* P = p.params;
  const float* W = p.wt;
  const int tid = threadIdx.x;
  float* xc = m.xw + ST_HALO * 64;  // frame 0 of the residual stream; the layer's history sits in the rows in front of it
  float* g = m.g;
  float* skip = m.skip;
  st_dense<FT>(W + n.w_first, 64, n.in_pad, 1, 1, in, ST_LD, nv,
               [&](int f, int co, float a) { xc[f * 64 + co] = P[n.b_first + co] + a; });
  for (int i = tid; i < nv * 64; i += ST_THREADS) skip[i] = 0.f;
  __syncthreads();
  for (int l = 0; l < n.L; l++) {
    const StLayer y = p.layers[n.layer0 + l];
    float* st = p.state + (long long)s * p.state_stride + y.state_off;
    const int hl = y.halo * 64;
    for (int i = tid; i < hl; i += ST_THREADS) xc[i - hl] = st[i];
    __syncthreads();
    st_dense<FT>(W + y.w_conv, 128, 64, n.k, y.dil, xc, 64, nv,
                 [&](int f, int co, float a) { g[f * ST_LD + co] = (y.b_conv >= 0 ? P[y.b_conv + co] : 0.f) + a; });
    if (n.aux_ch > 0)  // (the same thread owns (f, co) in both calls)
      st_dense<FT>(W + y.w_aux, 128, n.aux_pad, 1, 1, m.cond, ST_LD, nv,
                   [&](int f, int co, float a) { g[f * ST_LD + co] += a; });
    // the layer's next history: the last halo rows of (old state | the nv new frames)
    for (int i = tid; i < hl; i += ST_THREADS) st[i] = xc[nv * 64 - hl + i];
    __syncthreads();
    st_gate(g, nv);
    __syncthreads();
    // [out | skip] as one 128-wide conv of z: residual (out + x) * sqrt(.5), skip sum
    st_dense<FT>(W + y.w_os, 128, 64, 1, 1, g, ST_LD, nv, [&](int f, int co, float a) {
      if (co < 64)
        st_residual(&xc[f * 64 + co], P, y.b_out, co, a, &xc[f * 64 + co]);
      else
        skip[f * 64 + co - 64] += st_skip_term(P, y.b_skip, co, a);
    });
    __syncthreads();
  }
  for (int i = tid; i < nv * 64; i += ST_THREADS) g[(i >> 6) * ST_LD + (i & 63)] = fmaxf(skip[i] * n.skip_scale, 0.f);
  __syncthreads();
  st_last<FT>(W, P, n, g, skip, nv, m);
}


// frames [r0, r0 + nv) of stream s (rows of the caller's (S, C, .) tensors): vqvae2.py:160-190
template <int FT>
__device__ void st_tile(const StP& p, int s, long long r0, int nv, const StLds& m) {
  const int tid = threadIdx.x;
  const float* P = p.params;
  st_load_input(p, r0, nv, m, [](int) { return true; });  // (every row of a causal tile has an input frame)
  if (p.enc_f0)
    for (int i = tid; i < nv * 4; i += ST_THREADS) {
      const int f = i >> 2, c = i & 3;
      m.cond[f * ST_LD + c] = c < 2 ? p.econd[(r0 + f) * p.lde + c] : 0.f;
    }
  __syncthreads();
  for (int n = 0; n < p.nst; n++) {
    st_net<FT>(p, p.enc[n], s, m.io, nv, m);
    const int D = p.emb_dim[n];
    for (int i = tid; i < nv * D; i += ST_THREADS) {
      const int f = i / D, c = i - f * D;
      p.encoded[n][(r0 + f) * D + c] = m.io[f * ST_LD + c];
    }
    __syncthreads();
  }
  // the quantized rows side by side in m.cond, top stack first: the last decoder's input
  int col = 0;
  for (int n = p.nst - 1; n >= 0; n--) {
    const int D = p.emb_dim[n];
    for (int i = tid; i < nv * D; i += ST_THREADS) {
      const int f = i / D, c = i - f * D;
      float v = p.encoded[n][(r0 + f) * D + c];
      if (n != p.nst - 1) v = v + m.io[f * ST_LD + c];  // enc[n] + dec (the top stack adds the integer 0)
      p.encoded[n][(r0 + f) * D + c] = v;
      m.g[f * ST_LD + c] = v;
    }
    __syncthreads();
    const float* cb = P + p.cb_off[n];
    if (D == 64) st_vq<64>(cb, p.emb_size[n], m.g, nv, m);
    else if (D == 32) st_vq<32>(cb, p.emb_size[n], m.g, nv, m);
    else if (D == 16) st_vq<16>(cb, p.emb_size[n], m.g, nv, m);
    else st_vq<128>(cb, p.emb_size[n], m.g, nv, m);
    for (int i = tid; i < nv * D; i += ST_THREADS) {
      const int f = i / D, c = i - f * D;
      const float e = cb[(size_t)m.idxs[f] * D + c], x = m.g[f * ST_LD + c];
      m.cond[f * ST_LD + col + c] = vq_st(x, e);
    }
    if (tid < nv) p.qidx[n][r0 + tid] = (long long)m.idxs[tid];
    __syncthreads();
    if (n != 0) st_net<FT>(p, p.dec[n], s, m.cond + col, nv, m);
    col += D;
  }
  for (int i = tid; i < nv * col; i += ST_THREADS) {
    const int f = i / col, c = i - f * col;
    m.io[f * ST_LD + c] = m.cond[f * ST_LD + c];
  }
  __syncthreads();
  {
    const int ap = p.dec[0].aux_pad;
    long long spk = p.spk[s];
    spk = spk < 0 ? 0 : (spk >= p.n_spk ? p.n_spk - 1 : spk);
    for (int i = tid; i < nv * ap; i += ST_THREADS) {
      const int f = i / ap, c = i - f * ap, e = c - p.dec_f0;
      float v = 0.f;
      if (c < p.dec_f0) v = p.dcond[(r0 + f) * p.ldd + c];
      else if (e < p.spk_dim) v = st_spk_value(p, P, spk, e);
      m.cond[f * ST_LD + c] = v;
    }
  }
  __syncthreads();
  st_net<FT>(p, p.dec[0], s, m.io, nv, m);
  const int oc = p.dec[0].out_ch;
  for (int i = tid; i < nv * oc; i += ST_THREADS) {
    const int f = i / oc, c = i - f * oc;
    p.decoded[(r0 + f) * oc + c] = m.io[f * ST_LD + c];
  }
  __syncthreads();
}

__global__ __launch_bounds__(ST_THREADS) void stream_push_kernel(const StP p) {
  extern __shared__ __attribute__((aligned(16))) float st_lds[];
  const StLds m = st_carve(st_lds);
  const int s = blockIdx.x;
  int total = p.n_valid ? p.n_valid[s] : p.C;
  total = min(max(total, 0), p.C);
  for (int t0 = 0; t0 < total; t0 += ST_TILE) {
    const int nv = min(ST_TILE, total - t0);
    const long long r0 = (long long)s * p.C + t0;
    // (two run lengths of the same per-element chains: a short tile does not pay for eight frames per thread)
    if (nv > 8) st_tile<8>(p, s, r0, nv, m);
    else st_tile<2>(p, s, r0, nv, m);
  }
}

// ------------------------------------------------------------------------------------------------------------ host
struct StreamH : StHandle { StP p; };

// ---- what both families' entry points are made of (stream_common.h)
int st_malloc(void** q, size_t bytes) {
  if (hipMalloc(q, bytes) != hipSuccess) return CRK_ERR_HIP;
  crk_count_alloc_();
  return CRK_OK;
}

int st_add_net(StTables* h, void* net, long long base, int in_ch, int out_ch, int aux_ch, StNet* out) {
  if (!net || in_ch < 1 || in_ch > 128 || out_ch < 1 || out_ch > 128 || aux_ch < 0 || aux_ch > 128) return CRK_ERR_UNSUPPORTED;
  StNet n;
  memset(&n, 0, sizeof(n));
  n.in_ch = in_ch; n.in_pad = st_pad4(in_ch); n.out_ch = out_ch; n.aux_ch = aux_ch; n.aux_pad = st_pad4(aux_ch);
  n.layer0 = (int)h->layers.size();
  auto table = [&](int cout, int cin, int k) {
    const long long o = h->wt_floats;
    h->wt_floats += (long long)k * st_pad4(cin) * cout;
    return o;
  };
  auto prep = [&](const long long* c, long long w_off, int ld, int col0) {
    StPrep q;
    q.off_g = base + c[4]; q.off_v = base + c[5]; q.w_off = w_off; q.row0 = h->rows; q.cout = (int)c[0]; q.cin = (int)c[1];
    q.cin_pad = st_pad4(q.cin); q.k = (int)c[2]; q.ld = ld; q.col0 = col0;
    h->rows += q.cout;
    h->preps.push_back(q);
  };
  auto bias = [&](const long long* c) { return c[3] >= 0 ? base + c[3] : -1ll; };
  const int count = crk_net_conv_count(net);
  bool first = false, last1 = false, last2 = false;
  for (int i = 0; i < count; i++) {
    long long c[9];
    if (crk_net_conv_info(net, i, c) != CRK_OK) return CRK_ERR_ARG;
    const int cout = (int)c[0], cin = (int)c[1], k = (int)c[2], dil = (int)c[6], role = (int)c[7], layer = (int)c[8];
    if (role == ST_ROLE_CONV) {
      if (layer != (int)h->layers.size() - n.layer0 || cout != 128 || cin != 64 || k < 1 || k > 5 || (k - 1) * dil > ST_HALO)
        return CRK_ERR_UNSUPPORTED;
      StLayer y;
      memset(&y, 0, sizeof(y));
      y.dil = dil; y.halo = (k - 1) * dil; y.state_off = h->state_floats; h->state_floats += (long long)y.halo * 64;
      y.w_conv = table(128, 64, k); y.b_conv = bias(c); y.w_aux = -1; y.w_os = -1;
      prep(c, y.w_conv, 128, 0);
      n.k = k;
      h->layers.push_back(y);
      continue;
    }
    if (role == ST_ROLE_AUX || role == ST_ROLE_OUT || role == ST_ROLE_SKIP) {
      if (h->layers.empty() || layer != (int)h->layers.size() - n.layer0 - 1 || k != 1) return CRK_ERR_UNSUPPORTED;
      StLayer& y = h->layers.back();
      if (role == ST_ROLE_AUX) {
        if (cout != 128 || cin != aux_ch) return CRK_ERR_UNSUPPORTED;
        y.w_aux = table(128, cin, 1);
        prep(c, y.w_aux, 128, 0);
      } else {
        if (cout != 64 || cin != 64) return CRK_ERR_UNSUPPORTED;
        if (y.w_os < 0) y.w_os = table(128, 64, 1);
        (role == ST_ROLE_OUT ? y.b_out : y.b_skip) = bias(c);
        prep(c, y.w_os, 128, role == ST_ROLE_OUT ? 0 : 64);
      }
      continue;
    }
    if (k != 1 || c[3] < 0) return CRK_ERR_UNSUPPORTED;
    if (role == ST_ROLE_FIRST && cout == 64 && cin == in_ch) {
      n.w_first = table(64, cin, 1); n.b_first = bias(c); prep(c, n.w_first, 64, 0); first = true;
    } else if (role == ST_ROLE_LAST1 && cout == 64 && cin == 64) {
      n.w_last1 = table(64, 64, 1); n.b_last1 = bias(c); prep(c, n.w_last1, 64, 0); last1 = true;
    } else if (role == ST_ROLE_LAST2 && cout == out_ch && cin == 64) {
      n.w_last2 = table(cout, 64, 1); n.b_last2 = bias(c); prep(c, n.w_last2, cout, 0); last2 = true;
    } else {
      return CRK_ERR_UNSUPPORTED;
    }
  }
  n.L = (int)h->layers.size() - n.layer0;
  if (!first || !last1 || !last2 || n.L < 1) return CRK_ERR_UNSUPPORTED;
  for (int l = 0; l < n.L; l++) {
    const StLayer& y = h->layers[n.layer0 + l];
    if (y.w_os < 0 || (aux_ch > 0) != (y.w_aux >= 0)) return CRK_ERR_UNSUPPORTED;
  }
  n.skip_scale = (float)sqrt(1.0 / n.L);
  *out = n;
  return CRK_OK;
}

int st_check_desc(const crk_stream_desc* d_, void* const* enc_nets, void* const* dec_nets, void** handle, bool causal, int* qsum_,
                  int* d_aux_) {
  if (!d_ || !enc_nets || !dec_nets || !handle) return CRK_ERR_ARG;
  *handle = nullptr;
  const crk_stream_desc& d = *d_;
  if (d.n_stacks < 1 || d.n_stacks > ST_MAX_STACKS || (d.causal != 0) != causal) return CRK_ERR_UNSUPPORTED;
  int qsum = 0;
  for (int n = 0; n < d.n_stacks; n++) {
    const int D = d.emb_dim[n];
    if ((D != 16 && D != 32 && D != 64 && D != 128) || d.emb_size[n] < 1 || d.cb_off[n] < 0) return CRK_ERR_UNSUPPORTED;
    qsum += D;
  }
  const int d_aux = (d.dec_f0 ? 2 : 0) + d.spk_dim;
  if (qsum > 128 || d.spk_dim < 0 || d_aux > 128 || d.n_spk < 1 || (d.spk_onehot && d.spk_dim != d.n_spk) ||
      (!d.spk_onehot && d.spk_dim > 0 && d.spk_off < 0))
    return CRK_ERR_UNSUPPORTED;
  *qsum_ = qsum; *d_aux_ = d_aux;
  return CRK_OK;
}

int st_reserve_tables(StHandle* h, int S, int C_max) {
  if (!h) return CRK_ERR_ARG;
  if (S < 1 || C_max < 1 || C_max > ST_MAX_CHUNK) return CRK_ERR_UNSUPPORTED;
  if (h->wt) return CRK_OK;
  int rc = st_malloc((void**)&h->wt, sizeof(float) * h->wt_floats);
  if (rc == CRK_OK) rc = st_malloc((void**)&h->d_layers, sizeof(StLayer) * h->layers.size());
  if (rc == CRK_OK) rc = st_malloc((void**)&h->d_preps, sizeof(StPrep) * h->preps.size());
  if (rc != CRK_OK) return rc;
  if (hipMemset(h->wt, 0, sizeof(float) * h->wt_floats) != hipSuccess ||
      hipMemcpy(h->d_layers, h->layers.data(), sizeof(StLayer) * h->layers.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_preps, h->preps.data(), sizeof(StPrep) * h->preps.size(), hipMemcpyHostToDevice) != hipSuccess)
    return CRK_ERR_HIP;
  return CRK_OK;
}

int st_zeroed(void** q, size_t bytes) {
  *q = nullptr;
  const int rc = st_malloc(q, bytes);
  if (rc != CRK_OK) return rc;
  if (hipMemset(*q, 0, bytes) == hipSuccess) return CRK_OK;
  (void)hipFree(*q);
  *q = nullptr;
  return CRK_ERR_HIP;
}

void st_free_tables(StHandle* h) {
  (void)hipFree(h->wt); (void)hipFree(h->state); (void)hipFree(h->d_layers); (void)hipFree(h->d_preps);
}

int st_prepare_launch(const StPrep* d_preps, int nprep, int rows, const float* params, float* wt, void* stream) {
  hipLaunchKernelGGL(stream_prepare_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, d_preps, nprep, params, wt);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

// ---- the causal family's entry points
extern "C" int crk_stream_create(const crk_stream_desc* desc, void* const* enc_nets, void* const* dec_nets, void** handle) {
  int qsum, d_aux;
  int rc = st_check_desc(desc, enc_nets, dec_nets, handle, true, &qsum, &d_aux);
  if (rc != CRK_OK) return rc;
  StreamH* h = new StreamH();
  rc = st_fill_model(h, h->p, *desc, enc_nets, dec_nets, qsum, d_aux);
  if (rc != CRK_OK) { delete h; return rc; }
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_stream_destroy(void* hh) {
  StreamH* h = (StreamH*)hh;
  if (!h) return;
  st_free_tables(h);
  delete h;
}

extern "C" long long crk_stream_state_bytes(void* hh, int S) {
  StreamH* h = (StreamH*)hh;
  return (!h || S < 0) ? -1 : (long long)S * h->state_floats * 4;
}

extern "C" int crk_stream_reserve(void* hh, int S, int C_max) {
  StreamH* h = (StreamH*)hh;
  int rc = st_reserve_tables(h, S, C_max);
  if (rc == CRK_OK) rc = crk_raise_lds((int)st_lds_bytes(), stream_push_kernel);
  if (rc != CRK_OK) return rc;
  if (S > h->S) {  // more streams: a new, zeroed state (every stream starts over)
    float* st;
    rc = st_zeroed((void**)&st, sizeof(float) * h->state_floats * S);
    if (rc != CRK_OK) return rc;
    (void)hipFree(h->state);
    h->state = st; h->S = S;
  }
  if (C_max > h->Cmax) h->Cmax = C_max;
  return CRK_OK;
}

extern "C" int crk_stream_prepare(void* hh, const float* params, unsigned long long version, void* stream) {
  StreamH* h = (StreamH*)hh;
  (void)version;  // (the caller's bookkeeping: one call per parameter version)
  return h ? st_prepare(h, h->p, params, stream) : CRK_ERR_ARG;
}

extern "C" int crk_stream_reset(void* hh, const int* stream_ids, int n, void* stream) {
  StreamH* h = (StreamH*)hh;
  if (!h) return CRK_ERR_ARG;
  return crk_zero_stream_rows(h->state, sizeof(float) * h->state_floats, h->S, stream_ids, n, (hipStream_t)stream);
}

extern "C" int crk_stream_push(void* hh, const float* x, int ldx, const float* dec_cond, int ldd, const float* enc_cond, int lde,
                               const long long* spk, const int* n_valid, int S, int C, float* decoded,
                               long long* const* qidx, float* const* encoded, void* stream) {
  StreamH* h = (StreamH*)hh;
  if (!h) return CRK_ERR_ARG;
  StP p = h->p;
  const int rc = st_push_args(h, p, x, ldx, dec_cond, ldd, enc_cond, lde, spk, n_valid, S, C, decoded, qidx, encoded);
  if (rc != CRK_OK) return rc;
  hipLaunchKernelGGL(stream_push_kernel, dim3(S), dim3(ST_THREADS), st_lds_bytes(), (hipStream_t)stream, p);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
