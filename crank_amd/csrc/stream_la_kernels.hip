// Look-ahead streaming conversion for non-causal generators (gfx950): the generator forward of crank/net/module/vqvae2.py:160-190
// - encoders, "enc[n] + dec", codebook search and lookup, decoders - followed at a fixed delay of LA = (receptive chain) / 2
// frames behind its input, for chunks of new frames of S independent streams, ONE launch per push, one workgroup per stream
// as in stream_kernels.hip.  What comes out is the offline forward of the whole utterance.
//
// Slots.  A non-causal residual block pads h = (k - 1) / 2 * dil zeros on both sides: it is the causal block with its output
// moved h frames back.  So every layer is walked over the same slots as in the causal kernel - slot u of a stream is its
// u-th step since the utterance began, T slots have received an input frame - and layer l's output at slot u is frame
// u - delay_l, delay_l the sum of h over the layer and every layer before it in the chain enc[0] .. enc[top], dec[top] ..
// dec[0].  The decoded row of frame t leaves at slot t + LA.  A push with the end flag runs LA more slots on zero input.
//
// Against the causal body: (1) the residual add takes the layer's input of the same frame, h rows back in the tile (the
// carried history is 2 h rows: the row is in LDS), and goes through the gate tile's free half because the rows it reads are
// rows other threads write; (2) a row whose frame lies outside [0, E) - E the utterance's length, out of reach until the
// end flag - is zero wherever a layer reads it: the first conv's output and every residual output are masked by position;
// (3) what meets a delayed layer per frame waits in per-stream rings in global memory, [stream][ring][frame mod capacity]
// [row]: conditioning rows with the speaker of the push that delivered the frame, each net's partially summed skip rows
// (layers add to a frame's row in layer order, so the order of additions per element is the offline one), enc[n] until
// dec[n + 1] of the frame arrives, the quantized rows of the upper stacks until the bottom one does, encoded[n] and qidx[n]
// until the decoded row exists.  A ring written at delay a and read at delay b holds 64 + b - a rows (a tile is at most 64 slots).
// Rings are never cleared: a frame in [0, E) is written before it is read, frames outside are not read.
//
// Arithmetic: the device bodies of stream_common.h and vq_common.h, fp32, one fmaf chain per output element in (tap, input
// channel) order: a frame's bits do not depend on how the utterance is cut into pushes.
//
// Host side: StHandle and the shared functions of stream_common.h (defined in stream_kernels.hip); this file adds the
// delays and ring layout at create, the rings and frame counters at reserve / reset, and its own push arguments.
#include <limits.h>

#include "stream_common.h"

struct LaRing { long long off; int cap, width; };  // off: floats from the stream's ring block

struct LaP {
  StNet enc[ST_MAX_STACKS], dec[ST_MAX_STACKS];
  int nst, emb_dim[ST_MAX_STACKS], emb_size[ST_MAX_STACKS];
  long long cb_off[ST_MAX_STACKS], spk_off, state_stride, ring_stride;
  int enc_f0, dec_f0, spk_dim, spk_onehot, n_spk, la;
  // skip rows of enc[n] / dec[n]; enc[n]'s output waiting for dec[n + 1]; quantized rows of stack n >= 1 waiting for stack 0;
  // encoded[n] / qidx[n] waiting for the decoded row; the conditioning rows [c0, c1, speaker (int bits), 0] of dec[0] / enc[0]
  LaRing r_skip_e[ST_MAX_STACKS], r_skip_d[ST_MAX_STACKS], r_wait[ST_MAX_STACKS], r_q[ST_MAX_STACKS], r_enc[ST_MAX_STACKS],
      r_idx[ST_MAX_STACKS], r_cd, r_ce;
  const StLayer* layers;
  const float* wt;
  const float* params;
  float* state;
  float* rings;
  int* count;  // [stream]: T, the slots that have received a frame since the utterance began
  const float* x; int ldx;
  const float* dcond; int ldd;
  const float* econd; int lde;
  const long long* spk;
  const int* n_valid;
  const int* end;
  int C, rows_out;
  float* decoded;
  long long* qidx[ST_MAX_STACKS];
  float* encoded[ST_MAX_STACKS];
  int *n_out, *first;
};

// one tile of one stream: slots [u0, u0 + nv), the utterance's length E (INT_MAX: not in reach), whether the carried
// history is to be left zero behind the tile (the last tile of an end push), the stream's ring block
struct LaTile { int s, u0, nv, E; bool last; float* rings; };

__device__ __forceinline__ bool la_in(int fr, int E) { return fr >= 0 && fr < E; }
__device__ __forceinline__ float* la_row(const LaTile& t, const LaRing& r, int fr) {
  return t.rings + r.off + (long long)(fr % r.cap) * r.width;
}

// One PWG generator stack without use_causal_conv (oracle/pwg.py ParallelWaveGANGenerator.forward) on the tile's slots:
// `in` (row stride ST_LD, n.in_pad columns), whose row f is frame u0 + f - delay -> m.io (n.out_ch columns), whose row f is
// frame u0 + f - (delay + the stack's sum of h); delay is moved on.  cond: the ring of the stack's conditioning rows when
// n.aux_ch > 0 (f0_cols of them lcf0 / uv, the rest the speaker's).
// (Inlined, like la_tile: out of line they would take the launch parameters by reference, which puts all of LaP - ring
// descriptors included - into scratch memory and makes every p.<field> a scratch load.)
template <int FT>
__device__ __forceinline__ void la_net(const LaP& p, const StNet& n, const LaTile& t, const float* in, const StLds& m, int& delay,
                       const LaRing& rskip, const LaRing& rcond, int f0_cols, bool speaker) {
  const float* P = p.params;
  const float* W = p.wt;
  const int tid = threadIdx.x, nv = t.nv;
  float* xc = m.xw + ST_HALO * 64;  // slot u0 of the residual stream; the layer's history sits in the rows in front of it
  float* g = m.g;
  {
    const int d0 = delay;  // (a tap outside the utterance is 0, not first_conv(0))
    st_dense<FT>(W + n.w_first, 64, n.in_pad, 1, 1, in, ST_LD, nv, [&](int f, int co, float a) {
      xc[f * 64 + co] = la_in(t.u0 + f - d0, t.E) ? P[n.b_first + co] + a : 0.f;
    });
  }
  __syncthreads();
  for (int l = 0; l < n.L; l++) {
    const StLayer y = p.layers[n.layer0 + l];
    float* st = p.state + (long long)t.s * p.state_stride + y.state_off;
    const int hl = y.halo * 64, h = y.halo / 2;
    const int out0 = t.u0 - (delay + h);  // the frame of the layer's output at the tile's first slot
    for (int i = tid; i < hl; i += ST_THREADS) xc[i - hl] = st[i];
    if (n.aux_ch > 0) {
      const int ap = n.aux_pad;
      for (int i = tid; i < nv * ap; i += ST_THREADS) {
        const int f = i / ap, c = i - f * ap, e = c - f0_cols, fr = out0 + f;
        float v = 0.f;
        if (la_in(fr, t.E)) {
          const float* row = la_row(t, rcond, fr);
          if (c < f0_cols) {
            v = row[c];
          } else if (speaker && e < p.spk_dim) {
            const int spk = __float_as_int(row[2]);
            v = st_spk_value(p, P, spk, e);
          }
        }
        m.cond[f * ST_LD + c] = v;
      }
    }
    __syncthreads();
    st_dense<FT>(W + y.w_conv, 128, 64, n.k, y.dil, xc, 64, nv,
                 [&](int f, int co, float a) { g[f * ST_LD + co] = (y.b_conv >= 0 ? P[y.b_conv + co] : 0.f) + a; });
    if (n.aux_ch > 0)  // (the same thread owns (f, co) in both calls)
      st_dense<FT>(W + y.w_aux, 128, n.aux_pad, 1, 1, m.cond, ST_LD, nv,
                   [&](int f, int co, float a) { g[f * ST_LD + co] += a; });
    // the layer's next history: the last halo rows of (old state | the nv new slots); zero behind an utterance's last slot
    for (int i = tid; i < hl; i += ST_THREADS) st[i] = t.last ? 0.f : xc[nv * 64 - hl + i];
    __syncthreads();
    st_gate(g, nv);
    __syncthreads();
    // [out | skip] as one 128-wide conv of z.  The residual takes the layer's input h rows back - rows this call's other
    // threads would overwrite - so it is parked in the gate tile's b half, which the conv does not read.
    st_dense<FT>(W + y.w_os, 128, 64, 1, 1, g, ST_LD, nv, [&](int f, int co, float a) {
      const bool in_utt = la_in(out0 + f, t.E);
      if (co < 64) {
        if (in_utt) st_residual(&g[f * ST_LD + 64 + co], P, y.b_out, co, a, &xc[(f - h) * 64 + co]);
        else g[f * ST_LD + 64 + co] = 0.f;
      } else if (in_utt) {
        float* sk = la_row(t, rskip, out0 + f) + co - 64;
        *sk = (l == 0 ? 0.f : *sk) + st_skip_term(P, y.b_skip, co, a);
      }
    });
    __syncthreads();
    for (int i = tid; i < nv * 64; i += ST_THREADS) xc[i] = g[(i >> 6) * ST_LD + 64 + (i & 63)];
    __syncthreads();
    delay += h;
  }
  for (int i = tid; i < nv * 64; i += ST_THREADS) {
    const int f = i >> 6, fr = t.u0 + f - delay;
    g[f * ST_LD + (i & 63)] = la_in(fr, t.E) ? fmaxf(la_row(t, rskip, fr)[i & 63] * n.skip_scale, 0.f) : 0.f;
  }
  __syncthreads();
  st_last<FT>(W, P, n, g, m.skip, nv, m);
}

// slots [t.u0, t.u0 + t.nv) of stream t.s; the first n_in of them take rows [r0, r0 + n_in) of the caller's inputs, the
// rest zero input (the flush); first_out: the frame of row 0 of the stream's outputs
template <int FT>
__device__ __forceinline__ void la_tile(const LaP& p, const LaTile& t, long long r0, int n_in, int first_out, const StLds& m) {
  const int tid = threadIdx.x, nv = t.nv;
  const float* P = p.params;
  const LaRing none = {0, 1, 0};
  st_load_input(p, r0, nv, m, [&](int f) { return f < n_in; });
  {
    // the frames' conditioning rows, with the speaker of this push
    long long spk = p.spk[t.s];
    spk = spk < 0 ? 0 : (spk >= p.n_spk ? p.n_spk - 1 : spk);
    for (int i = tid; i < n_in * 4; i += ST_THREADS) {
      const int f = i >> 2, c = i & 3;
      float v = 0.f;
      if (c < p.dec_f0) v = p.dcond[(r0 + f) * p.ldd + c];
      else if (c == 2) v = __int_as_float((int)spk);
      la_row(t, p.r_cd, t.u0 + f)[c] = v;
      if (p.enc_f0) la_row(t, p.r_ce, t.u0 + f)[c] = c < 2 ? p.econd[(r0 + f) * p.lde + c] : 0.f;
    }
  }
  __syncthreads();
  int delay = 0;
  for (int n = 0; n < p.nst; n++) {
    la_net<FT>(p, p.enc[n], t, m.io, m, delay, p.r_skip_e[n], n == 0 ? p.r_ce : none, 2, false);
    if (n != p.nst - 1) {  // enc[n] waits for dec[n + 1] of the same frame
      const int D = p.emb_dim[n];
      for (int i = tid; i < nv * D; i += ST_THREADS) {
        const int f = i / D, c = i - f * D, fr = t.u0 + f - delay;
        if (la_in(fr, t.E)) la_row(t, p.r_wait[n], fr)[c] = m.io[f * ST_LD + c];
      }
      __syncthreads();
    }
  }
  for (int n = p.nst - 1; n >= 0; n--) {
    const int D = p.emb_dim[n];
    for (int i = tid; i < nv * D; i += ST_THREADS) {
      const int f = i / D, c = i - f * D, fr = t.u0 + f - delay;
      float v = 0.f;
      if (la_in(fr, t.E)) {
        v = m.io[f * ST_LD + c];
        if (n != p.nst - 1) v = la_row(t, p.r_wait[n], fr)[c] + v;  // enc[n] + dec (the top stack adds the integer 0)
        la_row(t, p.r_enc[n], fr)[c] = v;
      }
      m.g[f * ST_LD + c] = v;
    }
    __syncthreads();
    const float* cb = P + p.cb_off[n];
    if (D == 64) st_vq<64>(cb, p.emb_size[n], m.g, nv, m);
    else if (D == 32) st_vq<32>(cb, p.emb_size[n], m.g, nv, m);
    else if (D == 16) st_vq<16>(cb, p.emb_size[n], m.g, nv, m);
    else st_vq<128>(cb, p.emb_size[n], m.g, nv, m);
    if (n != 0) {
      for (int i = tid; i < nv * D; i += ST_THREADS) {
        const int f = i / D, c = i - f * D, fr = t.u0 + f - delay;
        const float q = vq_st(m.g[f * ST_LD + c], cb[(size_t)m.idxs[f] * D + c]);
        m.cond[f * ST_LD + c] = q;
        if (la_in(fr, t.E)) la_row(t, p.r_q[n], fr)[c] = q;
      }
    } else {
      // the last decoder's input: the quantized rows of the frame side by side, top stack first, the upper ones from
      // their rings
      int col = 0;
      for (int u = p.nst - 1; u >= 1; u--) {
        const int Du = p.emb_dim[u];
        for (int i = tid; i < nv * Du; i += ST_THREADS) {
          const int f = i / Du, c = i - f * Du, fr = t.u0 + f - delay;
          m.io[f * ST_LD + col + c] = la_in(fr, t.E) ? la_row(t, p.r_q[u], fr)[c] : 0.f;
        }
        col += Du;
      }
      for (int i = tid; i < nv * D; i += ST_THREADS) {
        const int f = i / D, c = i - f * D;
        m.io[f * ST_LD + col + c] = vq_st(m.g[f * ST_LD + c], cb[(size_t)m.idxs[f] * D + c]);
      }
    }
    if (tid < nv && la_in(t.u0 + tid - delay, t.E)) *reinterpret_cast<int*>(la_row(t, p.r_idx[n], t.u0 + tid - delay)) = m.idxs[tid];
    __syncthreads();
    if (n != 0) la_net<FT>(p, p.dec[n], t, m.cond, m, delay, p.r_skip_d[n], none, 0, false);
    else la_net<FT>(p, p.dec[0], t, m.io, m, delay, p.r_skip_d[0], p.r_cd, p.dec_f0, true);
  }
  // delay == LA: row f is the decoded row of frame u0 + f - LA; with it leave the frame's encoded rows and indices
  const int oc = p.dec[0].out_ch;
  const long long o0 = (long long)t.s * p.rows_out;
  for (int i = tid; i < nv * oc; i += ST_THREADS) {
    const int f = i / oc, c = i - f * oc, fr = t.u0 + f - delay;
    if (la_in(fr, t.E)) p.decoded[(o0 + fr - first_out) * oc + c] = m.io[f * ST_LD + c];
  }
  for (int n = 0; n < p.nst; n++) {
    const int D = p.emb_dim[n];
    for (int i = tid; i < nv * D; i += ST_THREADS) {
      const int f = i / D, c = i - f * D, fr = t.u0 + f - delay;
      if (la_in(fr, t.E)) p.encoded[n][(o0 + fr - first_out) * D + c] = la_row(t, p.r_enc[n], fr)[c];
    }
    for (int f = tid; f < nv; f += ST_THREADS) {
      const int fr = t.u0 + f - delay;
      if (la_in(fr, t.E)) p.qidx[n][o0 + fr - first_out] = (long long)*reinterpret_cast<const int*>(la_row(t, p.r_idx[n], fr));
    }
  }
  __syncthreads();
}

// la_tile<2> out of line: the launch parameters then reach it by reference, through scratch memory.
__device__ __noinline__ void la_tile_short_call(const LaP& p, const LaTile& t, long long r0, int n_in, int first_out, const StLds& m) {
  la_tile<2>(p, t, r0, n_in, first_out, m);
}

// Two run lengths of the same per-element chains: a tile of more than LA_SHORT slots gives a thread runs of eight, a
// shorter one runs of two, so that it does not pay for eight frames per thread; a frame's bits do not depend on which one
// computed it.  Two instantiations, chosen per push by the host on C alone.  SHORT (C <= LA_SHORT: every tile of a push
// that is no end push is a short one) has both bodies inlined.  The other keeps the eight-slot body inlined and calls the
// two-slot body out of line for a remainder tile.  Each form was measured alone over the whole grid and is used where it
// was the faster one: profiles/stream_lookahead_kernel_forms.txt.
#define LA_SHORT 8
template <bool SHORT>
__global__ __launch_bounds__(ST_THREADS) void stream_la_push_kernel(const LaP p) {
  extern __shared__ __attribute__((aligned(16))) float st_lds[];
  const StLds m = st_carve(st_lds);
  const int s = blockIdx.x;
  int n_in = p.n_valid ? p.n_valid[s] : p.C;
  n_in = min(max(n_in, 0), p.C);
  const bool end = p.end && p.end[s] != 0;
  const int T = p.count[s];
  const int E = end ? T + n_in : INT_MAX;
  // an end flag on a stream that holds nothing flushes nothing: its history is zero already
  const int total = (end && E == 0) ? 0 : n_in + (end ? p.la : 0);
  const int first_out = max(T - p.la, 0);
  LaTile t;
  t.s = s; t.E = E; t.rings = p.rings + (long long)s * p.ring_stride;
  for (int t0 = 0; t0 < total; t0 += ST_TILE) {
    t.nv = min(ST_TILE, total - t0);
    t.u0 = T + t0;
    t.last = end && t0 + ST_TILE >= total;
    const long long r0 = (long long)s * p.C + t0;
    const int tile_in = min(max(n_in - t0, 0), t.nv);
    if (t.nv > LA_SHORT) la_tile<8>(p, t, r0, tile_in, first_out, m);
    else if (SHORT) la_tile<2>(p, t, r0, tile_in, first_out, m);
    else la_tile_short_call(p, t, r0, tile_in, first_out, m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.count[s] = end ? 0 : T + n_in;
    p.n_out[s] = max(min(T + total - p.la, E), 0) - first_out;
    p.first[s] = first_out;
  }
}

// ------------------------------------------------------------------------------------------------------------ host
struct LaStreamH : StHandle {
  LaP p;
  long long ring_floats = 0;
  float* rings = nullptr;
  int* count = nullptr;
};

// sum of h over the layers of one net, and over all but its first layer (what its skip rows wait); -1 for an even kernel
static int la_net_delays(const LaStreamH* h, const StNet& n, int* all, int* tail) {
  *all = *tail = 0;
  if (n.k % 2 == 0) return -1;
  for (int l = 0; l < n.L; l++) {
    const int hh = h->layers[n.layer0 + l].halo / 2;
    *all += hh;
    if (l > 0) *tail += hh;
  }
  return 0;
}

extern "C" int crk_lstream_create(const crk_stream_desc* desc, void* const* enc_nets, void* const* dec_nets, void** handle) {
  int qsum, d_aux;
  int rc = st_check_desc(desc, enc_nets, dec_nets, handle, false, &qsum, &d_aux);
  if (rc != CRK_OK) return rc;
  const crk_stream_desc& d = *desc;
  LaStreamH* h = new LaStreamH();
  LaP& p = h->p;
  const int nst = d.n_stacks;
  rc = st_fill_model(h, p, d, enc_nets, dec_nets, qsum, d_aux);
  // the delays along the chain: a[n] / b[n] the sums of h of enc[n] / dec[n]; quantizer n works at delay at_q[n]
  int a[ST_MAX_STACKS], b[ST_MAX_STACKS], ta[ST_MAX_STACKS], tb[ST_MAX_STACKS], at_q[ST_MAX_STACKS];
  for (int n = 0; n < nst && rc == CRK_OK; n++)
    if (la_net_delays(h, p.enc[n], &a[n], &ta[n]) != 0 || la_net_delays(h, p.dec[n], &b[n], &tb[n]) != 0) rc = CRK_ERR_UNSUPPORTED;
  if (rc != CRK_OK) { delete h; return rc; }
  int delay = 0, after_enc[ST_MAX_STACKS];
  for (int n = 0; n < nst; n++) { delay += a[n]; after_enc[n] = delay; }
  for (int n = nst - 1; n >= 0; n--) { at_q[n] = delay; delay += b[n]; }
  p.la = delay;
  auto ring = [&](int width, int wait) {
    LaRing r;
    r.off = h->ring_floats; r.cap = ST_TILE + wait; r.width = width;
    h->ring_floats += (long long)r.cap * width;
    return r;
  };
  p.r_cd = ring(4, p.la);
  p.r_ce = ring(d.enc_f0 ? 4 : 0, a[0]);
  for (int n = 0; n < nst; n++) {
    p.r_skip_e[n] = ring(64, ta[n]);
    p.r_skip_d[n] = ring(64, tb[n]);
    p.r_wait[n] = n == nst - 1 ? ring(0, 0) : ring(d.emb_dim[n], at_q[n] - after_enc[n]);  // (width 0: a ring nobody uses)
    p.r_q[n] = n == 0 ? ring(0, 0) : ring(d.emb_dim[n], at_q[0] - at_q[n]);
    p.r_enc[n] = ring(d.emb_dim[n], p.la - at_q[n]);
    p.r_idx[n] = ring(1, p.la - at_q[n]);
  }
  p.ring_stride = h->ring_floats;
  *handle = h;
  return CRK_OK;
}

extern "C" void crk_lstream_destroy(void* hh) {
  LaStreamH* h = (LaStreamH*)hh;
  if (!h) return;
  st_free_tables(h);
  (void)hipFree(h->rings); (void)hipFree(h->count);
  delete h;
}

extern "C" int crk_lstream_lookahead(void* hh) {
  LaStreamH* h = (LaStreamH*)hh;
  return h ? h->p.la : -1;
}

extern "C" long long crk_lstream_state_bytes(void* hh, int S) {
  LaStreamH* h = (LaStreamH*)hh;
  return (!h || S < 0) ? -1 : (long long)S * ((h->state_floats + h->ring_floats) * 4 + 4);
}

extern "C" int crk_lstream_reserve(void* hh, int S, int C_max) {
  LaStreamH* h = (LaStreamH*)hh;
  int rc = st_reserve_tables(h, S, C_max);
  if (rc == CRK_OK) rc = crk_raise_lds((int)st_lds_bytes(), stream_la_push_kernel<true>, stream_la_push_kernel<false>);
  if (rc != CRK_OK) return rc;
  if (S > h->S) {  // more streams: a new, zeroed state (every stream starts over); all three buffers or none
    float *st, *rg = nullptr;
    int* cnt = nullptr;
    rc = st_zeroed((void**)&st, sizeof(float) * (size_t)(h->state_floats > 0 ? h->state_floats : 1) * S);
    if (rc == CRK_OK) rc = st_zeroed((void**)&rg, sizeof(float) * h->ring_floats * S);
    if (rc == CRK_OK) rc = st_zeroed((void**)&cnt, sizeof(int) * S);
    if (rc != CRK_OK) {
      (void)hipFree(st); (void)hipFree(rg); (void)hipFree(cnt);
      return rc;
    }
    (void)hipFree(h->state); (void)hipFree(h->rings); (void)hipFree(h->count);
    h->state = st; h->rings = rg; h->count = cnt; h->S = S;
  }
  if (C_max > h->Cmax) h->Cmax = C_max;
  return CRK_OK;
}

extern "C" int crk_lstream_prepare(void* hh, const float* params, unsigned long long version, void* stream) {
  LaStreamH* h = (LaStreamH*)hh;
  (void)version;  // (the caller's bookkeeping: one call per parameter version)
  return h ? st_prepare(h, h->p, params, stream) : CRK_ERR_ARG;
}

extern "C" int crk_lstream_reset(void* hh, const int* stream_ids, int n, void* stream) {
  LaStreamH* h = (LaStreamH*)hh;
  if (!h) return CRK_ERR_ARG;
  const int rc = crk_zero_stream_rows(h->state, sizeof(float) * h->state_floats, h->S, stream_ids, n, (hipStream_t)stream);
  return rc != CRK_OK ? rc : crk_zero_stream_rows(h->count, sizeof(int), h->S, stream_ids, n, (hipStream_t)stream);
}

extern "C" int crk_lstream_push(void* hh, const float* x, int ldx, const float* dec_cond, int ldd, const float* enc_cond, int lde,
                                const long long* spk, const int* n_valid, const int* end, int S, int C, int rows_out,
                                float* decoded, long long* const* qidx, float* const* encoded, int* n_out, int* first,
                                void* stream) {
  LaStreamH* h = (LaStreamH*)hh;
  if (!h) return CRK_ERR_ARG;
  LaP p = h->p;
  const int rc = st_push_args(h, p, x, ldx, dec_cond, ldd, enc_cond, lde, spk, n_valid, S, C, decoded, qidx, encoded);
  if (rc != CRK_OK) return rc;
  if (!n_out || !first || rows_out < C + p.la) return CRK_ERR_ARG;
  p.rings = h->rings; p.count = h->count; p.end = end; p.rows_out = rows_out; p.n_out = n_out; p.first = first;
  if (C <= LA_SHORT)
    hipLaunchKernelGGL(stream_la_push_kernel<true>, dim3(S), dim3(ST_THREADS), st_lds_bytes(), (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(stream_la_push_kernel<false>, dim3(S), dim3(ST_THREADS), st_lds_bytes(), (hipStream_t)stream, p);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
