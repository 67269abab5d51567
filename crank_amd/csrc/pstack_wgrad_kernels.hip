// Weight gradients of plain convs from bf16 planes: dW[tap][co][ci] = sum_t G[t][co] * O[t + off0 + tap*dil][ci]
// with G the output-gradient plane the backward chain stored and O the input-operand plane the
// forward chain stored.  Workgroup (g, l): conv l of the table, group g = a run of 64-frame
// chunks of the batch.  Rows travel HBM -> registers (next chunk, behind the MFMAs) -> row-major
// LDS tiles -> ds_read_b64_tr_b16 fragments (the reduction axis is the frame axis).  Four
// waves share the (tap, cin-band, cout-band) tiles of the conv, at most 8 per wave.
// Partial sums per group in the layout of the table kernel; wnorm_bwd_kernel reduces them.
#include "conv_kernels.h"
#include "stack_common.h"

#define PW_FR 64
#define PW_SPAN 32
#define PW_MAXT 8
// Phase cycles (tools/phase_cycles.py pw, -DSK_PROF=1): per workgroup and wave [0] set-up
// [1] barrier + tiles -> LDS + barrier [2] next requests [3] fragments + MFMAs [4] partial sums out [5] whole kernel

// MAXT: (tap, cin band, cout band) tiles a wave may hold (accumulators: 16 VGPRs each).  8 covers the classifier's widest
// conv; the 1x1 convs around a gated stack need 2, and a kernel instantiated for 2 keeps twice the workgroups resident.
template <bool PRECISE, int MAXT = PW_MAXT, bool SA = false>
__device__ __forceinline__ void pstack_wgrad_body(const PwP& p, int g, int layer, unsigned char* smem) {
  const PwLayer LY = p.layers[layer];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  SK_PROF_BEGIN()
  const int wa32 = (LY.wa + 31) & ~31, wb32 = (LY.wb + 31) & ~31;
  const int RA = wa32 * 2 + 64, RB = wb32 * 2 + 64;
  const int span = (LY.k - 1) * LY.dil, brn = PW_FR + span;
  const int abytes = PW_FR * RA, bbytes = (PW_FR + PW_SPAN) * RB, plane = abytes + bbytes;
  unsigned char* at_hi = smem;
  unsigned char* bt_hi = smem + abytes;
  const sk_u32x4 Z4 = {0u, 0u, 0u, 0u};
  for (int i = tid; i < (PRECISE ? 2 : 1) * plane / 16; i += 256) reinterpret_cast<sk_u32x4*>(smem)[i] = Z4;

  const int ppa = LY.wa >> 3, ppb = LY.wb >> 3;  // 16-byte pieces per plane row
  const int na = PW_FR * ppa, nb = brn * ppb;    // pieces per chunk: <= 1024, <= 1536
  sk_u32x4 ra_h[4], ra_l[4], rb_h[6], rb_l[6];
  const int ncpu = (p.T + PW_FR - 1) / PW_FR;
  const int c_beg = g * p.cpg, c_end = min(p.B * ncpu, (g + 1) * p.cpg);
#define PW_FETCH(c)                                                                                  \
  {                                                                                                  \
    const int u_ = (c) / ncpu, f0_ = ((c) - u_ * ncpu) * PW_FR;                                       \
    const long nb_ = (long)u_ * p.T;                                                                 \
    _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                  \
      const int idx = tid + u * 256, r = idx / ppa, cc = idx - r * ppa, t = f0_ + r;                  \
      const bool on = idx < na && t < p.T;                                                           \
      const long off = (nb_ + t) * LY.wa + cc * 8;                                                   \
      ra_h[u] = on ? *reinterpret_cast<const sk_u32x4*>(p.abase + LY.a_hi + off) : Z4;                         \
      if (PRECISE) ra_l[u] = on ? *reinterpret_cast<const sk_u32x4*>(p.abase + LY.a_lo + off) : Z4;            \
    }                                                                                                \
    _Pragma("unroll") for (int u = 0; u < 6; u++) {                                                  \
      const int idx = tid + u * 256, r = idx / ppb, cc = idx - r * ppb, t = f0_ + LY.off0 + r;        \
      const bool on = idx < nb && t >= 0 && t < p.T;                                                 \
      const long off = (nb_ + t) * LY.wb + cc * 8;                                                   \
      rb_h[u] = on ? *reinterpret_cast<const sk_u32x4*>(p.bbase + LY.b_hi + off) : Z4;                         \
      if (PRECISE) rb_l[u] = on ? *reinterpret_cast<const sk_u32x4*>(p.bbase + LY.b_lo + off) : Z4;            \
    }                                                                                                \
  }
#define PW_COMMIT()                                                                                  \
  {                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                  \
      const int idx = tid + u * 256, r = idx / ppa, cc = idx - r * ppa;                               \
      if (idx < na) {                                                                                \
        *reinterpret_cast<sk_u32x4*>(at_hi + r * RA + cc * 16) = ra_h[u];                             \
        if (PRECISE) *reinterpret_cast<sk_u32x4*>(at_hi + plane + r * RA + cc * 16) = ra_l[u];        \
      }                                                                                              \
    }                                                                                                \
    _Pragma("unroll") for (int u = 0; u < 6; u++) {                                                  \
      const int idx = tid + u * 256, r = idx / ppb, cc = idx - r * ppb;                               \
      if (idx < nb) {                                                                                \
        *reinterpret_cast<sk_u32x4*>(bt_hi + r * RB + cc * 16) = rb_h[u];                             \
        if (PRECISE) *reinterpret_cast<sk_u32x4*>(bt_hi + plane + r * RB + cc * 16) = rb_l[u];        \
      }                                                                                              \
    }                                                                                                \
  }

  // ---- this wave's tiles: j = wave + 4m -> (cout band ct, cin band it, tap) ----
  const int nct = (LY.ca + 31) >> 5, nit = (LY.cb + 31) >> 5, ntiles = nct * nit * LY.k;
  const int i15 = lane & 15, grp = lane >> 4;
  const int rowoff = (grp >> 1) * 8 + (i15 >> 2);
  const int coloff = (grp & 1) * 16 + (i15 & 3) * 4;
  const int half = lane >> 5, l31 = lane & 31;
  int a_off[MAXT], b_off[MAXT];
  f32x16 acc[MAXT];
#pragma unroll
  for (int m = 0; m < MAXT; m++) {
    const int j = wave + 4 * m < ntiles ? wave + 4 * m : (wave < ntiles ? wave : 0);  // (a tile the wave does not have: its first)
    const int ct = j % nct, it = (j / nct) % nit, tap = j / (nct * nit);
    a_off[m] = rowoff * RA + (ct * 32 + coloff) * 2;
    b_off[m] = (rowoff + tap * LY.dil) * RB + (it * 32 + coloff) * 2;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[m][i] = 0.f;
  }
  float bsum = 0.f;
  const bool bias_wave = wave < nct && LY.pb >= 0;  // tile m = 0 of waves 0..nct-1 is (ct = wave, it 0, tap 0)

  if constexpr (!PRECISE) {
    // ---- plain bf16: chunks requested TWO ahead, nothing of the loop under a branch.  One wave per SIMD is all the
    // accumulators allow (MAXT = 8: 128 of them), so a chunk's HBM round trip was exposed once per chunk behind a
    // one-deep prefetch (12 k cycles per 64-frame chunk for 670 instructions: rocprof 49.5 us for the classifier's eight
    // convs).  Two register sets alternate; every load is a buffer load whose offset is out of range where the piece,
    // its frame or the chunk does not exist (it returns 0: no branch around a load, so the wait counts stay exact -
    // behind a branch the wait-count pass has to drain the queue), and the piece -> (row, column) divisions are done
    // once per thread instead of twice per chunk.  Same products in the same order: bit-identical partial sums. ----
    const __amdgpu_buffer_rsrc_t rA = sk_rsrc16(p.abase + LY.a_hi, (long)p.B * p.T * LY.wa);
    const __amdgpu_buffer_rsrc_t rB = sk_rsrc16(p.bbase + LY.b_hi, (long)p.B * p.T * LY.wb);
    int la[4], ga[4], qa[4], lb[6], gb[6], qb[6];  // LDS byte offset (-1: no piece), plane byte offset from the chunk's row 0, row
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int idx = tid + u * 256, r = idx / ppa, cc = idx - r * ppa;
      const bool ok = idx < na;
      la[u] = ok ? r * RA + cc * 16 : -1; ga[u] = (r * LY.wa + cc * 8) * 2; qa[u] = ok ? r : (1 << 24);
    }
#pragma unroll
    for (int u = 0; u < 6; u++) {
      const int idx = tid + u * 256, r = idx / ppb, cc = idx - r * ppb;
      const bool ok = idx < nb;
      lb[u] = ok ? r * RB + cc * 16 : -1; gb[u] = (r * LY.wb + cc * 8) * 2; qb[u] = ok ? r : (1 << 24);
    }
    int fu = c_beg / ncpu, ff = (c_beg - fu * ncpu) * PW_FR, fc = c_beg;  // the chunk the next request is for
    sk_u32x4 sa0[4], sb0[6], sa1[4], sb1[6];
#define PW_FETCH2(SA, SB)                                                                                    \
  {                                                                                                          \
    const bool live_ = fc < c_end;                                                                           \
    const int basea_ = (int)(((long)fu * p.T + ff) * LY.wa * 2), baseb_ = (int)(((long)fu * p.T + ff + LY.off0) * LY.wb * 2); \
    const int hia_ = live_ ? p.T - ff : 0, lob_ = -(ff + LY.off0), hib_ = live_ ? p.T - ff - LY.off0 : lob_;   \
    _Pragma("unroll") for (int u = 0; u < 4; u++)                                                            \
      SA[u] = __builtin_amdgcn_raw_buffer_load_b128(rA, qa[u] < hia_ ? basea_ + ga[u] : SK_OOB, 0, 0);        \
    _Pragma("unroll") for (int u = 0; u < 6; u++)                                                            \
      SB[u] = __builtin_amdgcn_raw_buffer_load_b128(rB, (qb[u] >= lob_ && qb[u] < hib_) ? baseb_ + gb[u] : SK_OOB, 0, 0); \
    fc++; ff += PW_FR;                                                                                       \
    if (ff >= p.T) { ff = 0; fu++; }                                                                         \
  }
#define PW_COMMIT2(SA, SB)                                                                                   \
  {                                                                                                          \
    _Pragma("unroll") for (int u = 0; u < 4; u++)                                                            \
      if (la[u] >= 0) *reinterpret_cast<sk_u32x4*>(at_hi + la[u]) = SA[u];                                    \
    _Pragma("unroll") for (int u = 0; u < 6; u++)                                                            \
      if (lb[u] >= 0) *reinterpret_cast<sk_u32x4*>(bt_hi + lb[u]) = SB[u];                                    \
  }
    // ONE code path for all MAXT accumulators, no guard around any MFMA: a wave with fewer tiles repeats its first tile
    // into accumulators nobody reads (the kernel is instantiated for the tile count the launch needs).  Fragments of k
    // step kc + 1 are read before the MFMAs of step kc where the registers allow two sets.  (With a run-time guard per
    // tile every MFMA sat in a basic block of its own behind its two transposing LDS reads: ~150 cycles of exposed
    // latency per 34-cycle MFMA.)
// SA: every tile of the wave lies in ONE cout band (tile j = wave + 4 m, band j % nct: true whenever nct divides 4 - 1, 2 or 4
// bands, i.e. every conv but the ones with 65 - 96 output channels): the dY fragment of a k step is then the same for all of
// them and is read once instead of once per tile (two transposing LDS reads per fragment: 12 instead of 20 LDS instructions
// per k step at five tiles - the reads, not the MFMAs, are what a k step takes).
#define PW_COMPUTE(SA)                                                                                       \
  {                                                                                                          \
    constexpr int NB = MAXT <= 4 ? 2 : 1, NA = (SA) ? 1 : MAXT;                                              \
    bf16x8 fa[NB][NA], fb[NB][MAXT];                                                                         \
    _Pragma("unroll") for (int m = 0; m < MAXT; m++) {                                                       \
      if (m < NA) fa[0][m] = sw_tr_frag(at_hi + a_off[m], RA);                                               \
      fb[0][m] = sw_tr_frag(bt_hi + b_off[m], RB);                                                           \
    }                                                                                                        \
    _Pragma("unroll") for (int kc = 0; kc < PW_FR / 16; kc++) {                                              \
      if (NB == 2 && kc + 1 < PW_FR / 16) {                                                                  \
        _Pragma("unroll") for (int m = 0; m < MAXT; m++) {                                                   \
          if (m < NA) fa[(kc + 1) % NB][m] = sw_tr_frag(at_hi + a_off[m] + (kc + 1) * 16 * RA, RA);          \
          fb[(kc + 1) % NB][m] = sw_tr_frag(bt_hi + b_off[m] + (kc + 1) * 16 * RB, RB);                      \
        }                                                                                                    \
      }                                                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      _Pragma("unroll") for (int m = 0; m < MAXT; m++) acc[m] = mfma_bf16(fa[kc % NB][(SA) ? 0 : m], fb[kc % NB][m], acc[m]); \
      if (bias_wave) bsum += sw_sum8(fa[kc % NB][0]);                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                                     \
      if (NB == 1 && kc + 1 < PW_FR / 16) {                                                                  \
        _Pragma("unroll") for (int m = 0; m < MAXT; m++) {                                                   \
          if (m < NA) fa[0][m] = sw_tr_frag(at_hi + a_off[m] + (kc + 1) * 16 * RA, RA);                      \
          fb[0][m] = sw_tr_frag(bt_hi + b_off[m] + (kc + 1) * 16 * RB, RB);                                  \
        }                                                                                                    \
      }                                                                                                      \
    }                                                                                                        \
  }
    PW_FETCH2(sa0, sb0)
    PW_FETCH2(sa1, sb1)
    SK_T(0)
    // (an odd run ends with one chunk of zeros: every MFMA of it adds 0)
    for (int c = c_beg; c < c_end; c += 2) {
      __syncthreads();  // previous chunk's fragments consumed (first pass: tiles zeroed)
      PW_COMMIT2(sa0, sb0)
      __syncthreads();
      SK_T(1)
      PW_FETCH2(sa0, sb0)
      SK_T(2)
      PW_COMPUTE(SA)
      SK_T(3)
      __syncthreads();
      PW_COMMIT2(sa1, sb1)
      __syncthreads();
      SK_T(1)
      PW_FETCH2(sa1, sb1)
      SK_T(2)
      PW_COMPUTE(SA)
      SK_T(3)
    }
#undef PW_FETCH2
#undef PW_COMMIT2
#undef PW_COMPUTE
  }
  if (PRECISE && c_end > c_beg) PW_FETCH(c_beg)
  for (int c = c_beg; PRECISE && c < c_end; c++) {
    __syncthreads();  // previous chunk's fragments consumed (first pass: tiles zeroed)
    PW_COMMIT()
    __syncthreads();
    if (c + 1 < c_end) PW_FETCH(c + 1)
#pragma unroll
    for (int kc = 0; kc < PW_FR / 16; kc++) {
#pragma unroll
      for (int m = 0; m < MAXT; m++) {
        if (wave + 4 * m < ntiles) {
          const bf16x8 a_hi = sw_tr_frag(at_hi + a_off[m] + kc * 16 * RA, RA);
          const bf16x8 b_hi = sw_tr_frag(bt_hi + b_off[m] + kc * 16 * RB, RB);
          acc[m] = mfma_bf16(a_hi, b_hi, acc[m]);
          if (m == 0 && bias_wave) bsum += sw_sum8(a_hi);
          if (PRECISE) {
            const bf16x8 a_lo = sw_tr_frag(at_hi + plane + a_off[m] + kc * 16 * RA, RA);
            const bf16x8 b_lo = sw_tr_frag(bt_hi + plane + b_off[m] + kc * 16 * RB, RB);
            acc[m] = mfma_bf16(a_lo, b_hi, acc[m]);
            acc[m] = mfma_bf16(a_hi, b_lo, acc[m]);
            if (m == 0 && bias_wave) bsum += sw_sum8(a_lo);
          }
        }
      }
    }
  }

#pragma unroll
  for (int m = 0; m < MAXT; m++) {
    const int j = wave + 4 * m;
    if (j < ntiles) {
      const int ct = j % nct, it = (j / nct) % nit, tap = j / (nct * nit);
      const int ci = it * 32 + l31;
      float* out = p.partials + LY.pt + ((long)g * LY.k + tap) * LY.ca * LY.cb;
      if (ci < LY.cb) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int co = ct * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
          if (co < LY.ca) out[(long)co * LY.cb + ci] = acc[m][i];
        }
      }
    }
  }
  if (bias_wave) {
    const float tot = bsum + __shfl_xor(bsum, 32);
    const int co = wave * 32 + l31;
    if (half == 0 && co < LY.ca) p.partials[LY.pb + (long)g * LY.ca + co] = tot;
  }
  SK_T(4)
  SK_PROF_END(5)
}

template <bool PRECISE, int MAXT = PW_MAXT>
__global__ __launch_bounds__(256) void pstack_wgrad_kernel(const PwP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (!PRECISE && MAXT > 5) {
    // the body for the tile count of THIS workgroup's conv (the classifier's first conv has 30 tiles, its others 20: with one
    // body for the widest, 3 of every 8 MFMAs of seven of its eight convs were idle repeats)
    const PwLayer& Y = p.layers[blockIdx.y];
    const int per = (((Y.ca + 31) >> 5) * ((Y.cb + 31) >> 5) * Y.k + 3) >> 2;
    const bool sa = (4 % ((Y.ca + 31) >> 5)) == 0;  // one cout band per wave (pstack_wgrad_body, PW_COMPUTE)
    if (per <= 3) { if (sa) pstack_wgrad_body<PRECISE, 3, true>(p, blockIdx.x, blockIdx.y, smem); else pstack_wgrad_body<PRECISE, 3>(p, blockIdx.x, blockIdx.y, smem); return; }
    if (per <= 5) { if (sa) pstack_wgrad_body<PRECISE, 5, true>(p, blockIdx.x, blockIdx.y, smem); else pstack_wgrad_body<PRECISE, 5>(p, blockIdx.x, blockIdx.y, smem); return; }
  }
  if (!PRECISE) {
    const PwLayer& Y = p.layers[blockIdx.y];
    if ((4 % ((Y.ca + 31) >> 5)) == 0) { pstack_wgrad_body<PRECISE, MAXT, !PRECISE>(p, blockIdx.x, blockIdx.y, smem); return; }
  }
  pstack_wgrad_body<PRECISE, MAXT>(p, blockIdx.x, blockIdx.y, smem);
}
// the plain convs of several nets in one launch (first conv and head of every generator stack; the speaker nets of a step):
// workgroup x belongs to the net whose range holds it, there to (conv, group) = (local / G, local % G) - the order a
// (G, convs) grid of that net alone is walked in
__device__ __forceinline__ int pw_net_of_block(const PwMP& m, int bx) {
  int r = 0;
  while (r + 1 < m.n && bx >= m.first[r + 1]) r++;
  return r;
}
template <int MAXT>
__global__ __launch_bounds__(256) void pstack_wgrad_multi_kernel(const PwMP m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int r = pw_net_of_block(m, blockIdx.x);
  const PwP& p = m.q[r];
  const int local = (int)blockIdx.x - m.first[r], layer = local / p.G;
  // (the shared dY fragment of pstack_wgrad_kernel is not used here: two tiles per wave at most, 33.9 -> 35.4 us with it)
  pstack_wgrad_body<false, MAXT>(p, local - layer * p.G, layer, smem);
}
// ... where a conv has more than two tiles per wave (whole plain nets: 20 - 30 tiles a conv): per workgroup the body
// pstack_wgrad_kernel<false, ..> runs for that conv launched alone - the instantiation for its tiles per wave (3, 5, 6 or
// 8; any body that holds the tiles adds the same products in the same order), the dY fragment read once per wave where
// every tile of a wave lies in one cout band, chunks requested two ahead.  A conv costs here what it costs there.
__global__ __launch_bounds__(256) void pstack_wgrad_multi_wide_kernel(const PwMP m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int r = pw_net_of_block(m, blockIdx.x);
  const PwP& p = m.q[r];
  const int local = (int)blockIdx.x - m.first[r], layer = local / p.G, g = local - layer * p.G;
  const PwLayer& Y = p.layers[layer];
  const int nct = (Y.ca + 31) >> 5;
  const int per = (nct * ((Y.cb + 31) >> 5) * Y.k + 3) >> 2;
  const bool sa = (4 % nct) == 0;  // one cout band per wave (pstack_wgrad_body, PW_COMPUTE)
  if (per <= 3) { if (sa) pstack_wgrad_body<false, 3, true>(p, g, layer, smem); else pstack_wgrad_body<false, 3>(p, g, layer, smem); return; }
  if (per <= 5) { if (sa) pstack_wgrad_body<false, 5, true>(p, g, layer, smem); else pstack_wgrad_body<false, 5>(p, g, layer, smem); return; }
  if (per <= 6) { if (sa) pstack_wgrad_body<false, 6, true>(p, g, layer, smem); else pstack_wgrad_body<false, 6>(p, g, layer, smem); return; }
  if (sa) pstack_wgrad_body<false, PW_MAXT, true>(p, g, layer, smem); else pstack_wgrad_body<false, PW_MAXT>(p, g, layer, smem);
}
int launch_pstack_wgrad_multi(const PwMP& m, int total_blocks, int max_wa, int max_wb, int max_tiles, double flops,
                              double bytes, hipStream_t s) {
  const int RA = ((max_wa + 31) & ~31) * 2 + 64, RB = ((max_wb + 31) & ~31) * 2 + 64;
  const int lds = PW_FR * RA + (PW_FR + PW_SPAN) * RB;
  if (total_blocks < 1) return CRK_ERR_ARG;
  CRK_RAISE_LDS_ONCE(160 * 1024, pstack_wgrad_multi_kernel<2>, pstack_wgrad_multi_wide_kernel)
  conv_prof_bytes(6, bytes);
  conv_prof_begin(6, flops, s);
  if (max_tiles <= 8) hipLaunchKernelGGL(pstack_wgrad_multi_kernel<2>, dim3(total_blocks), dim3(256), lds, s, m);  // <= 2 per wave
  else hipLaunchKernelGGL(pstack_wgrad_multi_wide_kernel, dim3(total_blocks), dim3(256), lds, s, m);
  conv_prof_end(6, s);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

int pstack_wgrad_supported(int ca, int cb, int wa, int wb, int k, int dil) {
  const int nct = (ca + 31) / 32, nit = (cb + 31) / 32;
  return nct * nit * k <= 4 * PW_MAXT && (k - 1) * dil <= PW_SPAN && wa <= 128 && wb <= 128 && (wa & 15) == 0 &&
         (wb & 15) == 0 && ca <= wa && cb <= wb;
}

// max_tiles: largest (tap, cin band, cout band) tile count of a layer of the table (0: unknown -> the widest instantiation)
int launch_pstack_wgrad(const PwP& p, int nlayers, int max_wa, int max_wb, bool precise, double flops, hipStream_t s, int max_tiles) {
  const int RA = ((max_wa + 31) & ~31) * 2 + 64, RB = ((max_wb + 31) & ~31) * 2 + 64;
  const int lds = (precise ? 2 : 1) * (PW_FR * RA + (PW_FR + PW_SPAN) * RB);
  CRK_RAISE_LDS_ONCE(160 * 1024, pstack_wgrad_kernel<true>, pstack_wgrad_kernel<false>, pstack_wgrad_kernel<false, 3>,
                     pstack_wgrad_kernel<false, 4>, pstack_wgrad_kernel<false, 5>, pstack_wgrad_kernel<false, 6>)
  dim3 grid(p.G, nlayers);
  conv_prof_bytes(6, 2.0 * (max_wa + max_wb) * (double)p.B * p.T * nlayers);  // upper bound: widest planes per conv
  conv_prof_begin(6, flops, s);
  // (plain bf16: every wave issues the MFMAs of `per` tiles unconditionally - the instantiation for the count needed)
  const int per = max_tiles > 0 ? (max_tiles + 3) / 4 : PW_MAXT;
  if (precise) hipLaunchKernelGGL(pstack_wgrad_kernel<true>, grid, dim3(256), lds, s, p);
  else if (per <= 3) hipLaunchKernelGGL((pstack_wgrad_kernel<false, 3>), grid, dim3(256), lds, s, p);
  else if (per == 4) hipLaunchKernelGGL((pstack_wgrad_kernel<false, 4>), grid, dim3(256), lds, s, p);
  else if (per == 5) hipLaunchKernelGGL((pstack_wgrad_kernel<false, 5>), grid, dim3(256), lds, s, p);
  else if (per == 6) hipLaunchKernelGGL((pstack_wgrad_kernel<false, 6>), grid, dim3(256), lds, s, p);
  else hipLaunchKernelGGL(pstack_wgrad_kernel<false>, grid, dim3(256), lds, s, p);
  conv_prof_end(6, s);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
