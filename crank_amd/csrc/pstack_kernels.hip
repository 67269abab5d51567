// Fused chains of plain Conv1d layers: every conv of the step that is not a gated residual
// block - the speaker classifier C and the speaker-adversarial net (stacks of dilated
// Conv1d + LeakyReLU: parallel_wavegan ParallelWaveGANDiscriminator, SURVEY.md Appendix A.4;
// call sites crank/bin/train.py:78-89, crank/net/module/spkradv.py:49-60), and the 1x1 first
// conv and the "act -> 1x1 -> act -> 1x1" head around every gated stack (Appendix A.1-A.3).
//
// One kernel runs a chain in EITHER direction: a layer is "rows x K weights per tap applied to
// a [frames][K] operand", followed by an epilogue that is an activation (forward) or a multiply
// by the activation derivative read from a saved plane (data gradient, weights in the
// transposed tap-flipped layout).  As in stack_kernels.hip a workgroup owns a window of
// 32*NW frames (+ the chain's halo), MFMA A = weights / B = operand so that a lane owns one
// frame, the operand of the next layer goes accumulator -> bf16 -> v_permlane32_swap ->
// LDS without leaving the CU, and the operand of EVERY layer is also stored as a bf16 plane:
// the forward's planes are the weight gradient's input operands and the activation-derivative
// masks, the backward's planes are its output-gradient operands.
//
// The generic per-layer kernels (conv_kernels.hip) remain as the fallback for shapes these
// kernels do not take; their floor per launch is the instruction-cache fill of ~50 KB of
// code, which is what made ~60 of them per step cost more than the gated stacks themselves.
#include "conv_kernels.h"
#include "stack_common.h"


// Weights reach LDS in CHUNKS of whole taps: as many consecutive taps of a layer as fit the staging registers
// (PS_MAXP 16-byte pieces per thread) and the chunk buffer (PsP::w_bytes).  The next chunk is fetched (global ->
// registers) before the MFMAs of the current one and committed (registers -> LDS) after them, so its L2 round trip
// hides behind tpc taps of MFMAs and the chain takes one barrier per chunk.  (One tap per chunk - the first version -
// left ~1.5 us per tap: a tap's MFMAs are ~0.3 us, the round trip ~1 us.)
#ifndef PS_ABL
#define PS_ABL 0  // ablation builds (tools/ps_ablate.sh): 1 no MFMA, 2 no plane stores, 4 no weight fragment reads, 8 no operand
#endif            // fragment reads, 16 no weight chunk traffic after the first chunk
// Phase cycles (tools/phase_cycles.py ps, -DSK_PROF=1): per workgroup and wave [0] prologue [1] tap MFMAs [2] waiting at the
// chunk barrier [3] weight commit (incl. waiting for the fetch) [4] epilogue (incl. its barrier) [5] whole kernel
#define PS_WFRAG(ptr) ((PS_ABL & 4) ? xb : lds_frag(ptr))
#define PS_XFRAG(ptr) ((PS_ABL & 8) ? x0 : lds_frag(ptr))
#define PS_MAXP(NT) ((NT) == 512 ? 4 : 8)
__host__ __device__ __forceinline__ int ps_tpc(int k, int rows_pad, int kp, int cap_pieces, int w_bytes) {
  int t = cap_pieces / (rows_pad * (kp >> 3));
  const int tl = w_bytes / (rows_pad * (kp * 2 + 16));
  if (tl < t) t = tl;
  if (t > k) t = k;
  return t < 1 ? 1 : t;
}

template <bool PRECISE, int NW>
__global__ __launch_bounds__(NW * 64, PRECISE ? 1 : 2) void pstack_kernel(const PsP p) {
  constexpr int NT = NW * 64, R = NW * 32, MAXP = PS_MAXP(NT);
  const int OS = p.os;  // row stride of the operand tile: widest K of the chain as bf16 + 16 B pad (a layer's weight rows: its own kp * 2 + 16)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  SK_PROF_BEGIN()
  const int b = blockIdx.x / p.tiles_per_utt, tile = blockIdx.x - b * p.tiles_per_utt;
  const int t0 = tile * p.tmo;
  const long nbase = (long)b * p.T, N = (long)p.B * p.T;

  unsigned char* os_hi = smem;  // [SK_GUARD + R + SK_GUARD][OS]
  unsigned char* os_lo = smem + p.o_olo;
  // weight buffer i as an OFFSET from the LDS base: a runtime-indexed array of pointers would decay to
  // generic pointers and every weight-fragment access to a FLAT instruction (vmcnt + lgkmcnt, i.e.
  // serialised with the global weight prefetch) instead of ds_read / ds_write
#define WS_HI(i) (smem + p.o_whi + ((PRECISE || (i) == 0) ? 0 : p.w_bytes))
  unsigned char* ws_lo = smem + p.o_wlo;

  const int row = wave * 32 + l31;
  const int t = t0 - p.hl + row;
  const bool rin = t >= 0 && t < p.T;
  const bool rout = rin && row >= p.hl && row < p.hl + p.tmo;
  const long n = nbase + t;

  // ---- weight chunk prefetch (ntaps x rows_pad x kp bf16 = ntaps*rows_pad*kp/8 16-byte pieces, <= MAXP * NT) ----
  sk_u32x4 wr_h[MAXP], wr_l[MAXP];
#define PS_FETCH(LYX, tap, ntaps)                                                            \
  {                                                                                          \
    const int total = (ntaps) * (LYX).rows_pad * ((LYX).kp >> 3);                            \
    const long base = (LYX).w_off + (long)(tap) * (LYX).rows_pad * (LYX).kp;                 \
    _Pragma("unroll") for (int u = 0; u < MAXP; u++) {                                       \
      const int idx = tid + u * NT;                                                          \
      const long off = base + (idx < total ? (long)idx * 8 : 0);                             \
      wr_h[u] = *reinterpret_cast<const sk_u32x4*>(p.whi + off);                             \
      if (PRECISE) wr_l[u] = *reinterpret_cast<const sk_u32x4*>(p.wlo + off);                \
    }                                                                                        \
  }
  /* rows of consecutive taps follow each other in the chunk buffer: row (tap - tap0) * rows_pad + r */          \
#define PS_COMMIT(LYX, ntaps, dhi)                                                           \
  {                                                                                          \
    const int ppr = (LYX).kp >> 3, total = (ntaps) * (LYX).rows_pad * ppr, wst = (LYX).kp * 2 + 16; \
    _Pragma("unroll") for (int u = 0; u < MAXP; u++) {                                       \
      const int idx = tid + u * NT;                                                          \
      if (idx < total) {                                                                     \
        const int r = idx / ppr, c = idx - r * ppr;                                          \
        *reinterpret_cast<sk_u32x4*>((dhi) + r * wst + c * 16) = wr_h[u];                    \
        if (PRECISE) *reinterpret_cast<sk_u32x4*>(ws_lo + r * wst + c * 16) = wr_l[u];       \
      }                                                                                      \
    }                                                                                        \
  }
#define PS_TPC(LYX) ps_tpc((LYX).k, (LYX).rows_pad, (LYX).kp, MAXP * NT, p.w_bytes)

  PsLayer LY = p.layers[0];
  int tpc = PS_TPC(LY);
  PS_FETCH(LY, 0, tpc)

  // ---- layer-0 operand, phase 1: every load of this lane's input row is issued before anything waits
  // (one memory round trip for the whole row instead of one per 16-channel group) ----
  const __amdgpu_buffer_rsrc_t rx = sk_rsrc(p.x, N * p.ldx);
  const bool vec = ((p.ldx & 3) == 0) && ((p.cin & 3) == 0) && ((((uintptr_t)p.x) & 15) == 0);
  const int nk0 = LY.kp >> 4;
  sk_u32x4 xa[8], xc[8];
#pragma unroll
  for (int kc = 0; kc < 8; kc++)
    if (kc < nk0) {
      const int c0 = 16 * kc + 8 * half;
      if (vec) {
        const int vo = rin ? (int)((n * p.ldx + c0) * 4) : SK_OOB;
        xa[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, c0 + 3 < p.cin ? vo : SK_OOB, 0, 0);
        xc[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, c0 + 7 < p.cin ? vo + 16 : SK_OOB, 0, 0);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          xa[kc][j] = __builtin_amdgcn_raw_buffer_load_b32(rx, (rin && c0 + j < p.cin) ? (int)((n * p.ldx + c0 + j) * 4) : SK_OOB, 0, 0);
          xc[kc][j] = __builtin_amdgcn_raw_buffer_load_b32(rx, (rin && c0 + 4 + j < p.cin) ? (int)((n * p.ldx + c0 + 4 + j) * 4) : SK_OOB, 0, 0);
        }
      }
    }

  // layer table and biases into LDS once (inside the layer loop they would be global loads - a full
  // memory round trip each - in front of every layer's first MFMA)
  PsLayer* lay_s = reinterpret_cast<PsLayer*>(smem + p.o_tab);  // [L (+1 with tail)]
  float* bias_s = reinterpret_cast<float*>(smem + p.o_bias);     // [L][128]
  {
    const int nl = p.L + (p.tail ? 1 : 0);
    for (int i = tid; i < nl * (int)(sizeof(PsLayer) / 4); i += NT)
      reinterpret_cast<int*>(lay_s)[i] = reinterpret_cast<const int*>(p.layers)[i];
    for (int i = tid; i < p.L * 128; i += NT) {
      const PsLayer Y = p.layers[i >> 7];
      const int c = i & 127;
      bias_s[i] = (Y.b_off >= 0 && c < Y.rows) ? p.params[Y.b_off + c] : 0.f;
    }
  }

  // ---- guard rows ----
  for (int i = tid; i < SK_GUARD * OS / 16; i += NT) {
    const sk_u32x4 z4 = {0u, 0u, 0u, 0u};
    reinterpret_cast<sk_u32x4*>(os_hi)[i] = z4;
    reinterpret_cast<sk_u32x4*>(os_hi + (SK_GUARD + R) * OS)[i] = z4;
    if (PRECISE) {
      reinterpret_cast<sk_u32x4*>(os_lo)[i] = z4;
      reinterpret_cast<sk_u32x4*>(os_lo + (SK_GUARD + R) * OS)[i] = z4;
    }
  }

  unsigned char* my_os_hi = os_hi + (SK_GUARD + row) * OS + 8 * half * 2;
  unsigned char* my_os_lo = os_lo + (SK_GUARD + row) * OS + 8 * half * 2;

  // ---- layer-0 operand, phase 2: fp32 -> act -> bf16 fragments -> LDS tile and saved plane ----
  {
    const float in_sc = p.in_num ? p.in_scale * (p.in_num[0] / p.in_den[1]) : p.in_scale;
    const __amdgpu_buffer_rsrc_t r_sh = sk_rsrc16(p.save_hi ? p.save_hi + LY.save_plane : (const uint16_t*)p.x, N * LY.kp);
    const __amdgpu_buffer_rsrc_t r_sl = sk_rsrc16((p.save_hi && PRECISE) ? p.save_lo + LY.save_plane : (const uint16_t*)p.x, N * LY.kp);
    const int voff_s = (rout && p.save_hi) ? (int)((n * LY.kp + 8 * half) * 2) : SK_OOB;
#pragma unroll
    for (int kc = 0; kc < 8; kc++)
      if (kc < nk0) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; j++) { v[j] = sk_u2f(xa[kc][j]); v[4 + j] = sk_u2f(xc[kc][j]); }
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = apply_act(v[j] * in_sc, p.in_act, p.slope);
        const sk_u32x4 fh = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
        *reinterpret_cast<sk_u32x4*>(my_os_hi + kc * 32) = fh;
        if (!(PS_ABL & 2)) __builtin_amdgcn_raw_buffer_store_b128(fh, r_sh, voff_s + kc * 32, 0, 0);
        if (PRECISE) {
#pragma unroll
          for (int j = 0; j < 8; j++) v[j] = sk_bf_lo(v[j]);
          const sk_u32x4 fl = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
          *reinterpret_cast<sk_u32x4*>(my_os_lo + kc * 32) = fl;
          __builtin_amdgcn_raw_buffer_store_b128(fl, r_sl, voff_s + kc * 32, 0, 0);
        }
      }
  }
  PS_COMMIT(LY, tpc, WS_HI(0))

  int cur = 0;
  f32x16 acc[4];
  __syncthreads();  // table, biases, layer-0 operand, first weight chunk: staged
  SK_T(0)

  for (int l = 0; l < p.L; l++) {
    const int ntl = LY.rows_pad >> 5, nkc = LY.kp >> 4;
    const bool last = l + 1 == p.L;
    const bool fin = last && !p.tail;  // this layer's output is the chain's fp32 output
    PsLayer LN = LY;
    if (!fin) LN = lay_s[l + 1];
    const int wst = LY.kp * 2 + 16;  // row stride of this layer's weight chunk in LDS
    const int tpcn = PS_TPC(LN);
    // (requesting the activation-derivative masks of the data-gradient chains here, a layer of MFMAs ahead of their use in
    // the epilogue, was measured: no change - the epilogue's time is barrier skew, not the mask round trip)
    // accumulators start from the bias (rows of D = output channels)
#pragma unroll
    for (int nt = 0; nt < 4; nt++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const sk_f32x4 bq = *reinterpret_cast<const sk_f32x4*>(bias_s + l * 128 + nt * 32 + 8 * g + 4 * half);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[nt][4 * g + j] = bq[j];
      }

    // The tap loop exists once per output-tile count (1..4 tiles of 32 channels), chosen per layer: with the
    // count as a run-time guard around each MFMA every MFMA sat in a basic block of its own behind its own
    // LDS round trip.  Inside, the k-steps run as a software pipeline: the fragments of step k+1 are loaded
    // before the MFMAs of step k are issued (the last step reloads its own fragments, branch-free).
#define PS_TAP_LOOP(NTL)                                                                                   \
  for (int c0 = 0; c0 < LY.k; c0 += tpc) {                                                                 \
    const int c1 = c0 + tpc < LY.k ? c0 + tpc : LY.k;                                                      \
    __syncthreads(); /* chunk `cur` committed; previous chunk's reads done; operand tile complete */       \
    SK_T(2)                                                                                                \
    const bool more = c1 < LY.k || !last;                                                                  \
    const int nnext = c1 < LY.k ? (LY.k - c1 < tpc ? LY.k - c1 : tpc) : (tpcn < LN.k ? tpcn : LN.k);       \
    if (!(PS_ABL & 16)) {                                                                                  \
      if (c1 < LY.k) PS_FETCH(LY, c1, nnext)                                                               \
      else if (!last) PS_FETCH(LN, 0, nnext)                                                               \
    }                                                                                                      \
    for (int tap = c0; tap < c1; tap++) {                                                                  \
      const unsigned char* wf_hi = WS_HI(cur) + ((tap - c0) * LY.rows_pad + l31) * wst + half * 16;        \
      const unsigned char* wf_lo = ws_lo + ((tap - c0) * LY.rows_pad + l31) * wst + half * 16;             \
      const int arow = SK_GUARD + row + LY.off0 + tap * LY.dil;                                            \
      const unsigned char* xf_hi = os_hi + arow * OS + half * 16;                                          \
      const unsigned char* xf_lo = os_lo + arow * OS + half * 16;                                          \
      const bf16x8 x0 = lds_frag(os_hi + (SK_GUARD + row) * OS + half * 16);                               \
      bf16x8 xb = PS_XFRAG(xf_hi), xl, wa[NTL], wl[NTL];                                                   \
      if (PRECISE) xl = lds_frag(xf_lo);                                                                   \
      _Pragma("unroll") for (int nt = 0; nt < NTL; nt++) {                                                 \
        wa[nt] = PS_WFRAG(wf_hi + nt * 32 * wst);                                                          \
        if (PRECISE) wl[nt] = lds_frag(wf_lo + nt * 32 * wst);                                             \
      }                                                                                                    \
      for (int kc = 0; kc < nkc; kc++) {                                                                   \
        const int kn = (kc + 1 < nkc ? kc + 1 : kc) * 32;                                                  \
        const bf16x8 nxb = PS_XFRAG(xf_hi + kn);                                                           \
        bf16x8 nxl, nwa[NTL], nwl[NTL];                                                                    \
        if (PRECISE) nxl = lds_frag(xf_lo + kn);                                                           \
        _Pragma("unroll") for (int nt = 0; nt < NTL; nt++) {                                               \
          nwa[nt] = PS_WFRAG(wf_hi + nt * 32 * wst + kn);                                                  \
          if (PRECISE) nwl[nt] = lds_frag(wf_lo + nt * 32 * wst + kn);                                     \
        }                                                                                                  \
        _Pragma("unroll") for (int nt = 0; nt < NTL; nt++) {                                               \
          if (!(PS_ABL & 1)) acc[nt] = mfma_bf16(wa[nt], xb, acc[nt]);                                     \
          else acc[nt][0] += __builtin_bit_cast(float, (unsigned)wa[nt][0] | ((unsigned)xb[0] << 16));     \
          if (PRECISE) {                                                                                   \
            acc[nt] = mfma_bf16(wa[nt], xl, acc[nt]);                                                      \
            acc[nt] = mfma_bf16(wl[nt], xb, acc[nt]);                                                      \
          }                                                                                                \
        }                                                                                                  \
        xb = nxb;                                                                                          \
        if (PRECISE) xl = nxl;                                                                             \
        _Pragma("unroll") for (int nt = 0; nt < NTL; nt++) {                                               \
          wa[nt] = nwa[nt];                                                                                \
          if (PRECISE) wl[nt] = nwl[nt];                                                                   \
        }                                                                                                  \
      }                                                                                                    \
    }                                                                                                      \
    if (PRECISE) __syncthreads();                                                                          \
    SK_T(1)                                                                                                \
    __builtin_amdgcn_sched_barrier(0); /* keep the commit (and its wait for the prefetch) behind the MFMAs */ \
    if (more && !(PS_ABL & 16)) {                                                                          \
      if (c1 < LY.k) PS_COMMIT(LY, nnext, WS_HI(PRECISE ? 0 : cur ^ 1))                                    \
      else PS_COMMIT(LN, nnext, WS_HI(PRECISE ? 0 : cur ^ 1))                                              \
    }                                                                                                      \
    if (!PRECISE) cur ^= 1;                                                                                \
    SK_T(3)                                                                                                \
  }
    if (ntl == 2) { PS_TAP_LOOP(2) }
    else if (ntl == 1) { PS_TAP_LOOP(1) }
    else if (ntl == 3) { PS_TAP_LOOP(3) }
    else { PS_TAP_LOOP(4) }
#undef PS_TAP_LOOP

    // ---- epilogue: activation (forward) or activation-derivative mask (data gradient) ----
    const bool is_mask = LY.epi >= 3;
    const int ekind = is_mask ? LY.epi - 2 : LY.epi;  // ACT_NONE / ACT_LRELU(1) / ACT_RELU(2)
    const __amdgpu_buffer_rsrc_t r_m = sk_rsrc16(is_mask ? p.mask_hi + LY.mask_plane : (const uint16_t*)p.x, N * LY.mask_w);
    if (!fin) {
      __syncthreads();  // every wave is past this layer's tap reads: the operand tile may be rewritten
      const __amdgpu_buffer_rsrc_t r_sh = sk_rsrc16(p.save_hi ? p.save_hi + LN.save_plane : (const uint16_t*)p.x, N * LN.kp);
      const __amdgpu_buffer_rsrc_t r_sl = sk_rsrc16((p.save_hi && PRECISE) ? p.save_lo + LN.save_plane : (const uint16_t*)p.x, N * LN.kp);
      const int voff_s = (rout && p.save_hi) ? (int)((n * LN.kp + 8 * half) * 2) : SK_OOB;
      const int nk2 = LN.kp >> 4;  // 16-channel groups of the next operand (<= 2 * ntl)
#pragma unroll
      for (int kc = 0; kc < 8; kc++)
        if (kc < nk2) {
          const int nt = kc >> 1, g0 = (kc & 1) * 2;
          sk_u32x2 qh[2], ql[2];
#pragma unroll
          for (int gg = 0; gg < 2; gg++) {
            const int g = g0 + gg, c0 = nt * 32 + 8 * g + 4 * half;
            float v[4];
            if (is_mask) {
              const sk_u32x2 m = __builtin_amdgcn_raw_buffer_load_b64(r_m, rin ? (int)((n * LY.mask_w + c0) * 2) : SK_OOB, 0, 0);
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const unsigned w = j < 2 ? m[0] : m[1];
                const float mv = sk_u2f((j & 1) ? (w & 0xffff0000u) : (w << 16));
                v[j] = acc[nt][4 * g + j] * act_grad(mv, ekind, p.slope);
              }
            } else {
#pragma unroll
              for (int j = 0; j < 4; j++) v[j] = apply_act(acc[nt][4 * g + j], ekind, p.slope);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = rin ? v[j] : 0.f;
            sk_quad<PRECISE>(v[0], v[1], v[2], v[3], qh[gg], ql[gg]);
          }
          const sk_u32x4 fh = sk_frag_bits(sk_swap_frag(qh[0], qh[1]));
          *reinterpret_cast<sk_u32x4*>(my_os_hi + kc * 32) = fh;
          if (!(PS_ABL & 2)) __builtin_amdgcn_raw_buffer_store_b128(fh, r_sh, voff_s + kc * 32, 0, 0);
          if (PRECISE) {
            const sk_u32x4 fl = sk_frag_bits(sk_swap_frag(ql[0], ql[1]));
            *reinterpret_cast<sk_u32x4*>(my_os_lo + kc * 32) = fl;
            __builtin_amdgcn_raw_buffer_store_b128(fl, r_sl, voff_s + kc * 32, 0, 0);
          }
        }
      SK_T(4)
      if (last) break;
      LY = LN;
      tpc = tpcn;
    } else {
      // ---- chain output, fp32 [N, rows] with the caller's row stride ----
      const bool youtp = rout && p.y != nullptr;  // (a chain may be run for its saved planes only)
      const __amdgpu_buffer_rsrc_t ry = sk_rsrc(p.y ? p.y : p.x, N * p.ldy);
      const bool vecy = ((p.ldy & 3) == 0) && ((LY.rows & 3) == 0) && ((((uintptr_t)p.y) & 15) == 0);
#pragma unroll
      for (int nt = 0; nt < 4; nt++)
        if (nt < ntl) {
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const int c0 = nt * 32 + 8 * g + 4 * half;
            float v[4];
            if (is_mask) {
              const sk_u32x2 m = __builtin_amdgcn_raw_buffer_load_b64(r_m, rin ? (int)((n * LY.mask_w + c0) * 2) : SK_OOB, 0, 0);
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const unsigned w = j < 2 ? m[0] : m[1];
                const float mv = sk_u2f((j & 1) ? (w & 0xffff0000u) : (w << 16));
                v[j] = acc[nt][4 * g + j] * act_grad(mv, ekind, p.slope) * p.out_scale;
              }
            } else {
#pragma unroll
              for (int j = 0; j < 4; j++) v[j] = apply_act(acc[nt][4 * g + j], ekind, p.slope) * p.out_scale;
            }
            if (vecy) {
              const sk_u32x4 q = {sk_f2u(v[0]), sk_f2u(v[1]), sk_f2u(v[2]), sk_f2u(v[3])};
              __builtin_amdgcn_raw_buffer_store_b128(q, ry, (youtp && c0 + 3 < LY.rows) ? (int)((n * p.ldy + c0) * 4) : SK_OOB, 0, 0);
            } else {
#pragma unroll
              for (int j = 0; j < 4; j++)
                __builtin_amdgcn_raw_buffer_store_b32(sk_f2u(v[j]), ry, (youtp && c0 + j < LY.rows) ? (int)((n * p.ldy + c0 + j) * 4) : SK_OOB, 0, 0);
            }
          }
        }
    }
  }
  SK_T(4)
  SK_PROF_END(5)
}

int pstack_plan(PsP& p, const PsLayer* host_layers, bool precise) {
  static int nw_env = -1;
  if (nw_env < 0) nw_env = crk_sw().ps_nw;
  p.hl = p.hr = 0;
  int max_kp = 16, max_rows = 32;
  for (int l = 0; l < p.L; l++) {
    const PsLayer& y = host_layers[l];
    const int o0 = y.off0, o1 = y.off0 + (y.k - 1) * y.dil;
    if (-o0 > SK_GUARD || o1 > SK_GUARD || o0 > 0 || o1 < 0) return CRK_ERR_UNSUPPORTED;
    if (y.rows_pad > 128 || y.kp > 128 || (y.rows_pad & 31) || (y.kp & 15) || y.k < 1 || y.k > 8) return CRK_ERR_UNSUPPORTED;
    if ((l + 1 < p.L || p.tail) && host_layers[l + 1].kp > y.rows_pad) return CRK_ERR_UNSUPPORTED;
    p.hl += -o0; p.hr += o1;
    if (y.kp > max_kp) max_kp = y.kp;
    if (y.rows_pad > max_rows) max_rows = y.rows_pad;
  }
  // 256-frame windows (8 waves, two per SIMD) measured ~2 % better than 128-frame ones for every chain
  // of the step, pointwise ones included; bf16x3 keeps 4 waves (LDS)
  p.nw = precise ? 4 : (nw_env == 4 || nw_env == 8 ? nw_env : 8);
  p.os = max_kp * 2 + 16;
  const int R = p.nw * 32;
  p.tmo = R - p.hl - p.hr;
  if (p.tmo < 32) return CRK_ERR_UNSUPPORTED;
  p.tiles_per_utt = ceil_div(p.T, p.tmo);
  p.tmo = ceil_div(p.T, p.tiles_per_utt);
  const int obytes = (SK_GUARD * 2 + R) * p.os;
  // chunk buffer: whole layers where they fit the staging registers and what LDS is left (two buffers; bf16x3 keeps
  // one hi + one lo), never less than one tap of the largest layer
  const int nl = p.L + (p.tail ? 1 : 0);
  const int misc = p.L * 128 * 4 + (p.L + 1) * (int)sizeof(PsLayer) + 64;
  static int lds_cap = -1;
  if (lds_cap < 0) lds_cap = 160;
  const int avail = (lds_cap * 1024 - (precise ? 2 : 1) * obytes - misc) / 2;
  const int cap = PS_MAXP(p.nw * 64) * p.nw * 64;
  int need = 0, one = 0;
  for (int l = 0; l < nl && l < p.L; l++) {
    const PsLayer& y = host_layers[l];
    const int tap_bytes = y.rows_pad * (y.kp * 2 + 16);
    if (y.rows_pad * (y.kp >> 3) > cap) return CRK_ERR_UNSUPPORTED;
    if (tap_bytes > one) one = tap_bytes;
    const int t = ps_tpc(y.k, y.rows_pad, y.kp, cap, avail);
    if (t * tap_bytes > need) need = t * tap_bytes;
  }
  if (one > avail) return CRK_ERR_UNSUPPORTED;
  p.w_bytes = (need + 15) & ~15;
  (void)max_rows;
  int off = obytes;
  p.o_olo = off; if (precise) off += obytes;
  p.o_whi = off; off += precise ? p.w_bytes : 2 * p.w_bytes;
  p.o_wlo = off; if (precise) off += p.w_bytes;
  p.o_bias = off; off += p.L * 128 * 4;
  p.o_tab = off; off += (p.L + 1) * (int)sizeof(PsLayer);
  p.lds_bytes = (off + 15) & ~15;
  {  // algorithmic bytes per frame: fp32 input row, fp32 output row, every kept operand plane, every mask plane read
    double b = 4.0 * p.cin + (p.y ? 4.0 * host_layers[p.L - 1].rows : 0.0);
    for (int l = 0; l < p.L; l++) {
      if (p.save_hi) b += 2.0 * host_layers[l].kp;
      if (host_layers[l].epi >= 3) b += 2.0 * host_layers[l].mask_w;
    }
    if (p.save_hi && p.tail) b += 2.0 * host_layers[p.L].kp;
    p.algo_bytes = b * (double)p.B * p.T;
  }
  return p.lds_bytes <= 160 * 1024 ? CRK_OK : CRK_ERR_UNSUPPORTED;
}

int launch_pstack(const PsP& p, bool precise, double flops, hipStream_t s) {
  CRK_RAISE_LDS_ONCE(160 * 1024, pstack_kernel<true, 4>, pstack_kernel<false, 4>, pstack_kernel<false, 8>)
  dim3 grid(p.B * p.tiles_per_utt);
  conv_prof_bytes(4, p.algo_bytes);
  conv_prof_begin(4, flops, s);
  if (precise) hipLaunchKernelGGL((pstack_kernel<true, 4>), grid, dim3(256), p.lds_bytes, s, p);
  else if (p.nw == 4) hipLaunchKernelGGL((pstack_kernel<false, 4>), grid, dim3(256), p.lds_bytes, s, p);
  else hipLaunchKernelGGL((pstack_kernel<false, 8>), grid, dim3(512), p.lds_bytes, s, p);
  conv_prof_end(4, s);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}
