// Included by conv_kernels.hip: the batched weight-gradient kernel.
#define WG_FR 64
#define WG_MAXJ 10
#define WG_LDS __attribute__((address_space(3)))
typedef short v4s __attribute__((ext_vector_type(4)));

// MFMA operand fragment (8 consecutive frames of one channel per lane) out of a ROW-MAJOR
// [frame][channel] bf16 LDS tile with the gfx950 transpose read: in every 16-lane group lane
// i supplies the address of (row i>>2, 4-channel chunk i&3) and receives rows 0..3 of
// column i (verified on hardware, tests/probe/tr_probe.hip).  p0 already includes this
// lane's (row, chunk) offset; the second read takes the 4 rows below.
__device__ __forceinline__ bf16x8 lds_tr_frag(const unsigned char* p0, int rs) {
  const v4s a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((WG_LDS v4s*)(p0));
  const v4s b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((WG_LDS v4s*)(p0 + 4 * rs));
  typedef short v8s __attribute__((ext_vector_type(8)));
  v8s r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return *reinterpret_cast<bf16x8*>(&r);
}

template <bool PRECISE>
__device__ __forceinline__ void wg_store_row(unsigned char* hi, unsigned char* lo, const float v[4]) {
  *reinterpret_cast<uint2*>(hi) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
  if (PRECISE) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = v[j] - bf2f(f2bf(v[j]));
    *reinterpret_cast<uint2*>(lo) = make_uint2(pack_bf2(r[0], r[1]), pack_bf2(r[2], r[3]));
  }
}

// row stride of a [frame][channel] bf16 tile: +64 B puts 4 consecutive rows on 4 distinct
// quarter bank-rows, which is what a 32-lane half of the transpose read touches
static __host__ __device__ inline int wg_row_stride(int ch_pad) { return ch_pad * 2 + 64; }

// ------------------------------------------------------------------------------
// weight gradient: dW[tap][co][ci] = sum_n dY[n,co] * Xp[n+off0+tap*dil, ci]
//
// One launch covers EVERY weight-gradient problem of a stack's backward pass
// (blockIdx.y = entry of a device table) for a group of utterances (blockIdx.x).
// A workgroup walks its utterances in 64-frame chunks.  dY and the conv input (with the
// forward prologue applied, plus the tap-span halo rows) are staged ROW-MAJOR as bf16 -
// coalesced 16-byte global loads, one 8-byte LDS store per 4 channels - and both MFMA
// operands, which must be contiguous along the reduction (frame) axis, come out of LDS
// through ds_read_b64_tr_b16.  A tap is just a row offset into the input tile, so every
// tap reuses the same tiles and the same dY fragments: a wave owns one 32-channel band of
// dY and up to 10 (tap, cin-band) output tiles.  Per-group partial sums are written once
// and reduced in fixed order by the weight-norm backward kernel (deterministic, no atomics).
// ------------------------------------------------------------------------------
// prefetch registers: 8 dY rows and up to 11 input rows per thread (named fields: they live
// across the runtime chunk loop, see WRegs)
struct WgRegs {
  float4 a0, a1, a2, a3, a4, a5, a6, a7;
  float4 b0, b1, b2, b3, b4, b5, b6, b7, b8, b9, b10;
};
#define WG_A_ALL(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define WG_B_ALL(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)

template <bool PRECISE>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradP* __restrict__ jobs, int B, int T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float bias_red[256 * 4];
  const WgradP p = jobs[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  if (g >= p.ngroups) return;  // this table entry uses fewer partial-sum groups than the widest one
  const bool is_aux = p.grp_aux != 0;
  const float* xsrc = is_aux ? p.xc : p.x;
  const int ldx = is_aux ? p.ldc : p.ldx;
  const int cx = is_aux ? p.cc : p.cx;
  const int cx_pad = is_aux ? p.cc_pad : p.cx_pad;  // multiples of 32
  const int ntap = is_aux ? 1 : p.grp_ntap;
  const int shift0 = is_aux ? 0 : p.off0 + p.grp_tap0 * p.dil;
  const int dil = is_aux ? 0 : p.dil;
  const int nfs = WG_FR + (ntap - 1) * dil;  // conv-input rows per chunk (64 + tap span)
  const int RA = wg_row_stride(p.ca_pad), RB = wg_row_stride(cx_pad);
  const int abytes = (WG_FR * RA + 15) & ~15, bbytes = (nfs * RB + 15) & ~15;
  unsigned char* at_hi = smem;
  unsigned char* at_lo = smem + abytes;
  unsigned char* bt_hi = smem + (PRECISE ? 2 : 1) * abytes;
  unsigned char* bt_lo = bt_hi + bbytes;

  const int nct = p.ca_pad >> 5, nit = cx_pad >> 5, njt = ntap * nit;
  const int nctp = nct <= 1 ? 1 : (nct <= 2 ? 2 : 4);
  const int ct = wave % nctp, j0 = wave / nctp, jstep = 4 / nctp;
  const bool wave_on = ct < nct;
  // transpose-read lane geometry
  const int i15 = lane & 15, grp = lane >> 4;
  const int rowoff = (grp >> 1) * 8 + (i15 >> 2);
  const int coloff = (grp & 1) * 16 + (i15 & 3) * 4;
  const int half = lane >> 5, l31 = lane & 31;

  f32x16 acc[WG_MAXJ];
#pragma unroll
  for (int a = 0; a < WG_MAXJ; a++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[a][i] = 0.f;
  const bool do_bias = p.bias_partial && !is_aux && p.grp_tap0 == 0;
  float bs[4] = {0.f, 0.f, 0.f, 0.f};  // this thread's 4 dY columns, summed over its rows

  // staging geometry: a thread owns one channel quad and walks rows
  const int nqa = p.ca_pad >> 2, nqb = cx_pad >> 2;  // 8..32 quads per row
  const int qa = tid % nqa, ra0 = tid / nqa, ras = 256 / nqa;
  const int qb = tid % nqb, rb0 = tid / nqb, rbs = 256 / nqb;
  const bool a_on = ra0 < ras, b_on = rb0 < rbs;
  const int ca4 = qa << 2, cb4 = qb << 2;
  const bool vec1 = ((p.lda1 & 3) == 0) && ((p.ca1 & 3) == 0) && ((((uintptr_t)p.a1) & 15) == 0);
  const bool vec2 = ((p.lda2 & 3) == 0) && ((p.ca1 & 3) == 0) && ((p.ca2 & 3) == 0) && ((((uintptr_t)p.a2) & 15) == 0);
  const bool vecX = ((ldx & 3) == 0) && ((cx & 3) == 0) && ((((uintptr_t)xsrc) & 15) == 0);
  // which dY source feeds this thread's quad (fixed for the whole kernel)
  const float* asrc = nullptr;
  int alda = 0, aoff = 0;
  float asc = 1.f;
  bool avec = false, amixed = false;
  if (ca4 + 3 < p.ca1) { asrc = p.a1; alda = p.lda1; aoff = ca4; asc = p.sa1; avec = vec1; }
  else if (ca4 >= p.ca1 && ca4 + 3 < p.ca) { asrc = p.a2; alda = p.lda2; aoff = ca4 - p.ca1; asc = p.sa2; avec = vec2; }
  else amixed = ca4 < p.ca;

  // ---- software-pipelined chunk loop: the next chunk's rows travel from HBM into
  // registers while the current chunk feeds the MFMAs (one or two workgroups per CU
  // cannot hide a load -> convert -> LDS chain any other way) ----
  // a group is a run of consecutive 64-frame chunks of the batch (chunk c = utterance c / ncpu,
  // frames (c % ncpu) * 64 ...): small problems get many short groups, i.e. many workgroups
  const int ncpu = (T + WG_FR - 1) / WG_FR;
  const int c_beg = g * p.cpg, c_end = min(B * ncpu, (g + 1) * p.cpg);
  const int nchunks = c_end > c_beg ? c_end - c_beg : 0;
  WgRegs R;
#define WG_FETCH_A(u)                                                                                   \
  {                                                                                                     \
    const int r = ra0 + u * ras, t = f0n + r;                                                           \
    float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);                                                        \
    if (a_on && r < WG_FR && t < T) {                                                                   \
      const long n = nbn + t;                                                                           \
      if (asrc && avec) f4 = *reinterpret_cast<const float4*>(asrc + n * alda + aoff);                  \
      else if (asrc) { f4.x = asrc[n * alda + aoff]; f4.y = asrc[n * alda + aoff + 1];                  \
                       f4.z = asrc[n * alda + aoff + 2]; f4.w = asrc[n * alda + aoff + 3]; }            \
      else if (amixed) {                                                                                \
        float m[4];                                                                                     \
        for (int j = 0; j < 4; j++) {                                                                   \
          const int c = ca4 + j;                                                                        \
          m[j] = 0.f;                                                                                   \
          if (c < p.ca1) m[j] = p.a1 ? p.a1[n * p.lda1 + c] * (p.sa1 / asc) : 0.f;                      \
          else if (c < p.ca) m[j] = p.a2 ? p.a2[n * p.lda2 + (c - p.ca1)] * (p.sa2 / asc) : 0.f;        \
        }                                                                                               \
        f4 = make_float4(m[0], m[1], m[2], m[3]);                                                       \
      }                                                                                                 \
    }                                                                                                   \
    R.a##u = f4;                                                                                        \
  }
#define WG_FETCH_B(u)                                                                                   \
  {                                                                                                     \
    const int r = rb0 + u * rbs, t = f0n + shift0 + r;                                                  \
    float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);                                                        \
    if (b_on && r < nfs && t >= 0 && t < T) {                                                           \
      const long n = nbn + t;                                                                           \
      if (vecX && cb4 + 3 < cx) f4 = *reinterpret_cast<const float4*>(xsrc + n * ldx + cb4);            \
      else {                                                                                            \
        if (cb4 < cx) f4.x = xsrc[n * ldx + cb4];                                                       \
        if (cb4 + 1 < cx) f4.y = xsrc[n * ldx + cb4 + 1];                                               \
        if (cb4 + 2 < cx) f4.z = xsrc[n * ldx + cb4 + 2];                                               \
        if (cb4 + 3 < cx) f4.w = xsrc[n * ldx + cb4 + 3];                                               \
      }                                                                                                 \
    }                                                                                                   \
    R.b##u = f4;                                                                                        \
  }
#define WG_COMMIT_A(u)                                                                                  \
  {                                                                                                     \
    const int r = ra0 + u * ras;                                                                        \
    if (a_on && r < WG_FR) {                                                                            \
      const float v[4] = {R.a##u.x * asc, R.a##u.y * asc, R.a##u.z * asc, R.a##u.w * asc};              \
      wg_store_row<PRECISE>(at_hi + r * RA + ca4 * 2, at_lo + r * RA + ca4 * 2, v);                     \
      /* the bias gradient sums what the MFMAs consume: plain bf16 the rounded values (as the fused kernels do) */ \
      for (int j = 0; j < 4; j++) bs[j] += PRECISE ? v[j] : bf2f(f2bf(v[j]));                           \
    }                                                                                                   \
  }
#define WG_COMMIT_B(u)                                                                                  \
  {                                                                                                     \
    const int r = rb0 + u * rbs;                                                                        \
    if (b_on && r < nfs) {                                                                              \
      float v[4] = {R.b##u.x, R.b##u.y, R.b##u.z, R.b##u.w};                                            \
      if (!is_aux) {                                                                                    \
        const long n = nbc + f0c + shift0 + r;                                                          \
        for (int j = 0; j < 4; j++) {                                                                   \
          float x = apply_act(v[j] * p.sx, p.act_in, p.slope);                                          \
          if (p.drop_p > 0.f) x *= dropout_scale(crk_seed(p.drop_seed, p.drop_seed_ptr), (unsigned long long)n * p.cx + cb4 + j, p.drop_p); \
          v[j] = (cb4 + j < cx) ? x : 0.f;                                                              \
        }                                                                                               \
      }                                                                                                 \
      wg_store_row<PRECISE>(bt_hi + r * RB + cb4 * 2, bt_lo + r * RB + cb4 * 2, v);                     \
    }                                                                                                   \
  }
  long nbn = (long)(c_beg / ncpu) * T;  // "next" chunk coordinates (the one being fetched)
  int f0n = (c_beg % ncpu) * WG_FR;
  if (nchunks > 0) { WG_A_ALL(WG_FETCH_A) WG_B_ALL(WG_FETCH_B) }
  for (int c = 0; c < nchunks; c++) {
    const long nbc = nbn;  // "current" = what the registers hold
    const int f0c = f0n;
    __syncthreads();  // previous chunk's fragments consumed
    if (!(p.dbg & 8192)) { WG_A_ALL(WG_COMMIT_A) }
    if (!(p.dbg & 4096)) { WG_B_ALL(WG_COMMIT_B) }
    __syncthreads();
    if (c + 1 < nchunks) {
      f0n += WG_FR;
      if (f0n >= T) { f0n = 0; nbn += T; }
      WG_A_ALL(WG_FETCH_A) WG_B_ALL(WG_FETCH_B)
    }
    (void)nbc; (void)f0c;
    if (wave_on && !(p.dbg & 2048)) {
      const unsigned char* ap_hi = at_hi + rowoff * RA + (ct * 32 + coloff) * 2;
      const unsigned char* ap_lo = at_lo + rowoff * RA + (ct * 32 + coloff) * 2;
      const unsigned char* bp_hi = bt_hi + rowoff * RB + coloff * 2;
      const unsigned char* bp_lo = bt_lo + rowoff * RB + coloff * 2;
#pragma unroll
      for (int kc = 0; kc < WG_FR / 16; kc++) {
        const bf16x8 a_hi = lds_tr_frag(ap_hi + kc * 16 * RA, RA);
        bf16x8 a_lo;
        if (PRECISE) a_lo = lds_tr_frag(ap_lo + kc * 16 * RA, RA);
#pragma unroll
        for (int a = 0; a < WG_MAXJ; a++) {
          const int jt = j0 + a * jstep;
          if (jt < njt) {
            const int tl = jt / nit, it = jt - tl * nit;
            const int boff = (kc * 16 + tl * dil) * RB + it * 64;
            const bf16x8 b_hi = lds_tr_frag(bp_hi + boff, RB);
            acc[a] = mfma_bf16(a_hi, b_hi, acc[a]);
            if (PRECISE) {
              const bf16x8 b_lo = lds_tr_frag(bp_lo + boff, RB);
              acc[a] = mfma_bf16(a_lo, b_hi, acc[a]);
              acc[a] = mfma_bf16(a_hi, b_lo, acc[a]);
            }
          }
        }
      }
    }
  }
#undef WG_FETCH_A
#undef WG_FETCH_B
#undef WG_COMMIT_A
#undef WG_COMMIT_B

  // ---- write this group's partial sums ----
  if (wave_on) {
#pragma unroll
    for (int a = 0; a < WG_MAXJ; a++) {
      const int jt = j0 + a * jstep;
      if (jt < njt) {
        const int tl = jt / nit, it = jt - tl * nit;
        const int ci = it * 32 + l31;
        float* out = is_aux ? p.partial_aux + (long)g * p.ca * p.cc
                            : p.partial + ((long)g * p.ktaps + p.grp_tap0 + tl) * p.ca * p.cx;
        if (ci < cx) {
#pragma unroll
          for (int i = 0; i < 16; i++) {
            const int co = ct * 32 + cd_row(i, half);
            if (co < p.ca) out[(long)co * cx + ci] = acc[a][i];
          }
        }
      }
    }
  }
  if (do_bias) {  // fixed-order reduction over the row groups that share a quad
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) bias_red[tid * 4 + j] = a_on ? bs[j] : 0.f;
    __syncthreads();
    if (tid < p.ca) {
      const int q = tid >> 2, j = tid & 3;
      float s = 0.f;
      for (int r = 0; r < ras; r++) s += bias_red[(r * nqa + q) * 4 + j];
      p.bias_partial[(long)g * p.ca + tid] = s;
    }
  }
}

// LDS bytes one table entry needs
int wgrad_entry_lds(const WgradP& p, bool precise) {
  const int cxp = p.grp_aux ? p.cc_pad : p.cx_pad;
  const int nfs = WG_FR + (p.grp_aux ? 0 : (p.grp_ntap - 1) * p.dil);
  const int abytes = round_up(WG_FR * wg_row_stride(p.ca_pad), 16), bbytes = round_up(nfs * wg_row_stride(cxp), 16);
  return (precise ? 2 : 1) * (abytes + bbytes);
}
