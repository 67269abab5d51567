// One wave's tile of a residual layer, the one body of vocoder_kernels.hip (voc_layer_kernel) and voc_stream_kernels.hip
// (vs_layer_kernel): tap gather -> gate GEMM -> tanh * sigmoid -> out / skip GEMM -> epilogue (and, in the last layer, the
// tail).  Included as text inside the kernel's tile scope - as a function the same statements reach the scheduler in another
// order and the offline kernel measured 2.3 % slower (profiles/voc_stream_ab.txt); included, its tile loop compiles to the
// instruction sequence it had before the body moved here.  Lane (r, h) owns sample n (column r) and half h of every k-step.
// Expects in scope:
//   P, FIRST, LAST       the kernel's template flags
//   aw                   const VocLayerW&: the layer's weights
//   lds                  const unsigned char*: the layer's hi fragments in LDS (voc_layer_fill_lds)
//   n, valid, dil, lane  the lane's sample, whether it is one, the layer's dilation, the lane in its wave
//   loc                  where sample positions live:
//     inside(m)            position m is a sample of n's utterance (a tap outside it is zero)
//     noise(m)             the noise sample (FIRST: first_conv is computed on the fly)
//     xin(m) / xout(n)     the row of 64 residual channels the layer reads / writes
//     skip(n)              the row of 64 partial skip sums
//     chi(n) / clo(n)      the row of auxp conditioning values, bf16 hi / lo
//     y(n)                 the waveform sample (LAST)
  const int kq = aw.kq, h = lane >> 5;
  const unsigned char* lgate = lds;
  const unsigned char* los = lds + (size_t)4 * kq * 64 * 16;
  const float rs = 0.70710678118654752f;  // sqrt(0.5)
  f32x16 acc[4];
  for (int t = 0; t < 4; ++t) acc[t] = (f32x16){0.f};
  // gate conv: three dilated taps of x (k-steps 0..11) ...
#pragma unroll 1
  for (int tap = 0; tap < 3; ++tap) {
    const int m = n + (tap - 1) * dil;
    const bool in = valid && loc.inside(m);
    for (int cb = 0; cb < 4; ++cb) {
      float v[8];
      const int c0 = cb * 16 + 8 * h;
      if (in) {
        if (FIRST) {
          const float nz = loc.noise(m);
          for (int j = 0; j < 8; ++j) v[j] = fmaf(aw.first[c0 + j], nz, aw.first[VOC_RES + c0 + j]);
        } else {
          const float* xr = loc.xin(m);
          const float4 p = *reinterpret_cast<const float4*>(xr + c0);
          const float4 q = *reinterpret_cast<const float4*>(xr + c0 + 4);
          v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
        }
      } else {
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
      }
      bf16x8 bh, bl;
      voc_split8<P>(v, bh, bl);
      const int q = tap * 4 + cb;
      for (int t = 0; t < 4; ++t) {
        const size_t fi = ((size_t)(t * kq + q) * 64 + lane);
        acc[t] = voc_mma<P>(acc[t], lds_frag(lgate + fi * 16), aw.gw_lo + fi * 8, bh, bl);
      }
    }
  }
  // ... and the upsampled conditioning (k-steps 12..kq-1): conv1x1_aux
#pragma unroll 1
  for (int cb = 0; cb < (aw.auxp >> 4); ++cb) {
    uint4 uh = make_uint4(0, 0, 0, 0), ul = make_uint4(0, 0, 0, 0);
    if (valid) {
      const int o = cb * 16 + 8 * h;
      uh = *reinterpret_cast<const uint4*>(loc.chi(n) + o);
      if (P) ul = *reinterpret_cast<const uint4*>(loc.clo(n) + o);
    }
    const bf16x8 bh = __builtin_bit_cast(bf16x8, uh), bl = __builtin_bit_cast(bf16x8, ul);
    const int q = 12 + cb;
    for (int t = 0; t < 4; ++t) {
      const size_t fi = ((size_t)(t * kq + q) * 64 + lane);
      acc[t] = voc_mma<P>(acc[t], lds_frag(lgate + fi * 16), aw.gw_lo + fi * 8, bh, bl);
    }
  }
  // gate: z[c] = tanh(a[c]) * sigmoid(a[c + 64]); register i of tile t holds row (i&3) + 8(i>>2) + 4h
  bf16x8 zh[4], zl[4];
  for (int mt = 0; mt < 2; ++mt) {
    float z[16];
    for (int i = 0; i < 16; ++i) {
      const int c = 32 * mt + (i & 3) + 8 * (i >> 2) + 4 * h;
      z[i] = voc_tanh(acc[mt][i] + aw.gb[c]) * voc_sigmoid(acc[mt + 2][i] + aw.gb[64 + c]);
    }
    // registers 8s..8s+7 are the B fragment of k-step (mt, s); the A fragments carry the matching k permutation
    voc_split8<P>(z, zh[2 * mt], zl[2 * mt]);
    voc_split8<P>(z + 8, zh[2 * mt + 1], zl[2 * mt + 1]);
  }
  f32x16 o[4];
  for (int t = 0; t < 4; ++t) {
    o[t] = (f32x16){0.f};
    for (int ks = 0; ks < 4; ++ks) {
      const size_t fi = ((size_t)(t * 4 + ks) * 64 + lane);
      o[t] = voc_mma<P>(o[t], lds_frag(los + fi * 16), aw.ow_lo + fi * 8, zh[ks], zl[ks]);
    }
  }
  // epilogue: x' = (out + b + x) sqrt(.5); skip += s + b
  for (int g = 0; g < 4; ++g) {
    if (!LAST && valid) {
      for (int t = 0; t < 2; ++t) {
        const int c = 32 * t + 8 * g + 4 * h;
        float xr[4];
        if (FIRST) {
          const float nz = loc.noise(n);
          for (int k = 0; k < 4; ++k) xr[k] = fmaf(aw.first[c + k], nz, aw.first[VOC_RES + c + k]);
        } else {
          const float4 p = *reinterpret_cast<const float4*>(loc.xin(n) + c);
          xr[0] = p.x; xr[1] = p.y; xr[2] = p.z; xr[3] = p.w;
        }
        float4 w;
        w.x = (o[t][4 * g + 0] + aw.ob[c + 0] + xr[0]) * rs;
        w.y = (o[t][4 * g + 1] + aw.ob[c + 1] + xr[1]) * rs;
        w.z = (o[t][4 * g + 2] + aw.ob[c + 2] + xr[2]) * rs;
        w.w = (o[t][4 * g + 3] + aw.ob[c + 3] + xr[3]) * rs;
        *reinterpret_cast<float4*>(loc.xout(n) + c) = w;
      }
    }
    for (int t = 2; t < 4; ++t) {
      const int c = 32 * (t - 2) + 8 * g + 4 * h;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!FIRST && valid) p = *reinterpret_cast<const float4*>(loc.skip(n) + c);
      p.x += o[t][4 * g + 0] + aw.ob[64 + c + 0];
      p.y += o[t][4 * g + 1] + aw.ob[64 + c + 1];
      p.z += o[t][4 * g + 2] + aw.ob[64 + c + 2];
      p.w += o[t][4 * g + 3] + aw.ob[64 + c + 3];
      if (LAST) {
        o[t][4 * g + 0] = p.x; o[t][4 * g + 1] = p.y; o[t][4 * g + 2] = p.z; o[t][4 * g + 3] = p.w;
      } else if (valid) {
        *reinterpret_cast<float4*>(loc.skip(n) + c) = p;
      }
    }
  }
  if (LAST) {
    // tail: y = w2 . relu(W1 relu(skip sqrt(1/L)) + b1) + b2; the skip tiles are W1's B operand in place
    bf16x8 sh[4], sl[4];
    for (int mt = 0; mt < 2; ++mt) {
      float v[16];
      for (int i = 0; i < 16; ++i) v[i] = fmaxf(o[mt + 2][i] * aw.skip_scale, 0.f);
      voc_split8<P>(v, sh[2 * mt], sl[2 * mt]);
      voc_split8<P>(v + 8, sh[2 * mt + 1], sl[2 * mt + 1]);
    }
    float part = 0.f;
    for (int t = 0; t < 2; ++t) {
      f32x16 y1 = (f32x16){0.f};
      for (int ks = 0; ks < 4; ++ks) {
        const size_t fi = ((size_t)(t * 4 + ks) * 64 + lane);
        const bf16x8 ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(aw.tw_hi + fi * 8));
        y1 = voc_mma<P>(y1, ah, aw.tw_lo + fi * 8, sh[ks], sl[ks]);
      }
      for (int i = 0; i < 16; ++i) {
        const int c = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
        part = fmaf(aw.tail[64 + c], fmaxf(y1[i] + aw.tail[c], 0.f), part);
      }
    }
    part += __shfl_xor(part, 32);
    if (valid && h == 0) *loc.y(n) = part + aw.tail[128];
  }
