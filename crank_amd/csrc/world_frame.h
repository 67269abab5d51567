// The arithmetic of WORLD synthesis, one body per piece (DESIGN.md sections 6b and 6p): the energy recursion of a
// mel-cepstrum, a frame's sp / ap bin, one sample of the time base (its phase increment, the wrap and the pulse test) and
// one pulse's response.  The offline kernels (world_kernels.hip) and the streaming kernels (world_stream_kernels.hip) call
// the same bodies, so a stream holds the bits the whole utterance gives.  Every `#pragma clang fp contract(off)` stays
// with the body it protects.
#pragma once
#include "signal_common.h"

#define W_IRLEN 1024
#define W_MAX_ORDER1 128
#define W_CHUNK 2048
#define W_SAFE 1e-12
#define W_DEFAULT_F0 500.0

// cos(x) for x in [0, pi] as the Taylor polynomial in x^2 (16 terms, Horner), each operation rounded on its own.
// WORLD's delay takes sin as sqrt(1 - cos^2), which turns a last-bit difference of cos at small x into a large one of
// sin; tests/world_synth_ref.py evaluates the same polynomial, so both get the same bits.
static __constant__ double W_COS[16] = {1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07, 2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16, 4.110317623312165e-19, -8.896791392450574e-22, 1.6117375710961184e-24, -2.4795962632247976e-27, 3.279889237069838e-30, -3.7699876288159054e-33};
__device__ inline double w_cos(double x) {
#pragma clang fp contract(off)
  const double x2 = x * x;
  double r = W_COS[15];
  for (int n = 14; n >= 0; --n) r = r * x2 + W_COS[n];
  return r;
}

// ---------------------------------------------------------------------------------------------------------- per frame
// mc2e of one mel-cepstrum row by one wave: c = freqt(mc, 1024, -alpha) through `at`, then SPTK c2ir's recursion with h in
// the wave's LDS row; lane l holds k c_k for k = l + 64 j in registers.  Every lane returns sum h^2.
__device__ __forceinline__ double w_energy_row(const double* __restrict__ mc, int m1, const double* __restrict__ at,
                                               double* h, int lane) {
  double kc[W_IRLEN / 64];
#pragma unroll
  for (int j = 0; j < W_IRLEN / 64; ++j) kc[j] = 0.0;
  for (int i = 0; i < m1; ++i) {
    const double v = mc[i];
    const double* row = at + (size_t)i * W_IRLEN + lane;
#pragma unroll
    for (int j = 0; j < W_IRLEN / 64; ++j) kc[j] = fma(row[64 * j], v, kc[j]);
  }
  const double c0 = __shfl(kc[0], 0);
#pragma unroll
  for (int j = 0; j < W_IRLEN / 64; ++j) kc[j] *= (double)(lane + 64 * j);
  double h0 = exp(c0);
  if (lane == 0) h[0] = h0;
  double en = h0 * h0;
  for (int n = 1; n < W_IRLEN; ++n) {
    __builtin_amdgcn_wave_barrier();
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < W_IRLEN / 64; ++j) {
      const int k = lane + 64 * j;
      if (64 * j <= n && k >= 1 && k <= n) acc = fma(kc[j], h[n - k], acc);
    }
    const double hn = w_wave_sum(acc) / n;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) h[n] = hn;
    en = fma(hn, hn, en);
  }
  return en;
}

// sp and decoded ap of bin k of one frame; e: the frame's (mcep, rmcep) energies, or null without power modification
__device__ __forceinline__ void w_frame_bin(const double* __restrict__ mc, const double* __restrict__ cp, int m1, int bands,
                                            int fs, int k, const double* __restrict__ wt, const double* __restrict__ e,
                                            double* __restrict__ sp, double* __restrict__ ap) {
  double acc = 0.0;
  for (int i = 0; i < m1; ++i) {
    double v = mc[i];
    if (i == 0 && e) v += log(e[1] / e[0]) / 2.0;
    acc = fma(wt[(size_t)i * W_K + k], v, acc);
  }
  *sp = exp(acc);
  // WORLD DecodeAperiodicity: knots (0, -60 dB), (3000 b, cap[b-1]), (fs / 2, -1e-12); unvoiced frames 1 - 1e-12
  double mean = 0.0;
  for (int b = 0; b < bands; ++b) mean += cp[b];
  mean /= bands;
  double a = 1.0 - W_SAFE;
  if (!(mean > -0.5)) {
    const double fk = (double)fs / W_N * k;
    int j = 0;
    while (j + 1 <= bands && 3000.0 * (j + 1) <= fk) ++j;  // the last knot at or below fk, at most `bands`
    const double x0 = 3000.0 * j, x1 = j + 1 <= bands ? 3000.0 * (j + 1) : fs / 2.0;
    const double y0 = j == 0 ? -60.0 : cp[j - 1], y1 = j + 1 <= bands ? cp[j] : -W_SAFE;
    const double s = (fk - x0) / (x1 - x0);
    a = pow(10.0, (y0 + s * (y1 - y0)) / 20.0);
  }
  *ap = a;
}

// ---------------------------------------------------------------------------------------------------------- time base
// The frame of sample i: the last j in [0, T - 1] with j fp <= i / fs (WORLD's histc), from the quotient and two walks.
__device__ __forceinline__ long long w_frame_of(long long i, long long T, double fsd, double fp) {
#pragma clang fp contract(off)
  const double xi = (double)i / fsd;
  long long j = (long long)(xi / fp);
  j = max(0LL, min(j, T - 1));
  while (j > 0 && (double)j * fp > xi) --j;
  while (j + 1 < T && (double)(j + 1) * fp <= xi) ++j;
  return j;
}

// Sample i's phase increment 2 pi f / fs and its vuv, from the coarse F0 of frames j and j + 1 of a contour of T frames
// (f0(j), j < T: the raw row; knot T is the extrapolated point 2 cf(T-1) - cf(T-2)).
template <class F0>
__device__ __forceinline__ double w_phase_increment(long long i, long long T, int fs, double fp, F0 f0, unsigned char* vuv) {
#pragma clang fp contract(off)
  const double fsd = (double)fs, two_pi = 2.0 * M_PI;
  const double lowest = (double)(fs / W_N) + 1.0;
  auto cf = [&](long long j) {  // coarse F0 / vuv at knot j (j == T: the extrapolated point)
    if (j < T) return f0(j) < lowest ? 0.0 : f0(j);
    const double p = f0(T - 1) < lowest ? 0.0 : f0(T - 1), q = f0(T - 2) < lowest ? 0.0 : f0(T - 2);
    return p * 2 - q;
  };
  auto cv = [&](long long j) {
    if (j < T) return cf(j) == 0.0 ? 0.0 : 1.0;
    return (cf(T - 1) == 0.0 ? 0.0 : 1.0) * 2 - (cf(T - 2) == 0.0 ? 0.0 : 1.0);
  };
  const double xi = (double)i / fsd;
  const long long j = w_frame_of(i, T, fsd, fp);
  const double x0 = (double)j * fp, x1 = (double)(j + 1) * fp;
  const double s = (xi - x0) / (x1 - x0);
  const double v0 = cv(j), v1 = cv(j + 1);
  const double v = v0 + s * (v1 - v0) > 0.5 ? 1.0 : 0.0;
  double fr = W_DEFAULT_F0;
  if (v != 0.0) {
    const double g0 = cf(j), g1 = cf(j + 1);
    fr = g0 + s * (g1 - g0);
  }
  *vuv = (unsigned char)(v != 0.0);
  return two_pi * fr / fsd;
}

__device__ __forceinline__ double w_wrap(double total) { return fmod(total, 2.0 * M_PI); }

// a pulse lies at sample i when the wrapped phase of i + 1 (w1) jumps from that of i (w0)
__device__ __forceinline__ bool w_is_pulse(double w0, double w1) {
#pragma clang fp contract(off)
  return fabs(w1 - w0) > M_PI;
}

__device__ __forceinline__ double w_pulse_shift(double w0, double w1, double fsd) {
#pragma clang fp contract(off)
  const double y1 = w0 - 2.0 * M_PI, y2 = w1;
  return -y1 / (y2 - y1) / fsd;
}

// ---------------------------------------------------------------------------------------------------------- per pulse
struct WPulseTables {
  const double* noise; long long noise_len;
  const double* twc; const double* tws; const double* dcw;
  int fs; double fp;
};

// The response (W_N doubles at `out`) of the pulse at sample s of a contour of T frames, by one workgroup of W_THREADS:
// ns its noise size (0: the utterance's last pulse, a zero response), nbase its offset into the randn table; sp_row(j) /
// ap_row(j) give frame j's W_K values for j in [0, T - 1].  Envelope and ratio, both minimum-phase spectra, the noise
// spectrum and both inverse transforms in four 1024-point fp64 LDS FFTs (two real sequences per complex transform).
template <class SpRow, class ApRow>
__device__ void w_pulse_response(long long s, long long T, int ns, double shift, double vuv, long long nbase,
                                 const WPulseTables& a, SpRow sp_row, ApRow ap_row, double* __restrict__ out) {
#pragma clang fp contract(off)  // 1 - c * c below: a fused c * c would differ from the restatement at small angles
  __shared__ double2 Z[W_N];
  __shared__ double2 Yb[W_N];
  __shared__ double env[W_K], rat[W_K];
  __shared__ double tc[W_N / 2], ts[W_N / 2];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  w_stage_twiddles(tc, ts, a.twc, a.tws);
  // envelope and aperiodic ratio at t = s / fs (WORLD GetSpectralEnvelope / GetAperiodicRatio)
  const double q = (double)s / (double)a.fs / a.fp;
  const long long lo = min(T - 1, (long long)floor(q)), hi = min(T - 1, (long long)ceil(q));
  const double w1 = q - lo;
  const double* sl = sp_row(lo);
  const double* sh = sp_row(hi);
  const double* al = ap_row(lo);
  const double* ah = ap_row(hi);
  for (int k = tid; k < W_K; k += W_THREADS) {
    const double ql = fmax(0.001, fmin(0.999999999999, al[k]));
    if (lo == hi) {
      env[k] = fabs(sl[k]);
      rat[k] = ql * ql;
    } else {
      const double qh = fmax(0.001, fmin(0.999999999999, ah[k]));
      env[k] = (1.0 - w1) * fabs(sl[k]) + w1 * fabs(sh[k]);
      const double r = (1.0 - w1) * ql + w1 * qh;
      rat[k] = r * r;
    }
  }
  __syncthreads();
  const bool per_on = vuv > 0.5 && rat[0] <= 0.999 && ns > 0;
  if (ns <= 0) {  // the last pulse of an utterance: no noise, periodic part times sqrt(0)
    for (int i = tid; i < W_N; i += W_THREADS) out[i] = 0.0;
    return;
  }
  // both log amplitudes as one complex even sequence: FFT -> (periodic cepstrum, aperiodic cepstrum)
  for (int n = tid; n < W_N; n += W_THREADS) {
    const int k = n <= W_N / 2 ? n : W_N - n;
    const double la = per_on ? log(env[k] * (1.0 - rat[k]) + W_SAFE) / 2.0 : 0.0;
    const double lb = vuv != 0.0 ? log(env[k] * rat[k] + W_SAFE) / 2.0 : log(env[k] + W_SAFE) / 2.0;
    Z[w_brev(n)] = make_double2(la, lb);
  }
  __syncthreads();
  w_fft(Z, tc, ts, -1.0);
  // fold (c0, 2 c_1 .. 2 c_{N/2-1}, c_{N/2}, zeros) and transform both folded cepstra at once
  for (int n = tid; n < W_N; n += W_THREADS) {
    double2 c = make_double2(0.0, 0.0);
    if (n <= W_N / 2) {
      const double g = (n == 0 || n == W_N / 2) ? 1.0 : 2.0;
      c = make_double2(g * Z[n].x, g * Z[n].y);
    }
    Yb[w_brev(n)] = c;
  }
  __syncthreads();
  w_fft(Yb, tc, ts, -1.0);
  // zero-mean noise of min(ns, N) samples from the fixed randn stream, zero padded
  const int m = min(ns, W_N);
  double part = 0.0;
  for (int n = tid; n < m; n += W_THREADS) part += a.noise[max(0LL, min(nbase + n, a.noise_len - 1))];
  const double mean = w_block_sum(part, red) / m;
  for (int n = tid; n < W_N; n += W_THREADS)
    Z[w_brev(n)] = make_double2(n < m ? a.noise[max(0LL, min(nbase + n, a.noise_len - 1))] - mean : 0.0, 0.0);
  __syncthreads();
  w_fft(Z, tc, ts, -1.0);
  // spectra: periodic P = exp(A / N) e^{-i theta}, aperiodic Q = exp(B / N) * noise; V = P + i Q, Hermitian halves
  const double coef = 2.0 * M_PI * shift * a.fs / W_N;
  double2 P[3], Q[3];  // k = tid + 256 r
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int k = tid + W_THREADS * r;
    if (k > W_N / 2) break;
    const double2 yk = Yb[k], ym = Yb[(W_N - k) & (W_N - 1)];
    const double Ar = 0.5 * (yk.x + ym.x), Ai = 0.5 * (yk.y - ym.y);
    const double dr = yk.x - ym.x, di = yk.y + ym.y;
    const double Br = 0.5 * di, Bi = -0.5 * dr;
    double2 pk = make_double2(0.0, 0.0);
    if (per_on) {
      const double ea = exp(Ar / W_N), re = ea * cos(Ai / W_N), im = ea * sin(Ai / W_N);
      const double c = w_cos(coef * k), sn = sqrt(fmax(1.0 - c * c, 0.0));
      pk = make_double2(re * c + im * sn, im * c - re * sn);
    }
    const double eb = exp(Br / W_N), mr = eb * cos(Bi / W_N), mi = eb * sin(Bi / W_N);
    const double2 nzk = Z[k];
    double2 qk = make_double2(mr * nzk.x - mi * nzk.y, mr * nzk.y + mi * nzk.x);
    if (k == 0 || k == W_N / 2) { pk.y = 0.0; qk.y = 0.0; }  // a real inverse transform ignores them
    P[r] = pk;
    Q[r] = qk;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int k = tid + W_THREADS * r;
    if (k > W_N / 2) break;
    const double2 pk = P[r], qk = Q[r];
    Z[w_brev(k)] = make_double2(pk.x - qk.y, pk.y + qk.x);
    if (k > 0 && k < W_N / 2) Z[w_brev(W_N - k)] = make_double2(pk.x + qk.y, -pk.y + qk.x);
  }
  __syncthreads();
  w_fft(Z, tc, ts, 1.0);
  // fftshift; the periodic part's DC removal; (periodic sqrt(ns) + aperiodic) / N
  double dcp = 0.0;
  if (per_on) {
    for (int n = tid; n < W_N / 2; n += W_THREADS) dcp += Z[n].x;
    dcp = w_block_sum(dcp, red);
  }
  const double sq = sqrt((double)ns);
  for (int i = tid; i < W_N; i += W_THREADS) {
    const double2 v = Z[(i + W_N / 2) & (W_N - 1)];
    double per = 0.0;
    if (per_on) per = i < W_N / 2 ? -dcp * a.dcw[i] : v.x - dcp * a.dcw[i];
    out[i] = (per * sq + v.y) / W_N;
  }
}
