// Griffin-Lim waveform synthesis for log-mel models on the device (gfx950), all in float64, for a ragged batch of
// utterances.
//
// Replaces the reference's crank.utils.mlfb2wav (crank/utils/utils.py:94-144, 210-269: logmelspc_to_linearspc, then
// librosa.griffinlim with momentum 0.99, centred reflect-padded STFT, periodic Hann window).  The oracle is the CPU
// restatement tests/griffin_lim_ref.py; parity with librosa is unpinned.  Structure:
//  * gl_linear_kernel: one workgroup per frame: 10^mlfb in LDS, then |sum_m 10^mlfb[m] P[k][m]| per bin, ascending m.
//  * gl_frame_kernel<MODE>: one workgroup per frame, the 1024-point fp64 LDS FFT of signal_common.h.
//      GL_INIT    S * angles0 -> inverse FFT -> windowed frame.
//      GL_ITER    gather the padded frame from the previous iteration's windowed frames (overlap-add in ascending frame
//                 order, divided by the window-sum-square envelope, reflected at the two ends), window, FFT, read tprev and
//                 write rebuilt in place, phase update, times S, inverse FFT, window, into the other frame buffer.
//                 rebuilt[t] is consumed only by frame t's phase update, so neither the new spectrogram nor the angles
//                 leave the workgroup un-normalised.
//      GL_STFT / GL_ISTFT   the two projections alone (tests).
//  * gl_ola_kernel: one thread per output sample: the same overlap-add, envelope division, trim and the clip.
// n_iter + 2 launches per call.  No atomics; a frame reads only its own utterance, so an utterance's bits do not depend on
// the batch around it.
#include "../../include/crank_hip.h"
#include "signal_common.h"

#define GL_MAX_MELS 256
#define GL_CLIP_HI 0.999969482421875  // 1 - 2^-15: the reference's upper clip
#define GL_TINY 2.2250738585072014e-308  // the smallest normal float64: below it the envelope does not divide
#define GL_MOMENTUM 0.99
#define GL_PHASE_EPS 1e-16

struct Gl {
  int fs, win, hop, n_mels;
  double coef;     // momentum / (1 + momentum)
  double* tables;  // one device block: tw cos [W_N/2], tw sin [W_N/2], window [W_N], window^2 [W_N], pinv^T [n_mels][W_K]
  const double *twc, *tws, *window, *wsq, *pt;
};

enum { GL_INIT = 0, GL_ITER = 1, GL_STFT = 2, GL_ISTFT = 3 };

struct GlArgs {
  const double* S;         // [F][W_K] magnitudes
  const double2* ang0;     // [F][W_K] initial unit phasors (GL_INIT)
  double2* R;              // [F][W_K] rebuilt of the previous iteration, replaced in place (GL_ITER)
  const double* fin;       // [F][W_N] windowed inverse frames of the previous iteration (GL_ITER)
  double* fout;            // [F][W_N] windowed inverse frames written
  const double* x;         // waveforms (GL_STFT)
  double2* spec_out;       // [F][W_K] (GL_STFT)
  const double2* spec_in;  // [F][W_K] (GL_ISTFT)
  const long long* foff; const long long* soff; int n_utts;
  const double* twc; const double* tws; const double* window; const double* wsq;
  int hop, first;
  double coef;
};

// Sample q of an utterance's overlap-added signal before the trim (q = output sample + W_N / 2), divided by the
// window-sum-square envelope where that exceeds the smallest normal number.  Both sums run over the frames that cover q in
// ascending order, the restatement's order; no contraction, the envelope test hangs on the sum's value.
__device__ __forceinline__ double gl_ola(const double* __restrict__ fr, const double* __restrict__ wsq, long long T,
                                         int hop, long long q) {
#pragma clang fp contract(off)
  const long long lo = q < W_N ? 0 : (q - (W_N - 1) + hop - 1) / hop;
  const long long hi = min(T - 1, q / hop);
  double acc = 0.0, env = 0.0;
  for (long long f = lo; f <= hi; ++f) {
    const int o = (int)(q - f * hop);
    acc += fr[f * W_N + o];
    env += wsq[o];
  }
  return env > GL_TINY ? acc / env : acc;
}

template <int MODE>
__global__ __launch_bounds__(W_THREADS) void gl_frame_kernel(GlArgs a) {
  __shared__ double2 Z[W_N];
  __shared__ double tc[W_N / 2], ts[W_N / 2];
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  const int u = w_find(a.foff, a.n_utts, f);
  const long long F0 = a.foff[u], T = a.foff[u + 1] - F0, t = f - F0;
  w_stage_twiddles(tc, ts, a.twc, a.tws);
  double2 sp[3];  // the spectrum to invert at bins tid, tid + 256 and (thread 0) 512
#pragma unroll
  for (int r = 0; r < 3; ++r) sp[r] = make_double2(0.0, 0.0);

  if (MODE == GL_ITER || MODE == GL_STFT) {
    // the utterance's samples; one reflection suffices when n > W_N / 2
    const long long n = MODE == GL_STFT ? a.soff[u + 1] - a.soff[u] : (long long)a.hop * (T - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = tid + W_THREADS * r;
      long long s = t * a.hop + j - W_N / 2;
      if (s < 0) s = -s;
      if (s >= n) s = 2 * (n - 1) - s;
      s = max(0LL, min(s, n - 1));  // never binds for an admissible utterance; keeps any other inside its buffers
      const double v = MODE == GL_STFT ? a.x[a.soff[u] + s] : gl_ola(a.fin + F0 * W_N, a.wsq, T, a.hop, s + W_N / 2);
      Z[w_brev(j)] = make_double2(v * a.window[j], 0.0);
    }
    __syncthreads();
    w_fft(Z, tc, ts, -1.0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int k = tid + W_THREADS * r;
      if (k < W_K) {
        const double2 z = Z[k];
        if (MODE == GL_STFT) {
          a.spec_out[f * W_K + k] = z;
        } else {
#pragma clang fp contract(off)
          // angles = rebuilt - c tprev; angles /= |angles| + 1e-16, rounded as the restatement's complex arithmetic
          // rounds: the product, the difference, hypot, one reciprocal of the real divisor, two products
          double2 tp = make_double2(0.0, 0.0);
          if (!a.first) tp = a.R[f * W_K + k];
          a.R[f * W_K + k] = z;
          const double ar = z.x - a.coef * tp.x, ai = z.y - a.coef * tp.y;
          const double scl = 1.0 / (hypot(ar, ai) + GL_PHASE_EPS);
          const double s = a.S[f * W_K + k];
          sp[r] = make_double2(s * (ar * scl), s * (ai * scl));
        }
      }
    }
    if (MODE == GL_STFT) return;
    __syncthreads();  // every bin is read before the inverse transform's input overwrites Z
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int k = tid + W_THREADS * r;
      if (k < W_K) {
        if (MODE == GL_INIT) {
          const double s = a.S[f * W_K + k];
          const double2 p = a.ang0[f * W_K + k];
          sp[r] = make_double2(s * p.x, s * p.y);
        } else {
          sp[r] = a.spec_in[f * W_K + k];
        }
      }
    }
  }
  // irfft: the Hermitian extension; the imaginary parts of bin 0 and bin W_N / 2 are dropped
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int k = tid + W_THREADS * r;
    if (k < W_K) {
      if (k == 0 || k == W_N / 2) {
        Z[w_brev(k)] = make_double2(sp[r].x, 0.0);
      } else {
        Z[w_brev(k)] = sp[r];
        Z[w_brev(W_N - k)] = make_double2(sp[r].x, -sp[r].y);
      }
    }
  }
  __syncthreads();
  w_fft(Z, tc, ts, 1.0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = tid + W_THREADS * r;
    a.fout[f * W_N + j] = Z[j].x * (1.0 / W_N) * a.window[j];
  }
}

__global__ __launch_bounds__(W_THREADS) void gl_ola_kernel(const double* __restrict__ fr, const long long* __restrict__ foff,
                                                           const long long* __restrict__ soff, int n_utts, long long S,
                                                           const double* __restrict__ wsq, int hop, int clip,
                                                           double* __restrict__ y) {
  const long long g = (long long)blockIdx.x * W_THREADS + threadIdx.x;
  if (g >= S) return;
  const int u = w_find(soff, n_utts, g);
  const long long i = g - soff[u], F0 = foff[u], T = foff[u + 1] - F0;
  double v = 0.0;
  if (i < (long long)hop * (T - 1)) v = gl_ola(fr + F0 * W_N, wsq, T, hop, i + W_N / 2);
  if (clip) v = v < -1.0 ? -1.0 : (v > GL_CLIP_HI ? GL_CLIP_HI : v);
  y[g] = v;
}

// S[f][k] = sum_m 10^mlfb[f][m] P[k][m] (its absolute value with `magnitude`), m ascending, fused multiply-add
__global__ __launch_bounds__(W_THREADS) void gl_linear_kernel(const double* __restrict__ mlfb, const double* __restrict__ pt,
                                                              int n_mels, int magnitude, double* __restrict__ S) {
  __shared__ double m[GL_MAX_MELS];
  const long long f = blockIdx.x;
  for (int i = threadIdx.x; i < n_mels; i += W_THREADS) m[i] = pow(10.0, mlfb[f * n_mels + i]);
  __syncthreads();
  for (int k = threadIdx.x; k < W_K; k += W_THREADS) {
    double acc = 0.0;
    for (int i = 0; i < n_mels; ++i) acc = fma(m[i], pt[(size_t)i * W_K + k], acc);
    S[f * W_K + k] = magnitude ? fabs(acc) : acc;
  }
}

// ---------------------------------------------------------------------------------------------------------- host side
extern "C" int crk_gl_create(int fs, int n_fft, int win_length, int hop, int n_mels, const double* pinv_basis,
                             void** handle) {
  if (!handle) return CRK_ERR_ARG;
  *handle = nullptr;
  if (!pinv_basis || fs < 1) return CRK_ERR_ARG;
  if (n_fft != W_N || win_length < 1 || win_length > W_N || hop < 1 || hop > W_N || n_mels < 1 || n_mels > GL_MAX_MELS)
    return CRK_ERR_UNSUPPORTED;
  // the periodic Hann window of win_length, zero-padded symmetrically to W_N
  std::vector<double> w(W_N, 0.0), wsq(W_N), pt;
  const int lpad = (W_N - win_length) / 2;
  for (int i = 0; i < win_length; ++i) w[lpad + i] = 0.5 - 0.5 * cos(2.0 * M_PI * i / win_length);
  for (int i = 0; i < W_N; ++i) wsq[i] = w[i] * w[i];
  for (int m = 0; m < n_mels; ++m)
    for (int k = 0; k < W_K; ++k) pt.push_back(pinv_basis[(size_t)k * n_mels + m]);
  WTables tb;
  const size_t o_tw = tb.add_twiddles(W_N, W_N / 2), o_w = tb.add(w), o_wsq = tb.add(wsq), o_pt = tb.add(pt);
  Gl* g = new Gl();
  g->fs = fs; g->win = win_length; g->hop = hop; g->n_mels = n_mels;
  g->coef = GL_MOMENTUM / (1.0 + GL_MOMENTUM);
  if (!tb.upload(&g->tables)) {
    delete g;
    return CRK_ERR_HIP;
  }
  g->twc = g->tables + o_tw;
  g->tws = g->twc + W_N / 2;
  g->window = g->tables + o_w;
  g->wsq = g->tables + o_wsq;
  g->pt = g->tables + o_pt;
  *handle = g;
  return CRK_OK;
}

extern "C" void crk_gl_destroy(void* h) {
  Gl* g = (Gl*)h;
  if (!g) return;
  (void)hipFree(g->tables);
  delete g;
}

struct GlWs {
  double *fa, *fb; double2* R;
  size_t bytes;
};

static GlWs gl_ws(long long F, unsigned char* base) {
  GlWs r;
  WCarve c{base};
  r.fa = c.take<double>((size_t)F * W_N);
  r.fb = c.take<double>((size_t)F * W_N);
  r.R = c.take<double2>((size_t)F * W_K);
  r.bytes = c.bytes;
  return r;
}

static bool gl_shape_ok(int n_utts, long long F, long long S) {
  return n_utts >= 1 && F >= 2 && F <= (1LL << 31) - 1 && S >= 1 && (S + W_THREADS - 1) / W_THREADS <= (1LL << 31) - 1;
}

extern "C" long long crk_gl_workspace_bytes(int n_utts, long long total_frames, long long total_samples) {
  if (!gl_shape_ok(n_utts, total_frames, total_samples)) return -1;
  return (long long)gl_ws(total_frames, nullptr).bytes;
}

extern "C" int crk_gl_linear_spectrum(void* h, const double* mlfb, long long total_frames, int magnitude, double* S,
                                      void* stream) {
  Gl* g = (Gl*)h;
  if (!g || !mlfb || !S || total_frames < 1 || total_frames > (1LL << 31) - 1) return CRK_ERR_ARG;
  gl_linear_kernel<<<dim3((unsigned)total_frames), dim3(W_THREADS), 0, (hipStream_t)stream>>>(mlfb, g->pt, g->n_mels,
                                                                                              magnitude, S);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

static GlArgs gl_args(const Gl* g, const long long* foff, const long long* soff, int n_utts) {
  GlArgs a{};
  a.foff = foff; a.soff = soff; a.n_utts = n_utts;
  a.twc = g->twc; a.tws = g->tws; a.window = g->window; a.wsq = g->wsq;
  a.hop = g->hop; a.coef = g->coef;
  return a;
}

static int gl_launch_ola(const Gl* g, const double* frames, const long long* foff, const long long* soff, int n_utts, long long S,
                  int clip, double* y, hipStream_t st) {
  const long long blocks = (S + W_THREADS - 1) / W_THREADS;
  gl_ola_kernel<<<dim3((unsigned)blocks), dim3(W_THREADS), 0, st>>>(frames, foff, soff, n_utts, S, g->wsq, g->hop, clip, y);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_gl_run(void* h, const double* S, const double* angles0, const long long* frame_offsets,
                          const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                          int n_iter, int clip, double* y, void* workspace, long long workspace_bytes, void* stream) {
  Gl* g = (Gl*)h;
  if (!g || !S || !angles0 || !frame_offsets || !sample_offsets || !y || !workspace || n_iter < 0 ||
      !gl_shape_ok(n_utts, total_frames, total_samples))
    return CRK_ERR_ARG;
  GlWs ws = gl_ws(total_frames, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)total_frames), block(W_THREADS);
  GlArgs a = gl_args(g, frame_offsets, sample_offsets, n_utts);
  a.S = S; a.ang0 = (const double2*)angles0; a.R = ws.R;
  double *cur = ws.fa, *other = ws.fb;
  a.fout = cur;
  gl_frame_kernel<GL_INIT><<<grid, block, 0, st>>>(a);
  CRK_CHECK_LAUNCH();
  for (int it = 0; it < n_iter; ++it) {
    a.fin = cur; a.fout = other; a.first = it == 0;
    gl_frame_kernel<GL_ITER><<<grid, block, 0, st>>>(a);
    CRK_CHECK_LAUNCH();
    double* tmp = cur; cur = other; other = tmp;
  }
  return gl_launch_ola(g, cur, frame_offsets, sample_offsets, n_utts, total_samples, clip, y, st);
}

extern "C" int crk_gl_stft(void* h, const double* x, const long long* frame_offsets, const long long* sample_offsets,
                           int n_utts, long long total_frames, long long total_samples, double* spec, void* stream) {
  Gl* g = (Gl*)h;
  if (!g || !x || !frame_offsets || !sample_offsets || !spec || !gl_shape_ok(n_utts, total_frames, total_samples))
    return CRK_ERR_ARG;
  GlArgs a = gl_args(g, frame_offsets, sample_offsets, n_utts);
  a.x = x; a.spec_out = (double2*)spec;
  gl_frame_kernel<GL_STFT><<<dim3((unsigned)total_frames), dim3(W_THREADS), 0, (hipStream_t)stream>>>(a);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

extern "C" int crk_gl_istft(void* h, const double* spec, const long long* frame_offsets, const long long* sample_offsets,
                            int n_utts, long long total_frames, long long total_samples, double* y, void* workspace,
                            long long workspace_bytes, void* stream) {
  Gl* g = (Gl*)h;
  if (!g || !spec || !frame_offsets || !sample_offsets || !y || !workspace ||
      !gl_shape_ok(n_utts, total_frames, total_samples))
    return CRK_ERR_ARG;
  GlWs ws = gl_ws(total_frames, (unsigned char*)workspace);
  if (workspace_bytes < (long long)ws.bytes) return CRK_ERR_ARG;
  GlArgs a = gl_args(g, frame_offsets, sample_offsets, n_utts);
  a.spec_in = (const double2*)spec; a.fout = ws.fa;
  gl_frame_kernel<GL_ISTFT><<<dim3((unsigned)total_frames), dim3(W_THREADS), 0, (hipStream_t)stream>>>(a);
  CRK_CHECK_LAUNCH();
  return gl_launch_ola(g, ws.fa, frame_offsets, sample_offsets, n_utts, total_samples, 0, y, (hipStream_t)stream);
}
