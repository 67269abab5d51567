/* crank_hip.h - C ABI of libcrank_hip.so, the MI355X (gfx950) implementation of the
 * VQ-VAE voice-conversion training step's hot path.
 *
 * The reference (k2kobayashi/crank) has no FFI layer: its step calls torch modules
 * from Python.  Each entry point below replaces one torch-op cluster of that step and
 * cites the reference code it stands in for; INTEGRATION.md shows the ctypes binding
 * a maintainer of the reference would add (crank_amd/_lib.py is that binding).
 *
 * Conventions
 *  - plain C types only: device pointers, sizes, strides; no torch types.
 *  - every function returns 0 on success (CRK_OK) or a CRK_ERR_* code; none throws.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it; the compute entry
 *    points neither synchronise the device nor allocate: what a net handle needs for a batch
 *    shape is made by crk_net_reserve, outside the step.
 *  - activations are "frames x channels" row-major fp32, frame n = b*T + t, with an
 *    explicit row stride `ld*` in elements (the reference's (B,T,C) tensors as they
 *    are; its internal (B,C,T) transposes disappear).
 */
#ifndef CRANK_HIP_H
#define CRANK_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define CRK_OK 0
#define CRK_ERR_ARG 1
#define CRK_ERR_HIP 2
#define CRK_ERR_UNSUPPORTED 3

/* flags for crk_net_forward / crk_net_backward */
#define CRK_FLAG_PRECISE 1      /* bf16x3 split operands (~fp32 accuracy) instead of plain bf16 */
#define CRK_FLAG_NO_PARAM_GRAD 2 /* skip weight gradients (they would be discarded) */
#define CRK_FLAG_NO_SAVE 4       /* forward only: no backward will follow, do not store per-layer activations */
#define CRK_FLAG_DEFER_WNORM 8   /* backward only: leave the weight-norm backward (partial sums -> dg, dv, dbias) to a
                                  * crk_nets_wnorm_bwd call over all nets of the model; `params` / `grads` must stay
                                  * valid until then */

#define CRK_FLAG_SEED_ON_DEVICE 16 /* `seed` is the address of a device-resident uint64 (written by crk_seed_next on the same
                                  * stream) instead of the value itself: nothing per call lives in kernel arguments, so
                                  * a call with dropout can sit in a captured HIP graph and draw fresh masks every replay */
#define CRK_FLAG_FWD_PRECISE 32  /* backward only, without CRK_FLAG_PRECISE: the forward of this call ran with
                                  * CRK_FLAG_PRECISE | CRK_FLAG_BWD_PLAIN; the backward arithmetic is plain bf16 */
#define CRK_FLAG_BWD_PLAIN 64    /* forward only, with CRK_FLAG_PRECISE: the backward of this call will run WITHOUT
                                  * CRK_FLAG_PRECISE (and with CRK_FLAG_FWD_PRECISE) - the "bf16x3f" pairing: split-operand
                                  * forward (losses within 1e-3 of the fp32 reference), plain-bf16 backward.  Lets the forward
                                  * save only what that backward reads, in the layout it reads it.  The pair runs the fused
                                  * kernels only where the shape's routes of BOTH arithmetics do, else both directions run per
                                  * layer; a backward whose kernel family is not the forward's is CRK_ERR_ARG */

/* ---- convolutional stacks -----------------------------------------------------
 * Replaces the parallel_wavegan networks the reference instantiates (third-party,
 * un-vendored): ParallelWaveGANGenerator (crank/net/module/vqvae2.py:237-273),
 * ResidualParallelWaveGANDiscriminator (crank/bin/train.py:108-118),
 * ParallelWaveGANDiscriminator (crank/net/module/spkradv.py:49-60,
 * crank/bin/train.py:78-89), all with torch.nn.utils.weight_norm on every conv. */
typedef struct crk_net_desc {
  int kind;          /* 0 gated-residual generator, 1 gated-residual discriminator, 2 plain conv stack */
  int in_ch, out_ch, kernel_size, layers, stacks;
  int res_ch, gate_ch, skip_ch, aux_ch;   /* kinds 0/1: must be 64/128/64; aux_ch <= 0: none */
  int conv_ch;       /* kind 2 hidden width */
  int causal;        /* use_causal_conv */
  int use_bias;
  float slope;       /* LeakyReLU negative slope */
  float dropout;     /* residual-block input dropout (kind 1) */
} crk_net_desc;

void* crk_net_create(const crk_net_desc* desc);
void crk_net_destroy(void* net);
long long crk_net_param_count(void* net);
int crk_net_conv_count(void* net);
/* out[9] = cout, cin, k, off_bias(-1: none), off_g, off_v, dilation, role, layer;
 * offsets are element offsets into the net's flat fp32 parameter block; weight_v is
 * stored (cout, cin, k) like torch's Conv1d.weight_v, weight_g (cout). */
int crk_net_conv_info(void* net, int i, long long* out9);
long long crk_net_saved_bytes(void* net, int B, int T);
/* The handle's own device memory for batch shape (B, T) - the backward's gradient planes, the weight-gradient partial sums
 * (crk_net_scratch_bytes of them) and the per-shape descriptor tables - allocated HERE, once per shape and outside the step
 * (it calls hipMalloc / hipMemcpy: a device-wide synchronisation; not inside a stream capture).  crk_net_forward /
 * crk_net_backward* never allocate: at a shape that was not reserved they launch nothing and return CRK_ERR_ARG.  Buffers
 * outgrown by a later reserve stay alive until crk_net_destroy (a captured HIP graph may still hold them). */
int crk_net_reserve(void* net, int B, int T);
long long crk_net_scratch_bytes(void* net, int B, int T);
/* y[N,out_ch] = net(x[N,in_ch], c[N,aux_ch]); `saved` (crk_net_saved_bytes) keeps what
 * the backward needs; `version` changes whenever `params` was modified. */
int crk_net_forward(void* net, const float* params, unsigned long long version, const float* x, int ldx,
                    const float* c, int ldc, float* y, int ldy, float* saved, int B, int T, int flags,
                    unsigned long long seed, void* stream);
/* accumulates parameter gradients into `grads` (same layout as params) and writes the
 * input gradients dx (scaled by dx_scale: gradient reversal of spkradv.py:63-72 is
 * dx_scale = -lambda) and dc (aux) when non-null. */
int crk_net_backward(void* net, const float* params, unsigned long long version, float* grads, const float* x,
                     int ldx, const float* c, int ldc, const float* dy, int lddy, float* dx, int lddx, float dx_scale,
                     float* dc, int lddc, const float* saved, int B, int T, int flags, unsigned long long seed,
                     void* stream);
/* crk_net_backward of dy * (dy_num[0] / dy_den[1]), the factor read on the device: the backward of a mean cross entropy
 * (crank/net/trainer/utils.py:26, trainer_vqvae.py:177-198) on the net's output - dy = softmax - onehot as crk_ce_fwd wrote
 * it, dy_num = upstream gradient, dy_den = crk_ce_fwd's out2 {loss, count} - without a scaling launch in between.  Chains
 * of plain convs (kind 2) on the fused path only: CRK_ERR_UNSUPPORTED otherwise (crk_ce_bwd, then crk_net_backward). */
int crk_net_backward_scaled(void* net, const float* params, unsigned long long version, float* grads, const float* x,
                            int ldx, const float* c, int ldc, const float* dy, int lddy, float* dx, int lddx, float dx_scale,
                            float* dc, int lddc, const float* saved, int B, int T, int flags, unsigned long long seed,
                            const float* dy_num, const float* dy_den, void* stream);
/* crk_net_backward for a conditioning input whose columns [c0, c0 + E) are table[idx[u * run]] on every frame of utterance u
 * (run == T; crk_concat_embed_run built it) and whose other columns need no gradient.  No per-frame dc is computed: the
 * weight-gradient launch also sums every block's gate gradient per utterance, and one small launch adds
 * sum_l Waux_l[:, c0:c0+E]^T . sums of the utterances of each label, in ascending utterance order, to dtable [n_rows][E]
 * (fixed order, no atomics).  dx and the parameter gradients are those of crk_net_backward; the table gradient differs from
 * the frame sum of dc by fp32 reassociation.  Gated stacks with conditioning on the fused kernels only -
 * crk_net_embed_grad_supported(net, B, T, flags) == 1 - and CRK_ERR_UNSUPPORTED otherwise (crk_net_backward with dc, then
 * crk_embed_bwd_run).  The sums live in the scratch crk_net_reserve made. */
int crk_net_embed_grad_supported(void* net, int B, int T, int flags);
int crk_net_backward_embed(void* net, const float* params, unsigned long long version, float* grads, const float* x, int ldx,
                           const float* c, int ldc, const float* dy, int lddy, float* dx, int lddx, float dx_scale,
                           const float* saved, int B, int T, int flags, unsigned long long seed, const long long* idx,
                           long long run, int c0, int E, int n_rows, float* dtable, void* stream);

/* Dropout seeds on the device (D's ResidualBlock dropout, crank/bin/train.py:114; torch draws its Philox offsets on the
 * host, which a captured graph would freeze): *out = mix(*state), *state advances.  One thread; `state` is a uint64 the
 * caller seeds once (per net), `out` the uint64 a forward call and its backward both receive (CRK_FLAG_SEED_ON_DEVICE). */
int crk_seed_next(unsigned long long* state, unsigned long long* out, void* stream);

/* The sub-nets of one model (the generator has four stacks) share an optimizer step; these do for all of them in
 * ONE launch what the per-net calls do in one launch each.  crk_nets_wnorm_bwd: the weight-norm backward of every net
 * with one pending (CRK_FLAG_DEFER_WNORM); must precede any reader of the gradients.  crk_nets_prepare: the weight
 * preparation of every net whose (params[i], version) changed - otherwise crk_net_forward / _backward prepare their
 * net on their first call after the change.  bump_step (may be NULL): an Adam step count to advance by one in the same
 * launch (crk_adam_step, clear_grads bit 1). */
int crk_nets_wnorm_bwd(int n_nets, void* const* nets, void* stream);
int crk_nets_prepare(int n_nets, void* const* nets, const float* const* params, unsigned long long version,
                     float* bump_step, void* stream);
/* Both calls take the nets of SEVERAL models whose updates are adjacent in the step and independent of each other (the
 * speaker-adversarial net and the speaker classifier): crk_nets_wnorm_bwd then also runs the weight gradients their
 * CRK_FLAG_DEFER_WNORM backward calls left pending - plain-conv nets defer them like the first conv and head of a gated
 * stack - as one launch over all of them.  crk_nets_prepare_models: crk_nets_prepare with a version per net (each
 * model counts its own) and up to 4 step counts, each advanced by one in the preparation launch. */
int crk_nets_prepare_models(int n_nets, void* const* nets, const float* const* params, const unsigned long long* versions,
                            int n_bumps, float* const* bump_steps, void* stream);

/* ---- VQ codebook (crank/net/module/vqvae2.py:286-347) --------------------------- */
/* Quantizer.vq + lookup + straight-through value: idx[n] = argmin_k ||x_n - w_k||^2
 * (reference fp32 expression, first index on ties), e = W[idx], qx = x + (e - x). */
int crk_vq_forward(const float* x, int ldx, const float* codebook, int N, int D, int K, long long* idx, float* e,
                   int lde, float* qx, int ldq, void* stream);
/* crk_vq_forward with the quantizer's surroundings in the same launch (D = 64, K <= 512; CRK_ERR_UNSUPPORTED otherwise -
 * compose the separate entry points then): add (NULL: none) - the quantizer's input is x + add ("enc[n] + dec",
 * crank/net/module/vqvae2.py:177), written to xsum (NULL: not kept); commit_out2 (NULL: none) = {mean over the frames
 * mask selects (NULL: all) of (input - e)^2, element count}: the commitment loss of trainer_vqvae.py:227-237, exactly what
 * crk_masked_loss_fwd(input, e, mask, mode 1) returns up to summation order; scratch: crk_loss_scratch_floats() floats.
 * xsum may alias x or add (the sum formed in place): every output is that of the inputs as they were passed. */
int crk_vq_forward_fused(const float* x, int ldx, const float* add, int ldadd, float* xsum, int ldsum, const float* codebook,
                         int N, int D, int K, long long* idx, float* e, int lde, float* qx, int ldq,
                         const unsigned char* mask, float* commit_out2, float* scratch, const void* image, void* stream);
/* What the search derives from the codebook alone (Quantizer.vq's `w ** 2` term and the operands of its `x @ w.t()`,
 * crank/net/module/vqvae2.py:338-347, in the search kernel's form: split-f16 fragment planes, squared norms, per-code scales),
 * prepared ONCE per codebook update instead of by every workgroup of every call.  crk_vq_image_bytes: size of the caller-owned
 * buffer (0: shape without an image - pass image = NULL).  crk_vq_image_build_multi: up to 4 codebooks in one launch (the
 * quantizers of a forward).  The caller keeps the image valid: rebuild after ANY write to the codebook (EMA blend,
 * load_state_dict, optimizer step of a trained codebook).  crk_vq_forward_fused(image = NULL) derives everything per call as
 * before; indices, e and qx are identical either way. */
long long crk_vq_image_bytes(int K, int D);
int crk_vq_image_build_multi(int nq, const float* const* codebooks, const int* K, int D, void* const* images, void* stream);
/* vqvae2.py:316-321: counts[K] (int32) and sums[D][K] (int64, 2^-28 fixed point: integer
 * sums are exact and order independent).  `scratch` holds per-chunk partial tables
 * (crk_vq_ema_scratch_bytes; -1: unsupported K).  Under data parallelism all-reduce counts
 * and sums between stats and apply.  crk_vq_ema_stats, crk_vq_ema_partial and crk_vq_ema_apply are the nq = 1 case
 * of the *_multi entry points below (after their own argument checks): the same kernels, so the same bits. */
long long crk_vq_ema_scratch_bytes(int N, int D, int K);
int crk_vq_ema_stats(const float* x, int ldx, const long long* idx, int N, int D, int K, int* counts, long long* sums,
                     void* scratch, void* stream);
/* vqvae2.py:316-330: EMA blend, Laplace smoothing (stored back), codebook refresh.
 * ema_w is (D,K), codebook (K,D), like the reference buffers. */
int crk_vq_ema_apply(const int* counts, const long long* sums, float* ema_size, float* ema_w, float* codebook, int D,
                     int K, double decay, double eps, void* stream);
/* The same update for every quantizer of a generator forward (vqvae2.py:171-190 calls the quantizers one after the
 * other; nothing reads a codebook between them) with fewer launches than four per quantizer:
 * crk_vq_ema_partial per quantizer or ONE crk_vq_ema_partial_multi (per-chunk tables into scratch[q]), ONE
 * crk_vq_ema_reduce_multi (tables -> counts[q], sums[q]; all-reduce them here under data parallelism), ONE
 * crk_vq_ema_apply_multi (a size launch and a blend launch for all quantizers).  nq <= 4. */
int crk_vq_ema_partial(const float* x, int ldx, const long long* idx, int N, int D, int K, void* scratch, void* stream);
int crk_vq_ema_reduce_multi(int nq, const void* const* scratch, const int* N, const int* D, const int* K,
                            int* const* counts, long long* const* sums, void* stream);
int crk_vq_ema_apply_multi(int nq, const int* const* counts, const long long* const* sums, float* const* ema_size,
                           float* const* ema_w, float* const* codebook, const int* D, const int* K, double decay,
                           double eps, void* stream);
/* Fewer launches for the same update in a single process (nothing is all-reduced between the steps): the per-chunk tables
 * of all quantizer calls of a forward in one launch (crk_vq_ema_partial_multi, <= 4 calls), tables -> counts / sums AND the
 * cluster-size update (the first half of crk_vq_ema_apply_multi: the same device function) in one launch
 * (crk_vq_ema_reduce_size_multi), then the blend (crk_vq_ema_blend_multi): 3 launches per generator forward instead of 5. */
int crk_vq_ema_partial_multi(int nq, const float* const* x, const int* ldx, const long long* const* idx, const int* N,
                             const int* D, const int* K, void* const* scratch, void* stream);
int crk_vq_ema_reduce_size_multi(int nq, const void* const* scratch, const int* N, const int* D, const int* K,
                                 int* const* counts, long long* const* sums, float* const* ema_size, double decay, double eps,
                                 void* stream);
int crk_vq_ema_blend_multi(int nq, const long long* const* sums, float* const* ema_size, float* const* ema_w,
                           float* const* codebook, const int* D, const int* K, double decay, void* stream);
/* crk_vq_ema_blend_multi that also leaves each codebook's search image (crk_vq_image_bytes(K, 64) bytes, see
 * crk_vq_image_build_multi) current - the bytes crk_vq_image_build_multi would derive from the blended codebook - in the same
 * launch; nq <= 4, D = 64 and K <= 512 for every quantizer (CRK_ERR_UNSUPPORTED otherwise: blend, then build). */
int crk_vq_ema_blend_image_multi(int nq, const long long* const* sums, float* const* ema_size, float* const* ema_w,
                                 float* const* codebook, const int* D, const int* K, double decay, void* const* images,
                                 void* stream);

/* ---- losses ----------------------------------------------------------------------- */
/* `scratch` of the loss entry points: crk_loss_scratch_floats() floats; calls on one stream may share it. */
int crk_loss_scratch_floats(void);
/* masked mean of |x-y| (mode 0) or (x-y)^2 (mode 1): CustomFeatureLoss l1/mse
 * (crank/net/module/loss.py:30-47) and the masked_select + MSELoss pairs of
 * trainer_vqvae.py:227-237, trainer_lsgan.py:154-170 (y == NULL: constant target).
 * mask: one byte per frame or NULL.  out2 = {mean, element count}. */
int crk_masked_loss_fwd(const float* x, int ldx, const float* y, int ldy, float yconst, const unsigned char* mask,
                        long long N, int D, int mode, float* out2, float* scratch, void* stream);
int crk_masked_loss_bwd(const float* x, int ldx, const float* y, int ldy, float yconst, const unsigned char* mask,
                        long long N, int D, int mode, const float* stat2, const float* gout, float* dx, int lddx,
                        float* dy, int lddy, void* stream);
/* L1 and MSE means of the same (x, y, mask) in one pass: out4 = {L1 mean, count, MSE mean, count}; each half is a
 * stat2 for crk_masked_loss_bwd with the matching mode (the trainers take both of the decoded features,
 * trainer_vqvae.py:215-225) */
int crk_masked_loss_both_fwd(const float* x, int ldx, const float* y, int ldy, const unsigned char* mask, long long N,
                             int D, float* out4, float* scratch, void* stream);
/* the same with dx = add * add_scale[0] + (loss gradient): a second gradient of x (add, row stride ldadd; NULL: none;
 * add_scale: device scalar, NULL = 1) joins in the launch instead of a separate addition - the commitment loss next to
 * the quantizer's straight-through gradient (trainer_vqvae.py:227-237 + vqvae2.py:343-347), the L1 loss of the decoded
 * features next to the unit gradient of the STFT loss (trainer_vqvae.py:215-225) */
int crk_masked_loss_bwd_acc(const float* x, int ldx, const float* y, int ldy, float yconst, const unsigned char* mask,
                            long long N, int D, int mode, const float* stat2, const float* gout, float* dx, int lddx,
                            float* dy, int lddy, const float* add, int ldadd, const float* add_scale, void* stream);
/* Backward of the commitment loss (trainer_vqvae.py:227-237: mse of the quantizer's input x against e.detach(), masked
 * mean; stat2 / gout as for crk_masked_loss_bwd, mode mse) where the other gradients of the same tensors meet it
 * (vqvae2.py:171-190): t = (a1 + a2) + loss gradient -> dsum (the gradient of the tensor that was added to x inside the
 * quantizer op; NULL: not wanted), t + a3 -> dx.  a1: the straight-through gradient of qx, a2: a second consumer of qx
 * (the last decoder's concatenation), a3: a second consumer of x (the speaker-adversarial net, spkradv.py:74-76); each
 * optional, each with its own row stride.  The sums are the ones autograd's accumulation makes, bit for bit.
 * CRK_ERR_UNSUPPORTED unless D, the strides and the pointers are multiples of 4 floats. */
int crk_vq_commit_bwd(const float* x, int ldx, const float* e, int lde, const unsigned char* mask, long long N, int D,
                      const float* stat2, const float* gout, float* dx, int lddx, float* dsum, int ldsum,
                      const float* a1, int ld1, const float* a2, int ld2, const float* a3, int ld3, void* stream);
/* nn.CrossEntropyLoss(ignore_index) over frames (crank/net/trainer/utils.py:26). */
int crk_ce_fwd(const float* logits, int ldl, const long long* target, long long N, int C, int ignore_index,
               float* out2, float* dlogits_unscaled, float* scratch, void* stream);
int crk_ce_bwd(float* dlogits_unscaled, long long N, int C, const float* stat2, const float* gout, float* dlogits,
               void* stream);
/* one resolution of the STFT-magnitude loss along the frame axis
 * (crank/net/module/loss.py:50-114); n_fft/hop_length/win_length as torch.stft
 * receives them (i.e. after the reference's argument shuffle). */
int crk_stft_loss_fwd(const float* x, int ldx, const float* y, int ldy, int B, int T, int D, int n_fft,
                      int hop_length, int win_length, const float* window, float logratio, float weight,
                      int accumulate, float* out1, float* scratch, void* stream);
int crk_stft_loss_bwd(const float* x, int ldx, const float* y, int ldy, int B, int T, int D, int n_fft,
                      int hop_length, int win_length, const float* window, float logratio, float weight,
                      const float* gout, float* dx, int lddx, void* stream);

/* every resolution of MultiSizeSTFTLoss (loss.py:88-114) in one launch per direction: out1[0] = mean over resolutions.
 * CRK_ERR_UNSUPPORTED (win_length > 64 or more than 4 resolutions): loop over the single-resolution entry points. */
int crk_stft_loss_multi_fwd(const float* x, int ldx, const float* y, int ldy, int B, int T, int D, int nres,
                            const int* n_fft, const int* hop_length, const int* win_length, const float* const* windows,
                            float logratio, float* out1, float* scratch, void* stream);
/* loss and gradient in one pass: dx_unit (zero-initialised) += d out1 / d x; the backward of the loss is then
 * upstream gradient * dx_unit (no second evaluation of the DFTs) */
int crk_stft_loss_multi_fwd_grad(const float* x, int ldx, const float* y, int ldy, int B, int T, int D, int nres,
                                 const int* n_fft, const int* hop_length, const int* win_length,
                                 const float* const* windows, float logratio, float* out1, float* dx_unit, int lddx,
                                 float* scratch, void* stream);
int crk_stft_loss_multi_bwd(const float* x, int ldx, const float* y, int ldy, int B, int T, int D, int nres,
                            const int* n_fft, const int* hop_length, const int* win_length, const float* const* windows,
                            float logratio, const float* gout, float* dx, int lddx, void* stream);

/* L1 mean, MSE mean and the multi-resolution STFT loss of the decoded features against their target - the three terms
 * trainer_vqvae.py:215-225 (calculate_vqvae_loss) forms on the same pair with CustomFeatureLoss / MultiSizeSTFTLoss
 * (crank/net/module/loss.py:18-114) - as ONE launch (+ a finishing one) per direction, without atomics:
 *   out5 = {L1 mean, count, MSE mean, count, STFT loss};
 *   grad (crk_recon_grad_floats floats; NULL: no gradient wanted) = d STFT loss / d x for an upstream gradient of 1, in a
 *   compact per-frame layout that only crk_recon_loss_bwd reads;
 *   tables[r] = crk_stft_twiddles(n_fft[r], win_length[r], hann window of resolution r), crk_stft_twiddle_floats floats,
 *   built once per criterion.
 * Geometry: crk_recon_supported (hop_length >= win_length + 3: frames that do not overlap - what quirk Q1 of
 * MultiSizeSTFTLoss makes of the default stft_params; win_length <= 64; <= 4 resolutions); otherwise
 * CRK_ERR_UNSUPPORTED and the caller uses crk_masked_loss_both_fwd + crk_stft_loss_multi_*.
 * crk_recon_loss_bwd: dx = g1[0] dL1 + g2[0] dMSE + g3[0] dSTFT (device scalars; NULL = term not differentiated). */
int crk_recon_supported(int T, int nres, const int* n_fft, const int* hop_length, const int* win_length);
long long crk_stft_twiddle_floats(int n_fft, int win_length);
int crk_stft_twiddles(int n_fft, int win_length, const float* window, float* table, void* stream);
long long crk_recon_grad_floats(int B, int T, int D, int nres, const int* hop_length, const int* win_length);
int crk_recon_loss_fwd(const float* x, int ldx, const float* y, int ldy, const unsigned char* mask, int B, int T, int D,
                       int nres, const int* n_fft, const int* hop_length, const int* win_length,
                       const float* const* tables, float logratio, float* out5, float* grad, float* scratch,
                       void* stream);
int crk_recon_loss_bwd(const float* x, int ldx, const float* y, int ldy, const unsigned char* mask, int B, int T, int D,
                       int nres, const int* n_fft, const int* hop_length, const int* win_length, const float* out5,
                       const float* grad, const float* g1, const float* g2, const float* g3, float* dx, int lddx,
                       void* stream);

/* The trainers' loss totals ("loss[G] += alpha * term", crank/net/trainer/basetrainer.py:200-206 and the
 * _parse_*_loss functions of trainer_vqvae.py / trainer_lsgan.py / trainer_cyclegan.py): out[0] = sum_i weights[i] *
 * terms[i][0] + constant over <= 16 device scalars in one launch; backward grads[i] = weights[i] * gout[0]. */
int crk_weighted_sum(int n, const float* const* terms, const float* weights, float constant, float* out, void* stream);
int crk_weighted_sum_bwd(int n, const float* weights, const float* gout, float* grads, void* stream);

/* ---- optimiser / glue -------------------------------------------------------------- */
/* torch.optim.Adam defaults on one flat block (crank/net/trainer/utils.py:40-58);
 * lr_dev[0] and step_dev[0] live in device memory (no host sync, graph friendly).  clear_grads bit 0: the gradient
 * block is zeroed as it is consumed (optimizer.zero_grad() of the next step without a memset launch); bit 1: the step
 * count is NOT advanced by this call - the caller hands step_dev to the crk_nets_prepare call that follows the update
 * (one launch less per optimizer step). */
int crk_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long long n, const float* lr_dev,
                  float* step_dev, float beta1, float beta2, float eps, int clear_grads, void* stream);
/* crk_adam_step over up to CRK_ADAM_MAX_BLOCKS flat blocks in ONE launch: each block with its own parameters,
 * gradients, moments, length, device lr and device step count; the arithmetic per element and the clear_grads bits are
 * crk_adam_step's (bit 1 clear: every step count advances by one, in one launch behind the update).  CRK_ERR_ARG, before
 * any launch, for a null pointer, a negative length, a step count named twice or more blocks than the record holds. */
#define CRK_ADAM_MAX_BLOCKS 4
typedef struct crk_adam_block {
  float *params, *grads, *exp_avg, *exp_avg_sq;
  long long n;
  const float* lr_dev;
  float* step_dev;
} crk_adam_block;
int crk_adam_step_multi(int n_blocks, const crk_adam_block* blocks, float beta1, float beta2, float eps, int clear_grads,
                        void* stream);
/* torch_optimizer.RAdam(lr) (crank/net/trainer/utils.py:44-45; the package is absent from the reference tree: its
 * published update, Liu et al. Alg. 2 - betas (0.9, 0.999), eps 1e-8, no weight decay, rectified adaptive update where the
 * approximated SMA length N_sma >= 5, momentum-only update below).  Arguments and clear_grads bits as crk_adam_step;
 * the betas and eps are the host's doubles (the packages form 1 - beta in double before the fp32 arithmetic). */
int crk_radam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long long n, const float* lr_dev,
                   float* step_dev, double beta1, double beta2, double eps, int clear_grads, void* stream);
/* pytorch_lamb.Lamb(lr) (crank/net/trainer/utils.py:46-47; absent third party: its published update, You et al. Alg. 2 as
 * that package states it - betas (0.9, 0.999), eps 1e-6, no weight decay, no bias correction, per parameter tensor
 * trust ratio clamp(||w||, 0, 10) / ||m / (sqrt(v) + eps)||, 1 where a norm is 0).  The caller describes the block's
 * parameter tensors once: tiles[4 * t] = {offset, length <= crk_lamb_tile(), tensor, 0} (no tile crosses a tensor, the
 * tiles of a tensor are consecutive; 16-byte aligned), tensors[2 * s] = {first tile, tiles}; upd: one float per element of
 * the block, part: 2 * n_tiles floats (both
 * caller-owned scratch), ratio_out (may be NULL): the trust ratio of every tensor.  clear_grads bits as crk_adam_step;
 * the gradient is cleared over the tiles. */
int crk_lamb_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* upd, const int* tiles, int n_tiles,
                  const int* tensors, int n_tensors, float* part, float* ratio_out, const float* lr_dev, float* step_dev,
                  double beta1, double beta2, double eps, int clear_grads, void* stream);
int crk_lamb_tile(void);
/* out[n,:] = [a[n,:ca] | b[n,:cb] | table[idx[n],:E]] (vqvae2.py:154-158,
 * trainer_lsgan.py:194-206) and the embedding-table gradient. */
int crk_concat_embed(const float* a, int lda, int ca, const float* b, int ldb, int cb, const float* table, int E,
                     const long long* idx, long long N, float* out, int ldo, void* stream);
/* dtable[r,:] += sum of dcat[n, c0:c0+E] over frames with idx[n] == r; fixed summation order
 * (bit-reproducible); scratch: crk_embed_bwd_scratch_floats floats. */
long long crk_embed_bwd_scratch_floats(long long N, int E, int n_rows);
int crk_embed_bwd(const float* dcat, int ld, int c0, int E, const long long* idx, long long N, int n_rows,
                  float* dtable, float* scratch, void* stream);
/* The same two with frames [j * run, (j + 1) * run) all carrying the label idx[j * run]: the reference overwrites every
 * frame's label with its utterance's first (basetrainer.py:303-308 "h[:, :] = h[:, 0:1]", trainer_lsgan.py:202-204)
 * before the lookup; with run = frames per utterance the lookup reads the label tensor as the batch holds it (-100 pads
 * behind the first frame included) and no filled copy is made.  run = 1: one label per frame. */
int crk_concat_embed_run(const float* a, int lda, int ca, const float* b, int ldb, int cb, const float* table, int E,
                         const long long* idx, long long run, long long N, float* out, int ldo, void* stream);
int crk_embed_bwd_run(const float* dcat, int ld, int c0, int E, const long long* idx, long long run, long long N,
                      int n_rows, float* dtable, float* scratch, void* stream);

/* ---- on-the-fly log-mel front end (crank/net/module/mlfb.py:134-171, use_raw) ------ */
/* raw[B, n_samples] -> logmel[B*T, n_mels]; STFT n_fft with a win_length window, |.|, mel
 * matvec, clamp(eps), log10, optional (x-mean)/std.  center = 0: frame t starts at sample
 * t*hop (the training step, vqvae2.py:60); center = 1: frame t is centred on t*hop over the
 * reflect-padded signal, T = 1 + n_samples / hop (the offline extraction,
 * crank/feature/feature.py:126-145 -> parallel_wavegan logmelfilterbank).
 * CRK_ERR_ARG, nothing launched: n_fft not a power of two in 2 .. 2048, win_length outside
 * 1 .. n_fft, n_mels outside 1 .. 256, B, T, hop or n_samples < 1, ldo < n_mels, ld_raw <
 * n_samples, center with n_samples <= n_fft / 2.  A clamped cell is (float)log10((double)eps). */
int crk_logmel_fwd(const float* raw, int ld_raw, int B, int n_samples, int T, int n_fft, int hop, int win_length,
                   const float* window, const float* mel_basis /* [n_bins][n_mels] */, int n_mels, float eps,
                   const float* mean, const float* std, float* out, int ldo, int center, void* stream);

/* ---- Streaming log-mel front end ---------------------------------------------------------------------------------
 * crk_logmel_fwd's frames for up to n_streams concurrent streams that receive their utterances as pushes of new samples,
 * at most max_samples each per push.  With n the samples a stream has received in its utterance and h = n_fft / 2:
 *   center = 1: frame t covers [t hop - h, t hop + h) with the reflect rule at both ends; ready(n) = 0 for n <= h, else
 *     (n - h) / hop + 1.  A push whose end flag is set for a stream emits everything up to 1 + n / hop, the right mirror
 *     taken at the final n (nothing when n <= h: the offline call refuses such an utterance), and returns that stream to
 *     the start-of-utterance state.
 *   center = 0: frame t covers [t hop, t hop + n_fft); ready(n) = 0 for n < n_fft, else (n - n_fft) / hop + 1; the end flag
 *     emits nothing more and resets the stream.
 * A push emits frames ready(before) .. ready(after) - 1 and nothing else; over an utterance these are the frames of
 * crk_logmel_fwd on the whole signal, however it is cut into pushes.  Every frame is transformed alone: its bits
 * depend on its own n_fft samples and the configuration alone (not on the cut, S, the row or the frames beside it), and
 * agree with crk_logmel_fwd's within fp32 rounding, not bit for bit (its n_fft = 1024 kernel pairs frames).  Clamp, log10,
 * the value of a clamped cell and (v - mean) / std are crk_logmel_fwd's.
 *
 * crk_logmel_stream_create is the one call that allocates (it synchronises): per stream a ring of the last n_fft samples
 * and two 64-bit counts, and the handle's own copies of window [win_length], mel_basis [n_bins][n_mels], mean / std
 * [n_mels] (both or neither; host or device pointers) with the twiddle and filter-run tables made from them.
 * CRK_ERR_ARG: n_fft not a power of two in 256 .. 2048, win_length outside 1 .. n_fft, hop < 1, n_mels outside 1 .. 256,
 * n_streams or max_samples < 1, a null window, basis or handle.  crk_logmel_stream_state_bytes: the size of the
 * allocation.  crk_logmel_stream_max_frames: the largest count one push can emit over all histories, the end flush
 * included - (max_samples + hop - 1) / hop uncentred, 1 + (h + max_samples) / hop centred.
 * crk_logmel_stream_reset: the streams listed in the HOST array stream_ids (NULL: every stream) start a new utterance.
 * crk_logmel_stream_push: x fp32 [S][C] with row stride ldx, n_valid / end DEVICE int32 [S] (NULL: C / 0; samples at and
 * past n_valid are ignored, n_valid may be 0), out fp32 [S][max_frames][n_mels] with row stride ldo, n_frames DEVICE
 * int32 [S]: the frames written per stream from the start of its block, written for every stream; frames at and past
 * n_frames are not written.  Stream i is row i.  Judged before any launch, output and state untouched: CRK_ERR_ARG for
 * a null pointer, S < 1, C < 0, ldx < C, ldo < n_mels; CRK_ERR_UNSUPPORTED for S > n_streams or C > max_samples.  Every
 * position lives on the device: a push never allocates, never synchronises and reads nothing back (it can be captured in
 * a graph), and launches 2 kernels whatever S, C, n_valid and end are. */
int crk_logmel_stream_create(int n_fft, int hop, int win_length, const float* window, const float* mel_basis, int n_mels,
                             float eps, const float* mean, const float* stdv, int center, int n_streams, int max_samples,
                             void** handle);
void crk_logmel_stream_destroy(void* st);
long long crk_logmel_stream_state_bytes(void* st);
int crk_logmel_stream_max_frames(void* st);
int crk_logmel_stream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_logmel_stream_push(void* st, const float* x, int ldx, const int* n_valid, const int* end, int S, int C, float* out,
                           int ldo, int* n_frames, void* stream);

/* ---- batch assembly from an HBM-resident corpus -----------------
 * Replaces the numpy work of BaseDataset.__getitem__ in the reference's DataLoader workers,
 * torch's default collate and the per-batch host->device copy
 * (crank/net/trainer/dataset.py:58-139 sample dict, :158-198 + :239-258 pad / crop rule,
 * :229-236 speaker codes, :288-293 convert_f0).  The corpus lives in HBM once: every
 * utterance's frames packed one after the other, frame-major fp32 rows. */

/* sklearn StandardScaler.transform (inverse = 0: fl32(fl64(fl32(fl64(x) - mean)) / scale)) and
 * inverse_transform (inverse = 1: fl32(fl64(fl32(fl64(x) * scale)) + mean)) exactly as sklearn
 * evaluates them on a float32 array with float64 statistics (dataset.py:146-150,
 * basetrainer.py:341-345).  x[N, D] row stride ldx -> y[N, D] row stride ldy; y may be x.
 * mean / scale: D doubles in device memory. */
int crk_scaler_apply(const float* x, int ldx, float* y, int ldy, long long N, int D, const double* mean,
                     const double* scale, int inverse, void* stream);

/* ---- fitting the scalers (recipe stage 2, crank/bin/extract_statistics.py) ----------------
 * What sklearn's StandardScaler.partial_fit, called once per utterance in file order, leaves in
 * mean_ / var_ / n_samples_seen_, over a packed block x[F_total, ld] (fp32) of which columns
 * [col0, col0 + D) are fitted.  Two launches: the moments of every utterance alone, then the
 * sequential merge of each group's utterances.  Everything is float64.
 *
 * The workspace carries the moments from the first entry to the second.  Layout (every part starts
 * at a multiple of 256 bytes, in this order; tiles = (D + 63) / 64):
 *   int status[U * tiles]   0 fine, 1 a non-finite value in that utterance, 2 bad device offsets
 *   long long n[U]          frames of the utterance
 *   double sum[U * D]       sum x
 *   double m2[U * D]        sum (x - T)^2 - (sum (x - T))^2 / n  with T = sum / n
 * crk_scaler_workspace_bytes returns its size, -1 for U < 1 or D < 1.
 *
 * Neither compute entry allocates or synchronises; both can be captured into a graph.  Both take
 * the offsets twice: the device copy the kernel reads and a host copy that is checked before
 * anything is launched.  CRK_ERR_ARG, with nothing launched: a workspace shorter than
 * crk_scaler_workspace_bytes(U, D), U < 1, D < 1, ld < col0 + D, an empty utterance
 * (utt_start[u + 1] <= utt_start[u]), offsets outside [0, F_total], an empty group, a group member
 * outside [0, U). */
long long crk_scaler_workspace_bytes(int U, int D);
/* One workgroup per utterance and tile of 64 columns; 16-byte loads when ld, col0 and D are
 * multiples of 4 and x is 16-byte aligned, scalar loads otherwise, in the same summation order:
 * the result depends on the utterance's values, its length and D alone, never on the load width,
 * the other utterances or the call. */
int crk_scaler_moments(const float* x, int ld, int col0, int D, long long F_total, const long long* utt_start,
                       const long long* utt_start_host, int U, void* workspace, long long workspace_bytes,
                       void* stream);
/* Groups as a CSR pair: group g merges utterances group_utts[group_start[g] .. group_start[g + 1]) in
 * that order, one thread per (group, column), by sklearn's update:
 *   last_sum = mean * count;  mean' = (last_sum + sum) / (count + n);  r = count / n;
 *   m2' = var * count + m2 + r / (count + n) * (last_sum / r - sum)^2   (the first utterance: m2' = m2);
 *   var' = m2' / (count + n).
 * mean, var: [G, D] doubles; count: [G] (all device memory). */
int crk_scaler_merge(const void* workspace, long long workspace_bytes, int U, int D, const long long* group_start,
                     const int* group_utts, const long long* group_start_host, const int* group_utts_host, int G,
                     double* mean, double* var, long long* count, void* stream);

/* ---- per-speaker histograms of packed contours (csrc/histogram_kernels.hip) ----
 * The reduction of the recipe's stage 1, crank/bin/generate_histogram.py:31-74,109-146: plt.hist(np.hstack(f0s),
 * bins=200, range=(40, 700)) and the same over (-70, 20) for the frame power, per speaker.  The counts are
 * numpy.histogram(x, bins=bins, range=(first, last)), count for count: a value is kept when first <= x <= last (a NaN
 * or an infinity never is); its index is int((x - first) * norm), an index equal to bins moves down by one, and the
 * index is then corrected by one step against the edges, down when x < edges[i], up when x >= edges[i + 1] and
 * i != bins - 1.  The caller makes edges = linspace(first, last, bins + 1) and norm = bins / (last - first) as numpy
 * does and uploads the edges (bins + 1 doubles, device memory).  Float64 throughout.
 *
 * x: N doubles on the device; utterance u is x[utt_start[u] .. utt_start[u + 1]) and belongs to group utt_group[u].
 * counts [G, bins] and seen [G, 3] (values, kept, not finite) are device memory and are ADDED to, with integer adds:
 * the result does not depend on the launch shape, on the order of the utterances or on how a call is split, and a
 * group without an utterance keeps its row.  One workgroup per utterance and tile of 4096 values, an LDS table of
 * 32-bit counters, the non-zero bins flushed with 64-bit global adds; 16-byte loads where the tile starts on a 16-byte
 * boundary, 8-byte loads otherwise.
 *
 * The entry never allocates and never synchronises; it can be captured into a graph.  It takes the offsets and the
 * groups twice: the device copies the kernel reads and host copies that are checked before anything is launched.
 * CRK_ERR_ARG, with nothing launched: U < 1, G < 1, bins < 1, bins > 4096 (the LDS table next to the staged edges),
 * !(first < last) or a limit that is not finite, norm not positive, an empty utterance, offsets outside [0, N], a
 * group outside [0, G). */
int crk_hist_accumulate(const double* x, long long N, const long long* utt_start, const long long* utt_start_host,
                        const int* utt_group, const int* utt_group_host, int U, int G, const double* edges, double first,
                        double last, double norm, int bins, long long* counts, long long* seen, void* stream);

#define CRK_COLLATE_MAX_STREAMS 8
/* one continuous feature of the batch dict: columns [col0, col0 + ncols) of the packed
 * rows src[F_total, ld] -> dst (B, T, ncols), tail-padded with 0.0 */
typedef struct crk_collate_stream {
  const float* src;
  int ld, col0, ncols;
  float* dst;
} crk_collate_stream;
typedef struct crk_collate_desc {
  int n_streams;
  crk_collate_stream streams[CRK_COLLATE_MAX_STREAMS];
  const long long* utt_start; /* [n_utt + 1] first packed frame of each utterance */
  const int* utt_spk;         /* [n_utt] speaker index (position in scp["train"]["spkrs"]) */
  int n_utt, n_spk;
  const float* lcf0_raw;        /* [F_total] unscaled continuous log-F0, for cv_lcf0 (null: not produced) */
  const double* spk_lcf0_mean;  /* [n_spk] scaler[spkr]["lcf0"].mean_ */
  const double* spk_lcf0_std;   /* [n_spk] sqrt(scaler[spkr]["lcf0"].var_) */
  const float* raw;             /* use_raw: packed waveforms [sum samples] (null: none) */
  const long long* raw_start;   /* [n_utt + 1] first sample of each utterance */
  int fftl, hop;                /* conf["feature"]["fftl"], ["hop_size"] */
} crk_collate_desc;
/* picks (device, int32 [3][B]): utterance index, first kept frame p (used when the utterance is
 * longer than T; the reference draws it with random.choice, dataset.py:161) and conversion-target
 * speaker (dataset.py:84-86) of every batch row.  Outputs, each optional (null: skip):
 * cv_lcf0 (B,T) fp32 = convert_f0 in float64 rounded once, 0 on padding; org_h / cv_h (B,T) int64
 * with -100 on padding; one-hot codes (B,T,n_spk) fp32; mask (B,T) bytes 1/0; flen (B) int64 =
 * the utterance's own length (also when cropped); raw_out (B, fftl + hop*T - 1) fp32 = the waveform
 * padded / cropped like padding_raw (dataset.py:261-285), incl. its "no left padding when the crop
 * start is 0" quirk. */
int crk_collate_batch(const crk_collate_desc* desc, const int* picks, int B, int T, float* cv_lcf0,
                      long long* org_h, long long* cv_h, float* org_onehot, float* cv_onehot,
                      unsigned char* mask, long long* flen, float* raw_out, void* stream);

/* ---- decode-side F0 post-processing ------------------------------
 * BaseTrainer._store_features / _get_cvf0 (crank/net/trainer/basetrainer.py:311-320, :372-385):
 * lcf0 (B,T) fp32 normalised by the global lcf0 scaler -> inverse scaler (float32, as sklearn) ->
 * convert_f0 org_spk[b] -> cv_spk[b] in float64 -> cv_lcf0, f0 = exp(cv_lcf0) * uv and
 * normed_lcf0 = (cv_lcf0 - mean) / scale, all (B,T) float64, each optional.
 * has_lcf0_scaler = 0: "lcf0" is listed in ignore_scaler.  The spectral features use
 * crk_scaler_apply(inverse = 1). */
int crk_decode_f0(const float* lcf0, const float* uv, int B, int T, const int* org_spk, const int* cv_spk,
                  double lcf0_mean, double lcf0_scale, int has_lcf0_scaler, const double* spk_lcf0_mean,
                  const double* spk_lcf0_std, double* cv_lcf0, double* f0, double* normed_lcf0, void* stream);

/* ---- MCD evaluation with FastDTW alignment --------------------------
 * crank/bin/evaluate_mcd.py:61-77 for P utterance pairs at once: cv / gt are the voiced-frame
 * mel-cepstra (float64, [sum n][D] packed, pair p owns rows off[p]..off[p+1]); the warping path is
 * the third-party `fastdtw(cv, gt, dist=euclidean)` of the reference (radius 1 by default;
 * restated from its published algorithm, oracle/mcd.py) and mcd[p] = mean over the path of
 * 10 / ln 10 * sqrt(2 * sum_d (cv - gt)^2).  path_out (optional): path_stride ints per pair,
 * (i, j) pairs from start to end; path_len[p] = number of pairs.  status[p] = 1: pair too long
 * for the scratch / LDS sizing (max_nx, max_ny must bound every pair).  One wavefront per pair.
 * CRK_ERR_ARG for a non-positive count or a null pointer, CRK_ERR_UNSUPPORTED for max(max_nx, max_ny)
 * above 6398 (three rows of max + 2 doubles must fit 150 KB of LDS); the sizes are judged first. */
long long crk_mcd_scratch_bytes(int P, int max_nx, int max_ny, int D, int radius);
int crk_mcd_fastdtw(const double* cv, const long long* cv_off, const double* gt, const long long* gt_off, int P, int D,
                    int radius, int max_nx, int max_ny, double* mcd, int* path_len, int* path_out,
                    long long path_stride, void* scratch, int* status, void* stream);

/* ---- measurement -------------------------------------------------------------------
 * HIP-event timing of the conv kernels on their launch stream (bench.py's roofline leg),
 * one class per kernel: 0 conv_tile_kernel (generic per-layer conv), 1 stack_fwd_kernel,
 * 2 stack_bwd_kernel, 3 wgrad_kernel (table), 4 pstack_kernel, 5 stack_wgrad_kernel,
 * 6 pstack_wgrad_kernel, 7 the VQ codebook search (crk_vq_forward / _fused; bytes = 520 B per frame), 8 logmel_kernel
 * (crk_logmel_fwd).  crk_prof_enable(1) resets and starts recording, crk_prof_report
 * synchronises on the recorded events. */
int crk_prof_enable(int on);
int crk_prof_report(int cls, long long* count, double* total_ms, double* total_flops);
/* summed ALGORITHMIC HBM bytes of the class's launches (inputs read once + outputs and saved planes written
 * once), for the bandwidth side of the roofline */
int crk_prof_report_bytes(int cls, double* total_bytes);

/* The nearest-code search of crk_vq_forward / crk_vq_forward_fused (D = 64, K <= 512) runs on the f16 matrix pipe with
 * split operands and re-scores, with the exact fp32 chain, the frames whose two best candidates it cannot separate
 * (vq_kernels.hip: vq_forward_f16_kernel; indices identical to the exact search by construction).
 * crk_debug_vq_set_f16(0) selects the exact fp32-MFMA search instead (A/B runs, the equality test);
 * crk_debug_vq_flags: frames decided by [1] the two-candidate re-scoring, [2] the full exact scan since the last reset. */
int crk_debug_vq_set_f16(int on);
int crk_debug_vq_set_lc(int mode); /* CRK_VQ_LC from here on: 0 frame-per-lane, 1 code-per-lane, 2 matrix pipe (tests: all in one process) */
int crk_debug_vq_flags(unsigned long long* host_out3, int reset);

/* Measurement aid: bytes > 0 puts a read-modify-write pass over a private buffer of that size (choose > 256 MiB, the
 * Infinity Cache) in front of every conv-stack kernel launch from here on, 0 removes it again.  A/B runs only: with the
 * pass in place no kernel finds its producer's output in a cache (tools/mall_ab.sh). */
int crk_debug_flush_before(long long bytes);

/* ---- Parallel WaveGAN vocoder inference (recipe stage 6) ----------------------
 * Replaces `parallel-wavegan-decode` (egs/vaevc/template/run.sh:217-226, voc=PWG, run.sh:39): the third-party
 * ParallelWaveGANGenerator.inference(c, x) with a ConvInUpsampleNetwork, non-causal, 64 / 128 / 64 channels, kernel 3,
 * for a ragged batch of utterances, forward only.
 *
 * crk_voc_create: one handle per generator; `params` is a HOST fp32 block with weight norm already folded (g v / ||v||),
 * torch layouts, in this order:
 *   first_conv weight [64], bias [64]; upsample_net.conv_in weight [aux][aux][2 win + 1];
 *   per upsample scale s: the (1, 2s+1) Conv2d kernel [2s + 1];
 *   per layer: conv weight [128][64][3], conv bias [128], conv1x1_aux weight [128][aux], conv1x1_out weight [64][64],
 *              bias [64], conv1x1_skip weight [64][64], bias [64];
 *   last_conv_layers.1 weight [64][64], bias [64]; last_conv_layers.3 weight [64], bias [1].
 * Lays the weights out for the kernels and allocates the handle's device memory (this is the one allocation; it
 * synchronises the device).  NULL on an unsupported configuration: aux > 128, a scale outside 1..16, more than 8 scales.
 *
 * c: fp32 [total_frames][aux] row-major, frames of utterance u = rows frame_offsets[u] .. frame_offsets[u+1]-1
 * (frame_offsets: DEVICE int64 [n_utts + 1], frame_offsets[0] = 0, every utterance >= 1 frame); noise / out: fp32
 * [total_frames * hop], the samples of utterance u at frame_offsets[u] * hop.  workspace: device memory of at least
 * crk_voc_workspace_bytes(voc, n_utts, total_frames) bytes.  The compute entries never allocate.
 * flags: CRK_FLAG_PRECISE - split hi + lo bf16 operands (bf16x3; forward only, so bf16x3f is the same); else plain bf16. */
void* crk_voc_create(int layers, int stacks, int aux_ch, int aux_window, const int* scales, int n_scales, const float* params);
void crk_voc_destroy(void* voc);
long long crk_voc_workspace_bytes(void* voc, int n_utts, int total_frames);
int crk_voc_forward(void* voc, const float* c, const long long* frame_offsets, int n_utts, int total_frames,
                    const float* noise, float* out, void* workspace, long long workspace_bytes, int flags, void* stream);
/* the aux path alone (conv_in + upsampling network, fp32): out fp32 [total_frames * hop][aux] */
int crk_voc_upsample(void* voc, const float* c, const long long* frame_offsets, int n_utts, int total_frames, float* out,
                     void* workspace, long long workspace_bytes, void* stream);

/* ---- Streaming Parallel WaveGAN vocoding ------------------------------------------------------------------------
 * The generator of a crk_voc handle (its weights and fragments are shared, nothing is laid out twice) for chunks of new
 * frames of up to n_streams concurrent streams, at most max_chunk frames each per push.  The published generator is not
 * causal: a stream runs LA = win + ceil((D + A) / H) frames behind its input (H = prod(scales), D = sum of the layers'
 * dilations, A = sum_i H / prod_{j<i} scales[j]; 16 frames for the published default).  A stream that has received T
 * frames of its utterance has emitted max(0, T - LA) H samples; a push whose end flag is set for a stream emits
 * everything up to T H with the utterance's right-edge rules and returns that stream to the start-of-utterance state.
 * The emitted samples equal crk_voc_forward's for the whole utterance with the same noise bit for bit, in both
 * precisions and however the utterance is cut into pushes.  An utterance holds at most 2^30 - 1 samples: frames past
 * that are not taken (n_out tells).
 *
 * crk_voc_stream_create is the one call that allocates (state of every stream; it synchronises); the crk_voc handle must
 * outlive it.  crk_voc_stream_state_bytes: the size of that allocation.  crk_voc_stream_lookahead: LA.
 * crk_voc_stream_reset: the streams listed in the HOST array stream_ids (NULL: every stream) start a new utterance.
 * crk_voc_stream_push: c fp32 [S][C][aux], noise fp32 [S][C * H], n_valid / end DEVICE int32 [S] (NULL: C / 0; frames
 * and noise at and past n_valid are ignored), wave fp32 [S][(C + LA) * H], n_out DEVICE int32 [S]: the samples written
 * per stream, from the start of its row; samples past n_out are not written.  S <= n_streams, C <= max_chunk; stream i
 * is row i.  Every position lives on the device: a push never allocates and reads nothing back (it can be captured in
 * a graph), and launches 3 + n_scales + layers kernels whatever S, C, n_valid and end are.
 * flags: CRK_FLAG_PRECISE as crk_voc_forward. */
int crk_voc_stream_create(void* voc, int n_streams, int max_chunk, void** handle);
void crk_voc_stream_destroy(void* st);
long long crk_voc_stream_state_bytes(void* st);
int crk_voc_stream_lookahead(void* st);
int crk_voc_stream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_voc_stream_push(void* st, const float* c, const float* noise, const int* n_valid, const int* end, int S, int C,
                        float* wave, int* n_out, int flags, void* stream);

/* ---- WORLD waveform synthesis for mel-cepstral models (recipe stage 5, output_feat_type mcep) ---------------------
 * Replaces the reference's world2wav (sprocket Synthesizer.synthesis: mod_power, pysptk mc2sp, pyworld
 * decode_aperiodicity + synthesize), all in float64, for a ragged batch of utterances.  Parity with pyworld / pysptk is
 * unpinned; the oracle is tests/world_synth_ref.py.  CRANK_AMD_PRECISION does not apply.
 *
 * crk_world_create: one handle per (fs, fftl, shiftms, alpha, mcep order + 1, bands); precomputes the freqt / mc2sp
 * matrices, FFT twiddles and the DC remover and allocates them (one allocation; synchronises).  NULL unless fftl = 1024,
 * order1 <= 128 and bands = int(min(15000, fs/2 - 3000) / 3000).  pulse_capacity: pulses per response buffer (the
 * workspace holds pulse_capacity * 1024 doubles; a call with more pulses runs several rounds of it, in order).
 * crk_world_reserve: WORLD's randn stream (reseeded, as every synthesis reseeds) for utterances of up to max_samples
 * output samples; allocates (synchronises) only when the table grows.
 *
 * f0: [total_frames] (Hz, 0 unvoiced); mcep, rmcep: [total_frames][order1] (rmcep NULL: no power modification); cap:
 * [total_frames][bands] (dB); frames of utterance u = rows frame_offsets[u] .. frame_offsets[u+1]-1, at least 2 per
 * utterance.  sample_offsets: utterance u owns y[sample_offsets[u] .. sample_offsets[u+1]), its length
 * int(frames * shiftms * fs / 1000) (the caller computes it).  Both offset arrays: DEVICE int64 [n_utts + 1].
 * workspace: device memory of at least crk_world_workspace_bytes(h, n_utts, total_frames, total_samples) bytes.  The
 * compute entries never allocate.  crk_world_synthesis reads the batch's pulse count back to the host once (it sizes
 * the pulse launches; the call synchronises its stream there) and stores it in *n_pulses when that is not NULL;
 * max_samples is the longest utterance's sample count (at most what crk_world_reserve covered). */
void* crk_world_create(int fs, int fftl, double shiftms, double alpha, int order1, int bands, int pulse_capacity);
void crk_world_destroy(void* world);
int crk_world_reserve(void* world, long long max_samples);
long long crk_world_workspace_bytes(void* world, int n_utts, long long total_frames, long long total_samples);
int crk_world_synthesis(void* world, const double* f0, const double* mcep, const double* rmcep, const double* cap,
                        int order1, int bands, const long long* frame_offsets, const long long* sample_offsets, int n_utts,
                        long long total_frames, long long total_samples, long long max_samples, double* y,
                        long long* n_pulses, void* workspace, long long workspace_bytes, void* stream);
/* the per-frame stage alone: sp, ap [total_frames][513] (power-modified sp when rmcep is given); uses the first
 * 16 * total_frames bytes of the workspace */
int crk_world_frames(void* world, const double* mcep, const double* rmcep, const double* cap, int order1, int bands,
                     long long total_frames, double* sp, double* ap, void* workspace, long long workspace_bytes, void* stream);
/* the time base alone: utterance u's pulses at pulse_pos / pulse_shift (seconds) / pulse_vuv [sample_offsets[u] + i],
 * i < pulse_count[u] (pulse_pos: the sample within the utterance); the slot arrays hold total_samples entries */
int crk_world_pulses(void* world, const double* f0, const long long* frame_offsets, const long long* sample_offsets,
                     int n_utts, int* pulse_pos, double* pulse_shift, unsigned char* pulse_vuv, long long* pulse_count,
                     void* stream);

/* ---- The spectral half of WORLD analysis (csrc/world_analysis_kernels.hip) ----
 * What the reference's evaluate_mcd.py runs on a converted waveform, without F0 estimation and aperiodicity: low-cut
 * FIR, CheapTrick spectral envelope (pyworld cheaptrick), pysptk sp2mc and sprocket spc2npow, all in float64, for a ragged
 * batch of utterances and a GIVEN F0 contour per utterance.  Parity with pyworld / pysptk is unpinned; the oracle is
 * tests/world_analysis_ref.py.  CRANK_AMD_PRECISION does not apply.
 *
 * crk_wana_create: one handle per (fs, fftl, shiftms, alpha, mcep order + 1); precomputes the FFT twiddles and the freqt
 * matrix and allocates them (one allocation; synchronises).  NULL unless fftl = 1024 and order1 <= 128.
 * crk_wana_reserve: WORLD's randn stream (reseeded once per utterance) for utterances that draw up to max_draws values:
 * a frame draws 2 * half + 1 + 513 values, half = round(1.5 fs / F0) <= 511, so frames * 1536 always suffices.
 * Allocates (synchronises) only when the table grows.
 *
 * x: [total_samples] waveforms, utterance u = x[sample_offsets[u] .. sample_offsets[u+1]); f0: [total_frames] (Hz; at or
 * below 3 fs / 1021 the frame is analysed at 500 Hz; at most fs / 4), utterance u = rows frame_offsets[u] ..
 * frame_offsets[u+1]-1, frame i centred at sample round(i * shiftms / 1000 * fs + 0.001).  Both offset arrays: DEVICE int64
 * [n_utts + 1].  workspace: device memory of at least crk_wana_workspace_bytes(n_utts, total_frames, total_samples) bytes.
 * The compute entries never allocate and never synchronise; max_draws (the largest draw count of one utterance, or a bound
 * of it) above what crk_wana_reserve covered is CRK_ERR_ARG. */
void* crk_wana_create(int fs, int fftl, double shiftms, double alpha, int order1);
void crk_wana_destroy(void* wana);
int crk_wana_reserve(void* wana, long long max_draws);
long long crk_wana_workspace_bytes(int n_utts, long long total_frames, long long total_samples);
/* y[g] = sum_k taps[k] x[g - k] within the utterance (zero history); taps: DEVICE [n_taps], n_taps <= 256.  One workgroup
 * filters crk_wana_lowcut_tile() consecutive samples. */
int crk_wana_lowcut(void* wana, const float* x, const double* taps, int n_taps, const long long* sample_offsets, int n_utts,
                    long long total_samples, double* y, void* stream);
int crk_wana_lowcut_tile(void);
/* sp: [total_frames][513], the spectral envelope */
int crk_wana_cheaptrick(void* wana, const double* x, const double* f0, const long long* frame_offsets,
                        const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                        long long max_draws, double* sp, void* workspace, long long workspace_bytes, void* stream);
/* mcep: [total_frames][order1] = sp2mc(sp, order1 - 1, alpha), from the envelope's cepstrum; sp (optional, may be NULL)
 * as above.  order1 must be the handle's. */
int crk_wana_mcep(void* wana, const double* x, const double* f0, const long long* frame_offsets,
                  const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                  long long max_draws, int order1, double* mcep, double* sp, void* workspace, long long workspace_bytes,
                  void* stream);
/* npow: [total_frames], 10 log10 of each frame's power over its utterance's mean power */
int crk_wana_npow(void* wana, const double* sp, const long long* frame_offsets, int n_utts, long long total_frames,
                  double* npow, void* workspace, long long workspace_bytes, void* stream);
/* debug: the integers the CheapTrick kernel forms per frame: shapes [total_frames][4] = frame origin (sample), half
 * window, DC-correction limit, smoothing boundary; draw_offsets [total_frames] = where the frame's randn draws start in
 * its utterance's stream */
int crk_wana_frame_shapes(void* wana, const double* f0, const long long* frame_offsets, int n_utts, long long total_frames,
                          int* shapes, long long* draw_offsets, void* stream);

/* ---- D4C aperiodicity and its coding (csrc/d4c_kernels.hip), on the crk_wana handle ----
 * pyworld d4c(x, f0, i * shiftms / 1000, fs, threshold, fft_size = 1024) and code_aperiodicity in float64 for a ragged
 * batch with a GIVEN F0 contour (0 = unvoiced, at most fs / 4); x, f0 and the offset arrays as above.  The oracle is
 * tests/d4c_ref.py; parity with pyworld is unpinned.  Handles of 13640 <= fs <= 24052 only (both of D4C's transforms are
 * 2048 points there): any other is CRK_ERR_UNSUPPORTED.
 *
 * The randn stream is the handle's (crk_wana_reserve).  A voiced frame draws 2 round(1.5 fs / max(f0, 40)) + 1 values in
 * the Love-Train pass and, where it passes the threshold, 3 (2 round(2 fs / max(f0, 47)) + 1) in the general pass, so
 * frames * crk_wana_d4c_draws_per_frame() bounds an utterance.  max_draws above the reservation is CRK_ERR_ARG.
 * workspace: at least crk_wana_d4c_workspace_bytes(n_utts, total_frames) bytes.  The compute entries never allocate and
 * never synchronise. */
long long crk_wana_d4c_workspace_bytes(int n_utts, long long total_frames);
int crk_wana_d4c_draws_per_frame(void* wana);
/* ap: [total_frames][513] and / or cap: [total_frames][bands] in dB, bands = int(min(15000, fs / 2 - 3000) / 3000); either
 * may be NULL, not both.  cap alone evaluates only the two bins around each band's knot. */
int crk_wana_d4c(void* wana, const double* x, const double* f0, const long long* frame_offsets,
                 const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                 long long max_draws, double threshold, double* ap, double* cap, void* workspace, long long workspace_bytes,
                 void* stream);
/* cap of a given ap table (any handle whose fs has 1 .. 3 bands) */
int crk_wana_d4c_code(void* wana, const double* ap, long long total_frames, double* cap, void* stream);
/* debug: what the kernels form before the general pass: shapes [total_frames][8] = frame origin, Love-Train half window,
 * general half window, the two centroid origins, DC-correction limit, smoothing boundaries of width f0 / 2 and f0 (zero
 * but the origin for an unvoiced frame); pass [total_frames] = 1 where the general pass runs; lt_offsets, gb_offsets
 * [total_frames] = where the frame's draws of either pass start in its utterance's stream */
int crk_wana_d4c_frame_shapes(void* wana, const double* x, const double* f0, const long long* frame_offsets,
                              const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples,
                              long long max_draws, double threshold, int* shapes, int* pass, long long* lt_offsets,
                              long long* gb_offsets, void* workspace, long long workspace_bytes, void* stream);

/* ---- Harvest F0 estimation (csrc/f0_kernels.hip) ----
 * pyworld.harvest as sprocket's FeatureExtractor.analyze calls it, in float64, for a ragged batch of utterances with a
 * search range each.  The definition is tests/harvest_ref.py; parity with pyworld is unpinned.
 *
 * The caller forms the batch's layout on the host (crank_amd/world.py HarvestF0._layout) and passes DEVICE tables:
 *   utt     int64 [n_utts][12]: sample offset, samples, decimated offset, decimated samples (ceil(samples / r)), 1 ms frame
 *           offset, 1 ms frames (int(1000 samples / fs) + 1), channel offset, channels (<= 192), raw-table offset (cells),
 *           output frame offset, output frames, 0
 *   range   double [n_utts][2]: 0.9 minf0, 1.1 maxf0
 *   chan_bf double [total_channels]: centre frequencies;  chan int64 [total_channels][4]: half filter length
 *           round(2 fs_d / bf) <= 672, offset of the channel's 4 event streams (doubles), capacity of one stream, utterance
 * total_events is the sum of 4 * capacity.  The kernels trust these tables.
 *
 * crk_f0_create: one handle per (fs, shiftms); cheby: HOST [8] = b[4], a[4] of the decimation low-pass (order-3 Chebyshev-I,
 * 0.05 dB, 0.8 / r of Nyquist, r = clamp(round(fs / 8000), 1, 12)).  Allocates the twiddle table (synchronises).  NULL
 * unless 8000 <= fs <= 48000.  crk_f0_reserve: the event streams' storage, kept and grown (allocates and synchronises
 * only then).  The compute entries never allocate and never synchronise; total_events above the reservation, or a
 * workspace below crk_f0_workspace_bytes, is CRK_ERR_ARG.  status: DEVICE int [n_utts], 1 where an event stream
 * overflowed its capacity (its later events were dropped). */
void* crk_f0_create(int fs, int shiftms, const double* cheby);
void crk_f0_destroy(void* f0);
int crk_f0_reserve(void* f0, long long total_events);
long long crk_f0_workspace_bytes(int n_utts, long long total_samples, long long total_frames, long long total_channels);
/* f0: [total_out] at shiftms, utterance u = its output frames */
int crk_f0_harvest(void* f0h, const double* x, const long long* utt, const double* range, const double* chan_bf,
                   const long long* chan, int n_utts, long long total_samples, long long total_channels,
                   long long total_frames, long long total_events, long long total_out, double* f0, int* status,
                   void* workspace, long long workspace_bytes, void* stream);
/* the stages.  yd: decimated, mean-free signals at the decimated offsets */
int crk_f0_decimate(void* f0h, const double* x, const long long* utt, int n_utts, long long total_samples, double* yd,
                    void* workspace, long long workspace_bytes, void* stream);
/* raw: per utterance a (channels, 1 ms frames) table at its raw-table offset; 0 marks an empty cell */
int crk_f0_raw_candidates(void* f0h, const double* yd, const long long* utt, const double* range, const double* chan_bf,
                          const long long* chan, int n_utts, long long total_channels, long long total_frames,
                          long long total_events, double* raw, int* status, void* workspace, long long workspace_bytes,
                          void* stream);
/* cands: [total_frames][112]: 16 run means per frame, overlapped with the frames 1, 2, 3 before and after */
int crk_f0_candidates(void* f0h, const double* raw, const long long* utt, int n_utts, long long total_frames, double* cands,
                      void* workspace, long long workspace_bytes, void* stream);
/* refined, scores: [total_frames][112]; 0 where the candidate is empty or rejected */
int crk_f0_refine(void* f0h, const double* x, const double* cands, const long long* utt, const double* range, int n_utts,
                  long long total_frames, double* refined, double* scores, void* stream);
/* f0_1ms: [total_frames] */
int crk_f0_contour(void* f0h, const double* refined, const double* scores, const long long* utt, int n_utts,
                   long long total_frames, double* f0_1ms, void* workspace, long long workspace_bytes, void* stream);
/* the reference's convert_continuos_f0 and lf0 / lcf0; frame_offsets: DEVICE int64 [n_utts + 1]; status [n_utts]: 1 for an
 * utterance without a voiced frame (its outputs are not written) */
int crk_f0_continuous(const double* f0, const long long* frame_offsets, int n_utts, long long total_frames, float* uv,
                      double* f0_filled, double* cf0, double* lf0, double* lcf0, int* status, void* stream);

/* ---- streaming F0 conditioning: Harvest on a block grid (csrc/f0_stream_kernels.hip) ----
 * Samples in, the lcf0 / uv rows crk_stream_push takes for a decoder_f0 model out, for up to n_streams concurrent streams
 * of at most max_samples each per push (the definition is tests/f0_stream_ref.py).  All grid
 * arithmetic is in whole milliseconds and integers.  Block j = the stream's 1 ms frames [j block, (j + 1) block); it is
 * ready once the stream holds ((j + 1) block + ahead) ms; its window is the signal over [max(j block - back, 0) ms,
 * ((j + 1) block + ahead) ms), truncated at the stream's start and, under the end flag, at the last sample; its 1 ms contour
 * is those frames of crk_f0_harvest of the window alone, through f0h, a crk_f0_create handle with a frame period of 1 ms.
 * Output frame t sits at 1 ms frame t shiftms, or with hop_size at (2000 t hop + fs) / (2 fs); exactly one of the two is
 * positive.  With n_taps > 0 the signal is first filtered by the causal FIR taps (HOST float64), zero history at the
 * stream's start, by crk_wana_lowcut's arithmetic.  A push with the end flag emits every remaining block up to the one
 * holding the last 1 ms frame int(1000 n / fs), the frames below the offline count (int(1000 n / fs / shiftms) + 1, or
 * 1 + n / hop) with their 1 ms index clamped to that frame - nothing when n < 64 - and returns the stream to its start
 * state.  Per window: g = the contour at the output frames the window holds; uv, cf0 = convert_continuos_f0 of g as
 * crk_f0_continuous has it, or uv = 0 and cf0 = the stream's carry (the last cf0 it emitted; exp(spk_lcf0_mean[org_spk])
 * before any) where g has no voiced frame; lcf0 = convert_f0(log cf0) org -> cv as crk_decode_f0, then (v - lcf0_mean) /
 * lcf0_scale if has_lcf0_scaler; float64, rounded once.  Only the block's frames are written.
 *
 * crk_f0_stream_create allocates once (synchronises): per stream a power-of-two ring of raw samples holding back + block +
 * ahead ms, the n_taps - 1 samples the filter reaches back and one push, two 64-bit counts, the carry and a flag word;
 * and one round's windows and contours.  CRK_ERR_ARG: fs outside 8000 .. 48000; back, ahead or block outside 1 .. 10000 ms
 * or not on a whole sample ((ms fs) % 1000 != 0); block or back below 64 samples; both or neither of shiftms, hop_size;
 * hop_size below 1 ms; n_taps outside 0 .. 256.  crk_f0_stream_max_frames: the most frames one push emits over all
 * histories, the end flush included.  crk_f0_stream_max_rounds: the most rounds.  crk_f0_stream_reset: the streams in the
 * HOST array stream_ids (NULL: all) return to their start state, flags cleared.
 *
 * The handle keeps the counts on the host too.  A ROUND of a push is the streams with a further block ready.
 * crk_f0_stream_plan (host only): n_valid / end HOST int32 [S] (NULL: C / 0); writes n_rounds, round_n [max_rounds],
 * ids and lens [max_rounds][S] (row stride S): per round the ready streams, ascending, and their windows' samples.  The
 * caller lays each round out as crk_f0_harvest's batch (utterance u = stream ids[u], lens[u] samples, output frames = 1 ms
 * frames) and passes the DEVICE tables in crk_f0_stream_round, ids as DEVICE int32 [n_ready].
 * crk_f0_stream_push: x fp32 [S][C], row stride ldx; n_valid / end on the HOST and the same values as DEVICE int32 [S]
 * (n_valid_dev / end_dev; both NULL or neither); org_spk / cv_spk DEVICE int32 [S], spk_lcf0_mean / std DEVICE double
 * [n_spk]; lcf0, uv fp32 [S][max_frames]; n_frames DEVICE int32 [S], written for every stream; raw (the contour) and cv_f0
 * (exp(cv_lcf0) uv) double [S][max_frames], optional; workspace as crk_f0_harvest takes it, for the largest round, whose
 * events crk_f0_reserve covers.  Judged before any launch, state and outputs untouched, sizes before pointers:
 * CRK_ERR_ARG for S < 1, C < 0, ldx < C, n_valid outside 0 .. C, rounds that are not this push's plan, a null pointer;
 * CRK_ERR_UNSUPPORTED for S > n_streams, C > max_samples.  A push never allocates, never synchronises and reads nothing
 * back; it launches 1 kernel when no block is ready and 2 + crk_f0_harvest's per round otherwise.  It cannot be captured
 * in a graph: what it launches depends on the counts.  crk_f0_stream_status synchronises and copies the sticky flags to
 * HOST int32 [n_streams]: 1 a Harvest event stream overflowed, 2 a round's tables did not fit the device's counts. */
typedef struct crk_f0_stream_round {
  const int* ids;
  const long long* utt;
  const double* range;
  const double* chan_bf;
  const long long* chan;
  int n_ready;
  long long total_samples, total_channels, total_frames, total_events;
} crk_f0_stream_round;
int crk_f0_stream_create(int fs, int back_ms, int ahead_ms, int block_ms, int shiftms, int hop_size, const double* taps,
                         int n_taps, int n_streams, int max_samples, void** handle);
void crk_f0_stream_destroy(void* st);
long long crk_f0_stream_state_bytes(void* st);
int crk_f0_stream_max_frames(void* st);
int crk_f0_stream_max_rounds(void* st);
int crk_f0_stream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_f0_stream_plan(void* st, const int* n_valid, const int* end, int S, int C, int* n_rounds, int* round_n, int* ids,
                       long long* lens);
int crk_f0_stream_push(void* st, void* f0h, const float* x, int ldx, const int* n_valid, const int* end,
                       const int* n_valid_dev, const int* end_dev, int S, int C, const crk_f0_stream_round* rounds,
                       int n_rounds, const int* org_spk, const int* cv_spk, const double* spk_lcf0_mean,
                       const double* spk_lcf0_std, int n_spk, double lcf0_mean, double lcf0_scale, int has_lcf0_scaler,
                       float* lcf0, float* uv, int* n_frames, double* raw, double* cv_f0, void* workspace,
                       long long workspace_bytes, void* stream);
int crk_f0_stream_status(void* st, int* flags, void* stream);

/* ---- Streaming CheapTrick / mel-cepstrum analysis (csrc/wana_stream_kernels.hip) ---------------
 * The frames crk_wana_mcep writes for a whole utterance, from a live stream: samples and F0 rows in, every frame out
 * bit for bit as soon as its window is complete.  `wana` is a crk_wana_create handle (fs, shiftms, alpha, order1 are
 * its own); it must outlive the stream handle, and crk_wana_stream_create reserves its randn table for
 * max_utt_frames * 1536 draws (crk_wana_reserve; 1536 = the most one frame draws).  Per stream the handle keeps, on the
 * device: the analysed signal y - the causal FIR taps (HOST float64, n_taps in 0 .. 255; 0: y = (double)x) with zero
 * history at the utterance's start, by crk_wana_lowcut's arithmetic, each sample filtered once - in a power-of-two
 * float64 ring of at least ring_capacity samples addressed by absolute position; the last raw samples the filter reaches;
 * a queue of at most f0_capacity F0 rows (row k of an utterance is frame k) that have arrived and whose frames have not
 * left; 64-bit counts of samples, rows and frames that left; the randn draw offset of the next frame; a sticky flag word.
 * crk_wana_stream_create is the one call that allocates (it synchronises).  CRK_ERR_ARG: a null pointer, a size below 1,
 * n_taps outside 0 .. 255, ring_capacity < max_samples; CRK_ERR_UNSUPPORTED: more than 65535 streams, f0_capacity or
 * max_f0_in above 65536, ring_capacity above 2^26, max_utt_frames * 1536 above 2^31, use_mcep_0th == 0 with order1 == 1.
 * crk_wana_stream_max_frames: f0_capacity, the most frames one push emits.  crk_wana_stream_reset: the streams in the
 * HOST array stream_ids (NULL: all) return to their start state, flags cleared.
 *
 * crk_wana_stream_push: x fp32 [S][C] (row stride ldx), f0 double [S][R] (row stride ldf; raw contour, 0 = unvoiced);
 * n_valid, n_f0, end DEVICE int32 [S] or NULL (C, R, 0; the counts are clamped to 0 .. C and 0 .. R).  The samples and
 * rows are appended; then frame i of a stream leaves, in order, if its row has arrived and n >= origin_i + 512, origin_i
 * crk_wana_frame_shapes' origin of frame i, n the samples so far - or, with end[s] != 0, every waiting frame leaves with
 * its window clamped at n, and the stream returns to its start state.  Frame j to leave writes row j of mcep
 * [S][max_frames][order1], of sp [S][max_frames][513] (optional) and of feats fp32 [S][max_frames][order1 - first]
 * (first = 0 with use_mcep_0th, else 1): column m - first = mcep[m], or (mcep[m] - mean[m]) / scale[m] with mean / scale
 * DEVICE double [order1] (both or neither), in float64 without contraction, rounded once.  Rows at and past n_frames[s]
 * are not written.  n_frames, first, n_dropped DEVICE int32 [S] are written for every stream.  Sticky flags: 1 a frame's
 * window start had left the ring (origin - half < n - ring_capacity): the frame is dropped and counted in n_dropped, its
 * draws still consumed; 2 the queue overflowed: the newest rows that do not fit are dropped and counted; 4 a draw offset
 * passed the reserved table: the kernel's clamp applies, the frame is emitted; 8 at an end push, rows k with
 * k shift > n + shift (shift = shiftms / 1000 fs, what the offline call refuses) or rows with n == 0: dropped and
 * counted; 16 an F0 row that is not finite, negative or above fs / 4: analysed as 0.  Judged before any launch, state
 * and outputs untouched: CRK_ERR_ARG for S < 1, C or R < 0, a stride below its width, a null pointer (sp, mean / scale
 * and the three int inputs excepted); CRK_ERR_UNSUPPORTED for S > n_streams, C > max_samples, R > max_f0_in.  Four
 * launches whose grids depend on the handle and S alone; never allocates, never synchronises, reads nothing back:
 * capturable.  crk_wana_stream_status synchronises and copies the flags of all n_streams streams to HOST int32. */
int crk_wana_stream_create(void* wana, const double* taps, int n_taps, int n_streams, int max_samples, int max_f0_in,
                           int f0_capacity, int ring_capacity, int max_utt_frames, int use_mcep_0th, void** handle);
void crk_wana_stream_destroy(void* st);
long long crk_wana_stream_state_bytes(void* st);
int crk_wana_stream_max_frames(void* st);
int crk_wana_stream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_wana_stream_push(void* st, const float* x, int ldx, const int* n_valid, int C, const double* f0, int ldf,
                         const int* n_f0, int R, const int* end, int S, const double* mean, const double* scale,
                         double* mcep, double* sp, float* feats, int* n_frames, int* first, int* n_dropped, void* stream);
int crk_wana_stream_status(void* st, int* flags, void* stream);

/* ---- Streaming WORLD synthesis (csrc/world_stream_kernels.hip) ----------------------------------
 * The samples crk_world_synthesis writes for a whole utterance, from a live stream of frame rows: F0, mel-cepstrum, coded
 * aperiodicity (and rmcep with power modification) in, every sample out bit for bit as soon as no pulse can reach it.
 * `world` is a crk_world_create handle of the stream's own (fs, shiftms, alpha, order1, bands are its); it must outlive
 * the stream handle and no other call may use it: crk_wsyn_stream_create reserves its randn table for max_utt_samples
 * values (crk_world_reserve) and a captured push reads that table.  Per stream the handle keeps, on the device: a queue of
 * at most row_capacity frame rows (F0, sp [513], ap [513]; row k of an utterance is frame k, at k % row_capacity); the
 * time base's float64 phase total, the last sample's wrapped phase and vuv; 64-bit counts of rows, samples with a phase
 * and samples that left; the utterance's first pulse; the pending pulse (found, not yet added); a power-of-two float64
 * ring of at least ring_capacity samples addressed by absolute position; a sticky flag word; and per push a list of
 * max_pulses + 1 pulses and max_pulses responses of 1024 doubles.  crk_wsyn_stream_create is the one call that allocates
 * (it synchronises).  CRK_ERR_ARG: a null pointer, n_streams, max_rows_in, max_pulses, max_out or max_utt_samples below 1,
 * row_capacity below 2, ring_capacity below 1024, f0_ceil not in (0, fs / 4]; CRK_ERR_UNSUPPORTED: more than 65535
 * streams, max_rows_in above 4096, row_capacity above 65536, ring_capacity or max_out above 2^24, max_pulses above 65535,
 * max_utt_samples above 2^31, fewer than 2 samples per frame.  crk_wsyn_stream_max_out: the most samples one push emits.
 * crk_wsyn_stream_reset: the streams in the HOST array stream_ids (NULL: all) return to their start state, ring zeroed,
 * flags cleared.
 *
 * crk_wsyn_stream_push: f0 double [S][R] (Hz, 0 = unvoiced), mcep [S][R][order1], codeap [S][R][bands], rmcep
 * [S][R][order1] (given exactly when the handle has power_mod, R > 0), all contiguous DEVICE float64; n_rows, end DEVICE
 * int32 [S] or NULL (R, 0; n_rows is clamped to 0 .. R).  The rows are appended; the time base runs over every sample
 * whose frame is at most rows - 2 (at an end: to y_length(rows) with the offline clamp and extrapolated knot); a pulse at
 * i is found when sample i + 1 has its phase and added when its successor is found (at an end the last one with noise
 * size 0); sample i leaves, in order, once i + 511 < B, B the pending pulse or else the last sample with a phase; at an
 * end every sample below y_length leaves and the stream returns to its start state.  The j-th sample to leave is y
 * [S][max_out] column j (clamped to [-1, 1] with clip != 0); columns at and past n_samples[s] are not written.
 * n_samples, n_dropped DEVICE int32 [S] are written for every stream.  Sticky flags: 1 a push needed more than
 * ring_capacity samples of ring (adds past it are lost); 2 the row queue overflowed: the newest rows are dropped and
 * counted in n_dropped; 4 a pulse's noise offset passed max_utt_samples: the kernel's clamp applies; 8 an end push on a
 * stream holding one row: the row is dropped and counted, nothing leaves (an end on an empty stream is a no-op); 16 an F0
 * row not finite, negative or above f0_ceil: synthesised as 0; 32 a push found more pulses than max_pulses (the last are
 * lost); 64 more samples were ready than max_out (the rest are lost).  Every index into queue, ring, list and responses
 * is masked or clamped.  Judged before any launch, state and outputs untouched: CRK_ERR_ARG for S < 1, R < 0, a null
 * pointer (n_rows, end excepted; the row inputs only when R > 0), rmcep missing with power_mod or given without;
 * CRK_ERR_UNSUPPORTED for S > n_streams, R > max_rows_in.  Five launches, six with power_mod, whose grids depend on the
 * handle and S alone; never allocates, never synchronises, reads nothing back, no atomics: capturable.
 * crk_wsyn_stream_status synchronises and copies the flags of all n_streams streams to HOST int32. */
int crk_wsyn_stream_create(void* world, int n_streams, int max_rows_in, int row_capacity, int ring_capacity, int max_pulses,
                           int max_out, double f0_ceil, int power_mod, long long max_utt_samples, void** handle);
void crk_wsyn_stream_destroy(void* st);
long long crk_wsyn_stream_state_bytes(void* st);
int crk_wsyn_stream_max_out(void* st);
int crk_wsyn_stream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_wsyn_stream_push(void* st, const double* f0, const double* mcep, const double* codeap, const double* rmcep,
                         const int* n_rows, int R, const int* end, int S, int clip, double* y, int* n_samples,
                         int* n_dropped, void* stream);
int crk_wsyn_stream_status(void* st, int* flags, void* stream);

/* ---- Griffin-Lim waveform synthesis for log-mel models (csrc/griffin_lim_kernels.hip) ----
 * Replaces the reference's mlfb2wav (crank/utils/utils.py:94-107, 210-269: logmelspc_to_linearspc, griffin_lim -> librosa.griffinlim
 * with momentum 0.99, centred reflect-padded STFT, periodic Hann window; called by BaseTrainer._save_decoded_mlfb,
 * crank/net/trainer/basetrainer.py:400-417, and crank/bin/griffin_lim.py), all in float64, for a ragged batch of utterances.
 * Parity with librosa is unpinned; the oracle is tests/griffin_lim_ref.py.  CRANK_AMD_PRECISION does not apply.
 *
 * crk_gl_create: one handle per (fs, n_fft, win_length, hop, n_mels, basis); pinv_basis is the HOST float64 pseudo-inverse of
 * the mel basis, [n_fft / 2 + 1][n_mels] row-major.  Uploads it with the FFT twiddles and the window (one allocation;
 * synchronises) and stores the handle in *handle.  CRK_ERR_UNSUPPORTED unless n_fft = 1024, 1 <= win_length <= 1024,
 * 1 <= hop <= 1024 and n_mels <= 256.
 *
 * Frames of utterance u = rows frame_offsets[u] .. frame_offsets[u+1]-1 (T_u of them); it owns the samples
 * sample_offsets[u] .. sample_offsets[u+1], hop * (T_u - 1) of them (the caller computes it), which must exceed n_fft / 2
 * so that one reflection pads it.  Both offset arrays: DEVICE int64 [n_utts + 1].  Spectra are [total_frames][513],
 * complex ones as interleaved (re, im) float64.  workspace: device memory of at least
 * crk_gl_workspace_bytes(n_utts, total_frames, total_samples) bytes; too small is CRK_ERR_ARG and launches nothing.  The
 * compute entries never allocate and never synchronise. */
int crk_gl_create(int fs, int n_fft, int win_length, int hop, int n_mels, const double* pinv_basis, void** handle);
void crk_gl_destroy(void* gl);
long long crk_gl_workspace_bytes(int n_utts, long long total_frames, long long total_samples);
/* utils.py:210-234 (logmelspc_to_linearspc): S[f][k] = sum_m 10^mlfb[f][m] pinv_basis[k][m], signed as the reference
 * returns it; magnitude != 0 stores its absolute value, the np.abs of utils.py:257.  mlfb: [total_frames][n_mels] */
int crk_gl_linear_spectrum(void* gl, const double* mlfb, long long total_frames, int magnitude, double* S, void* stream);
/* utils.py:237-269 (griffin_lim): n_iter iterations from the unit phasors angles0 (complex [total_frames][513]), then the
 * final inverse STFT into y [total_samples]; clip != 0 clips y to [-1, 1 - 2^-15] as utils.py:258-268 does.  n_iter + 2 launches. */
int crk_gl_run(void* gl, const double* S, const double* angles0, const long long* frame_offsets,
               const long long* sample_offsets, int n_utts, long long total_frames, long long total_samples, int n_iter,
               int clip, double* y, void* workspace, long long workspace_bytes, void* stream);
/* the two projections alone (librosa.stft / librosa.istft as griffinlim calls them): spec complex [total_frames][513].
 * crk_gl_stft takes waveforms of any length above n_fft / 2: T_u = 1 + length / hop */
int crk_gl_stft(void* gl, const double* x, const long long* frame_offsets, const long long* sample_offsets, int n_utts,
                long long total_frames, long long total_samples, double* spec, void* stream);
int crk_gl_istft(void* gl, const double* spec, const long long* frame_offsets, const long long* sample_offsets, int n_utts,
                 long long total_frames, long long total_samples, double* y, void* workspace, long long workspace_bytes,
                 void* stream);

/* ---- streaming conversion for causal generators (csrc/stream_kernels.hip) ----
 * The generator forward of crank/net/module/vqvae2.py:160-190 (encoders, "enc[n] + dec", codebook search and lookup, decoders,
 * the last decoder on cat[q_top .. q_0] with cat[lcf0, uv, speaker embedding or one-hot code]) for a chunk of C new frames of S
 * independent streams in ONE launch, one workgroup per stream, fp32.  use_causal_conv only: every residual layer keeps the
 * last (k - 1) * dilation frames of its input per stream (zero after a reset) in the handle's state buffer
 * [stream][layer][frame][64 channels]; a frame's result does not depend on how the utterance is cut into pushes, bit for bit.
 * No EMA update.  The codebook indices are crk_vq_forward's on the same rows.
 *
 * crk_stream_create reads the conv tables of the model's existing stack handles (crk_net_conv_info); offsets in the
 * descriptor are element offsets into the model's flat fp32 parameter block.  CRK_ERR_UNSUPPORTED: not causal, n_stacks
 * outside 1..3, emb_dim not 16/32/64/128, more than 128 channels anywhere (inputs, outputs, conditioning, sum of emb_dim),
 * kernel size above 5, (k - 1) * dilation above 64.
 * crk_stream_reserve is the only call that allocates (weight table, state, layer tables; it synchronises): S streams, pushes
 * of at most C_max frames (any C_max >= 1; the kernel walks a push in tiles of 64 frames).  Asking for more streams than
 * before replaces the state by a zeroed one.  crk_stream_state_bytes: the size of the state of S streams.
 * crk_stream_prepare: effective weights g * v / ||v|| of every conv for the parameters at `params`, once per parameter
 * version; `params` (biases, codebooks, the speaker table are read from it by every push) must stay valid.
 * crk_stream_reset: zeroes the state of the n streams listed in the HOST array stream_ids (NULL: every stream).
 * crk_stream_push: x [S][C][in_ch] (row stride ldx), dec_cond [S][C][2] = (lcf0, uv) when decoder_f0 (row stride ldd),
 * enc_cond likewise when encoder_f0, spk [S] int64, n_valid [S] int32 in 0..C (NULL: C for every stream) on the device.
 * Frames past n_valid[s] are neither computed into the state nor written; a stream with 0 is left as it was.  Outputs,
 * contiguous: decoded [S][C][out_ch], qidx[n] [S][C] int64 and encoded[n] [S][C][emb_dim[n]] (the quantizer's input x_n) for
 * n = 0 .. n_stacks-1, bottom stack first; qidx / encoded are HOST arrays of device pointers.  Never allocates, never
 * synchronises, one launch: capturable.  CRK_ERR_UNSUPPORTED without a launch for S or C beyond what was reserved. */
typedef struct crk_stream_desc {
  int n_stacks, in_ch, out_ch;
  int emb_dim[3], emb_size[3];
  long long cb_off[3], enc_base[3], dec_base[3];
  int causal, enc_f0, dec_f0;   /* encoder_f0 / decoder_f0: two conditioning columns (lcf0, uv) */
  int spk_dim, spk_onehot, n_spk; /* speaker columns of the last decoder's conditioning; one-hot: spk_dim == n_spk */
  long long spk_off;            /* the embedding table [n_spk][spk_dim] (not read when spk_onehot) */
} crk_stream_desc;
int crk_stream_create(const crk_stream_desc* desc, void* const* enc_nets, void* const* dec_nets, void** handle);
void crk_stream_destroy(void* st);
int crk_stream_reserve(void* st, int S, int C_max);
long long crk_stream_state_bytes(void* st, int S);
int crk_stream_prepare(void* st, const float* params, unsigned long long version, void* stream);
int crk_stream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_stream_push(void* st, const float* x, int ldx, const float* dec_cond, int ldd, const float* enc_cond, int lde,
                    const long long* spk, const int* n_valid, int S, int C, float* decoded, long long* const* qidx,
                    float* const* encoded, void* stream);

/* ---- look-ahead streaming conversion for non-causal generators (csrc/stream_la_kernels.hip) ----
 * The same forward for a generator built without use_causal_conv, followed LA = crk_lstream_lookahead frames behind its
 * input: the sum over every residual layer of the chain of (k - 1) / 2 * dilation.  After T frames of an utterance
 * max(0, T - LA) of its frames have been emitted; a push with the end flag runs LA more steps on zero input, emits the rest
 * and starts the stream over.  The emitted rows are the offline forward of the whole utterance and do not depend on how it
 * is cut into pushes, bit for bit.  One launch per push, one workgroup per stream; the cost of a push is that of
 * n_valid (+ LA under the end flag) steps of the causal kernel plus ring traffic.
 *
 * crk_lstream_create takes crk_stream_desc with causal = 0 and the stack handles as crk_stream_create does.
 * CRK_ERR_UNSUPPORTED: causal != 0, what crk_stream_create refuses, an even kernel size.  The state per stream is each
 * layer's last (k - 1) * dilation input rows, a frame counter, and rings [ring][frame mod capacity][row] for what waits
 * for a delayed layer per frame: conditioning rows with the speaker of the push that delivered the frame, each stack's
 * partially summed skip rows, enc[n] until dec[n + 1] arrives, quantized rows of the upper stacks, encoded / qidx until the
 * decoded row exists.  crk_lstream_state_bytes counts all of it.
 * crk_lstream_reserve / prepare / reset: as crk_stream_*; a reset stream's next frame is frame 0 of an utterance.
 * crk_lstream_push: inputs as crk_stream_push, plus end [S] int32 on the device (NULL: no stream ends), non-zero where
 * this push carries the utterance's last frames (n_valid may be 0).  Outputs have rows_out >= C + LA rows per stream:
 * decoded [S][rows_out][out_ch], qidx[n] [S][rows_out] int64, encoded[n] [S][rows_out][emb_dim[n]]; row j is frame
 * first[s] + j of the stream's utterance, rows at and past n_out[s] are not written; n_out, first [S] int32 on the device.
 * The speaker of a frame is spk[s] of the push that delivered it.  Never allocates, never synchronises, reads nothing
 * back, one launch: capturable.  CRK_ERR_UNSUPPORTED without a launch for S or C beyond what was reserved. */
int crk_lstream_create(const crk_stream_desc* desc, void* const* enc_nets, void* const* dec_nets, void** handle);
void crk_lstream_destroy(void* st);
int crk_lstream_lookahead(void* st);
int crk_lstream_reserve(void* st, int S, int C_max);
long long crk_lstream_state_bytes(void* st, int S);
int crk_lstream_prepare(void* st, const float* params, unsigned long long version, void* stream);
int crk_lstream_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_lstream_push(void* st, const float* x, int ldx, const float* dec_cond, int ldd, const float* enc_cond, int lde,
                     const long long* spk, const int* n_valid, const int* end, int S, int C, int rows_out, float* decoded,
                     long long* const* qidx, float* const* encoded, int* n_out, int* first, void* stream);

/* ---- Frame join and the live loop's back-half affine (join_kernels.hip) -----------------------
 * crk_join_*: a two-input row join for up to n_streams streams.  Input A has rows of width_a floats, input B rows of
 * width_b floats (the live loop: log-mel frames and [lcf0, uv]); row k of A and row k of B of an utterance leave together
 * as pair k.  Per stream the handle keeps a ring of at most cap_a waiting A rows, one of at most cap_b waiting B rows
 * (either may be 0), the waiting counts and `first`, the pairs emitted so far in this utterance.
 * crk_join_create is the one call that allocates (it synchronises).  max_in_a / max_in_b: the most rows a push brings
 * per side.  CRK_ERR_ARG: a null handle, n_streams, a width or a max_in below 1, a negative capacity; CRK_ERR_UNSUPPORTED:
 * more than 65535 streams, or a side above 2^20 rows or floats per row.  crk_join_state_bytes: the size of the allocation.
 * crk_join_max_frames: min(cap_a + max_in_a, cap_b + max_in_b), the most pairs one push can emit.
 * crk_join_reset: the streams listed in the HOST array stream_ids (NULL: every stream) drop what waits, start at pair 0
 * and clear their overflow flags.
 * crk_join_push: a fp32 [S][max_in_a] rows with row stride lda, n_a DEVICE int32 [S] (clamped to 0 .. max_in_a): rows
 * [0, n_a[s]) of stream s are new; b, ldb, n_b likewise; end DEVICE int32 [S] or NULL.  With a0, b0 the waiting counts,
 * take = min(a0 + n_a, b0 + n_b) pairs leave: row j of out_a [S][C_out] rows (row stride ldoa) and of out_b (ldob) is
 * pair first + j - waiting rows first, oldest first, then new ones; rows at and past take are not written.  The longer
 * side's surplus waits in its ring; what does not fit is not kept (the newest rows go) and sets the stream's sticky
 * overflow flag (bit 0: ring A, bit 1: ring B).  With end[s] != 0 the surplus is discarded instead, its count goes to
 * n_dropped[s] (0 otherwise) and the stream starts over at pair 0 with empty rings; that is no error.  n_out (= take),
 * first_out (`first` before the push) and n_dropped, DEVICE int32 [S], are written for every stream.  Judged before any
 * launch, outputs and state untouched: CRK_ERR_ARG for a null pointer (end excepted), S < 1, a row stride below its
 * width, C_out < crk_join_max_frames; CRK_ERR_UNSUPPORTED for S > n_streams or a stream's block (max_in or C_out rows
 * times the row stride) above INT_MAX floats.  Two launches whose grids depend on the
 * handle and S alone; never allocates, never synchronises: capturable.
 * crk_join_status synchronises and copies the overflow flags of all n_streams streams to the HOST array flags.
 *
 * crk_feat_renorm: out[s][j][c] = ((x[s][j][c] * scale[c] + mean[c]) - vmean[c]) / vscale[c] for j < n_valid[s] (DEVICE
 * int32 [S], clamped to 0 .. C), x and out [S][C] rows of `width` floats with row strides ldx / ldo; four separately
 * rounded fp32 operations, nothing contracted.  Rows at and past n_valid are not written.  One launch, capturable.
 * Nothing launched: CRK_ERR_ARG for a null pointer, S, C or width below 1, a stride below width; CRK_ERR_UNSUPPORTED for
 * S > 65535 or C rows times the width or a stride above INT_MAX floats. */
int crk_join_create(int n_streams, int width_a, int width_b, int max_in_a, int max_in_b, int cap_a, int cap_b, void** handle);
void crk_join_destroy(void* st);
long long crk_join_state_bytes(void* st);
int crk_join_max_frames(void* st);
int crk_join_reset(void* st, const int* stream_ids, int n, void* stream);
int crk_join_push(void* st, const float* a, int lda, const int* n_a, const float* b, int ldb, const int* n_b, const int* end,
                  int S, float* out_a, int ldoa, float* out_b, int ldob, int C_out, int* n_out, int* first_out,
                  int* n_dropped, void* stream);
int crk_join_status(void* st, int* flags, void* stream);
int crk_feat_renorm(const float* x, int ldx, const float* scale, const float* mean, const float* vmean, const float* vscale,
                    const int* n_valid, int S, int C, int width, float* out, int ldo, void* stream);

/* number of device allocations net handles have made since the library was loaded (tests pin "none inside the step") */
long long crk_debug_alloc_count(void);

/* which kernel generation crk_net_forward / crk_net_backward pick for batch shape (B, T): bit 0 a generator stack (kind 0) runs
 * the channel-split kernels in plain bf16, bit 1 its CRK_FLAG_PRECISE | CRK_FLAG_BWD_PLAIN forward runs the channel-split
 * split-operand kernel, bit 2 a discriminator (kind 1) runs channel-split, bit 3 a chain of plain convs (kind 2) runs fused.
 * The fallbacks compute the same values more slowly, as far as tests/test_gpu_per_layer.py and tests/test_gpu_fallback.py
 * compare them ("What reaches the per-layer kernels"); tests pin the bits at the benchmark shape. */
int crk_debug_net_paths(void* net, int B, int T);
/* The layout of reserved batch shape (B, T): out[0..7] = weight-gradient groups and 64-frame chunks per group of the gated
 * blocks' region (Gs, cpg_s), groups and chunks per group of the generic region (Gg, cpg), per-utterance sum segments per
 * group (nseg), the 64-frame tiles per window the channel-split data-gradient chain was planned with (ft), the window rows
 * of the plain-bf16 channel-split forward, 0.  A value that does not apply to the net or its route is 0.  Tests assert the
 * layout a case is named after before they compare values.  CRK_ERR_ARG: the shape is not reserved. */
int crk_debug_net_layout(void* net, int B, int T, int* out);
/* The weight-gradient partial sums (per group, before the weight-norm backward reduces them) the last backward of shape
 * (B, T) left in the handle: returns their count and copies the first min(count, cap) floats to `out` (device memory);
 * -1: the shape is not reserved.  Tests compare one launch over several nets with the single-net launches on them. */
long long crk_debug_net_partials(void* net, int B, int T, float* out, long long cap, void* stream);

const char* crk_version(void);

#ifdef __cplusplus
}
#endif
#endif
