// Host-side orchestration of the convolutional networks of the step, exposed through
// the C ABI declared in include/crank_hip.h.
//
// A "net" is one of the three third-party stacks crank instantiates (SURVEY.md
// Appendix A; call sites crank/net/module/vqvae2.py:237-273, spkradv.py:49-60,
// crank/bin/train.py:78-128):
//   kind 0  gated-residual generator  (ParallelWaveGANGenerator, ReLU head, optional aux)
//   kind 1  gated-residual discriminator (ResidualParallelWaveGANDiscriminator, LeakyReLU)
//   kind 2  plain dilated conv stack + LeakyReLU (ParallelWaveGANDiscriminator)
// All parameters of a net live in one flat fp32 block (weight_g / weight_v / bias per
// conv); the handle owns the weight-normalised bf16 operand planes, the per-utterance
// weight-gradient partials and the backward scratch.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <vector>

#include "conv_kernels.h"

#include "../../include/crank_hip.h"

enum { ROLE_FIRST = 0, ROLE_CONV = 1, ROLE_AUX = 2, ROLE_OUT = 3, ROLE_SKIP = 4, ROLE_LAST1 = 5, ROLE_LAST2 = 6, ROLE_PLAIN = 7 };

struct ConvMeta {
  int role, layer, dilation;
};

// The compute entry points (crk_net_forward / _backward*) never allocate: every device buffer and table a batch shape needs is
// made by crk_net_reserve(net, B, T), outside the step ("takes raw device pointers, sizes and a stream;
// never allocates").  g_may_alloc is true only inside crk_net_create / crk_net_reserve; an allocation site reached with it
// false returns CRK_ERR_ARG (the shape was not reserved).  g_net_allocs counts the allocations (crk_debug_alloc_count).
static bool g_may_alloc = false;
static long long g_net_allocs = 0;
static hipError_t net_malloc_(void** p, size_t bytes) {
  if (!g_may_alloc) return hipErrorInvalidValue;
  g_net_allocs++;
  return hipMalloc(p, bytes);
}
#define NET_MALLOC(pp, bytes) net_malloc_(reinterpret_cast<void**>(pp), (bytes))
struct AllocScope {
  bool was;
  AllocScope() : was(g_may_alloc) { g_may_alloc = true; }
  ~AllocScope() { g_may_alloc = was; }
};
static int not_reserved(const char* what) {
  fprintf(stderr, "[crank_hip] %s: this batch shape needs device buffers / tables the handle does not hold - call "
                  "crk_net_reserve(net, B, T) once per batch shape, outside the step (the compute entry points never allocate)\n", what);
  return CRK_ERR_ARG;
}

#define PS_MAXL 16
// host copies of the fused plain-conv chain tables (pstack_kernels.hip, pstack_wgrad_kernels.hip): [0] first/forward, [1] head forward / backward,
// [2] head backward, [3] first backward; w: the weight-gradient table
struct PsTables { PsLayer t[4][PS_MAXL]; int L[4]; PwLayer w[PS_MAXL]; int nw; int max_wa, max_wb, max_tiles; double wflops_per_frame; };
// what a batch shape needs: scratch / partial-sum floats, the slot counts of the two weight-gradient regions, the 64-frame
// chunks per group of the plain convs (cpg) and of the gated blocks (cpg_s), the latter's per-utterance segments per group
struct ShapeNeed { long long need_s, need_p; int Gs, Gg, cpg, cpg_s, nseg; };
// The kernels a net runs at a batch shape in one arithmetic (route_of).  It depends on the net, the shape, the arithmetic and
// the process-wide switches only, never on a call's pointers, so a backward always reads the plane layout its forward wrote.
// Every other path computes the same values, only slower (tests/test_gpu_per_layer.py, tests/test_gpu_fallback.py).
struct Route {
  bool fused;       // forward, data-gradient chain and weight gradient on the fused kernels (else one kernel per layer)
  bool gen_split;   // generator, plain bf16: forward and chain channel-split, gate planes in the lane-record layout
  bool x3f;         // generator: a bf16x3f forward ahead of this (plain) route's backward runs channel-split too
  bool disc_split;  // discriminator, plain bf16: blocks and chain channel-split, gate planes in the lane-record layout
  bool usums;       // gated stack with conditioning, fused: an embedding behind the conditioning gets its gradient from the
                    // weight-gradient launch's per-utterance dG sums (crk_net_backward_embed), the chain computes no dc
  unsigned char ps_fwd;      // fused plain chain: the forward's kernel (CHAIN_*)
  unsigned char ps_fwd_x3f;  // ... of a bf16x3f forward, in the split-operand route: pstack2x_kernel, or pstack_kernel<PRECISE>
  unsigned char ps_bwd[2];   // ... of the data-gradient chain: [0] down to dx, [1] stopped one layer early (PsP::tail, no dx)
  bool fold_fwd;     // generator, plain bf16: first conv, blocks and head in one stack2_fwd_kernel launch (with gen_split, or on
                     // row-layout planes where only the chain cannot split)
  bool blocks_s2;    // fused gated stack, plain bf16, not folded: the blocks run stack2_fwd_kernel (else stack_fwd_kernel)
  bool fold_bwd_fs;  // generator, plain bf16: the frame-split chain folds head and first conv in (its 8-wave window only)
};
enum { CHAIN_PS = 0, CHAIN_PS2 = 1, CHAIN_PS2X = 2 };  // pstack_kernel, pstack2_kernel, pstack2x_kernel
// Everything batch shape (B, T) needs besides the growing buffers, made by crk_net_reserve: plane offsets are multiples of
// N = B*T, partial-sum offsets of the slot counts Gs / Gg.
struct Shape {
  int B, T;
  ShapeNeed q;
  Route route[2];                    // [precise]
  bool pair_fused;                   // a bf16x3f forward / backward pair runs the fused kernels (routes_pair_fused)
  std::vector<ConvEntry> abs;        // the conv entries with absolute partial offsets and slot counts ...
  ConvEntry* d_ents = nullptr;       // ... on the device
  PsTables ps;                       // fused plain-conv chain tables (nets of at most PS_MAXL layers) ...
  PsLayer* d_ps = nullptr;           // ... on the device: [4][PS_MAXL]
  PwLayer* d_pw = nullptr;           // [PS_MAXL]
  StackWLayer* d_wlayers = nullptr;  // gated nets: fused weight-gradient layer table
};

struct Net {
  crk_net_desc d;
  std::vector<ConvEntry> ents;
  std::vector<ConvMeta> meta;
  ConvEntry* d_ents = nullptr;  // the table weight preparation reads (it reads no partial-sum offsets)
  long long n_params = 0;
  long long wprep_elems = 0, norm_elems = 0;
  uint16_t *whi = nullptr, *wlo = nullptr;
  float* norms = nullptr;
  unsigned long long prepared_version = ~0ull;
  const float* prepared_params = nullptr;
  // weight-norm backward deferred by CRK_FLAG_DEFER_WNORM (wn_shape: pending, for that shape): the per-group partial sums
  // wait in `partials`
  const Shape* wn_shape = nullptr; const float* wn_params = nullptr; float* wn_grads = nullptr;
  // ... and, with it, the weight gradients of the plain convs around a gated stack (first conv, head): their planes stay in
  // `scratch` / the caller's `saved` until the group call
  const Shape* pw_shape = nullptr; PwP pw_params;
  // grown by crk_net_reserve
  float* partials = nullptr; long long partial_cap = 0;
  float* scratch = nullptr; long long scratch_cap = 0;
  // weight-gradient partial sums: two regions with their own slot counts - the gated blocks'
  // convs (utterance groups, stack_wgrad_kernel) and everything else (chunk groups, table kernel)
  long long pt_floats_stack = 0, pt_floats_gen = 0;
  int L = 0;
  int idx_first = -1, idx_last1 = -1, idx_last2 = -1;
  std::vector<int> idx_conv, idx_aux, idx_out, idx_skip, idx_plain;
  StackLayer* d_layers = nullptr;  // fused-forward layer table (kinds 0/1)
  StackBLayer* d_blayers = nullptr;  // fused data-gradient layer table
  // One record per reserved batch shape, looked up once per compute call.  Records live as long as the net, so a captured HIP
  // graph - which holds the pointers of the shape it was captured with - keeps seeing that shape's tables whatever ran in
  // between (a short last batch of an epoch, a dev batch).  Buffers that grow are retired, not freed, for the same reason.
  // Growth is bounded by the number of DISTINCT (B, T) a run feeds a net: training has one (batch_len is fixed, dataset.py
  // crops / pads to it), decoding one per flag (batch_len = longest utterance); a record is a few KB, so nothing is evicted.
  std::deque<Shape> shapes;  // (a deque: deferred work points at its record)
  std::vector<void*> retired;  // outgrown partial-sum / scratch buffers (freed with the net)
  // How each recent forward laid out the planes in the caller's `saved` workspace (keyed by its address; the last 32 calls):
  // mode 0 plain bf16, 1 split operands with hi + lo planes (CRK_FLAG_PRECISE), 2 split-operand forward that saved what a
  // PLAIN backward reads (CRK_FLAG_PRECISE | CRK_FLAG_BWD_PLAIN); x3f: the channel-split split-operand forward wrote them.
  // crk_net_backward checks its flags against the tag instead of trusting the caller to pair the two calls.
  // fused: the fused kernels wrote them (bf16 planes), not the per-layer ones (fp32 planes only).
  struct FwdTag { const float* saved; int B, T; unsigned char mode; bool x3f, fused; };
  FwdTag fwd_tags[32]; int fwd_tag_next = 0; int fwd_tag_count = 0;
  std::vector<WgradP> jobs;  // weight-gradient problems queued by the running backward
  WgradP* d_jobs = nullptr;
  // pinned upload ring for the job table (a slot is reused only after its copy completed)
  WgradP* h_slot[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t slot_ev[4];
  int slot_next = 0;
};

static int pad16(int c) { return round_up(c, 16); }
static int pad32(int c) { return round_up(c, 32); }

static void add_conv(Net* n, int role, int layer, int cout, int cin, int k, int dil, bool bias) {
  ConvEntry e;
  memset(&e, 0, sizeof(e));
  e.cout = cout; e.cin = cin; e.k = k;
  if (bias) { e.off_b = n->n_params; n->n_params += cout; } else e.off_b = -1;
  e.off_g = n->n_params; n->n_params += cout;
  e.off_v = n->n_params; n->n_params += (long long)cout * cin * k;
  e.norm_off = n->norm_elems; n->norm_elems += cout;
  e.bw_off = -1; e.fr_off = -1; e.fr_mode = 0; e.bfr_off = -1; e.bfr_mode = 0;
  n->ents.push_back(e);
  n->meta.push_back({role, layer, dil});
}

static long long alloc_w(Net* n, long long elems) {
  long long o = n->wprep_elems;
  n->wprep_elems += (elems + 7) & ~7ll;  // keep 16-byte alignment of every plane
  return o;
}
static long long alloc_pt(Net* n, long long floats_per_group, bool stack) {
  long long& tot = stack ? n->pt_floats_stack : n->pt_floats_gen;
  const long long o = tot;
  tot += floats_per_group;
  return o;
}

// a host table copied into a new device allocation (*d is set as soon as it is allocated: the caller frees it on failure)
template <class E> static int upload(E** d, const E* h, size_t count) {
  if (NET_MALLOC(d, sizeof(E) * count) != hipSuccess) return CRK_ERR_HIP;
  return hipMemcpy(*d, h, sizeof(E) * count, hipMemcpyHostToDevice) == hipSuccess ? CRK_OK : CRK_ERR_HIP;
}
extern "C" void* crk_net_create(const crk_net_desc* desc) {
  AllocScope may_allocate;
  if (!desc) return nullptr;
  if (conv_kernels_init() != CRK_OK) return nullptr;
  Net* n = new Net();
  n->d = *desc;
  const crk_net_desc& d = n->d;
  if (d.kind == 0 || d.kind == 1) {
    if (d.res_ch != 64 || d.gate_ch != 128 || d.skip_ch != 64 || d.layers % d.stacks != 0 ||
        (d.kernel_size % 2 == 0 && !d.causal) || d.in_ch > 128 || d.out_ch > 128 || d.aux_ch > 128) {
      fprintf(stderr, "[crank_hip] net_create: unsupported gated-residual configuration\n");
      delete n;
      return nullptr;
    }
    n->L = d.layers;
    const int lps = d.layers / d.stacks;
    n->idx_first = (int)n->ents.size();
    add_conv(n, ROLE_FIRST, -1, 64, d.in_ch, 1, 1, true);
    for (int l = 0; l < d.layers; l++) {
      const int dil = 1 << (l % lps);
      n->idx_conv.push_back((int)n->ents.size());
      add_conv(n, ROLE_CONV, l, 128, 64, d.kernel_size, dil, d.use_bias);
      if (d.aux_ch > 0) {
        n->idx_aux.push_back((int)n->ents.size());
        add_conv(n, ROLE_AUX, l, 128, d.aux_ch, 1, 1, false);
      }
      n->idx_out.push_back((int)n->ents.size());
      add_conv(n, ROLE_OUT, l, 64, 64, 1, 1, d.use_bias);
      n->idx_skip.push_back((int)n->ents.size());
      add_conv(n, ROLE_SKIP, l, 64, 64, 1, 1, d.use_bias);
    }
    n->idx_last1 = (int)n->ents.size();
    add_conv(n, ROLE_LAST1, -1, 64, 64, 1, 1, true);
    n->idx_last2 = (int)n->ents.size();
    add_conv(n, ROLE_LAST2, -1, d.out_ch, 64, 1, 1, true);
  } else if (d.kind == 2) {
    if (d.kernel_size % 2 == 0 || d.conv_ch > 128 || d.in_ch > 128 || d.out_ch > 128 || d.layers < 1) {
      delete n;
      return nullptr;
    }
    n->L = d.layers;
    int cin = d.in_ch;
    for (int i = 0; i < d.layers - 1; i++) {
      const int dil = (i == 0) ? 1 : i;  // dilation_factor == 1
      n->idx_plain.push_back((int)n->ents.size());
      add_conv(n, ROLE_PLAIN, i, d.conv_ch, cin, d.kernel_size, dil, d.use_bias);
      cin = d.conv_ch;
    }
    n->idx_plain.push_back((int)n->ents.size());
    add_conv(n, ROLE_PLAIN, d.layers - 1, d.out_ch, cin, d.kernel_size, 1, d.use_bias);
  } else {
    delete n;
    return nullptr;
  }
  // ---- operand-plane and partial layouts ----
  for (size_t i = 0; i < n->ents.size(); i++) {
    ConvEntry& e = n->ents[i];
    const ConvMeta& m = n->meta[i];
    e.pt_scale = 1.f;
    switch (m.role) {
      case ROLE_OUT: {
        // combined [out|skip] planes are laid out when the OUT entry is visited
        ConvEntry& sk = n->ents[i + 1];
        e.fw_rows = sk.fw_rows = 128; e.fw_kp = sk.fw_kp = 64;
        e.fw_off = sk.fw_off = alloc_w(n, 128 * 64);
        e.fw_row0 = 0; sk.fw_row0 = 64;
        e.bw_rows = sk.bw_rows = 64; e.bw_kp = sk.bw_kp = 128;
        e.bw_off = sk.bw_off = alloc_w(n, 64 * 128);
        e.bw_col0 = 0; sk.bw_col0 = 64;
        e.pt_rows = sk.pt_rows = 128; e.pt_cx = sk.pt_cx = 64; e.pt_taps = sk.pt_taps = 1;
        e.pt_groups = sk.pt_groups = 1;
        e.pt_off = sk.pt_off = alloc_pt(n, 128 * 64, true);
        e.pb_off = sk.pb_off = alloc_pt(n, 128, true);
        e.pt_row0 = 0; sk.pt_row0 = 64;
        e.pt_scale = 0.70710678118654752440f; sk.pt_scale = 1.f;
        e.fr_off = sk.fr_off = alloc_w(n, 4 * 4 * 64 * 8); e.fr_mode = 3; sk.fr_mode = 4;
        e.bfr_off = sk.bfr_off = alloc_w(n, 64 * 128);
        break;
      }
      case ROLE_SKIP:
        break;  // filled with its OUT sibling
      default: {
        e.fw_rows = pad32(e.cout); e.fw_kp = pad16(e.cin); e.fw_row0 = 0;
        // the conditioning 1x1 of a gated block is consumed by the fused forward kernel as one more
        // 128 x 64 weight chunk (zero columns beyond aux_ch), exactly like a tap
        if (m.role == ROLE_AUX && e.cin <= 64) e.fw_kp = 64;
        e.fw_off = alloc_w(n, (long long)e.k * e.fw_rows * e.fw_kp);
        e.bw_rows = pad32(e.cin); e.bw_kp = pad16(e.cout); e.bw_col0 = 0;
        e.bw_off = alloc_w(n, (long long)e.k * e.bw_rows * e.bw_kp);
        e.pt_rows = e.cout; e.pt_row0 = 0; e.pt_cx = e.cin; e.pt_taps = e.k;
        e.pt_groups = (m.role == ROLE_CONV || m.role == ROLE_AUX) ? 1 : 0;
        e.pt_off = alloc_pt(n, (long long)e.k * e.cout * e.cin, e.pt_groups != 0);
        e.pb_off = alloc_pt(n, e.cout, e.pt_groups != 0);
        if (m.role == ROLE_CONV && e.cin == 64 && e.cout == 128) { e.fr_off = alloc_w(n, (long long)e.k * 4 * 4 * 64 * 8); e.fr_mode = 1; }
        if (m.role == ROLE_AUX && e.cin <= 64 && e.cout == 128) { e.fr_off = alloc_w(n, 4 * 4 * 64 * 8); e.fr_mode = 2; }
        if ((m.role == ROLE_FIRST || m.role == ROLE_LAST1 || m.role == ROLE_LAST2) && e.k == 1) {
          e.fr_off = alloc_w(n, (long long)(e.fw_rows >> 5) * (e.fw_kp >> 4) * 64 * 8); e.fr_mode = 5;
        }
        if (d.kind == 0 && (m.role == ROLE_CONV || m.role == ROLE_AUX || m.role == ROLE_FIRST || m.role == ROLE_LAST1 ||
                            m.role == ROLE_LAST2))
          e.bfr_off = alloc_w(n, (long long)e.k * e.bw_rows * e.bw_kp);
        // the discriminator's data-gradient chain runs channel-split too (round 4): its transposed tap weights in A-fragment order
        if (d.kind == 1 && m.role == ROLE_CONV && e.cin == 64 && e.cout == 128) e.bfr_off = alloc_w(n, (long long)e.k * e.bw_rows * e.bw_kp);
        if (m.role == ROLE_PLAIN) {  // kind-2 chains: both layouts in fragment order, a tile's fragments in one run
          e.fr_off = alloc_w(n, (long long)e.k * e.fw_rows * e.fw_kp); e.fr_mode = 6;
          e.bfr_off = alloc_w(n, (long long)e.k * e.bw_rows * e.bw_kp); e.bfr_mode = 1;
        }
        break;
      }
    }
  }
  bool ok = true;
  ok = ok && NET_MALLOC(&n->whi, sizeof(uint16_t) * n->wprep_elems) == hipSuccess;
  ok = ok && NET_MALLOC(&n->wlo, sizeof(uint16_t) * n->wprep_elems) == hipSuccess;
  ok = ok && NET_MALLOC(&n->norms, sizeof(float) * n->norm_elems) == hipSuccess;
  ok = ok && hipMemset(n->whi, 0, sizeof(uint16_t) * n->wprep_elems) == hipSuccess;
  ok = ok && hipMemset(n->wlo, 0, sizeof(uint16_t) * n->wprep_elems) == hipSuccess;
  if (ok && (d.kind == 0 || d.kind == 1)) {
    std::vector<StackLayer> lt(n->L);
    for (int l = 0; l < n->L; l++) {
      const ConvEntry& ec = n->ents[n->idx_conv[l]];
      const ConvEntry& eo = n->ents[n->idx_out[l]];
      const ConvEntry& es = n->ents[n->idx_skip[l]];
      StackLayer& y = lt[l];
      y.w_conv = ec.fw_off; y.w_os = eo.fw_off;
      y.w_aux = d.aux_ch > 0 ? n->ents[n->idx_aux[l]].fw_off : 0;
      y.f_conv = ec.fr_off; y.f_os = eo.fr_off;
      y.f_aux = d.aux_ch > 0 ? n->ents[n->idx_aux[l]].fr_off : -1;
      y.b_conv = ec.off_b; y.b_out = eo.off_b; y.b_skip = es.off_b;
      y.dil = n->meta[n->idx_conv[l]].dilation;
      y.off0 = d.causal ? -(ec.k - 1) * y.dil : -((ec.k - 1) / 2) * y.dil;
    }
    ok = upload(&n->d_layers, lt.data(), n->L) == CRK_OK;
    std::vector<StackBLayer> bt(n->L);
    for (int l = 0; l < n->L; l++) {
      const ConvEntry& ec = n->ents[n->idx_conv[l]];
      const ConvEntry& eo = n->ents[n->idx_out[l]];
      StackBLayer& y = bt[l];
      y.w_conv = ec.bw_off; y.w_os = eo.bw_off;
      y.w_aux = d.aux_ch > 0 ? n->ents[n->idx_aux[l]].bw_off : 0;
      y.dil = n->meta[n->idx_conv[l]].dilation;
      const int off0 = d.causal ? -(ec.k - 1) * y.dil : -((ec.k - 1) / 2) * y.dil;
      y.off0 = -off0 - (ec.k - 1) * y.dil;
      y.f_conv = ec.bfr_off; y.f_os = eo.bfr_off;
      y.f_aux = d.aux_ch > 0 ? n->ents[n->idx_aux[l]].bfr_off : -1;
    }
    ok = ok && upload(&n->d_blayers, bt.data(), n->L) == CRK_OK;
  }
  ok = ok && upload(&n->d_ents, n->ents.data(), n->ents.size()) == CRK_OK;  // (batch shapes get their own in crk_net_reserve)
  if (!ok) {
    fprintf(stderr, "[crank_hip] net_create: device allocation failed\n");
    delete n;
    return nullptr;
  }
  return n;
}

static void free_shape(Shape& r) {
  (void)hipFree(r.d_ents); (void)hipFree(r.d_ps); (void)hipFree(r.d_pw); (void)hipFree(r.d_wlayers);
}
extern "C" void crk_net_destroy(void* h) {
  Net* n = (Net*)h;
  if (!n) return;
  for (Shape& r : n->shapes) free_shape(r);
  for (void* q : n->retired) (void)hipFree(q);
  (void)hipFree(n->whi); (void)hipFree(n->wlo); (void)hipFree(n->norms); (void)hipFree(n->d_ents);
  for (int k = 0; k < 4; k++) if (n->h_slot[k]) { (void)hipHostFree(n->h_slot[k]); (void)hipEventDestroy(n->slot_ev[k]); }
  (void)hipFree(n->partials); (void)hipFree(n->scratch); (void)hipFree(n->d_jobs); (void)hipFree(n->d_layers); (void)hipFree(n->d_blayers);
  delete n;
}

extern "C" long long crk_net_param_count(void* h) { return ((Net*)h)->n_params; }
extern "C" int crk_net_conv_count(void* h) { return (int)((Net*)h)->ents.size(); }
// out[0..8] = cout, cin, k, off_bias, off_g, off_v, dilation, role, layer
extern "C" int crk_net_conv_info(void* h, int i, long long* out) {
  Net* n = (Net*)h;
  if (i < 0 || i >= (int)n->ents.size()) return CRK_ERR_ARG;
  const ConvEntry& e = n->ents[i];
  out[0] = e.cout; out[1] = e.cin; out[2] = e.k; out[3] = e.off_b; out[4] = e.off_g; out[5] = e.off_v;
  out[6] = n->meta[i].dilation; out[7] = n->meta[i].role; out[8] = n->meta[i].layer;
  return CRK_OK;
}

static int stack_aux_pad(const Net* n) { return n->d.aux_ch > 0 ? n->ents[n->idx_aux[0]].fw_kp : 16; }
// ---- workspace layouts -------------------------------------------------------------------
// `saved` (caller-owned, forward -> backward):
//   kind 2: [fp32 pre-activations H_0..H_{L-2} (per-layer fallback only)] then bf16 operand planes
//           O_i [N, kp_i] of every conv, hi block then lo block
//   gated : fp32 planes X | TA | SB | Z | SKIP | H1 (TA, SB, Z, H1: per-layer fallback only), then bf16:
//           Xb Zb Tb Sg (block input, z, tanh, sigmoid; hi[L] lo[L], [N,64] each), Cb_hi Cb_lo ([N,aux_pad]), F_hi F_lo (first-conv input [N,kpF]),
//           head_hi = S|H1 ([N,64] each), head_lo
struct GatedF32 {  // float offsets of the gated stacks' fp32 planes: [N,64] each, block l's at + l * N * 64
  long long x, ta, sb, z, skip, h1, saved_total;  // in `saved`
  long long ds, dh1, dx, dg, scratch_total;       // in n->scratch: dX_l, l = 0..L (dX_L is never written: it is zero), then
};                                                // dG_l [N,128] at dg + l * 2 * N * 64
static GatedF32 gated_f32(const Net* n, long long N) {
  const long long P = N * 64, LP = n->L * P;
  return {0, LP, 2 * LP, 3 * LP, 4 * LP, 4 * LP + P, 4 * LP + 2 * P, 0, P, 2 * P, 3 * P + LP, 3 * P + 3 * LP};
}
static long long saved_f32_floats(const Net* n, long long N) {
  return n->d.kind == 2 ? (long long)(n->L - 1) * N * n->d.conv_ch : gated_f32(n, N).saved_total;
}
static long long plain_planes_w(const Net* n) {  // sum of the operand-plane widths of a kind-2 net
  long long w = 0;
  for (int i = 0; i < n->L; i++) w += n->ents[n->idx_plain[i]].fw_kp;
  return w;
}
static long long plain_gplanes_w(const Net* n) {  // ... of its output-gradient planes
  long long w = 0;
  for (int i = 0; i < n->L; i++) w += n->ents[n->idx_plain[i]].bw_kp;
  return w;
}
struct GatedB16 {  // element offsets inside the gated forward bf16 region
  long long xb_hi, xb_lo, zb_hi, zb_lo, tb_hi, tb_lo, sg_hi, sg_lo, cb_hi, cb_lo, f_hi, f_lo, head_hi, head_lo, total;
};
static long long ts_plane_stride(long long N) { return ((N + 31) & ~31ll) * 64; }
static GatedB16 gated_b16(const Net* n, long long N) {
  GatedB16 g;
  const long long P = N * 64, LP = (long long)n->L * P, ca = N * stack_aux_pad(n), kf = N * n->ents[n->idx_first].fw_kp;
  // the tanh / sigmoid planes may be kept in blocks of 32 frames (StackP::ts_stride): room for a last partial block
  const long long LPt = (long long)n->L * ts_plane_stride(N);
  g.xb_hi = 0; g.xb_lo = LP; g.zb_hi = 2 * LP; g.zb_lo = 3 * LP;
  g.tb_hi = 4 * LP; g.tb_lo = g.tb_hi + LPt; g.sg_hi = g.tb_lo + LPt; g.sg_lo = g.sg_hi + LPt;
  g.cb_hi = g.sg_lo + LPt; g.cb_lo = g.cb_hi + ca;
  g.f_hi = g.cb_lo + ca; g.f_lo = g.f_hi + kf;
  g.head_hi = g.f_lo + kf; g.head_lo = g.head_hi + 2 * P;
  g.total = g.head_lo + 2 * P;
  return g;
}
static long long saved_floats(const Net* n, long long N) {
  if (n->d.kind == 2) return saved_f32_floats(n, N) + N * plain_planes_w(n);  // 2 planes (hi, lo) x 2 bytes
  return saved_f32_floats(n, N) + (gated_b16(n, N).total + 1) / 2;
}
extern "C" long long crk_net_saved_bytes(void* h, int B, int T) { return saved_floats((Net*)h, (long long)B * T) * 4; }

static int net_nmax(const Net* n) {  // largest cin * k of the net's convs
  int m = 1;
  for (const auto& e : n->ents) if (e.cin * e.k > m) m = e.cin * e.k;
  return m;
}
static int ensure_prepared(Net* n, const float* params, unsigned long long version, hipStream_t s) {
  if (n->prepared_version == version && n->prepared_params == params) return CRK_OK;
  int rc = launch_weight_prep(n->d_ents, (int)n->ents.size(), net_nmax(n), params, n->whi, n->wlo, n->norms, s);
  if (rc) return rc;
  n->prepared_version = version;
  n->prepared_params = params;
  return CRK_OK;
}

// partial sums -> dg / dv / dbias: now, or (deferred) when the caller finishes all its nets with crk_nets_wnorm_bwd
static int finish_wnorm(Net* n, const Shape* r, const float* params, float* grads, bool defer, hipStream_t s) {
  if (defer) { n->wn_shape = r; n->wn_params = params; n->wn_grads = grads; return CRK_OK; }
  return launch_wnorm_bwd(r->d_ents, (int)n->ents.size(), params, grads, n->partials, n->norms, s);
}
static int flush_pending_plain_wgrad(Net* n, hipStream_t s);
static int flush_pending_wnorm(Net* n, hipStream_t s) {
  if (!n->wn_shape) return CRK_OK;
  { int rc = flush_pending_plain_wgrad(n, s); if (rc) return rc; }
  const Shape* r = n->wn_shape;
  n->wn_shape = nullptr;
  return launch_wnorm_bwd(r->d_ents, (int)n->ents.size(), n->wn_params, n->wn_grads, n->partials, n->norms, s);
}

static ConvP base_conv(const Net* n, int B, int T) {
  ConvP p;
  memset(&p, 0, sizeof(p));
  p.scaleA = p.scaleB = 1.f; p.out_scale = 1.f; p.res_scale = 1.f;
  p.slope = n->d.slope;
  p.B = B; p.T = T; p.tiles_per_utt = ceil_div(T, CRK_TM);
  p.ktaps = 1; p.dil = 1; p.off0 = 0;
  return p;
}
// conv e of the per-layer kernels, in [N, e.cin] -> out; the caller adds taps, prologue and epilogue
static ConvP conv_fw(const Net* n, int B, int T, const ConvEntry& e, const float* params, const float* in, int ldin, float* out, int ldo) {
  ConvP p = base_conv(n, B, T);
  p.w_hi = n->whi + e.fw_off; p.w_lo = n->wlo + e.fw_off;
  p.cin = e.cin; p.cin_pad = e.fw_kp; p.cout = e.cout; p.cout_pad = e.fw_rows;
  p.bias = e.off_b >= 0 ? params + e.off_b : nullptr;
  p.xa = in; p.lda = ldin; p.cinA = e.cin; p.y = out; p.ldy = ldo;
  return p;
}
// ... and its data gradient, in [N, e.cout] -> out: "cin" = forward cout, "cout" = forward cin
static ConvP conv_bw(const Net* n, int B, int T, const ConvEntry& e, const float* in, int ldin, float* out, int ldo) {
  ConvP p = base_conv(n, B, T);
  p.w_hi = n->whi + e.bw_off; p.w_lo = n->wlo + e.bw_off;
  p.cin = e.cout; p.cin_pad = e.bw_kp; p.cout = e.cin; p.cout_pad = e.bw_rows;
  p.xa = in; p.lda = ldin; p.cinA = e.cout; p.y = out; p.ldy = ldo;
  return p;
}
static int fwd_off0(const Net* n, int k, int dil) { return n->d.causal ? -(k - 1) * dil : -((k - 1) / 2) * dil; }

static unsigned long long layer_seed(unsigned long long seed, int l) { return seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(l + 1); }

#define RUN(x) do { int rc_ = (x); if (rc_ != CRK_OK) return rc_; } while (0)

static int conv_go(ConvP& p, int mode, bool precise, hipStream_t s) {
  conv_fill_lds(p, mode, precise);
  return launch_conv(p, mode, precise, s);
}

// flags bit0: precise (bf16x3 split) arithmetic
// ---- fused plain-conv chains (pstack_kernels.hip): layer tables --------------------------------
static PsLayer ps_layer_fwd(const Net* n, int ei, int epi) {
  const ConvEntry& e = n->ents[ei];
  PsLayer y; memset(&y, 0, sizeof(y));
  y.w_off = e.fw_off; y.b_off = e.off_b; y.rows = e.cout; y.rows_pad = e.fw_rows; y.kp = e.fw_kp;
  y.k = e.k; y.dil = n->meta[ei].dilation; y.off0 = -((e.k - 1) / 2) * y.dil; y.epi = epi;
  y.f_off = e.fr_mode == 6 ? e.fr_off : -1;
  return y;
}
static PsLayer ps_layer_bwd(const Net* n, int ei, int epi) {  // the conv transposed: data gradient
  const ConvEntry& e = n->ents[ei];
  PsLayer y; memset(&y, 0, sizeof(y));
  y.w_off = e.bw_off; y.b_off = -1; y.rows = e.cin; y.rows_pad = e.bw_rows; y.kp = e.bw_kp;
  y.k = e.k; y.dil = n->meta[ei].dilation; y.off0 = ((e.k - 1) / 2) * y.dil - (e.k - 1) * y.dil; y.epi = epi;
  y.f_off = e.bfr_mode == 1 ? e.bfr_off : -1;
  return y;
}
static PwLayer pw_layer(const Net* n, const ConvEntry* abs, int ei, long long a_hi, long long a_lo, long long b_hi, long long b_lo) {
  const ConvEntry& e = n->ents[ei];
  const ConvEntry& a = abs[ei];
  PwLayer y; memset(&y, 0, sizeof(y));
  y.a_hi = a_hi; y.a_lo = a_lo; y.b_hi = b_hi; y.b_lo = b_lo;
  y.wa = e.bw_kp; y.wb = e.fw_kp; y.ca = e.cout; y.cb = e.cin;
  y.k = e.k; y.dil = n->meta[ei].dilation; y.off0 = -((e.k - 1) / 2) * y.dil;
  y.pt = a.pt_off; y.pb = e.off_b >= 0 ? a.pb_off : -1;
  return y;
}
static bool pw_ok(const Net* n, int ei) {
  const ConvEntry& e = n->ents[ei];
  return pstack_wgrad_supported(e.cout, e.cin, e.bw_kp, e.fw_kp, e.k, n->meta[ei].dilation) != 0;
}
struct GatedS16 {  // element offsets inside the gated backward bf16 region (n->scratch)
  long long gb_hi, gb_lo, dxb_hi, dxb_lo, dsb_hi, dsb_lo, hb_hi, hb_lo, total;
};
static GatedS16 gated_s16(const Net* n, long long N) {
  GatedS16 g;
  const long long P = N * 64, L = n->L, hb = N * n->ents[n->idx_last2].bw_kp + P;
  g.gb_hi = 0; g.gb_lo = 2 * L * P; g.dxb_hi = 4 * L * P; g.dxb_lo = g.dxb_hi + (L + 1) * P;
  g.dsb_hi = g.dxb_lo + (L + 1) * P; g.dsb_lo = g.dsb_hi + P;
  g.hb_hi = g.dsb_lo + P; g.hb_lo = g.hb_hi + hb; g.total = g.hb_lo + hb;
  return g;
}
// the chain tables of a batch shape; abs: the conv entries of its slot counts (the weight-gradient table's partial offsets)
static void ps_build(const Net* n, long long N, const ConvEntry* abs, PsTables& T) {
  memset(&T, 0, sizeof(T));
  const crk_net_desc& d = n->d;
  if (d.kind == 2) {
    const int L = n->L;
    long long ooff[PS_MAXL], goff[PS_MAXL], ow = 0, gw = 0;
    for (int i = 0; i < L; i++) {
      ooff[i] = N * ow; goff[i] = N * gw;
      ow += n->ents[n->idx_plain[i]].fw_kp; gw += n->ents[n->idx_plain[i]].bw_kp;
    }
    for (int i = 0; i < L; i++) {
      T.t[0][i] = ps_layer_fwd(n, n->idx_plain[i], i < L - 1 ? ACT_LRELU : 0);
      T.t[0][i].save_plane = ooff[i];
      const int j = L - 1 - i;  // position in the backward chain
      T.t[1][j] = ps_layer_bwd(n, n->idx_plain[i], i > 0 ? 2 + ACT_LRELU : 0);
      T.t[1][j].save_plane = goff[i];
      if (i > 0) { T.t[1][j].mask_plane = ooff[i]; T.t[1][j].mask_w = n->ents[n->idx_plain[i]].fw_kp; }
      T.w[i] = pw_layer(n, abs, n->idx_plain[i], goff[i], N * gw + goff[i], ooff[i], N * ow + ooff[i]);
    }
    T.L[0] = T.L[1] = L; T.nw = L;
  } else {
    const int hact = d.kind == 1 ? ACT_LRELU : ACT_RELU;
    const long long P = N * 64, kpY = n->ents[n->idx_last2].bw_kp;
    const GatedB16 gf = gated_b16(n, N);
    const GatedS16 gs = gated_s16(n, N);
    T.t[0][0] = ps_layer_fwd(n, n->idx_first, d.kind == 1 ? ACT_LRELU : 0); T.L[0] = 1;
    T.t[1][0] = ps_layer_fwd(n, n->idx_last1, hact); T.t[1][0].save_plane = 0;
    T.t[1][1] = ps_layer_fwd(n, n->idx_last2, 0); T.t[1][1].save_plane = P; T.L[1] = 2;
    T.t[2][0] = ps_layer_bwd(n, n->idx_last2, 2 + hact); T.t[2][0].mask_plane = P; T.t[2][0].mask_w = 64; T.t[2][0].save_plane = 0;
    T.t[2][1] = ps_layer_bwd(n, n->idx_last1, 2 + hact); T.t[2][1].mask_plane = 0; T.t[2][1].mask_w = 64; T.t[2][1].save_plane = N * kpY;
    T.L[2] = 2;
    T.t[3][0] = ps_layer_bwd(n, n->idx_first, 0); T.L[3] = 1;
    T.w[0] = pw_layer(n, abs, n->idx_first, gs.dxb_hi, gs.dxb_lo, gf.f_hi, gf.f_lo);
    T.w[1] = pw_layer(n, abs, n->idx_last1, gs.hb_hi + N * kpY, gs.hb_lo + N * kpY, gf.head_hi, gf.head_lo);
    T.w[2] = pw_layer(n, abs, n->idx_last2, gs.hb_hi, gs.hb_lo, gf.head_hi + P, gf.head_lo + P);
    T.nw = 3;
  }
  for (int i = 0; i < T.nw; i++) {
    if (T.w[i].wa > T.max_wa) T.max_wa = T.w[i].wa;
    if (T.w[i].wb > T.max_wb) T.max_wb = T.w[i].wb;
    const int tiles = ((T.w[i].ca + 31) / 32) * ((T.w[i].cb + 31) / 32) * T.w[i].k;  // (tap, cin band, cout band) tiles
    if (tiles > T.max_tiles) T.max_tiles = tiles;
    T.wflops_per_frame += 2.0 * T.w[i].ca * T.w[i].cb * T.w[i].k;
  }
}
static double ps_flops(const PsLayer* t, int L, long long N) {
  double f = 0.0;
  for (int i = 0; i < L; i++) f += 2.0 * (double)N * t[i].rows * t[i].kp * t[i].k;
  return f;
}
static PsP ps_base(const Net* n, int B, int T, const float* params) {
  PsP p; memset(&p, 0, sizeof(p));
  p.in_scale = 1.f; p.out_scale = 1.f; p.params = params; p.whi = n->whi; p.wlo = n->wlo;
  p.B = B; p.T = T; p.slope = n->d.slope;
  return p;
}
// chain c of shape r (PsTables::t[c], p.L layers of it) on pstack_kernel: the plan fills the LDS carve-up
static int pstack_go(const Shape* r, int c, PsP& p, bool precise, hipStream_t s) {
  p.layers = r->d_ps + c * PS_MAXL;
  RUN(pstack_plan(p, r->ps.t[c], precise));
  return launch_pstack(p, precise, ps_flops(r->ps.t[c], p.L, (long long)p.B * p.T), s);
}
// can this kind-2 net / the first conv and head of this gated net run through the fused chains?
static bool plain_chains_ok(const Net* n, int B, int T, bool precise, const PsTables& Tb) {
  const int nchains = n->d.kind == 2 ? 2 : 4;
  for (int c = 0; c < nchains; c++) {
    if (Tb.L[c] > PS_MAXL) return false;
    PsP p = ps_base(n, B, T, nullptr);
    p.L = Tb.L[c];
    if (pstack_plan(p, Tb.t[c], precise) != CRK_OK) return false;
  }
  if (n->d.kind == 2) { for (int i = 0; i < n->L; i++) if (!pw_ok(n, n->idx_plain[i])) return false; }
  else if (!pw_ok(n, n->idx_first) || !pw_ok(n, n->idx_last1) || !pw_ok(n, n->idx_last2)) return false;
  return true;
}

static void stack_halo(const Net* n, int* hl, int* hr, int* max_off, int* max_dil) {
  *hl = *hr = *max_off = 0; *max_dil = 1;
  for (int l = 0; l < n->L; l++) {
    const int dil = n->meta[n->idx_conv[l]].dilation;
    const int o0 = n->d.causal ? -(n->d.kernel_size - 1) * dil : -((n->d.kernel_size - 1) / 2) * dil;
    const int o1 = o0 + (n->d.kernel_size - 1) * dil;
    *hl += -o0; *hr += o1;
    if (-o0 > *max_off) *max_off = -o0;
    if (o1 > *max_off) *max_off = o1;
    if (dil > *max_dil) *max_dil = dil;
  }
}
// the shape parts of a gated stack's launch parameters: the launches add the pointers, the planners the window
static StackP stack_fwd_shape(const Net* n, int B, int T) {
  StackP sp; memset(&sp, 0, sizeof(sp));
  int md;
  stack_halo(n, &sp.hl, &sp.hr, &sp.max_off, &md);
  sp.B = B; sp.T = T; sp.L = n->L; sp.ktaps = n->d.kernel_size;
  sp.aux_ch = n->d.aux_ch > 0 ? n->d.aux_ch : 0; sp.aux_pad = stack_aux_pad(n);
  return sp;
}
static StackBP stack_bwd_shape(const Net* n, int B, int T) {
  StackBP bp; memset(&bp, 0, sizeof(bp));
  int hl, hr, md;
  stack_halo(n, &hl, &hr, &bp.max_off, &md);
  bp.hl = hr; bp.hr = hl;  // the data gradient looks the other way
  bp.B = B; bp.T = T; bp.L = n->L; bp.ktaps = n->d.kernel_size;
  bp.aux_ch = n->d.aux_ch > 0 ? n->d.aux_ch : 0;
  return bp;
}

// The kernel path of net n at batch shape (B, T) in one arithmetic: the one place where the planners decide and the process
// switches are read.  Every planner is asked with what the call will hand it (the planners read shapes, never pointers), so
// the stored answer is the call's.  crk_net_reserve keeps both arithmetics' routes in the shape's record; the compute entry
// points read them there and call a planner only to fill the LDS offsets of a launch whose kind is already chosen.
static Route route_of(const Net* n, int B, int T, bool precise) {
  Route r = {};
  const crk_net_desc& d = n->d;
  const CrkSwitches& sw = crk_sw();
  // forward, data-gradient chain and weight gradient run fused together or not at all (the fused kernels exchange bf16
  // planes the generic kernels do not produce).  CRK_NO_FUSE=1 selects the per-layer kernels (debugging / A-B timing).
  if (sw.no_fuse || n->L > PS_MAXL) return r;
  PsTables Tb;
  ps_build(n, (long long)B * T, n->ents.data(), Tb);  // (relative partial offsets: the planners do not read them)
  if (d.kind == 2) {
    r.fused = plain_chains_ok(n, B, T, precise, Tb);
    if (!r.fused || sw.ps_v != 2) return r;  // CRK_PS_V=1: the frame-split chains
    PsP f = ps_base(n, B, T, nullptr);
    f.cin = d.in_ch; f.L = Tb.L[0];
    if (!precise && pstack2_plan(f, Tb.t[0]) == CRK_OK) r.ps_fwd = CHAIN_PS2;
    if (precise && sw.s2x && pstack2x_plan(f, Tb.t[0]) == CRK_OK) r.ps_fwd_x3f = CHAIN_PS2X;
    // the data-gradient chain; [1]: dx == nullptr and L >= 2, the chain is one layer shorter with tail = 1 and the planner is
    // asked with that L
    for (int tail = 0; tail < (Tb.L[1] >= 2 ? 2 : 1) && !precise; tail++) {
      PsP b = ps_base(n, B, T, nullptr);
      b.cin = d.out_ch; b.L = Tb.L[1] - tail; b.tail = tail;
      if (pstack2_plan(b, Tb.t[1]) == CRK_OK) r.ps_bwd[tail] = CHAIN_PS2;
    }
    return r;
  }
  int hl, hr, mo, max_dil;
  stack_halo(n, &hl, &hr, &mo, &max_dil);
  StackP sp = stack_fwd_shape(n, B, T);
  StackBP bp = stack_bwd_shape(n, B, T);
  r.fused = stack_fwd_plan(sp, precise) == CRK_OK && stack_bwd_plan(bp, precise) == CRK_OK &&
            stack_wgrad_supported(d.kernel_size, max_dil, sp.aux_ch) && plain_chains_ok(n, B, T, precise, Tb);
  r.usums = r.fused && d.aux_ch > 0;
  if (!r.fused || precise) return r;
  // plain bf16: the unfolded blocks on the channel-split kernel (stack2_kernels.hip); CRK_SK_V=1: the frame-split one
  StackP u = stack_fwd_shape(n, B, T);
  u.drop_p = d.dropout;
  r.blocks_s2 = sw.sk_v != 1 && stack2_fwd_plan(u) == CRK_OK;
  const bool split_sw = sw.sk_v == 2 && sw.skb_v == 2;
  if (d.kind == 0 && sw.sk_v == 2 && d.dropout == 0.f) {
    StackP f = stack_fwd_shape(n, B, T);
    f.x_in = reinterpret_cast<const float*>(n);  // (any non-null value: folded, the plan sizes the first conv's input tile)
    f.in_ch = d.in_ch; f.kp_first = n->ents[n->idx_first].fw_kp;
    StackP fx = f;
    StackBP b = stack_bwd_shape(n, B, T);
    // out_ch % 8 != 0 but % 4 == 0: the forward still folds, on row-layout planes; the backward stays frame-split and unfolded
    r.fold_fwd = d.in_ch % 8 == 0 && d.out_ch % 4 == 0 && stack2_fwd_plan(f) == CRK_OK;
    r.fold_bwd_fs = d.out_ch % 8 == 0 && stack_bwd_waves(false) == 8;
    // Generator stacks in plain bf16: forward and data-gradient chain both run channel-split (stack2_kernels.hip,
    // stack2b_kernels.hip), first conv and head folded in, and exchange the tanh / sigmoid planes in the lane-record layout.
    r.gen_split = r.fold_fwd && split_sw && d.out_ch % 8 == 0 && stack2_bwd_plan(b) == CRK_OK;
    // bf16x3f (forward in split-operand arithmetic, CRK_FLAG_PRECISE | CRK_FLAG_BWD_PLAIN; backward in plain bf16,
    // CRK_FLAG_FWD_PRECISE): the channel-split split-operand forward (stack2x_kernels.hip) leaves the hi planes in this route's
    // layout for this route's backward.  CRK_S2X=0: the round-4 pairing (frame-split stack_fwd_kernel<PRECISE>, frame-split
    // chain on row planes).
    r.x3f = r.gen_split && sw.s2x && stack2x_fwd_plan(fx) == CRK_OK;
  }
  if (d.kind == 1 && d.aux_ch == 0 && sw.disc_split && split_sw) {
    // The discriminator (no conditioning) in plain bf16, dropout or not: the forward's gated blocks (stack2_fwd_kernel, not
    // folded: first conv and head keep their own launches) and the data-gradient chain (stack2_bwd_kernel<.., FOLD = false>)
    // run channel-split.  CRK_DISC_SPLIT=0: the round-3 pairing (channel-split forward, frame-split chain, row-layout planes).
    StackBP b = stack_bwd_shape(n, B, T);
    r.disc_split = r.blocks_s2 && stack2_bwd_plan(b) == CRK_OK;
  }
  return r;
}
// bf16x3f (mode 2): the forward runs in split-operand arithmetic and reads the precise route, the backward in plain bf16 and
// reads the plain one, and the planes they exchange differ between the families - the per-layer forward writes fp32 planes
// only, the fused backward reads bf16 planes.  Both directions therefore take the fused kernels only where both routes are
// fused (or the plain route plans the x3f forward, which writes that route's own planes), and the per-layer kernels otherwise.
static bool routes_pair_fused(const Route rt[2]) { return rt[0].x3f || (rt[0].fused && rt[1].fused); }
static const Shape* find_shape(const Net* n, int B, int T) {
  for (const Shape& r : n->shapes)
    if (r.B == B && r.T == T) return &r;
  return nullptr;
}
// the route the compute entry points read: the shape's record, or (a shape that is not reserved) what the record would hold
static Route route_at(const Net* n, int B, int T, bool precise) {
  const Shape* r = find_shape(n, B, T);
  return r ? r->route[precise] : route_of(n, B, T, precise);
}

// What belongs to one call and not to its batch shape, read once at the top of the entry point.  in / out: x / y of a
// forward, dy / dx of a backward.
struct Call {
  bool precise, keep, defer_wn;    // CRK_FLAG_PRECISE; no CRK_FLAG_NO_SAVE: a backward will read the planes; CRK_FLAG_DEFER_WNORM
  bool want_dx, want_dc, want_w;   // backward: input, conditioning and parameter gradients are wanted
  bool in16, out16, in4;           // base 16-byte aligned and row stride a multiple of 4 floats (no `out`: true); base 4-byte aligned
  unsigned char mode;              // Net::FwdTag::mode: what a forward writes, what a backward expects to find
  unsigned long long seed_val; const unsigned long long* seed_ptr;  // the dropout seed: a value, or (CRK_FLAG_SEED_ON_DEVICE)
};                                                                  // the address of one in device memory
static bool rows16(const float* p, int ld) { return ld % 4 == 0 && (((uintptr_t)p) & 15) == 0; }
static Call call_facts(int flags, unsigned long long seed, bool forward, const float* in, int ldin, const float* out, int ldout,
                       const float* dc, const float* grads) {
  Call k;
  k.precise = flags & CRK_FLAG_PRECISE; k.keep = !(flags & CRK_FLAG_NO_SAVE); k.defer_wn = flags & CRK_FLAG_DEFER_WNORM;
  k.want_dx = out != nullptr; k.want_dc = dc != nullptr; k.want_w = !(flags & CRK_FLAG_NO_PARAM_GRAD) && grads;
  k.in16 = rows16(in, ldin); k.out16 = !out || rows16(out, ldout); k.in4 = (((uintptr_t)in) & 3) == 0;
  k.mode = k.precise ? ((forward && (flags & CRK_FLAG_BWD_PLAIN)) ? 2 : 1) : ((!forward && (flags & CRK_FLAG_FWD_PRECISE)) ? 2 : 0);
  k.seed_ptr = (flags & CRK_FLAG_SEED_ON_DEVICE) ? reinterpret_cast<const unsigned long long*>((uintptr_t)seed) : nullptr;
  k.seed_val = (flags & CRK_FLAG_SEED_ON_DEVICE) ? 0ull : seed;
  return k;
}

// the route a call reads: its arithmetic's, with a bf16x3f pair's choice of family on top
static Route call_route(const Shape* r, const Call& k) {
  Route rt = r->route[k.precise];
  if (k.mode == 2 && !r->pair_fused) rt.fused = rt.usums = false;
  return rt;
}

static void tag_forward(Net* n, const float* saved, int B, int T, const Call& k, bool x3f, bool fused) {
  if (!saved || !k.keep) return;
  const Net::FwdTag tag = {saved, B, T, k.mode, x3f, fused};
  for (int i = 0; i < n->fwd_tag_count; i++)
    if (n->fwd_tags[i].saved == saved) { n->fwd_tags[i] = tag; return; }
  n->fwd_tags[n->fwd_tag_next] = tag;
  n->fwd_tag_next = (n->fwd_tag_next + 1) % 32;
  if (n->fwd_tag_count < 32) n->fwd_tag_count++;
}
// CRK_ERR_ARG when the backward's flags do not describe the forward that filled `saved` (an unknown workspace - evicted from
// the ring, or written through another handle - passes: the caller's pairing is all there is then)
static int check_forward_tag(const Net* n, const float* saved, int B, int T, int flags, int want, bool expects_x3f, bool fused) {
  for (int i = 0; i < n->fwd_tag_count; i++) {
    const Net::FwdTag& t = n->fwd_tags[i];
    if (t.saved != saved) continue;
    if (t.B == B && t.T == T && t.mode == want && (want != 2 || t.x3f == expects_x3f)) {
      if (t.fused == fused) return CRK_OK;
      fprintf(stderr, "[crank_hip] crk_net_backward: the %s kernels would read a workspace the %s forward wrote (flags 0x%x, B %d, T %d)\n",
              fused ? "fused" : "per-layer", t.fused ? "fused" : "per-layer", flags, B, T);
      return CRK_ERR_ARG;
    }
    fprintf(stderr, "[crank_hip] crk_net_backward: flags 0x%x (plane layout %d%s, B %d, T %d) do not match the forward that wrote this "
                    "workspace (layout %d%s, B %d, T %d): CRK_FLAG_PRECISE pairs with CRK_FLAG_PRECISE, CRK_FLAG_PRECISE | CRK_FLAG_BWD_PLAIN "
                    "with CRK_FLAG_FWD_PRECISE, plain with plain\n", flags, want, expects_x3f ? " x3f" : "", B, T, t.mode, t.x3f ? " x3f" : "", t.B, t.T);
    return CRK_ERR_ARG;
  }
  return CRK_OK;
}

// ---- forward: one function per route ----------------------------------------------------------------------------------
struct FwdIo {  // the arguments of crk_net_forward
  const float* params; const float* x; int ldx; const float* c; int ldc; float* y; int ldy; float* saved; int B, T; hipStream_t s;
};
enum { FWD_CHAIN, FWD_CHAIN_LAYERS, FWD_FOLDED, FWD_FUSED, FWD_LAYERS };
// (route, call) -> the launch form of a forward, or the error the call returns
static int fwd_form(const Net* n, const Route& rt, const Call& k, bool x3f, int* form) {
  if (n->d.kind == 2) { *form = rt.fused ? FWD_CHAIN : FWD_CHAIN_LAYERS; return CRK_OK; }
  // per call: the folded kernels read x and write y in 16-byte pieces
  const bool io16 = k.in16 && k.out16;
  if ((x3f || rt.gen_split) && !io16) {
    // a channel-split route, whose backward reads the lane-record planes only the folded forward writes: the call fails
    fprintf(stderr, "[crank_hip] crk_net_forward: x / y must be 16-byte aligned with row strides that are multiples of 4 floats\n");
    return CRK_ERR_ARG;
  }
  if (x3f || (rt.fold_fwd && io16)) *form = FWD_FOLDED;
  else if (rt.gen_split) return CRK_ERR_UNSUPPORTED;  // (the route promised the plan)
  // a generator on a non-split route with x or y only 4-byte aligned lands here: the unfolded fused path, no error
  else *form = rt.fused ? FWD_FUSED : FWD_LAYERS;
  return CRK_OK;
}

// plain chain, fused: the whole stack in one launch; every conv's input operand is kept as a bf16 plane
static int fwd_chain(const Net* n, const Shape* r, const Call& k, const FwdIo& a) {
  if (!a.saved && k.keep) return CRK_ERR_ARG;
  const Route& rt = r->route[k.precise];
  const PsTables& Tb = r->ps;
  const long long N = (long long)a.B * a.T;
  PsP p = ps_base(n, a.B, a.T, a.params);
  p.x = a.x; p.ldx = a.ldx; p.cin = n->d.in_ch; p.y = a.y; p.ldy = a.ldy;
  if (k.keep) {
    p.save_hi = reinterpret_cast<uint16_t*>(a.saved + saved_f32_floats(n, N));
    p.save_lo = p.save_hi + N * plain_planes_w(n);
  }
  p.layers = r->d_ps; p.L = Tb.L[0];
  const double flops = ps_flops(Tb.t[0], Tb.L[0], N);
  const int kern = k.mode == 2 ? rt.ps_fwd_x3f : rt.ps_fwd;
  if (kern == CHAIN_PS2X) p.save_lo = nullptr;  // bf16x3f: split-operand forward, hi planes only
  if (kern == CHAIN_PS2X) { RUN(pstack2x_plan(p, Tb.t[0])); return launch_pstack2x(p, flops, a.s); }
  if (kern == CHAIN_PS2) { RUN(pstack2_plan(p, Tb.t[0])); return launch_pstack2(p, flops, a.s); }
  return pstack_go(r, 0, p, k.precise, a.s);
}
static int fwd_chain_layers(const Net* n, const Call& k, const FwdIo& a) {
  const crk_net_desc& d = n->d;
  const int L = n->L;
  const long long N = (long long)a.B * a.T;
  if (L > 1 && !a.saved) return CRK_ERR_ARG;
  const float* in = a.x; int ldin = a.ldx;
  for (int i = 0; i < L; i++) {
    const ConvEntry& e = n->ents[n->idx_plain[i]];
    const int dil = n->meta[n->idx_plain[i]].dilation;
    const bool last = i == L - 1;
    ConvP p = conv_fw(n, a.B, a.T, e, a.params, in, ldin, last ? a.y : a.saved + (long long)i * N * d.conv_ch, last ? a.ldy : d.conv_ch);
    p.act_in = (i == 0) ? ACT_NONE : ACT_LRELU;
    p.ktaps = e.k; p.dil = dil; p.off0 = -((e.k - 1) / 2) * dil;
    RUN(conv_go(p, MODE_PLAIN, k.precise, a.s));
    in = p.y; ldin = p.ldy;
  }
  return CRK_OK;
}
// a gated forward's launch parameters, all but the stack's input and output.  lo: hi + lo planes (the unfolded kernels); else
// the hi planes and the folded first conv's and head's
static StackP stack_fwd_params(const Net* n, const Call& k, const FwdIo& a, bool lo) {
  const long long N = (long long)a.B * a.T;
  const GatedB16 gf = gated_b16(n, N);
  uint16_t* b16 = reinterpret_cast<uint16_t*>(a.saved + saved_f32_floats(n, N));
  StackP sp = stack_fwd_shape(n, a.B, a.T);
  sp.c = a.c; sp.ldc = a.ldc; sp.params = a.params;
  sp.skip = a.saved + gated_f32(n, N).skip;  // (unused by the folded kernel; a valid base for its dummy descriptors)
  sp.whi = n->whi; sp.wlo = n->wlo; sp.layers = n->d_layers;
  if (!k.keep) return sp;
  sp.saved = a.saved;
  sp.xb_hi = b16 + gf.xb_hi; sp.zb_hi = b16 + gf.zb_hi; sp.tb_hi = b16 + gf.tb_hi; sp.sg_hi = b16 + gf.sg_hi;
  if (n->d.aux_ch > 0) sp.cb_hi = b16 + gf.cb_hi;
  if (!lo) { sp.fin_hi = b16 + gf.f_hi; sp.head_hi = b16 + gf.head_hi; return sp; }
  sp.xb_lo = b16 + gf.xb_lo; sp.zb_lo = b16 + gf.zb_lo; sp.tb_lo = b16 + gf.tb_lo; sp.sg_lo = b16 + gf.sg_lo;
  if (n->d.aux_ch > 0) sp.cb_lo = b16 + gf.cb_lo;
  return sp;
}
// generator stacks: first conv, gated blocks and head in ONE launch - plain bf16 (stack2_kernels.hip), or x3f: split-operand
// arithmetic that saves the plain route's planes (stack2x_kernels.hip)
static int fwd_folded(const Net* n, const Route& rt, const Call& k, const FwdIo& a, bool x3f) {
  const crk_net_desc& d = n->d;
  const ConvEntry& ef = n->ents[n->idx_first];
  const ConvEntry& e1 = n->ents[n->idx_last1];
  const ConvEntry& e2 = n->ents[n->idx_last2];
  StackP sp = stack_fwd_params(n, k, a, false);
  sp.x_in = a.x; sp.ldx_in = a.ldx; sp.in_ch = d.in_ch; sp.kp_first = ef.fw_kp;
  sp.f_first = ef.fr_off; sp.b_first = ef.off_b;
  sp.f_h1 = e1.fr_off; sp.b_h1 = e1.off_b; sp.f_h2 = e2.fr_off; sp.b_h2 = e2.off_b;
  sp.y = a.y; sp.ldy = a.ldy; sp.out_ch = d.out_ch; sp.head_scale = (float)sqrt(1.0 / n->L);
  // a channel-split route: the lane-record planes.  Not one (out_ch % 8 != 0 but % 4 == 0, or CRK_SKB_V=1): row-layout planes
  if (x3f || rt.gen_split) sp.ts_stride = ts_plane_stride((long long)a.B * a.T);
  if (x3f) { RUN(stack2x_fwd_plan(sp)); return launch_stack2x_fwd(sp, a.s); }
  RUN(stack2_fwd_plan(sp));
  return launch_stack2_fwd(sp, a.s);
}
// gated stack, fused and not folded: first conv, the blocks and the head, one launch each
static int fwd_fused(const Net* n, const Shape* r, const Call& k, const FwdIo& a) {
  const crk_net_desc& d = n->d;
  const Route& rt = r->route[k.precise];
  const long long N = (long long)a.B * a.T;
  const GatedF32 lay = gated_f32(n, N);
  const GatedB16 gf = gated_b16(n, N);
  uint16_t* b16 = reinterpret_cast<uint16_t*>(a.saved + saved_f32_floats(n, N));
  PsP f = ps_base(n, a.B, a.T, a.params);  // first conv (1x1; kind 1: + LeakyReLU) -> X_0, its input kept as a bf16 plane
  f.x = a.x; f.ldx = a.ldx; f.cin = d.in_ch; f.y = a.saved + lay.x; f.ldy = 64; f.L = 1;
  if (k.keep) { f.save_hi = b16 + gf.f_hi; f.save_lo = b16 + gf.f_lo; }
  RUN(pstack_go(r, 0, f, k.precise, a.s));
  StackP sp = stack_fwd_params(n, k, a, true);
  sp.x0 = a.saved + lay.x;
  if (d.dropout > 0.f) { sp.drop_p = d.dropout; sp.drop_seed = k.seed_val; sp.drop_seed_ptr = k.seed_ptr; }
  if (rt.disc_split) sp.ts_stride = ts_plane_stride(N);  // (its data-gradient chain reads lane records)
  if (rt.blocks_s2) { RUN(stack2_fwd_plan(sp)); RUN(launch_stack2_fwd(sp, a.s)); }
  else {
    if (sp.ts_stride) return CRK_ERR_UNSUPPORTED;  // (the route promised the plan)
    RUN(stack_fwd_plan(sp, k.precise));
    RUN(launch_stack_fwd(sp, k.precise, a.s));
  }
  // head: act(skips * sqrt(1/L)) -> 1x1 -> act -> 1x1, one launch; both operands kept as bf16 planes
  PsP p = ps_base(n, a.B, a.T, a.params);
  p.x = a.saved + lay.skip; p.ldx = 64; p.cin = 64; p.in_scale = (float)sqrt(1.0 / n->L); p.in_act = d.kind == 1 ? ACT_LRELU : ACT_RELU;
  p.y = a.y; p.ldy = a.ldy; p.L = 2;
  if (k.keep) { p.save_hi = b16 + gf.head_hi; p.save_lo = b16 + gf.head_lo; }
  return pstack_go(r, 1, p, k.precise, a.s);
}
static int fwd_layers(const Net* n, const Call& k, const FwdIo& a) {
  const crk_net_desc& d = n->d;
  const int L = n->L, head_act = d.kind == 1 ? ACT_LRELU : ACT_RELU;
  const long long N = (long long)a.B * a.T, P = N * 64;
  const GatedF32 lay = gated_f32(n, N);
  float *X = a.saved + lay.x, *SKIP = a.saved + lay.skip, *H1 = a.saved + lay.h1;
  ConvP f = conv_fw(n, a.B, a.T, n->ents[n->idx_first], a.params, a.x, a.ldx, X, 64);  // first conv (kind 1: + LeakyReLU)
  f.act_out = d.kind == 1 ? ACT_LRELU : ACT_NONE;
  RUN(conv_go(f, MODE_PLAIN, k.precise, a.s));
  for (int l = 0; l < L; l++) {
    const ConvEntry& ec = n->ents[n->idx_conv[l]];
    const ConvEntry& eo = n->ents[n->idx_out[l]];
    const ConvEntry& es = n->ents[n->idx_skip[l]];
    const int dil = n->meta[n->idx_conv[l]].dilation;
    ConvP p = conv_fw(n, a.B, a.T, ec, a.params, X + l * P, 64, (l < L - 1) ? X + (l + 1) * P : nullptr, 64);
    p.ktaps = ec.k; p.dil = dil; p.off0 = fwd_off0(n, ec.k, dil);
    if (d.dropout > 0.f) { p.drop_p = d.dropout; p.drop_seed = layer_seed(k.seed_val, l); p.drop_seed_ptr = k.seed_ptr; }
    if (d.aux_ch > 0) {
      const ConvEntry& ea = n->ents[n->idx_aux[l]];
      p.xc = a.c; p.ldc = a.ldc; p.cinC = ea.cin; p.cinC_pad = ea.fw_kp;
      p.wc_hi = n->whi + ea.fw_off; p.wc_lo = n->wlo + ea.fw_off;
    }
    p.w2_hi = n->whi + eo.fw_off; p.w2_lo = n->wlo + eo.fw_off;
    p.bias2a = eo.off_b >= 0 ? a.params + eo.off_b : nullptr;
    p.bias2b = es.off_b >= 0 ? a.params + es.off_b : nullptr;
    p.skip = SKIP; p.skip_init = (l == 0);
    p.sv_ta = a.saved + lay.ta + l * P; p.sv_sb = a.saved + lay.sb + l * P; p.sv_z = a.saved + lay.z + l * P;
    RUN(conv_go(p, MODE_RESFWD, k.precise, a.s));
  }
  // head: act(skips * sqrt(1/L)) -> 1x1 -> act -> 1x1
  ConvP h1 = conv_fw(n, a.B, a.T, n->ents[n->idx_last1], a.params, SKIP, 64, H1, 64);
  h1.scaleA = (float)sqrt(1.0 / L); h1.act_in = head_act;
  RUN(conv_go(h1, MODE_PLAIN, k.precise, a.s));
  ConvP h2 = conv_fw(n, a.B, a.T, n->ents[n->idx_last2], a.params, H1, 64, a.y, a.ldy);
  h2.act_in = head_act;
  return conv_go(h2, MODE_PLAIN, k.precise, a.s);
}
extern "C" int crk_net_forward(void* h, const float* params, unsigned long long version, const float* x, int ldx,
                               const float* c, int ldc, float* y, int ldy, float* saved, int B, int T, int flags,
                               unsigned long long seed, void* stream) {
  Net* n = (Net*)h;
  if (!n || !params || !x || !y || B <= 0 || T <= 0) return CRK_ERR_ARG;
  const FwdIo a = {.params = params, .x = x, .ldx = ldx, .c = c, .ldc = ldc, .y = y, .ldy = ldy, .saved = saved, .B = B, .T = T,
                   .s = (hipStream_t)stream};
  const Call k = call_facts(flags, seed, true, x, ldx, y, ldy, nullptr, nullptr);
  const Shape* r = find_shape(n, B, T);
  if (!r) return not_reserved("crk_net_forward");
  const Route rt = call_route(r, k);
  // bf16x3f: split-operand arithmetic that saves the plain route's planes
  const bool x3f = k.mode == 2 && r->route[0].x3f;
  RUN(ensure_prepared(n, params, version, a.s));
  if (n->d.kind != 2 && (!saved || (n->d.aux_ch > 0 && !c))) return CRK_ERR_ARG;
  int form;
  RUN(fwd_form(n, rt, k, x3f, &form));
  tag_forward(n, saved, B, T, k, x3f, form != FWD_LAYERS && form != FWD_CHAIN_LAYERS);
  switch (form) {
    case FWD_CHAIN: return fwd_chain(n, r, k, a);
    case FWD_CHAIN_LAYERS: return fwd_chain_layers(n, k, a);
    case FWD_FOLDED: return fwd_folded(n, rt, k, a, x3f);
    case FWD_FUSED: return fwd_fused(n, r, k, a);
  }
  return fwd_layers(n, k, a);
}

// Weight-gradient groups of a net's "stack region" (the gated blocks' launch is one workgroup per (group, block); the
// partial sums are read back `groups` times by the weight-norm backward): runs of 64-frame chunks, utterance after
// utterance.  32 groups of whole utterances by default; a gated stack of few blocks gets as many groups as fill the 256
// compute units with its (group, block) workgroups - 6 blocks x 32 groups are 192 workgroups of 16 chunks each (B = 64,
// T = 500), 6 x 40 are 240 of 13.  A stack of 8 blocks keeps its 32 groups of two utterances: same sums, bit for bit.
static int stack_cpg(const Net* n, int B, int T) {
  const int ncpu = (T + 63) / 64;
  const int groups = crk_sw().wg_groups;
  const int gsz = (B + groups - 1) / groups;  // utterances per group
  int cpg = gsz * ncpu;
  if (crk_sw().wg_fill && n->d.kind != 2 && n->L > 0 && 256 / n->L > groups) {
    const int fill = 256 / n->L;
    const int c = (B * ncpu + fill - 1) / fill;
    if (c >= 1 && c < cpg) cpg = c;
  }
  return cpg < 1 ? 1 : cpg;
}
static int stack_groups(const Net* n, int B, int T) {
  const int total = B * ((T + 63) / 64), cpg = stack_cpg(n, B, T);
  return (total + cpg - 1) / cpg;
}

// per-utterance dG sums (StackWP::usums) of a gated stack with conditioning: segments per group, floats, and their place
// behind the gradient planes in `scratch`
static int usum_nseg(const Net* n, int B, int T) {
  const int ncpu = (T + 63) / 64;
  return (stack_cpg(n, B, T) + 2 * ncpu - 2) / ncpu;  // a group of cpg chunks that starts at the last chunk of an utterance
}
static long long usum_floats(const Net* n, int B, int T) {
  if (n->d.kind == 2 || n->d.aux_ch <= 0) return 0;
  return (long long)stack_groups(n, B, T) * usum_nseg(n, B, T) * n->L * 128;
}
static long long usum_off(const Net* n, long long N) { return gated_f32(n, N).scratch_total + (gated_s16(n, N).total + 1) / 2; }
static ShapeNeed shape_need(const Net* n, int B, int T) {
  ShapeNeed q;
  const long long N = (long long)B * T;
  const long long cw = n->d.conv_ch > n->d.out_ch ? n->d.conv_ch : n->d.out_ch;
  // every layer keeps its own gradient buffers: the weight gradients of the whole stack
  // run as ONE launch after the data-gradient chain
  // gated stacks: dS | dH1 | dX_l (L+1) | dG_l (2L) fp32 planes, then the bf16 planes of the fused chain:
  // dGb_hi[L] dGb_lo[L] ([N,128]), dXb_hi[L+1] dXb_lo[L+1], dSb_hi dSb_lo ([N,64])
  // (+ head: dy and dH1 bf16 planes);  kind 2: per-layer fp32 gradients (fallback) + bf16 output-gradient planes
  q.need_s = n->d.kind == 2 ? (long long)n->L * N * cw + N * plain_gplanes_w(n)
                            : usum_off(n, N) + usum_floats(n, B, T);
  q.Gs = stack_groups(n, B, T); q.cpg_s = stack_cpg(n, B, T); q.nseg = usum_nseg(n, B, T);
  // generic convs: runs of 64-frame chunks, at most 32 groups: short runs = many workgroups hide the latency of the
  // table kernel's load -> MFMA chain, but every group is one more pass of the weight-norm backward over the
  // partial sums and one more set-up / partial-sum write-out (12 % + 21 % of a workgroup's life at 8 chunks per group).
  // Round 2, one-deep prefetch: 128 groups 2.14 ms/step, 64 groups 2.10, 51 groups 2.12.  Round 6, chunks requested two
  // ahead: 64 groups (8 chunks each) 1.490 ms/step, 43 groups 1.496, 32 groups (16 each) 1.481, 16 groups 1.512
  // (profiles/round6_c_envs.txt).
  // ... and a chain of few convs (the speaker-adversarial net: 3) keeps 64 groups: its launch is (groups x convs) workgroups,
  // 96 of them for 256 CUs at 32 groups (22.0 -> 30.5 us, profiles/round6_c_kernel_stats.csv)
  const int total_chunks = B * ((T + 63) / 64);
  const int groups = (n->d.kind == 2 && n->ents.size() <= 4) ? 64 : 32;
  q.cpg = (total_chunks + groups - 1) / groups;
  if (crk_sw().wg_cpg > 0) q.cpg = crk_sw().wg_cpg;
  q.Gg = (total_chunks + q.cpg - 1) / q.cpg;
  q.need_p = n->pt_floats_stack * q.Gs + n->pt_floats_gen * q.Gg;
  return q;
}
// a buffer that must hold `need` floats: outgrown ones are retired, not freed (a captured graph may still hold the pointer)
static int grow(Net* n, float** buf, long long* cap, long long need) {
  if (need <= *cap) return CRK_OK;
  if (*buf) n->retired.push_back(*buf);
  *buf = nullptr; *cap = 0;
  if (NET_MALLOC(buf, need * 4) != hipSuccess) return CRK_ERR_HIP;
  *cap = need;
  return CRK_OK;
}
static int build_shape(Net* n, Shape& r) {
  const crk_net_desc& d = n->d;
  // partial offsets are per group; the device table needs absolute offsets for the shape's slot counts:
  // [stack region: entry block x Gs slots][generic region: entry block x Gg slots]
  r.abs = n->ents;
  for (auto& e : r.abs) {
    const bool stack = e.pt_groups != 0;
    const long long base = stack ? 0 : n->pt_floats_stack * r.q.Gs;
    const int G = stack ? r.q.Gs : r.q.Gg;
    e.pt_off = base + e.pt_off * G; e.pb_off = base + e.pb_off * G; e.pt_groups = G;
  }
  RUN(upload(&r.d_ents, r.abs.data(), r.abs.size()));
  if (n->L <= PS_MAXL) {
    ps_build(n, (long long)r.B * r.T, r.abs.data(), r.ps);
    RUN(upload(&r.d_ps, &r.ps.t[0][0], 4 * PS_MAXL));
    RUN(upload(&r.d_pw, r.ps.w, PS_MAXL));
  }
  if (d.kind != 2) {  // the fused weight-gradient layer table of the gated stack (partial offsets of the Gs utterance groups)
    std::vector<StackWLayer> wt(n->L);
    for (int l = 0; l < n->L; l++) {
      const ConvEntry& ec = n->ents[n->idx_conv[l]];
      const ConvEntry& eo = n->ents[n->idx_out[l]];
      const ConvEntry& ac = r.abs[n->idx_conv[l]];
      const ConvEntry& ao = r.abs[n->idx_out[l]];
      StackWLayer& y = wt[l];
      y.pt_conv = ac.pt_off; y.pb_conv = ec.off_b >= 0 ? ac.pb_off : -1;
      y.pt_os = ao.pt_off; y.pb_os = eo.off_b >= 0 ? ao.pb_off : -1;
      y.pt_aux = d.aux_ch > 0 ? r.abs[n->idx_aux[l]].pt_off : 0;
      y.dil = n->meta[n->idx_conv[l]].dilation;
      y.off0 = fwd_off0(n, ec.k, y.dil);
    }
    RUN(upload(&r.d_wlayers, wt.data(), wt.size()));
  }
  return CRK_OK;
}
extern "C" int crk_net_reserve(void* h, int B, int T) {
  Net* n = (Net*)h;
  if (!n || B <= 0 || T <= 0) return CRK_ERR_ARG;
  if (find_shape(n, B, T)) return CRK_OK;
  AllocScope may_allocate;
  Shape r{};
  r.B = B; r.T = T; r.q = shape_need(n, B, T);
  r.route[0] = route_of(n, B, T, false);
  r.route[1] = route_of(n, B, T, true);
  r.pair_fused = routes_pair_fused(r.route);
  RUN(grow(n, &n->scratch, &n->scratch_cap, r.q.need_s));
  RUN(grow(n, &n->partials, &n->partial_cap, r.q.need_p));
  if (!n->d_jobs && NET_MALLOC(&n->d_jobs, sizeof(WgradP) * 256) != hipSuccess) return CRK_ERR_HIP;
  const int rc = build_shape(n, r);
  if (rc != CRK_OK) {  // (e.g. a new batch shape first seen inside a stream capture: run it eagerly once)
    free_shape(r);
    return rc;
  }
  n->shapes.push_back(r);
  return CRK_OK;
}
extern "C" long long crk_net_scratch_bytes(void* h, int B, int T) {
  Net* n = (Net*)h;
  if (!n || B <= 0 || T <= 0) return -1;
  const ShapeNeed q = shape_need(n, B, T);
  return (q.need_s + q.need_p) * 4;
}
extern "C" long long crk_debug_alloc_count(void) { return g_net_allocs; }
// vocoder_kernels.hip counts its handles' allocations here too
long long crk_count_alloc_(void) { return ++g_net_allocs; }
// which kernel generation the compute entry points pick for a batch shape (its route): bit 0 the generator stack runs
// channel-split in plain bf16 (stack2_fwd_kernel / stack2_bwd_kernel), bit 1 its bf16x3f forward runs on the channel-split
// split-operand kernel (stack2x_fwd_kernel), bit 2 the discriminator's blocks and chain run channel-split, bit 3 the net is a
// chain of plain convs that runs fused (pstack kernels).  Every fallback computes the same values, only slower - within what
// tests/test_gpu_per_layer.py and tests/test_gpu_fallback.py compare, DESIGN.md "What reaches the per-layer kernels": a test
// pins the bits at the benchmark shape so that a plan that starts failing does not pass as a timing.
extern "C" int crk_debug_net_paths(void* h, int B, int T) {
  Net* n = (Net*)h;
  if (!n || B <= 0 || T <= 0) return -1;
  const Route r = route_at(n, B, T, false);
  return (int)r.gen_split | (int)r.x3f << 1 | (int)r.disc_split << 2 | (int)(n->d.kind == 2 && r.fused) << 3;
}

// The layout of reserved shape (B, T), so that a test can assert that it runs the edge it is named after (tests/net_layout.py
// restates the rules): out = {Gs, cpg_s, Gg, cpg, nseg of the shape's ShapeNeed, the ft stack2_bwd_plan chose, the window rows
// of the plain-bf16 forward (stack2_fwd_kernel, or pstack2_kernel of a plain chain), 0}.  0 where a value does not apply: a
// plain chain has no stack region, a stack without conditioning no sum segments, a route whose chain or forward is not
// channel-split no ft / rows.  Host code only.  CRK_ERR_ARG: the shape is not reserved.
extern "C" int crk_debug_net_layout(void* h, int B, int T, int* out) {
  Net* n = (Net*)h;
  const Shape* r = n ? find_shape(n, B, T) : nullptr;
  if (!r || !out) return CRK_ERR_ARG;
  const Route& rt = r->route[0];
  const bool gated = n->d.kind != 2;
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (gated) { out[0] = r->q.Gs; out[1] = r->q.cpg_s; }
  out[2] = r->q.Gg; out[3] = r->q.cpg;
  if (usum_floats(n, B, T) > 0) out[4] = r->q.nseg;
  if (gated && (rt.gen_split || rt.disc_split)) {
    StackBP b = stack_bwd_shape(n, B, T);
    if (stack2_bwd_plan(b) == CRK_OK) out[5] = b.ft;
  }
  if (gated && (rt.fold_fwd || rt.blocks_s2)) {
    StackP f = stack_fwd_shape(n, B, T);
    if (rt.fold_fwd) {
      f.x_in = reinterpret_cast<const float*>(n);  // (as route_of: folded)
      f.in_ch = n->d.in_ch; f.kp_first = n->ents[n->idx_first].fw_kp;
    } else f.drop_p = n->d.dropout;
    if (stack2_fwd_plan(f) == CRK_OK) out[6] = 32 * (f.ft + (f.ft1 ? f.ft1 : f.ft)) * f.fh / 2;
  }
  if (!gated && rt.fused && rt.ps_fwd == CHAIN_PS2) {
    PsP f = ps_base(n, B, T, nullptr);
    f.cin = n->d.in_ch; f.L = r->ps.L[0];
    if (pstack2_plan(f, r->ps.t[0]) == CRK_OK) out[6] = 32 * f.nw;
  }
  return CRK_OK;
}

// The weight-gradient partial sums of shape (B, T) as the last backward left them (tests compare launch forms on them):
// returns their count and copies the first min(count, cap) floats to `out` (device memory); -1: the shape is not reserved.
extern "C" long long crk_debug_net_partials(void* h, int B, int T, float* out, long long cap, void* stream) {
  Net* n = (Net*)h;
  const Shape* r = n ? find_shape(n, B, T) : nullptr;
  if (!r || !n->partials || cap < 0 || (cap > 0 && !out)) return -1;
  const long long cnt = r->q.need_p < cap ? r->q.need_p : cap;
  if (cnt > 0 && hipMemcpyAsync(out, n->partials, sizeof(float) * cnt, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return -1;
  return r->q.need_p;
}

static WgradP base_wgrad(const Net* n, int B, int T) {
  WgradP w;
  memset(&w, 0, sizeof(w));
  w.sa1 = w.sa2 = w.sx = 1.f; w.slope = n->d.slope;
  w.B = B; w.T = T; w.ktaps = 1; w.dil = 1; w.off0 = 0;
  w.dbg = 0;
  return w;
}
// partial-sum slots of conv entry ei at shape r: pointers into the partial block, chunks per group, group count
static void wgrad_slots(const Net* n, const Shape* r, int ei, WgradP& w) {
  const ConvEntry& a = r->abs[ei];
  const bool stack = n->ents[ei].pt_groups != 0;
  w.partial = n->partials + a.pt_off;
  w.bias_partial = a.off_b >= 0 ? n->partials + a.pb_off : nullptr;
  w.ngroups = a.pt_groups;
  w.cpg = stack ? r->q.cpg_s : r->q.cpg;
}
// queue one weight-gradient problem; launched with the rest of the stack's by wgrad_flush
static int wgrad_go(Net* n, WgradP& w, bool precise) {
  w.ca_pad = pad32(w.ca); w.cx_pad = pad32(w.cx); w.cc_pad = w.has_aux ? pad32(w.cc) : 0;
  return wgrad_expand(w, precise, n->jobs);
}
// ... of conv entry ei: dY = a1 [N, cout], the conv's input = act_in(sx * x) [N, cin]
static int wgrad_conv(Net* n, const Shape* r, int ei, const float* a1, int lda1, const float* x, int ldx, int act_in, float sx, bool precise) {
  const ConvEntry& e = n->ents[ei];
  WgradP w = base_wgrad(n, r->B, r->T);
  w.a1 = a1; w.lda1 = lda1; w.ca1 = e.cout; w.ca = e.cout;
  w.x = x; w.ldx = ldx; w.cx = e.cin; w.sx = sx; w.act_in = act_in;
  w.ktaps = e.k; w.dil = n->meta[ei].dilation; w.off0 = -((e.k - 1) / 2) * w.dil;  // (plain convs: never causal)
  wgrad_slots(n, r, ei, w);
  return wgrad_go(n, w, precise);
}
static int wgrad_flush(Net* n, int B, int T, bool precise, hipStream_t s) {
  if (n->jobs.empty()) return CRK_OK;
  if (n->jobs.size() > 256) return CRK_ERR_UNSUPPORTED;
  const int k = n->slot_next;
  n->slot_next = (k + 1) & 3;
  if (!n->h_slot[k]) {
    if (hipHostMalloc((void**)&n->h_slot[k], sizeof(WgradP) * 256, hipHostMallocDefault) != hipSuccess) return CRK_ERR_HIP;
    if (hipEventCreateWithFlags(&n->slot_ev[k], hipEventDisableTiming) != hipSuccess) return CRK_ERR_HIP;
  } else if (hipEventSynchronize(n->slot_ev[k]) != hipSuccess) {
    return CRK_ERR_HIP;
  }
  memcpy(n->h_slot[k], n->jobs.data(), sizeof(WgradP) * n->jobs.size());
  if (hipMemcpyAsync(n->d_jobs, n->h_slot[k], sizeof(WgradP) * n->jobs.size(), hipMemcpyHostToDevice, s) != hipSuccess)
    return CRK_ERR_HIP;
  if (hipEventRecord(n->slot_ev[k], s) != hipSuccess) return CRK_ERR_HIP;
  int mg = 0;
  for (const auto& j : n->jobs) if (j.ngroups > mg) mg = j.ngroups;
  int rc = launch_wgrad_table(n->d_jobs, n->jobs, B, T, mg, precise, s);
  n->jobs.clear();
  return rc;
}

// weight gradients of the plain convs of a net from the bf16 planes of its fused chains at shape r
static PwP plain_wgrad_params(const Net* n, const Shape* r, const uint16_t* abase, const uint16_t* bbase) {
  PwP wp; memset(&wp, 0, sizeof(wp));
  wp.layers = r->d_pw; wp.abase = abase; wp.bbase = bbase; wp.partials = n->partials;
  wp.B = r->B; wp.T = r->T; wp.cpg = r->q.cpg; wp.G = r->q.Gg;
  return wp;
}
static int launch_plain_wgrad(const Shape* r, const PwP& wp, bool precise, hipStream_t s) {
  const PsTables& Tb = r->ps;
  return launch_pstack_wgrad(wp, Tb.nw, Tb.max_wa, Tb.max_wb, precise, Tb.wflops_per_frame * r->B * r->T, s, Tb.max_tiles);
}
static int flush_pending_plain_wgrad(Net* n, hipStream_t s) {
  if (!n->pw_shape) return CRK_OK;
  const Shape* r = n->pw_shape;
  n->pw_shape = nullptr;
  return launch_plain_wgrad(r, n->pw_params, false, s);
}

// flags bit0: precise; bit1: skip parameter gradients (they would be discarded);
// dx / dc may be null when the corresponding input needs no gradient.
// dx_scale multiplies the returned input gradient (gradient reversal: -lambda).
// the embedding table behind the conditioning columns [c0, c0 + E) (crk_net_backward_embed)
struct CondEmbed { const long long* idx; long long run; int c0, E, n_rows; float* dtable; };
// ---- backward: one function per route; the entry point finishes the weight gradients of all of them ----------------------
struct BwdIo {  // the arguments of crk_net_backward*
  const float* params; float* grads; const float* x; int ldx; const float* c; int ldc; const float* dy; int lddy;
  float* dx; int lddx; float dx_scale; float* dc; int lddc; const float* saved; int B, T;
  const float* dy_num; const float* dy_den; const CondEmbed* ce; hipStream_t s;
};
enum { BWD_CHAIN, BWD_CHAIN_LAYERS, BWD_FOLDED_SPLIT, BWD_FOLDED, BWD_FUSED_SPLIT, BWD_FUSED, BWD_LAYERS };
// (route, call) -> the launch form of a backward, or the error the call returns.  planes_precise: the forward left hi + lo
// row planes (FWD_PRECISE flags where the forward was not the x3f one, or bf16x3): the channel-split chains, which read gate
// planes in the lane-record layout only the plain-plane forwards write, are both off
static int bwd_form(const Net* n, const Route& rt, const Call& k, bool planes_precise, int* form) {
  if (n->d.kind == 2) { *form = rt.fused ? BWD_CHAIN : BWD_CHAIN_LAYERS; return CRK_OK; }
  if (!rt.fused) { *form = BWD_LAYERS; return CRK_OK; }
  // per call: the folds write dx in 16-byte pieces
  const bool ok_x = k.out16 && (!k.want_dx || n->d.in_ch % 4 == 0);
  if (rt.gen_split && !planes_precise) {
    // the channel-split fold also takes a dy whose rows are only 4-byte aligned: a column slice of a wider gradient
    if (!k.in4 || !ok_x) {
      // the forward wrote the gate planes for the channel-split chain: nothing else can read them
      fprintf(stderr, "[crank_hip] crk_net_backward: dy / dx must be 16-byte aligned with row strides that are multiples of 4 floats\n");
      return CRK_ERR_ARG;
    }
    *form = BWD_FOLDED_SPLIT;
  } else if (rt.disc_split && !planes_precise) *form = BWD_FUSED_SPLIT;  // the discriminator: the same chain without the folds
  // the frame-split fold reads dy in 16-byte pieces
  else *form = (rt.fold_bwd_fs && k.in16 && ok_x) ? BWD_FOLDED : BWD_FUSED;
  return CRK_OK;
}

// plain chain, fused: the data-gradient chain in one launch (output-gradient planes kept), then all weight gradients in one
static int bwd_chain(Net* n, const Shape* r, const Call& k, const BwdIo& a) {
  if (!a.saved) return CRK_ERR_ARG;
  const crk_net_desc& d = n->d;
  const PsTables& Tb = r->ps;
  const long long N = (long long)a.B * a.T;
  const long long cw = d.conv_ch > d.out_ch ? d.conv_ch : d.out_ch;
  const uint16_t* f16 = reinterpret_cast<const uint16_t*>(a.saved + saved_f32_floats(n, N));
  uint16_t* g16 = reinterpret_cast<uint16_t*>(n->scratch + (long long)n->L * N * cw);
  PsP p = ps_base(n, a.B, a.T, a.params);
  p.x = a.dy; p.ldx = a.lddy; p.cin = d.out_ch; p.y = a.dx; p.ldy = a.lddx; p.out_scale = a.dx_scale;
  p.in_num = a.dy_num; p.in_den = a.dy_den;
  p.save_hi = g16; p.save_lo = g16 + N * plain_gplanes_w(n); p.mask_hi = f16;
  p.layers = r->d_ps + PS_MAXL; p.L = Tb.L[1];
  // per call: nobody wants the input gradient (the classifier's input is data, the adversarial net's is detached in its own
  // update): the chain stops at the output-gradient plane of the first conv - its weight gradient needs that - and the
  // transposed first conv, the widest layer of the chain, is not computed (dx == nullptr and L >= 2: tail = 1)
  if (!k.want_dx && p.L >= 2) { p.L -= 1; p.tail = 1; }
  if (r->route[k.precise].ps_bwd[p.tail] == CHAIN_PS2) {
    RUN(pstack2_plan(p, Tb.t[1]));
    RUN(launch_pstack2(p, ps_flops(Tb.t[1], p.L, N), a.s));
  } else RUN(pstack_go(r, 1, p, k.precise, a.s));
  if (!k.want_w) return CRK_OK;
  const PwP wp = plain_wgrad_params(n, r, g16, f16);
  // CRK_FLAG_DEFER_WNORM, plain bf16: parked like the plain convs around a gated stack (gated_plain_wgrad) - the group call
  // runs it in one launch with the other nets' (the speaker nets of a step: two updates, one set of launches)
  if (k.defer_wn && !k.precise) { n->pw_shape = r; n->pw_params = wp; return CRK_OK; }
  return launch_plain_wgrad(r, wp, k.precise, a.s);
}
static int bwd_chain_layers(Net* n, const Shape* r, const Call& k, const BwdIo& a) {
  const crk_net_desc& d = n->d;
  const long long N = (long long)a.B * a.T;
  const long long cw = d.conv_ch > d.out_ch ? d.conv_ch : d.out_ch;
  const float* dcur = a.dy; int ldcur = a.lddy;
  for (int i = n->L - 1; i >= 0; i--) {
    const int ei = n->idx_plain[i];
    const ConvEntry& e = n->ents[ei];
    const int dil = n->meta[ei].dilation;
    const float* in = (i == 0) ? a.x : a.saved + (long long)(i - 1) * N * d.conv_ch;
    const int ldin = (i == 0) ? a.ldx : d.conv_ch;
    if (k.want_w) RUN(wgrad_conv(n, r, ei, dcur, ldcur, in, ldin, (i == 0) ? ACT_NONE : ACT_LRELU, 1.f, k.precise));
    if (i == 0 && !k.want_dx) break;
    float* out = i > 0 ? n->scratch + (long long)i * N * cw : a.dx;  // dH_{i-1}, kept for its weight gradient
    ConvP p = conv_bw(n, a.B, a.T, e, dcur, ldcur, out, i > 0 ? d.conv_ch : a.lddx);
    p.ktaps = e.k; p.dil = dil; p.off0 = -(-((e.k - 1) / 2) * dil) - (e.k - 1) * dil;
    if (i > 0) { p.dmask = in; p.ldm = ldin; p.dmask_act = ACT_LRELU; }
    else p.out_scale = a.dx_scale;
    RUN(conv_go(p, MODE_PLAIN, k.precise, a.s));
    dcur = out; ldcur = d.conv_ch;
  }
  return CRK_OK;
}

// the bf16 planes of a fused gated backward: the forward's in `saved`, this backward's in scratch
struct GatedPlanes { const uint16_t* f16; uint16_t* s16; GatedB16 gf; GatedS16 gs; };
static GatedPlanes gated_planes(const Net* n, const float* saved, long long N) {
  return {reinterpret_cast<const uint16_t*>(saved + saved_f32_floats(n, N)),
          reinterpret_cast<uint16_t*>(n->scratch + gated_f32(n, N).scratch_total), gated_b16(n, N), gated_s16(n, N)};
}
// the data-gradient chain's launch parameters, planned for the frame-split kernel (the channel-split plan goes on top)
static int stack_bwd_params(const Net* n, const Call& k, const BwdIo& a, StackBP& bp) {
  const crk_net_desc& d = n->d;
  const long long N = (long long)a.B * a.T;
  const GatedF32 lay = gated_f32(n, N);
  const GatedPlanes q = gated_planes(n, a.saved, N);
  bp = stack_bwd_shape(n, a.B, a.T);
  bp.dS = n->scratch + lay.ds; bp.saved = a.saved; bp.dX0 = n->scratch + lay.dx;
  bp.tb_hi = q.f16 + q.gf.tb_hi; bp.tb_lo = q.f16 + q.gf.tb_lo; bp.sg_hi = q.f16 + q.gf.sg_hi; bp.sg_lo = q.f16 + q.gf.sg_lo;
  bp.gb_hi = q.s16 + q.gs.gb_hi; bp.gb_lo = q.s16 + q.gs.gb_lo; bp.dxb_hi = q.s16 + q.gs.dxb_hi; bp.dxb_lo = q.s16 + q.gs.dxb_lo;
  bp.dsb_hi = q.s16 + q.gs.dsb_hi; bp.dsb_lo = q.s16 + q.gs.dsb_lo;
  bp.dc = (k.want_dc && d.aux_ch > 0) ? a.dc : nullptr; bp.lddc = a.lddc;
  bp.whi = n->whi; bp.wlo = n->wlo; bp.layers = n->d_blayers;
  if (d.dropout > 0.f) { bp.drop_p = d.dropout; bp.drop_seed = k.seed_val; bp.drop_seed_ptr = k.seed_ptr; }
  bp.mask_l0 = d.kind == 1; bp.slope = d.slope;
  return stack_bwd_plan(bp, k.precise);
}
// the chain's launch (split: the channel-split kernel, stack2b_kernels.hip), then the weight gradients of every block in one
// launch over (utterance group, block) and, for crk_net_backward_embed, the table gradient from its per-utterance dG sums
static int stack_bwd_go(const Net* n, const Shape* r, const Call& k, const BwdIo& a, StackBP& bp, bool split) {
  const long long N = (long long)a.B * a.T;
  if (split) { bp.ts_stride = ts_plane_stride(N); RUN(stack2_bwd_plan(bp)); }  // (the route promised the plan)
  // the planes the weight gradient reads after this chain as 4-frame records (StackBP::rec): the channel-split chain only
  bp.rec = (split && N % 4 == 0) ? 1 : 0;
  if (split) RUN(launch_stack2_bwd(bp, a.s));
  else RUN(launch_stack_bwd(bp, k.precise, a.s));
  if (!k.want_w) return CRK_OK;
  const crk_net_desc& d = n->d;
  const GatedPlanes q = gated_planes(n, a.saved, N);
  StackWP wp;
  memset(&wp, 0, sizeof(wp));
  wp.xb_hi = q.f16 + q.gf.xb_hi; wp.xb_lo = q.f16 + q.gf.xb_lo; wp.zb_hi = q.f16 + q.gf.zb_hi; wp.zb_lo = q.f16 + q.gf.zb_lo;
  wp.aux_pad = stack_aux_pad(n);
  if (d.aux_ch > 0) { wp.cb_hi = q.f16 + q.gf.cb_hi; wp.cb_lo = q.f16 + q.gf.cb_lo; }
  wp.gb_hi = bp.gb_hi; wp.gb_lo = bp.gb_lo; wp.dxb_hi = bp.dxb_hi; wp.dxb_lo = bp.dxb_lo;
  wp.dsb_hi = bp.dsb_hi; wp.dsb_lo = bp.dsb_lo;
  wp.layers = r->d_wlayers; wp.partials = n->partials;
  wp.B = a.B; wp.T = a.T; wp.L = n->L; wp.ktaps = d.kernel_size; wp.aux_ch = d.aux_ch > 0 ? d.aux_ch : 0;
  wp.cpg = r->q.cpg_s; wp.G = r->q.Gs;
  wp.rec_g = bp.rec;
  if (a.ce) { wp.usums = n->scratch + usum_off(n, N); wp.nseg = r->q.nseg; }
  RUN(launch_stack_wgrad(wp, k.precise, a.s));
  if (!a.ce) return CRK_OK;
  CondEmbedP ep;
  memset(&ep, 0, sizeof(ep));
  ep.usums = wp.usums; ep.nseg = wp.nseg; ep.cpg = wp.cpg;
  ep.whi = n->whi; ep.wlo = k.precise ? n->wlo : nullptr; ep.layers = n->d_blayers;
  ep.idx = a.ce->idx; ep.run = a.ce->run;
  ep.B = a.B; ep.T = a.T; ep.L = n->L; ep.c0 = a.ce->c0; ep.E = a.ce->E; ep.n_rows = a.ce->n_rows; ep.dtable = a.ce->dtable;
  return launch_cond_embed_bwd(ep, a.s);
}
// weight gradients of first conv + head from the planes
static int gated_plain_wgrad(Net* n, const Shape* r, const Call& k, const BwdIo& a) {
  if (!k.want_w) return CRK_OK;
  const GatedPlanes q = gated_planes(n, a.saved, (long long)a.B * a.T);
  const PwP wp = plain_wgrad_params(n, r, q.s16, q.f16);
  // CRK_FLAG_DEFER_WNORM on a non-precise fused gated backward: parked in pw_shape, not launched - it goes with the
  // weight-norm backward, one launch for all stacks of the model
  if (k.defer_wn && !k.precise) { n->pw_shape = r; n->pw_params = wp; return CRK_OK; }
  return launch_plain_wgrad(r, wp, k.precise, a.s);
}
// generator stacks, plain bf16: the head's and the first conv's data gradients run inside the chain's launch - the
// channel-split chain (split), or the frame-split one at its 8-wave window
static int bwd_folded(Net* n, const Shape* r, const Call& k, const BwdIo& a, bool split) {
  const crk_net_desc& d = n->d;
  const GatedPlanes q = gated_planes(n, a.saved, (long long)a.B * a.T);
  const ConvEntry& ef = n->ents[n->idx_first];
  const ConvEntry& e1 = n->ents[n->idx_last1];
  const ConvEntry& e2 = n->ents[n->idx_last2];
  StackBP bp;
  RUN(stack_bwd_params(n, k, a, bp));
  if (!split && bp.nw != 8) return CRK_ERR_UNSUPPORTED;  // (the route promised the window)
  bp.dy = a.dy; bp.lddy = a.lddy; bp.out_ch = d.out_ch; bp.kp_y = e2.bw_kp;
  bp.w_h2 = e2.bw_off; bp.w_h1 = e1.bw_off; bp.w_first = ef.bw_off;
  bp.hmask_hi = q.f16 + q.gf.head_hi; bp.hb_hi = q.s16 + q.gs.hb_hi; bp.head_scale = (float)sqrt(1.0 / n->L);
  bp.dx = a.dx; bp.lddx = a.lddx; bp.in_ch = d.in_ch; bp.in_rows = ef.bw_rows; bp.dx_scale = a.dx_scale;
  bp.f_h2 = e2.bfr_off; bp.f_h1 = e1.bfr_off; bp.f_first = ef.bfr_off;
  RUN(stack_bwd_go(n, r, k, a, bp, split));
  return gated_plain_wgrad(n, r, k, a);
}
// gated stack, fused and not folded: head, chain (split: the discriminator's channel-split one) and first conv, one launch each
static int bwd_fused(Net* n, const Shape* r, const Call& k, const BwdIo& a, bool split) {
  const long long N = (long long)a.B * a.T;
  const GatedF32 lay = gated_f32(n, N);
  const GatedPlanes q = gated_planes(n, a.saved, N);
  PsP h = ps_base(n, a.B, a.T, a.params);  // head backward: dy -> dH1 -> dS in one launch; dy and dH1 kept as bf16 planes
  h.x = a.dy; h.ldx = a.lddy; h.cin = n->d.out_ch; h.y = n->scratch + lay.ds; h.ldy = 64; h.out_scale = (float)sqrt(1.0 / n->L);
  h.save_hi = q.s16 + q.gs.hb_hi; h.save_lo = q.s16 + q.gs.hb_lo;
  h.mask_hi = q.f16 + q.gf.head_hi; h.L = 2;
  RUN(pstack_go(r, 2, h, k.precise, a.s));
  StackBP bp;
  RUN(stack_bwd_params(n, k, a, bp));
  if (!bp.dS) return CRK_ERR_ARG;
  RUN(stack_bwd_go(n, r, k, a, bp, split));
  if (k.want_dx) {  // first conv: dx through one transposed 1x1
    PsP p = ps_base(n, a.B, a.T, a.params);
    p.x = n->scratch + lay.dx; p.ldx = 64; p.cin = 64; p.y = a.dx; p.ldy = a.lddx; p.out_scale = a.dx_scale; p.L = 1;
    RUN(pstack_go(r, 3, p, k.precise, a.s));
  }
  return gated_plain_wgrad(n, r, k, a);
}
static int bwd_layers(Net* n, const Shape* r, const Call& k, const BwdIo& a) {
  const crk_net_desc& d = n->d;
  const int L = n->L;
  const long long N = (long long)a.B * a.T, P = N * 64;
  const GatedF32 lay = gated_f32(n, N);
  const float *X = a.saved + lay.x, *SKIP = a.saved + lay.skip, *H1 = a.saved + lay.h1;
  float *dS = n->scratch + lay.ds, *dH1 = n->scratch + lay.dh1;
  const int head_act = d.kind == 1 ? ACT_LRELU : ACT_RELU;
  const float sL = (float)sqrt(1.0 / L), rs = 0.70710678118654752440f;
  // head: dy -> dH1 -> dS, each conv's weight gradient in front of its data gradient
  if (k.want_w) RUN(wgrad_conv(n, r, n->idx_last2, a.dy, a.lddy, H1, 64, head_act, 1.f, k.precise));
  ConvP h2 = conv_bw(n, a.B, a.T, n->ents[n->idx_last2], a.dy, a.lddy, dH1, 64);
  h2.dmask = H1; h2.ldm = 64; h2.dmask_act = head_act;
  RUN(conv_go(h2, MODE_PLAIN, k.precise, a.s));
  if (k.want_w) RUN(wgrad_conv(n, r, n->idx_last1, dH1, 64, SKIP, 64, head_act, sL, k.precise));
  ConvP h1 = conv_bw(n, a.B, a.T, n->ents[n->idx_last1], dH1, 64, dS, 64);
  h1.dmask = SKIP; h1.ldm = 64; h1.dmask_act = head_act; h1.out_scale = sL;
  RUN(conv_go(h1, MODE_PLAIN, k.precise, a.s));
  const float* dxo = nullptr;  // gradient wrt the block output; the last block's x output is unused
  for (int l = L - 1; l >= 0; l--) {
    const ConvEntry& ec = n->ents[n->idx_conv[l]];
    const ConvEntry& eo = n->ents[n->idx_out[l]];
    const int dil = n->meta[n->idx_conv[l]].dilation;
    const int off0 = fwd_off0(n, ec.k, dil);
    float* dG = n->scratch + lay.dg + (long long)l * 2 * P;
    {  // gate backward: dz = [dxo*sqrt(.5) | dS] . [Wo;Ws]^T ; dG = gate'(dz)
      ConvP p = base_conv(n, a.B, a.T);
      p.w_hi = n->whi + eo.bw_off; p.w_lo = n->wlo + eo.bw_off;
      p.cin = 128; p.cin_pad = 128; p.cout = 64; p.cout_pad = 64;
      p.xa = dxo; p.lda = 64; p.cinA = 64; p.scaleA = rs;
      p.xb = dS; p.ldb = 64; p.cinB = 64;
      p.ta = a.saved + lay.ta + l * P; p.sb = a.saved + lay.sb + l * P;
      p.y = dG; p.ldy = 128;
      RUN(conv_go(p, MODE_BWDA, k.precise, a.s));
    }
    if (k.want_w) {
      WgradP w = base_wgrad(n, a.B, a.T);  // dilated conv (+ aux as an extra table entry)
      w.a1 = dG; w.lda1 = 128; w.ca1 = 128; w.ca = 128;
      w.x = X + l * P; w.ldx = 64; w.cx = 64;
      if (d.dropout > 0.f) { w.drop_p = d.dropout; w.drop_seed = layer_seed(k.seed_val, l); w.drop_seed_ptr = k.seed_ptr; }
      w.ktaps = ec.k; w.dil = dil; w.off0 = off0;
      wgrad_slots(n, r, n->idx_conv[l], w);
      if (d.aux_ch > 0) {
        const ConvEntry& ea = n->ents[n->idx_aux[l]];
        w.has_aux = 1; w.xc = a.c; w.ldc = a.ldc; w.cc = ea.cin; w.partial_aux = n->partials + r->abs[n->idx_aux[l]].pt_off;
      }
      RUN(wgrad_go(n, w, k.precise));
      WgradP v = base_wgrad(n, a.B, a.T);  // 1x1 out | skip on z
      v.a1 = dxo; v.lda1 = 64; v.ca1 = 64; v.a2 = dS; v.lda2 = 64; v.ca2 = 64; v.ca = 128;
      v.x = a.saved + lay.z + l * P; v.ldx = 64; v.cx = 64;
      wgrad_slots(n, r, n->idx_out[l], v);
      RUN(wgrad_go(n, v, k.precise));
    }
    if (k.want_dc && d.aux_ch > 0) {  // conditioning gradient, accumulated over layers
      const ConvEntry& ea = n->ents[n->idx_aux[l]];
      ConvP p = conv_bw(n, a.B, a.T, ea, dG, 128, a.dc, a.lddc);
      p.accumulate = (l != L - 1);
      RUN(conv_go(p, MODE_PLAIN, k.precise, a.s));
    }
    {  // dX_l = dxo*sqrt(.5) + convT(dG)   (kind 1, l == 0: times LeakyReLU'(X_0))
      float* out = n->scratch + lay.dx + (long long)l * P;
      ConvP p = conv_bw(n, a.B, a.T, ec, dG, 128, out, 64);
      p.ktaps = ec.k; p.dil = dil; p.off0 = -off0 - (ec.k - 1) * dil;
      // conv input was dropout(x): the conv path goes through the regenerated keep mask
      if (d.dropout > 0.f) { p.epi_drop_p = d.dropout; p.epi_drop_seed = layer_seed(k.seed_val, l); p.drop_seed_ptr = k.seed_ptr; }
      if (dxo) { p.res = dxo; p.ldr = 64; p.res_scale = rs; }
      if (l == 0 && d.kind == 1) { p.dmask = X; p.ldm = 64; p.dmask_act = ACT_LRELU; }
      RUN(conv_go(p, MODE_PLAIN, k.precise, a.s));
      dxo = out;
    }
  }
  // first conv
  if (k.want_w) RUN(wgrad_conv(n, r, n->idx_first, dxo, 64, a.x, a.ldx, ACT_NONE, 1.f, k.precise));
  if (!k.want_dx) return CRK_OK;
  ConvP p = conv_bw(n, a.B, a.T, n->ents[n->idx_first], dxo, 64, a.dx, a.lddx);
  p.out_scale = a.dx_scale;
  return conv_go(p, MODE_PLAIN, k.precise, a.s);
}
static int net_backward_impl(void* h, unsigned long long version, int flags, unsigned long long seed, const BwdIo& a) {
  Net* n = (Net*)h;
  if (!n || !a.params || !a.x || !a.dy || a.B <= 0 || a.T <= 0) return CRK_ERR_ARG;
  const Shape* r = find_shape(n, a.B, a.T);
  if (!r) return not_reserved("crk_net_backward");
  const Call k = call_facts(flags, seed, false, a.dy, a.lddy, a.dx, a.lddx, a.dc, a.grads);
  const Route rt = call_route(r, k);
  if (a.ce && !rt.usums) return CRK_ERR_UNSUPPORTED;  // (crk_net_backward_embed)
  if (a.dy_num && !(n->d.kind == 2 && rt.fused)) return CRK_ERR_UNSUPPORTED;  // (crk_net_backward_scaled)
  // CRK_FLAG_FWD_PRECISE: how the forward laid its planes out - unless that forward was the channel-split split-operand one
  // (generator stacks of the bf16x3f mode), which writes the plain route's planes
  const bool expects_x3f = k.mode == 2 && r->route[0].x3f;
  const bool planes_precise = k.precise || (k.mode == 2 && !expects_x3f);
  RUN(check_forward_tag(n, a.saved, a.B, a.T, flags, k.mode, expects_x3f, rt.fused));
  RUN(flush_pending_wnorm(n, a.s));  // a second backward of this net reuses the partial-sum buffer and the gradient planes
  RUN(ensure_prepared(n, a.params, version, a.s));
  n->jobs.clear();
  if (n->d.kind != 2 && !a.saved) return CRK_ERR_ARG;
  int form;
  RUN(bwd_form(n, rt, k, planes_precise, &form));
  switch (form) {
    case BWD_CHAIN: RUN(bwd_chain(n, r, k, a)); break;
    case BWD_CHAIN_LAYERS: RUN(bwd_chain_layers(n, r, k, a)); break;
    case BWD_FOLDED_SPLIT: case BWD_FOLDED: RUN(bwd_folded(n, r, k, a, form == BWD_FOLDED_SPLIT)); break;
    case BWD_FUSED_SPLIT: case BWD_FUSED: RUN(bwd_fused(n, r, k, a, form == BWD_FUSED_SPLIT)); break;
    default: RUN(bwd_layers(n, r, k, a));
  }
  if (k.want_w) {  // every route: the per-layer kernels' queued problems, then partial sums -> dg / dv / dbias
    RUN(wgrad_flush(n, a.B, a.T, k.precise, a.s));
    RUN(finish_wnorm(n, r, a.params, a.grads, k.defer_wn, a.s));
  }
  return CRK_OK;
}
extern "C" int crk_net_backward(void* h, const float* params, unsigned long long version, float* grads, const float* x,
                                int ldx, const float* c, int ldc, const float* dy, int lddy, float* dx, int lddx,
                                float dx_scale, float* dc, int lddc, const float* saved, int B, int T, int flags,
                                unsigned long long seed, void* stream) {
  const BwdIo a = {.params = params, .grads = grads, .x = x, .ldx = ldx, .c = c, .ldc = ldc, .dy = dy, .lddy = lddy, .dx = dx, .lddx = lddx,
                   .dx_scale = dx_scale, .dc = dc, .lddc = lddc, .saved = saved, .B = B, .T = T, .dy_num = nullptr, .dy_den = nullptr, .ce = nullptr,
                   .s = (hipStream_t)stream};
  return net_backward_impl(h, version, flags, seed, a);
}
// crk_net_backward of dy * (dy_num[0] / dy_den[1]), the factor read on the device by the chain's first kernel: the backward
// of a mean cross entropy on the net's output (dy = softmax - onehot, dy_num = upstream gradient, dy_den = {loss, count} as
// crk_ce_fwd leaves them) without a scaling launch in between.  Chains of plain convs only (kind 2, fused path):
// CRK_ERR_UNSUPPORTED otherwise - scale with crk_ce_bwd and call crk_net_backward.
extern "C" int crk_net_backward_scaled(void* h, const float* params, unsigned long long version, float* grads, const float* x,
                                       int ldx, const float* c, int ldc, const float* dy, int lddy, float* dx, int lddx,
                                       float dx_scale, float* dc, int lddc, const float* saved, int B, int T, int flags,
                                       unsigned long long seed, const float* dy_num, const float* dy_den, void* stream) {
  if (!h || !dy_num || !dy_den) return CRK_ERR_ARG;
  const BwdIo a = {.params = params, .grads = grads, .x = x, .ldx = ldx, .c = c, .ldc = ldc, .dy = dy, .lddy = lddy, .dx = dx, .lddx = lddx,
                   .dx_scale = dx_scale, .dc = dc, .lddc = lddc, .saved = saved, .B = B, .T = T, .dy_num = dy_num, .dy_den = dy_den, .ce = nullptr,
                   .s = (hipStream_t)stream};
  return net_backward_impl(h, version, flags, seed, a);
}
// 1: crk_net_backward_embed serves this net at this shape in the arithmetic of `flags` (a gated stack with conditioning on
// the fused kernels); 0: it returns CRK_ERR_UNSUPPORTED - take dc from crk_net_backward and reduce it (crk_embed_bwd_run).
extern "C" int crk_net_embed_grad_supported(void* h, int B, int T, int flags) {
  Net* n = (Net*)h;
  if (!n || B <= 0 || T <= 0) return 0;
  // (a shape that is not reserved: from route_of); the backward of a bf16x3f pair: only where the pair runs fused
  const Route rt[2] = {route_at(n, B, T, false), route_at(n, B, T, true)};
  if (!(flags & CRK_FLAG_PRECISE) && (flags & CRK_FLAG_FWD_PRECISE) && !routes_pair_fused(rt)) return 0;
  return rt[(flags & CRK_FLAG_PRECISE) ? 1 : 0].usums ? 1 : 0;
}
// crk_net_backward for a conditioning input c = [.. | table[idx[u * run]] | ..] whose columns [c0, c0 + E) are one row of an
// embedding table per utterance (run == T: every frame of utterance u carries the label idx[u * run]) and whose other
// columns need no gradient: no per-frame dc.  The weight-gradient launch also leaves the column sums of every block's dG per
// utterance, and one small launch adds  sum_l Waux_l[:, c0:c0+E]^T . sums  of the utterances of each label, in ascending
// utterance order, to dtable [n_rows][E].  Same dx and parameter gradients as crk_net_backward; the table gradient differs
// from the frame sum of dc by fp32 reassociation.  Needs parameter gradients (no CRK_FLAG_NO_PARAM_GRAD).
extern "C" int crk_net_backward_embed(void* h, const float* params, unsigned long long version, float* grads, const float* x,
                                      int ldx, const float* c, int ldc, const float* dy, int lddy, float* dx, int lddx,
                                      float dx_scale, const float* saved, int B, int T, int flags, unsigned long long seed,
                                      const long long* idx, long long run, int c0, int E, int n_rows, float* dtable,
                                      void* stream) {
  Net* n = (Net*)h;
  if (!n || !idx || !dtable || !grads || run != T || c0 < 0 || E < 1 || n_rows < 1 || c0 + E > n->d.aux_ch ||
      (flags & CRK_FLAG_NO_PARAM_GRAD))
    return CRK_ERR_ARG;
  const CondEmbed ce = {idx, run, c0, E, n_rows, dtable};
  const BwdIo a = {.params = params, .grads = grads, .x = x, .ldx = ldx, .c = c, .ldc = ldc, .dy = dy, .lddy = lddy, .dx = dx, .lddx = lddx,
                   .dx_scale = dx_scale, .dc = nullptr, .lddc = 0, .saved = saved, .B = B, .T = T, .dy_num = nullptr, .dy_den = nullptr, .ce = &ce,
                   .s = (hipStream_t)stream};
  return net_backward_impl(h, version, flags, seed, a);
}

__global__ void seed_next_kernel(unsigned long long* state, unsigned long long* out) {
  // splitmix64 of a Weyl sequence: distinct, well-mixed seeds; the per-layer / per-element hashing is dropout_scale's
  unsigned long long z = (*state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  *out = (z ^ (z >> 31)) & 0x3fffffffffffffffull;
}
extern "C" int crk_seed_next(unsigned long long* state, unsigned long long* out, void* stream) {
  if (!state || !out) return CRK_ERR_ARG;
  hipLaunchKernelGGL(seed_next_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, out);
  CRK_CHECK_LAUNCH();
  return CRK_OK;
}

// ---- several nets at once (the sub-nets of a model share one optimizer step) ---------------------------------
// The deferred weight-norm backward of every net that has one pending (crk_net_backward with CRK_FLAG_DEFER_WNORM),
// in ONE launch.  Nets without pending work are skipped.
static int flush_plain_wgrads(int n_nets, void* const* nets, hipStream_t s) {
  // the deferred weight gradients of the plain convs (first conv + head of every stack; every conv of a plain net), one
  // launch: the nets' (layer, group) workgroups side by side, each net with its own depth, taps and group count
  PwMP M; memset(&M, 0, sizeof(M));
  int blocks = 0, max_wa = 0, max_wb = 0, max_tiles = 0, pending = 0;
  double flops = 0.0, bytes = 0.0;
  Net* only = nullptr;
  for (int i = 0; i < n_nets; i++) {
    Net* n = (Net*)nets[i];
    if (!n) return CRK_ERR_ARG;
    if (n->pw_shape) { pending++; only = n; }
  }
  // a plain net on its own keeps the single-net launch (the instantiation for its tile count)
  if (pending == 1 && only->d.kind == 2) return flush_pending_plain_wgrad(only, s);
  for (int i = 0; i < n_nets; i++) {
    Net* n = (Net*)nets[i];
    const Shape* r = n->pw_shape;
    if (!r) continue;
    if (M.n == CRK_MAX_NETS_PW) { RUN(flush_pending_plain_wgrad(n, s)); continue; }
    const PsTables& Tb = r->ps;
    M.q[M.n] = n->pw_params;
    M.first[M.n] = blocks;
    blocks += Tb.nw * n->pw_params.G;
    if (Tb.max_wa > max_wa) max_wa = Tb.max_wa;
    if (Tb.max_wb > max_wb) max_wb = Tb.max_wb;
    if (Tb.max_tiles > max_tiles) max_tiles = Tb.max_tiles;
    flops += Tb.wflops_per_frame * r->B * r->T;
    bytes += 2.0 * (Tb.max_wa + Tb.max_wb) * (double)r->B * r->T * Tb.nw;
    M.n++;
    n->pw_shape = nullptr;
  }
  M.first[M.n] = blocks;
  if (M.n > 0) RUN(launch_pstack_wgrad_multi(M, blocks, max_wa, max_wb, max_tiles, flops, bytes, s));
  return CRK_OK;
}
extern "C" int crk_nets_wnorm_bwd(int n_nets, void* const* nets, void* stream) {
  if (n_nets < 0 || (n_nets > 0 && !nets)) return CRK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  RUN(flush_plain_wgrads(n_nets, nets, s));
  NetRefs R; memset(&R, 0, sizeof(R));
  int total = 0;
  for (int i = 0; i < n_nets; i++) {
    Net* n = (Net*)nets[i];
    if (!n) return CRK_ERR_ARG;
    if (!n->wn_shape) continue;
    if (R.n == CRK_MAX_NETS) {  // more nets than one launch holds: this one goes alone
      RUN(flush_pending_wnorm(n, s));
      continue;
    }
    NetRef& q = R.r[R.n++];
    q.ents = n->wn_shape->d_ents; q.n_ents = (int)n->ents.size(); q.first = total;
    q.params = n->wn_params; q.grads = n->wn_grads; q.partials = n->partials; q.norms = n->norms;
    total += q.n_ents;
    n->wn_shape = nullptr;
  }
  if (R.n == 0) return CRK_OK;
  return launch_wnorm_bwd_multi(R, total, s);
}

// Weight preparation (weight-norm fold + bf16 operand planes) of every net whose parameters changed, in ONE launch;
// what crk_net_forward / crk_net_backward would do one net at a time on their first call after an optimizer step.
// params[i] / versions[i]: the parameter block of nets[i] and its version, as for crk_net_forward (the nets of several
// models: each model counts its own); bump_steps: the Adam step counts of those models.
extern "C" int crk_nets_prepare_models(int n_nets, void* const* nets, const float* const* params,
                                       const unsigned long long* versions, int n_bumps, float* const* bump_steps,
                                       void* stream) {
  if (n_nets < 0 || (n_nets > 0 && (!nets || !params || !versions))) return CRK_ERR_ARG;
  if (n_bumps < 0 || n_bumps > CRK_MAX_BUMPS || (n_bumps > 0 && !bump_steps)) return CRK_ERR_ARG;
  for (int i = 0; i < n_bumps; i++) if (!bump_steps[i]) return CRK_ERR_ARG;
  for (int i = 0; i < n_nets; i++) if (!nets[i] || !params[i]) return CRK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  NetRefs R; memset(&R, 0, sizeof(R));
  int total = 0, nmax = 1;
  for (int i = 0; i < n_nets; i++) {
    Net* n = (Net*)nets[i];
    if (n->prepared_version == versions[i] && n->prepared_params == params[i]) continue;
    if (net_nmax(n) > nmax) nmax = net_nmax(n);
    if (R.n == CRK_MAX_NETS) { RUN(ensure_prepared(n, params[i], versions[i], s)); continue; }
    NetRef& q = R.r[R.n++];
    q.ents = n->d_ents; q.n_ents = (int)n->ents.size(); q.first = total;
    q.params = params[i]; q.whi = n->whi; q.wlo = n->wlo; q.norms = n->norms;
    total += q.n_ents;
    n->prepared_version = versions[i]; n->prepared_params = params[i];
  }
  if (R.n == 0) return n_bumps ? launch_step_bump(bump_steps, n_bumps, s) : CRK_OK;
  for (int i = 0; i < n_bumps; i++) R.bump[i] = bump_steps[i];
  R.n_bump = n_bumps;
  return launch_weight_prep_multi(R, total, nmax, s);
}
// ... of the nets of ONE model: one version, at most one step count
extern "C" int crk_nets_prepare(int n_nets, void* const* nets, const float* const* params, unsigned long long version,
                                float* bump_step, void* stream) {
  if (n_nets < 0 || (n_nets > 0 && (!nets || !params))) return CRK_ERR_ARG;
  const std::vector<unsigned long long> versions((size_t)n_nets + 1, version);
  return crk_nets_prepare_models(n_nets, nets, params, versions.data(), bump_step ? 1 : 0, &bump_step, stream);
}
