// The library's process-wide host side: the A/B switches, the per-kernel-class HIP-event timing, the cache-flush
// measurement aid and the version string.
#include "runtime.h"

#include <vector>

#include "../../include/crank_hip.h"

static int sw_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
const CrkSwitches& crk_sw() {
  static const CrkSwitches s = [] {
    CrkSwitches v;
    v.sk_v = sw_int("CRK_SK_V", 2); v.skb_v = sw_int("CRK_SKB_V", 2); v.ps_v = sw_int("CRK_PS_V", 2);
    v.no_fuse = sw_int("CRK_NO_FUSE", 0); v.s2x = sw_int("CRK_S2X", 1); v.disc_split = sw_int("CRK_DISC_SPLIT", 1);
    v.s2_cfg = sw_int("CRK_S2_CFG", 0);
    const int nw = sw_int("CRK_SK_NW", 0);
    v.sk_nw_fwd = nw > 10 ? nw / 10 : nw; v.sk_nw_bwd = nw > 10 ? nw % 10 : nw;
    v.ps_nw = sw_int("CRK_PS_NW", 0);
    v.wg_groups = sw_int("CRK_WG_GROUPS", 32); if (v.wg_groups < 1) v.wg_groups = 32;
    v.wg_cpg = sw_int("CRK_WG_CPG", 0); v.wg_fill = sw_int("CRK_WG_FILL", 1) != 0;
    v.vq_f16 = sw_int("CRK_VQ_F16", 1) != 0; v.vq_lc = sw_int("CRK_VQ_LC", 2); v.logmel_wave = sw_int("CRK_LOGMEL_WAVE", 1);
    return v;
  }();
  return s;
}

// ------------------------------------------------------------------------------
// optional per-kernel-class timing with HIP events on the launch stream (bench.py's
// roofline leg; the classes: runtime.h)
// ------------------------------------------------------------------------------
struct ProfClass {
  std::vector<hipEvent_t> ev;  // start/stop pairs
  size_t used = 0;
  double flops = 0.0;
  double bytes = 0.0;  // algorithmic HBM bytes (what the launch must move: DESIGN.md section 3)
};
static bool g_prof = false;
static ProfClass g_pc[CRK_PROF_CLASSES];

// Measurement aid (crk_debug_flush_before): a read-modify-write pass over a private buffer larger than the 256 MiB Infinity
// Cache in front of every profiled conv kernel, so that nothing its producer left in a cache is still there - the A/B that
// separates what a kernel reads from HBM from what it reads out of the last-level cache.
static long long g_flush_bytes = 0;
static float* g_flush_buf = nullptr;
static long long g_flush_cap = 0;
__global__ void cache_flush_kernel(float4* buf, long long n16) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x) {
    float4 v = buf[i];
    v.x += 1.f;
    buf[i] = v;
  }
}
extern "C" int crk_debug_flush_before(long long bytes) {
  if (bytes < 0) return CRK_ERR_ARG;
  if (bytes > g_flush_cap) {
    if (g_flush_buf) (void)hipFree(g_flush_buf);
    g_flush_buf = nullptr; g_flush_cap = 0;
    if (hipMalloc(&g_flush_buf, (size_t)bytes) != hipSuccess) return CRK_ERR_HIP;
    if (hipMemset(g_flush_buf, 0, (size_t)bytes) != hipSuccess) return CRK_ERR_HIP;
    g_flush_cap = bytes;
  }
  g_flush_bytes = bytes;
  return CRK_OK;
}
void conv_prof_begin(int cls, double flops, hipStream_t s) {
  if (g_flush_bytes > 0) hipLaunchKernelGGL(cache_flush_kernel, dim3(2048), dim3(256), 0, s, reinterpret_cast<float4*>(g_flush_buf), g_flush_bytes / 16);
  if (!g_prof) return;
  ProfClass& c = g_pc[cls];
  if (c.used + 2 > c.ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    c.ev.push_back(a); c.ev.push_back(b);
  }
  (void)hipEventRecord(c.ev[c.used], s);
  c.flops += flops;
}
void conv_prof_end(int cls, hipStream_t s) {
  if (!g_prof) return;
  ProfClass& c = g_pc[cls];
  if (c.used + 2 > c.ev.size()) return;
  (void)hipEventRecord(c.ev[c.used + 1], s);
  c.used += 2;
}
void conv_prof_bytes(int cls, double bytes) { if (g_prof) g_pc[cls].bytes += bytes; }
extern "C" int crk_prof_enable(int on) {
  g_prof = on != 0;
  if (on) for (auto& c : g_pc) { c.used = 0; c.flops = 0.0; c.bytes = 0.0; }
  return CRK_OK;
}
// summed algorithmic HBM bytes of one class since crk_prof_enable(1)
extern "C" int crk_prof_report_bytes(int cls, double* total_bytes) {
  if (cls < 0 || cls >= CRK_PROF_CLASSES || !total_bytes) return CRK_ERR_ARG;
  *total_bytes = g_pc[cls].bytes;
  return CRK_OK;
}
// synchronises on the recorded events; returns launches, summed kernel time and the
// summed algorithmic FLOPs of one class since crk_prof_enable(1)
extern "C" int crk_prof_report(int cls, long long* count, double* total_ms, double* total_flops) {
  if (cls < 0 || cls >= CRK_PROF_CLASSES || !count || !total_ms || !total_flops) return CRK_ERR_ARG;
  ProfClass& c = g_pc[cls];
  double ms = 0.0;
  for (size_t i = 0; i + 1 < c.used; i += 2) {
    if (hipEventSynchronize(c.ev[i + 1]) != hipSuccess) return CRK_ERR_HIP;
    float t = 0.f;
    if (hipEventElapsedTime(&t, c.ev[i], c.ev[i + 1]) != hipSuccess) return CRK_ERR_HIP;
    ms += t;
  }
  *count = (long long)(c.used / 2); *total_ms = ms; *total_flops = c.flops;
  return CRK_OK;
}

int crk_zero_stream_rows(void* base, size_t bytes_per_stream, int S, const int* ids, int n, hipStream_t stream) {
  if (!base || n < 0) return CRK_ERR_ARG;
  if (!ids) return hipMemsetAsync(base, 0, bytes_per_stream * S, stream) == hipSuccess ? CRK_OK : CRK_ERR_HIP;
  for (int i = 0; i < n; i++)
    if (ids[i] < 0 || ids[i] >= S) return CRK_ERR_ARG;
  for (int i = 0; i < n; i++)
    if (hipMemsetAsync((char*)base + (size_t)ids[i] * bytes_per_stream, 0, bytes_per_stream, stream) != hipSuccess)
      return CRK_ERR_HIP;
  return CRK_OK;
}

extern "C" const char* crk_version(void) { return "crank_hip 0.1 (gfx950)"; }
