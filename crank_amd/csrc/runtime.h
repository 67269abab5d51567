// What every kernel family's host side shares (runtime.hip): the process switches, the per-class HIP-event timing of
// bench.py's roofline leg, the dynamic-LDS limit helper, the streaming families' reset and the allocation counter.
#pragma once
#include "common.h"
#include "switches.h"

// Timing classes, one per kernel: 0 conv_tile_kernel (generic per-layer conv, all modes), 1 stack_fwd_kernel,
// 2 stack_bwd_kernel, 3 wgrad_kernel (table), 4 pstack_kernel, 5 stack_wgrad_kernel, 6 pstack_wgrad_kernel (0-6: crank_hip.h);
// 7 the VQ search; 8 the on-the-fly log-mel kernel.  A launcher brackets its launch with begin / end; they record
// nothing unless crk_prof_enable(1) ran; begin also puts the cache flush of crk_debug_flush_before in front, where one is set.
#define CRK_PROF_CLASSES 9
void conv_prof_begin(int cls, double flops, hipStream_t s);
void conv_prof_end(int cls, hipStream_t s);
void conv_prof_bytes(int cls, double bytes);  // algorithmic HBM bytes (what the launch must move: DESIGN.md section 3)

// Raises the dynamic-LDS limit of a group of kernel instantiations to `bytes`, all of them on the first call that reaches the
// statement and never again (one flag per call site and process; a steady-state launch pays one load of it).  Leaves the
// enclosing launcher with CRK_ERR_HIP where the runtime refuses.
template <typename... K>
inline int crk_raise_lds(int bytes, K*... kernels) {
  for (const void* f : {(const void*)kernels...})
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return CRK_ERR_HIP;
  return CRK_OK;
}
#define CRK_RAISE_LDS_ONCE(bytes, ...)                                        \
  {                                                                           \
    static bool lds_raised_ = false;                                          \
    if (!lds_raised_) {                                                       \
      if (crk_raise_lds(bytes, __VA_ARGS__) != CRK_OK) return CRK_ERR_HIP;    \
      lds_raised_ = true;                                                     \
    }                                                                         \
  }

// The reset of every streaming family: zeroes row i (bytes_per_stream bytes) of `base` for every i of the host array ids
// [n], or all S rows where ids is null.  Every id is checked before the first memset: CRK_ERR_ARG for one outside 0 .. S-1,
// nothing zeroed.
int crk_zero_stream_rows(void* base, size_t bytes_per_stream, int S, const int* ids, int n, hipStream_t stream);

long long crk_count_alloc_(void);  // net.hip: the allocation counter behind crk_debug_alloc_count
