// diffspectra_amd - the host side that every source's entry points share: the launch-status rule, the bare-layout check, and the
// small wrappers around stream calls and kernel attributes.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <initializer_list>

#include "../../include/diffspectra_hip.h"

// The whole library's launch-status rule: an entry point returns this after its last launch.
#define DST_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? DS_OK : DS_ERR_LAUNCH)

namespace dst {

// What the entry points that take a bare layout require of it (their kernels stage <= 32 node indices of a molecule in LDS)
inline bool layout_ok(const ds_layout* L) { return L && L->B > 0 && L->max_n <= DS_MAX_ATOMS && L->max_n <= L->N; }

inline bool clear(void* p, size_t bytes, hipStream_t s) { return hipMemsetAsync(p, 0, bytes, s) == hipSuccess; }
inline bool record(hipEvent_t ev, hipStream_t s) { return hipEventRecord(ev, s) == hipSuccess; }
inline bool wait(hipStream_t s, hipEvent_t ev) { return hipStreamWaitEvent(s, ev, 0) == hipSuccess; }

// true when every pointer is 16-byte aligned (NULL counts as aligned: whether a pointer may be NULL is the caller's check)
inline bool all_aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

// Lets `kernel` request `bytes` of dynamic LDS on the current device.  The attribute is per device, so `done` (one static per call
// site) remembers the devices it has been set on; two threads may both set it, which is harmless.  false: the runtime refused.
template <typename Kernel>
bool allow_dynamic_lds(std::atomic<uint64_t>& done, Kernel* kernel, size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const uint64_t bit = dev >= 0 && dev < 64 ? uint64_t(1) << dev : 0;     // (beyond 64 devices: set on every launch)
  if (done.load(std::memory_order_acquire) & bit) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  done.fetch_or(bit, std::memory_order_release);
  return true;
}

// ds_gemm of a->M rows through the tile form that a launch of route_rows >= a->M rows would take (ds_gemm.hip): the rows then carry
// the bits they have inside that larger launch.  The uniform step prologue runs its one time-MLP row this way.
int gemm_routed_as(const ds_gemm_args* a, int route_rows, void* stream);

}  // namespace dst
