// Host-side launch helpers shared by every kernel family: the dynamic-LDS opt-in, the persistent-grid rule and the reader of
// the environment switches (env_int.h).  The state of the first two (one grant table, one CU count per device, one call
// counter) lives in launch.hip.
#pragma once
#include "env_int.h"
#include "ipdm_common.h"

// Raises hipFuncAttributeMaxDynamicSharedMemorySize of `kernel` on the CURRENT device to `bytes` unless that much was granted
// there before (lds_table.h); requests of at most 64 KiB cost nothing.  The attribute is per device, so every launch above
// 64 KiB goes through here, at the launch site of the instantiation it launches: the steady state is one hipGetDevice and
// one table lookup, no HIP call that touches the kernel.  The FIRST launch of an instantiation on a device makes the
// hipFuncSetAttribute call, and that launch may sit inside a hipGraph capture (it has no stream and is not captured; the
// k-space kernels have always made it there).  Returns IPDM_OK or the HIP error; callers pass it on.
int ipdm_lds_optin_ptr(const void* kernel, size_t bytes);
template <typename K>
static inline int ipdm_lds_optin(K kernel, size_t bytes) {
  return ipdm_lds_optin_ptr(reinterpret_cast<const void*>(kernel), bytes);
}

// Grid of a persistent kernel that walks `nblk` tiles: 8 x min(ceil(nblk / 8), CUs / 8) workgroups -- the same count on each of
// the 8 XCDs (workgroups go to XCDs round-robin), at most one per CU.  The CU count is the current device's, asked once per
// device; 256 (MI355X) when the query fails or reports fewer than 8.
unsigned ipdm_persistent_grid(int64_t nblk);

// opt-in, launch, launch status
template <typename... Params, typename... Args>
static inline int ipdm_launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args) {
  const int rc = ipdm_lds_optin(kernel, lds);
  if (rc != IPDM_OK) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  return ipdm_launch_status();
}
