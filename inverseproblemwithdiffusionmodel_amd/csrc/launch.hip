// The process-wide state behind launch.h.
#include "launch.h"
#include <atomic>
#include <map>
#include <mutex>
#include "lds_table.h"

namespace {
IpdmLdsTable lds_table;
std::atomic<int64_t> optin_calls{0};

std::mutex cu_mutex;
std::map<int, int> xcd_cus;                  // device -> CUs / 8
}  // namespace

int ipdm_lds_optin_ptr(const void* kernel, size_t bytes) {
  if (bytes <= IPDM_LDS_DEFAULT_LIMIT) return IPDM_OK;
  int dev = 0;
  const hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  return lds_table.ensure(kernel, dev, bytes, [kernel](size_t n) {
    ++optin_calls;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n);
    return e == hipSuccess ? IPDM_OK : (int)e;
  });
}

unsigned ipdm_persistent_grid(int64_t nblk) {
  int dev = 0;
  int per_xcd = 32;                              // MI355X: 256 CUs in 8 XCDs
  if (hipGetDevice(&dev) == hipSuccess) {
    std::lock_guard<std::mutex> lock(cu_mutex);
    int& cached = xcd_cus[dev];
    if (!cached) {
      int cus = 0;
      const bool ok = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus >= 8;
      cached = ok ? cus / 8 : 32;
    }
    per_xcd = cached;
  }
  const int64_t want = (nblk + 7) / 8;
  return (unsigned)(8 * (want < per_xcd ? want : per_xcd));
}

extern "C" int64_t ipdm_debug_lds_optin_count(void) { return optin_calls.load(); }
