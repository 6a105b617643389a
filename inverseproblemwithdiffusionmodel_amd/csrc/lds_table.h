// The dynamic-LDS grants of a process, per (kernel, device): plain C++, no HIP in it (tests/host/lds_table_main.cpp drives it
// from host threads).  launch.h puts hipFuncSetAttribute behind the one process-wide table.
#pragma once
#include <stddef.h>
#include <map>
#include <mutex>
#include <utility>
#include "ipdm.h"

// a kernel may use this much dynamic LDS without asking
constexpr size_t IPDM_LDS_DEFAULT_LIMIT = 64 * 1024;

class IpdmLdsTable {
 public:
  // Makes sure `kernel` may be launched with `bytes` of dynamic LDS on device `dev`.  Requests within the default limit or
  // within what this (kernel, device) was granted before return IPDM_OK at once; otherwise `set(bytes)` runs under the table's
  // lock (two threads never raise one kernel's limit at the same time, and a smaller request never overtakes a larger one), a
  // successful grant is remembered, and set's value comes back unchanged.
  template <class Set>
  int ensure(const void* kernel, int dev, size_t bytes, Set&& set) {
    if (bytes <= IPDM_LDS_DEFAULT_LIMIT) return IPDM_OK;
    std::lock_guard<std::mutex> lock(mutex_);
    const auto key = std::make_pair(kernel, dev);
    const auto it = granted_.find(key);
    if (it != granted_.end() && bytes <= it->second) return IPDM_OK;
    const int rc = set(bytes);
    if (rc == IPDM_OK) granted_[key] = bytes;
    return rc;
  }

 private:
  std::mutex mutex_;
  std::map<std::pair<const void*, int>, size_t> granted_;
};
