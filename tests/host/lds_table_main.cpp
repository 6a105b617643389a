// Stand-alone check of IpdmLdsTable (csrc/lds_table.h; no HIP): built and run by tests/test_lds_table.py, and the program to run
// under -fsanitize=thread / address,undefined.  Exit status 0 and "ok" on success; the first failed check otherwise.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <thread>
#include <utility>
#include <vector>
#include "lds_table.h"

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

int main() {
  constexpr size_t KiB = 1024;
  const size_t requests[] = {32 * KiB, 70 * KiB, 150 * KiB, 70 * KiB, 150 * KiB};
  const int devices[] = {0, 1, 1000};             // no fixed device bound
  static const char fake_kernels[4] = {};

  // 8 threads x 4 kernels x 3 devices: set() runs under the table's lock, so the log needs none of its own
  IpdmLdsTable table;
  std::map<std::pair<const void*, int>, std::vector<size_t>> log;
  std::vector<std::thread> threads;
  for (int t = 0; t < 8; ++t)
    threads.emplace_back([&] {
      for (const char& k : fake_kernels)
        for (int dev : devices)
          for (size_t bytes : requests)
            CHECK(table.ensure(&k, dev, bytes, [&](size_t n) {
              log[{&k, dev}].push_back(n);
              return IPDM_OK;
            }) == IPDM_OK);
    });
  for (std::thread& th : threads) th.join();
  CHECK(log.size() == 4 * 3);
  for (const auto& entry : log) CHECK((entry.second == std::vector<size_t>{70 * KiB, 150 * KiB}));   // twice, never for 32 KiB

  // a failed set() is not recorded: the same request asks again, and the error comes back unchanged
  IpdmLdsTable failing;
  int calls = 0;
  const auto set = [&](size_t) { return ++calls == 1 ? 719 : IPDM_OK; };
  CHECK(failing.ensure(fake_kernels, 0, 70 * KiB, set) == 719 && calls == 1);
  CHECK(failing.ensure(fake_kernels, 0, 70 * KiB, set) == IPDM_OK && calls == 2);
  CHECK(failing.ensure(fake_kernels, 0, 70 * KiB, set) == IPDM_OK && calls == 2);
  CHECK(failing.ensure(fake_kernels, 0, 64 * KiB, set) == IPDM_OK && calls == 2);     // the default limit itself never asks
  std::puts("ok");
  return 0;
}
