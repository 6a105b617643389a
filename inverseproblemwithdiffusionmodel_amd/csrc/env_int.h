// The one reader of the IPDM_* environment switches: plain C++, no HIP in it (tests/host/wino_plan_main.cpp reads a switch
// from host threads).  A call site keeps its value in `static const int v = ipdm_env_int("IPDM_...", dflt);` -- read once per
// process, and the initialisation of a function-local static is thread-safe (C++11).
#pragma once
#include <stdlib.h>

// atoi(value) when `name` is set (an empty string gives 0), `dflt` when it is not
inline int ipdm_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
