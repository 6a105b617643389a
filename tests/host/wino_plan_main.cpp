// Stand-alone check of the 2-D Winograd launch plan and the switch reader (csrc/wino_plan.h, env_int.h; no HIP): built and run by
// tests/test_wino_plan.py, and the program to run under -fsanitize=thread / address,undefined.  Exit status 0 and "ok" on success;
// the first failed check otherwise.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include "wino_plan.h"

using namespace ipdm_conv;

static WinoShape g_shape;       // the input under test, for the failure message
static int g_setting = 0;
#define CHECK(cond)                                                                                                          \
  do {                                                                                                                       \
    if (!(cond)) {                                                                                                           \
      std::fprintf(stderr, "%s:%d: %s\n  at B %d Cin %d Cout %d H %d W %d dil %d hx %d pool2 %d stats %d x16 %d, switch setting %d\n", \
                   __FILE__, __LINE__, #cond, g_shape.B, g_shape.Cin, g_shape.Cout, g_shape.H, g_shape.W, g_shape.dil, g_shape.hx,     \
                   g_shape.pool2, g_shape.stats, g_shape.x16, g_setting);                                                    \
      std::exit(1);                                                                                                          \
    }                                                                                                                        \
  } while (0)

// what the kernels' own static_asserts and argument contracts ask of a plan that says IPDM_OK
static void check_plan(const WinoShape& s, const WinoPlan& p) {
  CHECK(p.nblk == (int64_t)s.B * p.tiles_x * p.tiles_y * p.co_tiles && p.nblk > 0 && p.nblk <= 0x7fffffff);
  CHECK(p.form != WINO_KSPLIT);
  if (p.form == WINO_CO32 || p.form == WINO_HALF) CHECK(s.hx);                                     // f16x2 only
  if (p.form == WINO_CO32 || p.form == WINO_HALF || p.form == WINO_POLY) CHECK(p.dma4 && !p.pool && !p.stats);
  if (p.form == WINO_HALF) CHECK(s.H == 16 && s.W == 16 && p.tiles_x == 1 && p.tiles_y == 2);
  if (p.form == WINO_CO32) CHECK(p.co_tiles * 32 == s.Cout);
  if (p.form != WINO_CO32) CHECK(p.co_tiles * 64 == s.Cout);
  if (p.stats) CHECK(p.form == WINO_WIDE && p.dma4);
  if (p.pool) CHECK(p.form == WINO_WIDE);
  if (p.dma4) CHECK(s.x16 && (p.form == WINO_POLY || s.W % 4 == 0));                               // 16-byte DMA: aligned quads
  CHECK(p.pool == s.pool2 && p.stats == s.stats);                                                  // no epilogue is dropped quietly
  if (p.form == WINO_SMALL_REG || p.form == WINO_SMALL_DMA) CHECK(wino_small(s));
  if (p.form == WINO_TILE || p.form == WINO_WIDE) CHECK(!wino_small(s));
}

int main() {
  // ---- the switch reader: read once, the same value in every thread ----
  unsetenv("IPDM_WBX3_POLY");
  setenv("IPDM_WBX3_SMALL_MIN", "77", 1);
  setenv("IPDM_WBX3_HALF", "", 1);
  CHECK(ipdm_env_int("IPDM_WBX3_POLY", 5) == 5 && ipdm_env_int("IPDM_WBX3_SMALL_MIN", 5) == 77 && ipdm_env_int("IPDM_WBX3_HALF", 5) == 0);
  int seen[8] = {};
  std::vector<std::thread> threads;
  for (int t = 0; t < 8; ++t) threads.emplace_back([&seen, t] { seen[t] = wino_switches().small_min; });
  for (std::thread& th : threads) th.join();
  for (int t = 0; t < 8; ++t) CHECK(seen[t] == 77);
  setenv("IPDM_WBX3_SMALL_MIN", "78", 1);
  CHECK(wino_switches().small_min == 77 && wino_switches().half == 0 && wino_switches().poly == 1);   // once per process

  // ---- the plan over the grid of tests/test_conv_plan_host.py x batch x epilogue x alignment x every single switch ----
  const int cins[] = {8, 16, 24, 32, 64, 256, 512}, couts[] = {32, 64, 128, 192, 256, 512};
  const int sides[] = {4, 6, 8, 12, 14, 16, 18, 24, 32, 48, 64, 128}, batches[] = {1, 2, 28, 160, 4096};
  std::vector<WinoSwitches> settings(9);
  settings[1].persist = 0; settings[2].poly = 0; settings[3].co32 = 0; settings[4].half = 0; settings[5].dma4 = 0;
  settings[6].ksplit = 0; settings[7].small_min = 0; settings[8].small_min = 1 << 30;
  long served = 0, forms[8] = {};
  for (g_setting = 0; g_setting < (int)settings.size(); ++g_setting) {
    const WinoSwitches& sw = settings[g_setting];
    for (int Cin : cins) for (int Cout : couts) for (int H : sides) for (int W : sides) for (int dil = 1; dil <= 5; ++dil) {
      for (int B : batches) for (int flags = 0; flags < 16; ++flags) {
        const WinoShape s = {B, Cin, Cout, H, W, dil, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0};
        g_shape = s;
        const WinoPlan p = wino_bx3_plan(s, sw);
        CHECK(p.rc == IPDM_OK || p.rc == IPDM_EUNSUPPORTED);
        if (p.rc != IPDM_OK) continue;
        CHECK(wino_bx3_shape_ok(s));
        check_plan(s, p);
        ++served;
        ++forms[p.form];
        // the split-K call: K halves of the shapes its rule names, 16-byte aligned input only
        const int ks = wino_bx3_ksplit_for(Cin, Cout, H, W, dil, sw);
        const WinoPlan k = wino_bx3_ksplit_plan(s, sw, 2);
        CHECK((k.rc == IPDM_OK) == (ks == 2 && s.x16));
        if (k.rc == IPDM_OK) CHECK(k.form == WINO_KSPLIT && k.dma4 && k.nblk == 2 * (int64_t)B * k.tiles_x * k.tiles_y * k.co_tiles);
        CHECK(wino_bx3_ksplit_plan(s, sw, 1).rc != IPDM_OK && wino_bx3_ksplit_plan(s, sw, 3).rc != IPDM_OK);
      }
      // the queries: the form of the f16x2 family's plain call ...
      const WinoShape q = wino_query_shape(Cin, Cout, H, W, dil, true, false, false);
      g_shape = q;
      const WinoPlan p = wino_bx3_plan(q, sw);
      const int form = wino_hx2_form(Cin, Cout, H, W, dil, sw);
      if (p.rc != IPDM_OK) CHECK(form == IPDM_EUNSUPPORTED && !wino_bx3_shape_ok(q));
      else CHECK(form == (p.form == WINO_POLY ? IPDM_WINO_FORM_POLY : p.form == WINO_HALF ? IPDM_WINO_FORM_HALF
                          : p.form == WINO_CO32 ? IPDM_WINO_FORM_CO32 : IPDM_WINO_FORM_OTHER));
      // ... and the statistics partials: served exactly where the plan serves the request with the DMA4 switch taken as on,
      // which is the closed form the query had before there was a plan
      WinoSwitches on = sw;
      on.dma4 = 1;
      for (int pool = 0; pool < 2; ++pool) {
        const WinoShape qs = wino_query_shape(Cin, Cout, H, W, dil, false, pool != 0, true);
        g_shape = qs;
        const WinoPlan ps = wino_bx3_plan(qs, on);
        const int partials = wino_stats_partials(Cin, Cout, H, W, dil, pool, sw);
        CHECK((partials > 0) == (ps.rc == IPDM_OK));
        const bool closed = wino_bx3_shape_ok(qs) && !wino_small(qs) && sw.persist && Cin >= 32 && W % 4 == 0 && !(pool && (H % 2 || W % 2));
        CHECK(partials == (closed ? 2 * ((W + 31) / 32) * ((H + 7) / 8) : 0));
      }
    }
  }
  for (int f = WINO_POLY; f <= WINO_WIDE; ++f) CHECK(forms[f] > 0);      // the sweep reached every form of the plain call
  CHECK(served > 0 && forms[WINO_KSPLIT] == 0);
  std::puts("ok");
  return 0;
}
