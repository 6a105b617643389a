// Which instantiation of the 2-D Winograd kernels (conv_wino_bx3.hip) serves a layer, as a function of the layer shape, the
// operand family, the epilogue, the input's alignment and the IPDM_WBX3_* switches: plain C++, no HIP in it
// (tests/host/wino_plan_main.cpp sweeps it on the host).  The launcher switches on the plan and the shape queries of the C ABI
// (_supported, _splitk, _hx2_form, _stats_partials) read the same plan, so a query cannot say anything else than what runs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "env_int.h"
#include "ipdm.h"

namespace ipdm_conv {

constexpr int X_KC = 16;                 // input channels per chunk (one bf16 MFMA k-step)
constexpr int X_CO = 64;                 // output channels per workgroup (CO32: 32)
constexpr int X_TX = 16, X_TY = 4;       // tiles of 2 x 2 output pixels per workgroup
constexpr int X_TILES = X_TX * X_TY;     // 64

// the IPDM_WBX3_* switches (tuning / fallback; all default to "on"), read once per process
struct WinoSwitches {
  int persist = 1;       // IPDM_WBX3_PERSIST=0: one workgroup per tile
  int poly = 1;          // IPDM_WBX3_POLY=0: dilated 16 x 16 images on the register-staged kernel
  int co32 = 1;          // IPDM_WBX3_CO32=0: no 32-channel workgroups
  int half = 1;          // IPDM_WBX3_HALF=0: CO32 where HALF would run
  int dma4 = 1;          // IPDM_WBX3_DMA4=0: dword LDS-DMA everywhere
  int ksplit = 1;        // IPDM_WBX3_KSPLIT=0: no split-K form
  int small_min = 160;   // IPDM_WBX3_SMALL_MIN: (image, channel tile) pairs from which the 8 x 8 block form runs
};
inline const WinoSwitches& wino_switches() {
  static const WinoSwitches sw = {ipdm_env_int("IPDM_WBX3_PERSIST", 1), ipdm_env_int("IPDM_WBX3_POLY", 1),
                                  ipdm_env_int("IPDM_WBX3_CO32", 1),    ipdm_env_int("IPDM_WBX3_HALF", 1),
                                  ipdm_env_int("IPDM_WBX3_DMA4", 1),    ipdm_env_int("IPDM_WBX3_KSPLIT", 1),
                                  ipdm_env_int("IPDM_WBX3_SMALL_MIN", 160)};
  return sw;
}

struct WinoShape {
  int B, Cin, Cout, H, W, dil;
  bool hx;               // f16x2 operands (else bf16x3)
  bool pool2, stats;     // the epilogue asked for
  bool x16;              // the input is 16-byte aligned (the launcher: from the pointer; shape queries: true)
};

// one value per family of instantiations
enum WinoForm {
  WINO_POLY,             // wide_kernel<., 8, 8, POLY>: dilated 16 x 16 images on the polyphase tile space
  WINO_HALF,             // wide_kernel<true, 8, 4, HALF>: (image, upper / lower eight rows, 64 channels) workgroups
  WINO_CO32,             // wide_kernel<true, 8, 8, CO32>: 32-channel workgroups
  WINO_SMALL_DMA,        // wide_kernel<., 8, 8>: an 8 x 8 tile block per image
  WINO_SMALL_REG,        // kernel<., true>: 64 tiles of the linear (polyphase) tile space, register-staged
  WINO_TILE,             // kernel<., false>: one workgroup per 16 x 4 tile block
  WINO_WIDE,             // wide_kernel<., 16, 4>: persistent, 16 x 4 tile blocks; the pooled and the statistics epilogue
  WINO_KSPLIT            // wide_kernel<., 8, 8, KSP>: K parts of the 8 x 8 form (wino_bx3_ksplit_plan only)
};

struct WinoPlan {
  int rc;                // IPDM_OK, or IPDM_EUNSUPPORTED: no form serves this (the other members then mean nothing)
  WinoForm form;
  bool dma4, pool, stats;   // template arguments of the form: 16-byte LDS-DMA, pooled epilogue, statistics epilogue
  int tiles_x, tiles_y, co_tiles;
  int64_t nblk;          // workgroup-sized pieces of work: the grid, or what a persistent grid walks
};

inline bool wino_small(const WinoShape& s) { return s.W < 32 || s.dil > 1; }

// the layer shapes the kernels serve at all (3 x 3 taps, no fused input normalisation: the caller's business)
inline bool wino_bx3_shape_ok(const WinoShape& s) {
  if (!(s.Cin % X_KC == 0 && s.Cout % X_CO == 0)) return false;
  if (s.dil < 1 || s.dil > 4) return false;
  // buffer descriptors: the tensor must end below the padding marker (2^29 + 2^29 register path, 2^30 DMA path)
  if ((size_t)s.B * s.Cin * s.H * s.W * 4 >= (wino_small(s) ? 0x1fffffffull : 0x3fffffffull)) return false;
  if (wino_small(s)) return s.H % (2 * s.dil) == 0 && s.W % (2 * s.dil) == 0 && (s.H * s.W) / 4 >= 32;
  return s.H % 2 == 0 && s.W % 2 == 0 && s.H >= 8;
}

// K parts that pay for a layer shape (a function of the SHAPE only, so that a sample's bits do not depend on its batch):
// undilated images of at most 16 x 16 pixels with fewer than 512 output channels -- (image, channel tile) pairs alone fill
// under half of the chip at the production batch -- run as two K halves when each half keeps at least two chunks
inline int wino_bx3_ksplit_for(int Cin, int Cout, int H, int W, int dilation, const WinoSwitches& sw) {
  if (!sw.ksplit || !sw.persist) return 1;
  if (dilation != 1 || W > 16 || H > 16 || W % 4 || H % 2 || Cout % X_CO || Cout >= 512) return 1;
  if (Cin % (2 * X_KC) || Cin / X_KC < 4) return 1;
  return 2;
}

inline WinoPlan wino_bx3_plan(const WinoShape& s, const WinoSwitches& sw) {
  WinoPlan p = {IPDM_EUNSUPPORTED, WINO_TILE, false, false, false, 0, 0, 0, 0};
  if (!wino_bx3_shape_ok(s)) return p;
  const bool small = wino_small(s), persist = sw.persist != 0;
  const bool deep = s.Cin >= 2 * X_KC;            // the persistent kernels run at least two chunks
  p.co_tiles = s.Cout / X_CO;
  // 16-pixel layers with fewer than 512 output channels: the shapes whose split-K rule says 2 (the f16x2 family's PLAIN call
  // then runs them as twice the workgroups, one launch instead of two K halves + a reduction)
  const bool co32 = sw.co32 && s.hx && s.dil == 1 && s.W <= 16 && s.H <= 16 && s.W % 4 == 0 && s.H % 2 == 0 && deep &&
                    s.Cout < 512 && !s.pool2 && !s.stats;
  if (sw.poly && persist && s.dil > 1 && s.H == 16 && s.W == 16 && 16 % (2 * s.dil) == 0 && deep && !s.pool2 && !s.stats && s.x16) {
    p.form = WINO_POLY;                           // first, for both operand families
    p.dma4 = true;
    p.tiles_x = p.tiles_y = 1;
  } else if (s.hx && small && persist && co32 && s.x16) {
    p.dma4 = true;
    if (sw.half && s.W == 16 && s.H == 16) {
      p.form = WINO_HALF;
      p.tiles_x = 1;
      p.tiles_y = 2;
    } else {
      p.form = WINO_CO32;
      p.tiles_x = (s.W + 15) / 16;
      p.tiles_y = (s.H + 15) / 16;
      p.co_tiles = s.Cout / 32;
    }
  } else {
    // the pooled and the statistics epilogue live in the persistent wide kernels only (the ConvMeanPool layers of the score
    // nets are 32..128 pixels wide); everything else is "unsupported" and the caller runs the pieces separately
    if (s.pool2 && (small || !persist || !deep || s.H % 2 || s.W % 2)) return p;
    if (s.stats && (small || !persist || !deep)) return p;
    const bool dma4 = sw.dma4 && s.W % 4 == 0 && s.x16;
    // undilated images of up to 16 x 16 pixels with enough (image, channel tile) pairs to fill the chip
    const bool small_dma = small && persist && s.dil == 1 && s.W <= 16 && s.H <= 16 && s.W % 2 == 0 && s.H % 2 == 0 && deep &&
                           (int64_t)s.B * (s.Cout / X_CO) >= sw.small_min;
    if (small_dma) {
      p.form = WINO_SMALL_DMA;
      p.dma4 = dma4;
      p.tiles_x = (s.W + 15) / 16;
      p.tiles_y = (s.H + 15) / 16;
    } else if (small) {
      p.form = WINO_SMALL_REG;
      p.tiles_x = ((s.H * s.W) / 4 + X_TILES - 1) / X_TILES;
      p.tiles_y = 1;
    } else {
      p.tiles_x = (s.W + 2 * X_TX - 1) / (2 * X_TX);
      p.tiles_y = (s.H + 2 * X_TY - 1) / (2 * X_TY);
      if (!(persist && deep)) {
        p.form = WINO_TILE;
      } else {
        if (s.stats && !dma4) return p;           // the statistics epilogue exists with 16-byte DMA only
        p.form = WINO_WIDE;
        p.dma4 = dma4;
        p.pool = s.pool2;
        p.stats = s.stats;
      }
    }
  }
  p.nblk = (int64_t)s.B * p.tiles_x * p.tiles_y * p.co_tiles;
  // applied to every form.  (POLY went without it: there wino_bx3_shape_ok holds B * Cin * 1 KiB below 2^29, so B < 2^14, and
  // only a layer of more than 2^23 output channels could get here -- with a tile count that no longer fits the kernel's int.)
  if (p.nblk > 0x7fffffff) return p;
  p.rc = IPDM_OK;
  return p;
}

// the split-K call: `ksplit` K parts of the 8 x 8 form (16-byte LDS-DMA only), each a workgroup-sized piece of its own
inline WinoPlan wino_bx3_ksplit_plan(const WinoShape& s, const WinoSwitches& sw, int ksplit) {
  WinoPlan p = {IPDM_EUNSUPPORTED, WINO_KSPLIT, true, false, false, (s.W + 15) / 16, (s.H + 15) / 16, s.Cout / X_CO, 0};
  if (!wino_bx3_shape_ok(s) || ksplit < 2 || ksplit != wino_bx3_ksplit_for(s.Cin, s.Cout, s.H, s.W, s.dil, sw) || !s.x16) return p;
  p.nblk = (int64_t)s.B * p.tiles_x * p.tiles_y * p.co_tiles * ksplit;
  if (p.nblk <= 0x7fffffff) p.rc = IPDM_OK;
  return p;
}

// ---- the shape queries of the C ABI: one image, 16-byte aligned input -------------------------------------------------------
inline WinoShape wino_query_shape(int Cin, int Cout, int H, int W, int dilation, bool hx, bool pool2, bool stats) {
  return WinoShape{1, Cin, Cout, H, W, dilation, hx, pool2, stats, true};
}

// ipdm_conv2d_wino_hx2_form: the form of the f16x2 family's plain call as IPDM_WINO_FORM_*
inline int wino_hx2_form(int Cin, int Cout, int H, int W, int dilation, const WinoSwitches& sw) {
  if (Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || dilation < 1) return IPDM_EUNSUPPORTED;
  const WinoPlan p = wino_bx3_plan(wino_query_shape(Cin, Cout, H, W, dilation, true, false, false), sw);
  if (p.rc != IPDM_OK) return IPDM_EUNSUPPORTED;
  return p.form == WINO_POLY ? IPDM_WINO_FORM_POLY : p.form == WINO_HALF ? IPDM_WINO_FORM_HALF
       : p.form == WINO_CO32 ? IPDM_WINO_FORM_CO32 : IPDM_WINO_FORM_OTHER;
}

// ipdm_conv2d_wino_bx3_stats_partials: partials per plane of the statistics epilogue, 0 where it does not serve the shape.
// Asked with the DMA4 switch taken as on: under IPDM_WBX3_DMA4=0 the answer stays what it always was, the call itself then
// says IPDM_EUNSUPPORTED and the host front end (ops.conv2d_wino_bx3) falls back on that.
inline int wino_stats_partials(int Cin, int Cout, int H, int W, int dilation, int pool2, WinoSwitches sw) {
  sw.dma4 = 1;
  const WinoPlan p = wino_bx3_plan(wino_query_shape(Cin, Cout, H, W, dilation, false, pool2 != 0, true), sw);
  return p.rc == IPDM_OK ? 2 * p.tiles_x * p.tiles_y : 0;
}

}  // namespace ipdm_conv
