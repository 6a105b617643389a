#!/usr/bin/env python3
"""in-kernel cycle split (a.dbg stamps) of the three pooled launches of a score evaluation: 12-position blob (averaging epilogue)
against the folded blob; B = 14, residual + statistics, one output"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverseproblemwithdiffusionmodel_amd import _lib, ops
B = 14
for ci, co, hw in [(128, 256, 128), (256, 256, 64), (256, 256, 32)]:
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, ci, hw, hw, device="cuda", generator=g)
    w = torch.randn(co, ci, 3, 3, device="cuda", generator=g) * 0.05
    bias = torch.randn(co, device="cuda", generator=g)
    r = torch.randn(B, co, hw // 2, hw // 2, device="cuda", generator=g)
    for name, U in (("averaged", ops.conv_wino1d_weight(w)), ("folded", ops.conv_wino1d_pool_weight(w))):
        run = lambda: ops.conv2d_wino_bx3(x, U, bias, r, pool2=True, want_stats=True)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            run()
        e1.record(); torch.cuda.synchronize()
        us10 = e0.elapsed_time(e1) * 100
        buf = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
        _lib.lib.ipdm_debug_set_stamp_buffer(_lib.P(buf.data_ptr()))
        e0.record(); run(); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        _lib.lib.ipdm_debug_set_stamp_buffer(_lib.P(0))
        t = buf.cpu()[:256 * 4].view(-1, 4).double()
        t = t[t[:, 0] != 0]
        tiles = B * (hw // 8) * (hw // 32) * (co // 128) / t.shape[0]
        nch = ci // 16
        print(f"{ci}->{co}@{hw} {name:9s}: {us10:.0f} us back to back; stamped launch {ms * 1e3:.0f} us; {t.shape[0]} WGs x {tiles:.2f} passes; "
              f"cycles total median {t[:, 0].median():.0f} max {t[:, 0].max():.0f} (clock {t[:, 0].max() / ms / 1e6:.2f} GHz); "
              f"prologue {t[:, 1].median():.0f}; per pass: loop {t[:, 2].median() / tiles:.0f} = {t[:, 2].median() / tiles / nch:.0f} per chunk, "
              f"epilogue {t[:, 3].median() / tiles:.0f}", flush=True)
