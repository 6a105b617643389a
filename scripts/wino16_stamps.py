#!/usr/bin/env python3
"""phase cycles (in-kernel s_memtime stamps: prologue / K loop / epilogue per workgroup) and launch time of the 16 x 16 Winograd
layers of the score network at B = 28, in the f16x2 form the network runs.  Environment switches (IPDM_WBX3_*) select the form."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverseproblemwithdiffusionmodel_amd import ops, _lib
B = int(os.environ.get("BENCH_B", 28))
SHAPES = [(256, 256, 1), (512, 256, 1), (256, 256, 2), (256, 512, 2), (512, 512, 2), (512, 512, 4), (512, 512, 1)]
print(f"B={B}  switches: " + " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("IPDM_WBX3")))
for ci, co, dil in SHAPES:
    x = torch.randn(B, ci, 16, 16, device="cuda"); w = torch.randn(co, ci, 3, 3, device="cuda") * 0.05
    U = ops.conv_wino_bx3_weight(w, fmt="hx2")
    fn = lambda: ops.conv2d_wino_bx3(x, U, dilation=dil)
    for _ in range(3): fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10): fn()
    g.replay(); torch.cuda.synchronize()
    us = 1e9
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        us = min(us, e0.elapsed_time(e1) * 100)
    buf = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    _lib.lib.ipdm_debug_set_stamp_buffer(_lib.P(buf.data_ptr()))
    fn(); torch.cuda.synchronize()
    _lib.lib.ipdm_debug_set_stamp_buffer(_lib.P(0))
    t = buf.cpu().view(-1, 4)
    t = t[t[:, 0] != 0].double()
    if t.shape[0] == 0:
        print(f"{ci:4d}->{co:4d} d{dil}: {us:6.1f} us per launch; no stamps (split-K form)")
        continue
    pro, loop, epi = (t[:, 1] - t[:, 0]).median(), (t[:, 2] - t[:, 1]).median(), (t[:, 3] - t[:, 2]).median()
    span = t[:, 3].max() - t[:, 0].min()
    nch = ci // 16
    flops = 2.0 * B * 256 * co * ci * 9
    print(f"{ci:4d}->{co:4d} d{dil}: {us:6.1f} us per launch ({flops / us * 1e-6:4.0f} TFLOP/s); {t.shape[0]:3d} workgroups; shader cycles: "
          f"prologue {pro:6.0f} loop {loop:6.0f} = {nch} x {loop / nch:5.0f} epilogue {epi:6.0f}; first start -> last end {span:6.0f}")
