#!/usr/bin/env python3
"""Device time of the coil-map estimator (ops.estimate_sens_maps: window, centred inverse FFT, RSS + maximum, Walsh
kernel) per call, from a hipGraph replay as scripts/bench_resample.py takes it, at the sizes DESIGN.md 4.4e quotes:
128x128 with 4 coils and 320x320 with 16 coils, radius 2, 3 power iterations; BENCH_B images per call (default 1)."""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverseproblemwithdiffusionmodel_amd import ops

B = int(os.environ.get("BENCH_B", 1))


def timeit(fn, iters=20):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e-3)
    return best


for H, W, n in [(128, 128, 4), (320, 320, 16), (128, 128, 32)]:
    y = torch.randn(n, B, H, W, dtype=torch.complex64, device="cuda")
    out, work = torch.empty_like(y), ops.csm_workspace(B, n, H, W, "cuda")
    t_all = timeit(lambda: ops.estimate_sens_maps(y, 12, 12, out=out, work=work))
    t_cal = timeit(lambda: ops.csm_calib_images(y, 12, 12))
    print(f"estimate_sens_maps {H}x{W} {n:2d} coils B={B}: {t_all * 1e6:8.1f} us per call "
          f"(calibration images alone {t_cal * 1e6:7.1f} us)", flush=True)
