#!/usr/bin/env python3
"""Device time of the mask-weighted time average (ops.kspace_time_average) per call, from a hipGraph replay of 20 calls
(best of 3) as scripts/bench_csm.py takes it, with the bytes it has to move -- y at the sampled positions, the mask bytes
of every pixel, ybar -- and the rate they give against the 6.29 TB/s of a float4 copy; and the wall time of the whole
SENSE.from_cine_measurement call (host checks, composite, maps, the copy of the maps to the host), best of 3.  Sizes as
DESIGN.md 4.4g quotes them: (n, T, H, W) = (4, 24, 128, 128) under the generated T = 24 line mask, and (32, 24, 320, 320)
under per-frame variable-density 2-D masks at R = 8."""
import os
import sys
import time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverseproblemwithdiffusionmodel_amd import ops
from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE, RandomUndersamplingFourier
from inverseproblemwithdiffusionmodel_amd.synthetic import vd_mask_2d

COPY_ROOF = 6.29e12


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


def masks(kind, T, H, W):
    if kind == "line":
        return RandomUndersamplingFourier(8, 0.05, (1, H, W), 0, mask_T=T).mask               # (T, 1, 1, W)
    return torch.cat([torch.as_tensor(vd_mask_2d(H, W, 8, center_frac=0.08, seed=t)) for t in range(T)], dim=0)


for n, T, H, W, kind in [(4, 24, 128, 128, "line"), (32, 24, 320, 320, "2d")]:
    mask = masks(kind, T, H, W)
    mu8 = ops._mask_u8(mask, H, W, "cuda")
    planes = mu8.bool() if mu8.dim() == 3 else mu8.bool()[:, None, :].expand(T, H, W)
    y = torch.randn(n, T, H, W, dtype=torch.complex64, device="cuda") * planes[None]
    out = torch.empty(n, H, W, dtype=torch.complex64, device="cuda")
    t_k = timeit(lambda: ops.kspace_time_average(y, mu8, out=out))
    sampled = int(planes.sum())
    moved = 8 * n * sampled + T * H * W + 8 * n * H * W
    print(f"kspace_time_average (n, T, H, W) = {(n, T, H, W)} {kind} masks, {sampled / (T * H * W):.3f} sampled: {t_k * 1e6:8.1f} us "
          f"per call; {moved / 1e6:.2f} MB moved (y sampled {8 * n * sampled / 1e6:.2f}, mask {T * H * W / 1e6:.2f}, ybar "
          f"{8 * n * H * W / 1e6:.2f}) = {moved / t_k / 1e12:.3f} TB/s, {100 * moved / t_k / COPY_ROOF:.1f} % of the float4-copy "
          f"rate; all of y would be {8 * n * T * H * W / 1e6:.2f} MB", flush=True)
    best = 1e9
    for _ in range(4):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        cal = SENSE.from_cine_measurement(y, mask, R=8, seed=0)
        torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
    print(f"from_cine_measurement {(n, T, H, W)}: {best * 1e3:.2f} ms wall per call, region {cal.region}", flush=True)
