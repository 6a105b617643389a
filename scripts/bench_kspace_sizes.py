#!/usr/bin/env python3
"""Cost of the k-space kernels by image size: ops.sense_forward and ops.ald_sense_step (B = 14, 4 coils, complex maps, a line
mask at R = 4, Philox noise) at sides with factors 3 and 5 beside their power-of-two neighbours, and beside the same operator
composed from torch.fft.fft2 on the device (maps * x -> ifftshift -> fft2 -> fftshift -> mask; the step adds the masked
residual, the inverse transform, the conj(maps)-weighted coil sum and the update).  Each arm is `--calls` calls captured
into one hipGraph, the best of three replays, as scripts/bench_resample.py.  Prints one table line per size.

    python scripts/bench_kspace_sizes.py [--sizes 96x96,128x128,...]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, calls):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / calls * 1e3)
    return best                                                              # us per call


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x96,128x128,96x160,192x192,256x256,320x320")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    from inverseproblemwithdiffusionmodel_amd import ops, synthetic
    B, n = 14, 4
    print(f"B={B} coils={n}; us per call | ns per pixel (B*H*W pixels)")
    print(f"{'size':>9s} {'class':>5s} | {'forward':>9s} {'torch.fft':>9s} | {'step':>9s} {'torch.fft':>9s} | "
          f"{'fwd ns/px':>9s} {'step ns/px':>10s}")
    for s in a.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        g = torch.Generator().manual_seed(1)
        sens = synthetic.complex_coil_maps(n, H, W, 2).to(torch.complex64).contiguous().cuda()
        m8 = (torch.rand(1, W, generator=g) < 0.25).to(torch.uint8)
        m8[:, W // 2 - 2:W // 2 + 2] = 1
        m8 = m8.cuda()
        mf = m8.float().view(1, 1, 1, W)
        x = torch.randn(2, B, H, W, generator=g).cuda()
        gr = torch.randn(2, B, H, W, generator=g).cuda()
        xc = torch.complex(x[0], x[1]).contiguous()
        y = ops.sense_forward(xc, sens, m8)
        work = ops.sense_workspace(B, n, H, W, "cuda")
        a_re, a_im = x[0].clone(), x[1].clone()
        coef = 0.05 / (n * W)

        def fft2c(t, inv=False):
            f = torch.fft.ifft2 if inv else torch.fft.fft2
            return torch.fft.fftshift(f(torch.fft.ifftshift(t, dim=(-1, -2)), norm="ortho"), dim=(-1, -2))

        def torch_forward(v):
            return mf * fft2c(sens[:, None] * v[None])

        nz = torch.randn(2, B, H, W, generator=g).cuda()
        zc = xc.clone()

        def torch_step():
            z = zc + 1e-3 * torch.complex(gr[0], gr[1]) + 0.03 * torch.complex(nz[0], nz[1])
            r = torch_forward(z) - y
            zc.copy_(z - coef * (sens.conj()[:, None] * fft2c(mf * r, True)).sum(0))

        t_fwd = timeit(lambda: ops.sense_forward(xc, sens, m8), a.calls)
        t_tfwd = timeit(lambda: torch_forward(xc), a.calls)
        t_step = timeit(lambda: ops.ald_sense_step(a_re, a_im, gr[0], gr[1], y, sens, m8, work, step=1e-3, noise_scale=0.03,
                                                   coef=coef, seed=1, step_id=3), a.calls)
        t_tstep = timeit(torch_step, a.calls)
        px = B * H * W
        print(f"{s:>9s} {ops.kspace_size_class(H, W):5d} | {t_fwd:9.1f} {t_tfwd:9.1f} | {t_step:9.1f} {t_tstep:9.1f} | "
              f"{t_fwd * 1e3 / px:9.3f} {t_step * 1e3 / px:10.3f}", flush=True)
