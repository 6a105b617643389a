#!/usr/bin/env python3
"""A/B of the 1-D convolution kernel (csrc/conv1d.hip) against the one-row route on the direct 2-D kernel (the IPDM_CONV1D=0
arm), both captured into a hipGraph and replayed (the method of scripts/bench_resample.py):
  * per-launch times of the NCSN1D census shapes at N = 512 sequences (a 128 x 128 temporal step: 512 sequences of 64 x 24);
  * the full NCSN1D forward (cine127_1d.yml size) at N = 512, the two arms in alternating runs in one process on one card
    (ops.USE_CONV1D is read per call; the weights of both routes are packed before the timed runs).
Output: the text kept as profiles/ncsn1d_ab.txt."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverseproblemwithdiffusionmodel_amd import ops                                      # noqa: E402
from inverseproblemwithdiffusionmodel_amd.helpers.load_model import reload_model           # noqa: E402

N = int(os.environ.get("BENCH_N", 512))


def timeit(fn, iters=10, reps=3):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(reps):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e-3)
    return best


def layer(Cin, Cout, L, k, d, pool=False):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, Cin, L, generator=gen).cuda()
    w = (torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5).cuda()
    b = torch.randn(Cout, generator=gen).cuda()
    r = torch.randn(N, Cout, L // 2 if pool else L, generator=gen).cuda()
    am = ops.absmax_per_image(x)
    wq, wr = ops.conv1d_weight(w), ops.conv1d_rows_weight(w)
    with ops.amax_scope():
        t_new = timeit(lambda: ops.conv1d(x, wq, b, r, d, act_out=ops.ACT_ELU, in_amax=am, want_amax=True, pool2=pool))
        if pool:
            def rows():
                y = ops.meanpool1d2(ops.conv1d_rows(x, wr, b, dilation=d, in_amax=am, want_amax=False))
                y = ops.add(y, r)
                return y, ops.act(y, ops.ACT_ELU)
        else:
            def rows():
                return ops.conv1d_rows(x, wr, b, residual=r, dilation=d, act_out=ops.ACT_ELU, in_amax=am, want_amax=True)
        t_row = timeit(rows)
    flop = 2.0 * N * L * Cin * Cout * k
    print(f"{Cin:4d} -> {Cout:4d}  L {L:3d}  k {k}  d {d}  {'pair mean' if pool else '         '}   conv1d {t_new * 1e6:8.1f} us "
          f"({flop / t_new / 1e12:6.1f} TFLOP/s)   one-row route {t_row * 1e6:8.1f} us   ratio {t_row / t_new:5.2f}x", flush=True)


if __name__ == "__main__":
    print(f"device: {torch.cuda.get_device_name(0)}   N = {N} sequences   (bias + residual + ELU copy + maxima in every launch)")
    for Cin, Cout in [(64, 128), (128, 128), (128, 256), (256, 256), (256, 128), (128, 64)]:
        layer(Cin, Cout, 24, 3, 1)
    for d in (1, 2, 4):
        layer(256, 256, 12, 3, d)
    layer(128, 256, 12, 1, 1)
    layer(128, 256, 24, 3, 1, pool=True)
    net = reload_model("Diffusion1D", "CINE127", device=torch.device("cuda"))
    x = torch.rand(N, 64, 24, device="cuda")
    labels = torch.randint(0, 400, (N,), device="cuda")
    times = {True: [], False: []}
    with torch.no_grad():
        for arm in (True, False):                             # pack both routes' weights outside the timed runs
            ops.USE_CONV1D = arm
            net(x, labels)
        for rep in range(3):
            for arm in (True, False):
                ops.USE_CONV1D = arm
                times[arm].append(timeit(lambda: net(x, labels), iters=2, reps=2))
    ops.USE_CONV1D = True
    for arm in (True, False):
        print(f"NCSN1D forward N = {N}, {'default (conv1d kernel)' if arm else 'IPDM_CONV1D=0 (one-row route)'}: "
              + "  ".join(f"{t * 1e3:7.2f} ms" for t in times[arm]) + f"   best {min(times[arm]) * 1e3:7.2f} ms")
    print(f"forward ratio one-row / conv1d: {min(times[False]) / min(times[True]):.2f}x")
