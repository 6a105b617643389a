#!/usr/bin/env python3
"""Device time of coil compression (ops.coil_gram, ops.coilcomp_matrix, ops.coil_apply and the one-call
ops.coil_compress) per call, from a hipGraph replay of 20 calls, best of 3, as scripts/bench_csm.py takes it, at the sizes
DESIGN.md 4.4f quotes: 16 -> 6, 32 -> 8 and 64 -> 8 coils at 128x128 and 320x320, one image; the streaming kernel's
bytes per second at 64 -> 8, 320x320, 16 images next to a plain streaming add (scripts/bench_resample.py's HBM figure);
and what compression buys: the one-step and the conjugate-gradient SENSE tails (scripts/bench_cg_prox.py's arms; 14 images,
128x128) at 16 and 32 physical against 6 and 8 virtual coils."""
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverseproblemwithdiffusionmodel_amd import ops
from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image


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


def stages(n, nv, H, W, B):
    y = torch.randn(n, B, H, W, dtype=torch.complex64, device="cuda")
    G = ops.coil_gram(y, 12, 12)
    A = ops.coilcomp_matrix(G, nv)
    out = torch.empty(nv, B, H, W, dtype=torch.complex64, device="cuda")
    work = ops.coilcomp_workspace(B, n, "cuda")
    t_g = timeit(lambda: ops.coil_gram(y, 12, 12, out=G))
    t_m = timeit(lambda: ops.coilcomp_matrix(G, nv))
    t_a = timeit(lambda: ops.coil_apply(y, A, out=out))
    t_all = timeit(lambda: ops.coil_compress(y, 12, 12, nv, work=work))
    nbytes = (n + nv) * B * H * W * 8
    print(f"coil_compress {n:2d} -> {nv} coils {H}x{W} B={B}: gram {t_g * 1e6:7.1f} us, matrix {t_m * 1e6:7.1f} us, apply "
          f"{t_a * 1e6:7.1f} us ({nbytes / 1e6:.1f} MB, {nbytes / t_a / 1e9:.0f} GB/s), one call {t_all * 1e6:7.1f} us", flush=True)


for H, W in ((128, 128), (320, 320)):
    for n, nv in ((16, 6), (32, 8), (64, 8)):
        stages(n, nv, H, W, 1)
stages(64, 8, 320, 320, 16)
stages(64, 32, 320, 320, 16)
x = torch.randn(28, 128, 128, 128, device="cuda")
z = torch.randn_like(x)
t = timeit(lambda: ops.add(x, z, out=z))
print(f"streaming add (28,128,128,128): {12 * x.numel() / 1e6:.1f} MB, {12 * x.numel() / t / 1e9:.0f} GB/s", flush=True)
del x, z

# the SENSE tails per iteration, by coil count
B, H, W = 14, 128, 128
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
x0 = torch.randn(2, B, 1, H, W, generator=gen).to(dev)
g = torch.randn(2, B, 1, H, W, generator=gen).to(dev)
kw = dict(step=1e-3, noise_scale=0.03, seed=1, sample_offset=0, step_id=3)
for n in (4, 6, 8, 16, 32):
    op = SENSE("exp", n, 40, 0.04, (1, H, W), seed=0, mask_T=1)
    sens, mask = op.sens_dev(dev), op.mask_u8(dev)
    y = op(phantom_image(H, W, seed=0).to(dev)).repeat(1, B, 1, 1, 1).contiguous()
    ahy = op.conj_op(y).contiguous()
    x = x0.clone()
    work_l2, work_cg = ops.sense_workspace(B, n, H, W, dev), ops.sense_cg_workspace(B, n, H, W, dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    t_l2 = timeit(lambda: ops.ald_sense_step(x[0], x[1], g[0], g[1], y, sens, mask, work_l2, coef=0.05 / (n * W), **kw))
    x.copy_(x0)
    t_cg = timeit(lambda: ops.ald_sense_cg_step(x[0], x[1], g[0], g[1], y, sens, mask, work_cg, coef=1.0, ahy=ahy, max_iter=10,
                                                tol=0.0, iters_out=iters, **kw))
    print(f"SENSE tails B={B} {H}x{W} {n:2d} coils: one-step {t_l2 * 1e3:.3f} ms, CG 10 iterations {t_cg * 1e3:.3f} ms", flush=True)
