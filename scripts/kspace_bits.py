#!/usr/bin/env python3
"""Bit patterns of seeded calls of every k-space entry point, for comparing two builds of the library:

    IPDM_LIB=_variants/libipdm_<tag>.so python scripts/kspace_bits.py dump a.pt      (a fresh process per library)
    python scripts/kspace_bits.py dump b.pt
    python scripts/kspace_bits.py compare a.pt b.pt                                   -> "<n> tensors, <k> differ"

Calls: fft2c both ways, sense_forward, sense_adjoint with and without the mask, sense_ssos, sense_l2prox, ald_sense_step,
singlecoil_prox / ald_singlecoil_step in modes 0-2, sense_cgprox and ald_sense_cg_step (3 iterations, tol 0), at B = 3 with 1
and 3 coils, real and complex maps, line masks with T = 1 and T = 3 and a 2-D mask, injected and Philox noise, host scalars
and a device schedule.  Default shapes: 8x16, 128x128, 128x256, 256x128 (--shapes 48x80,80x240 for others)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SCHED = [("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"), ("rsv", "f4")]


def dump(path, shapes):
    from inverseproblemwithdiffusionmodel_amd import ops, synthetic
    out = {}
    B = 3
    for H, W in shapes:
        g = torch.Generator().manual_seed(H * 4096 + W)
        rn = lambda *s: torch.randn(*s, generator=g).cuda()
        cx = lambda *s: torch.complex(torch.randn(*s, generator=g), torch.randn(*s, generator=g)).cuda()
        x, gr, nz = rn(2, B, H, W), rn(2, B, H, W), rn(2, B, H, W)
        xc = torch.complex(x[0], x[1]).contiguous()
        tag = f"{H}x{W}"
        out[f"{tag}/fft2c"] = ops.fft2c(xc)
        out[f"{tag}/ifft2c"] = ops.fft2c(xc, inverse=True)
        line1 = (torch.rand(1, W, generator=g) < 0.3).to(torch.uint8)
        line3 = (torch.rand(3, W, generator=g) < 0.3).to(torch.uint8)
        two_d = (torch.rand(3, H, W, generator=g) < 0.3).to(torch.uint8)
        for m in (line1, line3):
            m[:, W // 2 - 1:W // 2 + 1] = 1
        two_d[:, H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = 1
        masks = {"line1": line1.cuda(), "line3": line3.cuda(), "2d": two_d.cuda()}
        sched = np.zeros(1, dtype=SCHED)
        sched["step"], sched["ns"], sched["coef"], sched["id"] = 0.3, 0.7, 0.011, 1234
        dev_sched = torch.as_tensor(sched.view(np.uint8)).cuda()
        key = dict(seed=5, sample_offset=9, step_id=1234)
        y1 = cx(B, H, W)
        for mname, m8 in masks.items():
            for mode in (0, 1, 2):
                t = f"{tag}/{mname}/sc{mode}"
                out[t + "/prox"] = torch.stack(ops.singlecoil_prox(x[0], x[1], y1, m8, 0.3, mode))
                for noise in ("philox", "injected"):
                    a, b = x[0].clone(), x[1].clone()
                    kw = dict(noise_re=nz[0], noise_im=nz[1]) if noise == "injected" else {}
                    ops.ald_singlecoil_step(a, b, gr[0], gr[1], y1, m8, mode, step=0.3, noise_scale=0.7, coef=0.3, **key, **kw)
                    out[f"{t}/step_{noise}"] = torch.stack((a, b))
            out[f"{tag}/{mname}/forward_1coil"] = ops.sense_forward(xc, None, m8)
        for n in (1, 3):
            y = cx(n, B, H, W)
            cmaps = synthetic.complex_coil_maps(n, H, W, 2).to(torch.complex64).contiguous().cuda()
            for kind, sens in (("real", cmaps.abs().float().contiguous()), ("complex", cmaps)):
                base = f"{tag}/n{n}/{kind}"
                out[base + "/adjoint"] = ops.sense_adjoint(y, sens)
                out[base + "/ssos"] = ops.sense_ssos(y)
                for mname, m8 in masks.items():
                    t = f"{base}/{mname}"
                    out[t + "/forward"] = ops.sense_forward(xc, sens, m8)
                    out[t + "/adjoint_masked"] = ops.sense_adjoint(y, sens, m8, apply_mask=True)
                    ym = ops.sense_forward(torch.complex(gr[0], gr[1]).contiguous(), sens, m8)
                    for coef in (0.011, 0.0):
                        out[f"{t}/l2prox_{coef}"] = torch.stack(ops.sense_l2prox(x[0], x[1], ym, sens, m8, coef))
                    work = ops.sense_workspace(B, n, H, W, "cuda")
                    for noise in ("philox", "injected"):
                        kw = dict(noise_re=nz[0], noise_im=nz[1]) if noise == "injected" else {}
                        a, b = x[0].clone(), x[1].clone()
                        ops.ald_sense_step(a, b, gr[0], gr[1], ym, sens, m8, work, step=0.3, noise_scale=0.7, coef=0.011, **key, **kw)
                        out[f"{t}/step_{noise}"] = torch.stack((a, b))
                        a, b = x[0].clone(), x[1].clone()
                        ops.ald_sense_step(a, b, gr[0], gr[1], ym, sens, m8, work, dev_sched=dev_sched, **key, **kw)
                        out[f"{t}/step_{noise}_sched"] = torch.stack((a, b))
                        a, b = x[0].clone(), x[1].clone()
                        it = ops.ald_sense_cg_step(a, b, gr[0], gr[1], ym, sens, m8, None, step=0.3, noise_scale=0.7, coef=3.0,
                                                   max_iter=3, tol=0.0, **key, **kw)
                        out[f"{t}/cgstep_{noise}"] = torch.stack((a, b))
                        out[f"{t}/cgstep_{noise}_iters"] = it
                    ahy = ops.sense_adjoint(ym, sens, m8, apply_mask=True)
                    for name, extra in (("cg", {}), ("cg_ahy", dict(ahy=ahy))):
                        o_re, o_im, it = ops.sense_cgprox(x[0], x[1], ym, sens, m8, 3.0, max_iter=8, tol=1e-5, **extra)
                        out[f"{t}/{name}"] = torch.stack((o_re, o_im))
                        out[f"{t}/{name}_iters"] = it
    torch.cuda.synchronize()
    bits = {}
    for k, v in out.items():
        v = torch.view_as_real(v) if v.is_complex() else v
        assert torch.isfinite(v.float()).all(), k
        bits[k] = v.contiguous().view(torch.int32).cpu()
    torch.save(bits, path)
    print(f"{len(bits)} tensors -> {path} ({os.environ.get('IPDM_LIB', 'in-tree library')})")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert a.keys() == b.keys(), sorted(set(a) ^ set(b))
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    for k in bad:
        print("differs:", k, int((a[k] != b[k]).sum()), "of", a[k].numel())
    print(f"{len(a)} tensors, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["dump", "compare"])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--shapes", default="8x16,128x128,128x256,256x128")
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.paths[0], [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")])
    else:
        sys.exit(compare(*a.paths))
