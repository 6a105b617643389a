#!/usr/bin/env python3
"""Golden vectors for the exact multi-coil proximal and the multi-step L2Penalty: g37_cg_prox.npz.

Built like make_golden_csm.py (whose reference import, T = 1 mask patch and complex maps it reuses): the reference runs
here on the CPU, and only data is committed.  Recorded from the imported reference:
  * SENSE with complex maps, 32x32, 4 coils, B = 3 (three samples on purpose: the reference's loss puts 1/B on the
    1/2 |x - z|^2 term, and without it the num_steps = 4 result moves by about 1e-4): L2Penalty(num_steps = 2, 4);
  * a single-coil operator (RandomUndersamplingFourier, seed 2), B = 3: L2Penalty(num_steps = 3);
  * for a = alpha/lamda in {1, 10}: the solution x* of (I + a A^H A) x = z + a A^H y by conjugate gradients in float64
    on the reference operator's maps and mask (relative residual <= 1e-12), the reference's check_solution of x*, and -- for the
    record -- its check_solution of its own one-step L2Penalty output.

    python tests/golden/make_golden_cg.py
"""
import numpy as np

import make_golden as mg  # noqa: F401
from make_golden import torch, ref_uf, ref_prox, npy, quiet, MASK_PARAMS, t1_mask_patch, save
from make_golden_csm import complex_maps


def _c2(x, inverse):
    """centred orthonormal 2-D transform in the input's precision (the reference's i2k_complex / k2i_complex round
    to complex64, which would floor a float64 residual at 4e-8)"""
    x = torch.fft.ifftshift(x, dim=[-1, -2])
    x = (torch.fft.ifftn if inverse else torch.fft.fftn)(x, dim=[-1, -2], norm="ortho")
    return torch.fft.fftshift(x, dim=[-1, -2])


def cg_f64(op, z, y, a, rtol=1e-13, max_iter=400):
    """plain CG in complex128, per sample, from x0 = z, on A = M F S_c built from the reference operator's own maps
    and mask"""
    maps, mask = op.sens_maps.to(torch.complex128), op.random_under_fourier.mask
    A = lambda v: torch.stack([mask * _c2(maps[i] * v, False) for i in range(maps.shape[0])], 0)
    AH = lambda s: sum(maps[i].conj() * _c2(mask * s[i], True) for i in range(maps.shape[0]))
    N = lambda v: v + a * AH(A(v))
    dot = lambda u, v: (u.conj() * v).real.sum(dim=(1, 2, 3))
    b = z + a * AH(y)
    x = z.clone()
    r = b - N(x)
    p = r.clone()
    rr = dot(r, r)
    bn = dot(b, b).sqrt()
    for _ in range(max_iter):
        if bool((rr.sqrt() <= rtol * bn).all()):
            break
        q = N(p)
        alpha = (rr / dot(p, q)).view(-1, 1, 1, 1)
        x = x + alpha * p
        r = r - alpha * q
        rr_new = dot(r, r)
        p = r + (rr_new / rr).view(-1, 1, 1, 1) * p
        rr = rr_new
    res = dot(b - N(x), b - N(x)).sqrt() / bn
    assert float(res.max()) <= 1e-12, res
    return x


def g37_cg_prox():
    out = {}
    g = torch.Generator().manual_seed(37)
    H = W = 32
    B = 3
    orig = ref_uf.RandomUndersamplingFourier._generate_mask
    try:
        ref_uf.RandomUndersamplingFourier._generate_mask = t1_mask_patch(MASK_PARAMS["R8"])
        with quiet:
            op = ref_uf.SENSE("exp", 4, 8, 0.04, (1, H, W), seed=0)
            sc = ref_uf.RandomUndersamplingFourier(8, 0.04, (1, H, W), seed=2)
    finally:
        ref_uf.RandomUndersamplingFourier._generate_mask = orig
    maps = complex_maps(npy(op.sens_maps), seed=36)
    op.sens_maps = torch.from_numpy(maps)
    rnd = lambda *shape: torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))
    x, z = rnd(B, 1, H, W), rnd(B, 1, H, W)
    y = op(x)
    out["maps"] = maps
    out["mask"] = npy(op.random_under_fourier.mask)
    out["z"] = npy(z).astype(np.complex64)
    out["y"] = npy(y).astype(np.complex64)
    z = torch.from_numpy(out["z"])                     # the float32 values the GPU sees
    y = torch.from_numpy(out["y"])
    prox = ref_prox.L2Penalty(op)
    for i, (alpha, lamda) in enumerate([(3.0, 1.0), (9.0, 0.5)]):
        for k in (2, 4):
            with quiet:
                xs = prox(z, y, alpha, lamda, num_steps=k)
            torch.set_grad_enabled(True)
            out[f"l2_{i}_steps{k}_x"] = npy(xs).astype(np.complex64)
        out[f"l2_{i}_alpha_lamda"] = np.array([alpha, lamda], dtype=np.float64)
    # single coil
    ysc = sc(x)
    out["sc_mask"] = npy(sc.mask)
    out["sc_y"] = npy(ysc).astype(np.complex64)
    with quiet:
        xs = ref_prox.L2Penalty(sc)(z, torch.from_numpy(out["sc_y"]), 3.0, 0.5, num_steps=3)
    torch.set_grad_enabled(True)
    out["sc_l2_steps3_x"] = npy(xs).astype(np.complex64)
    out["sc_l2_alpha_lamda"] = np.array([3.0, 0.5], dtype=np.float64)
    # exact proximal, float64
    z128, y128 = z.to(torch.complex128), y.to(torch.complex128)
    import warnings
    for a in (1, 10):
        xstar = cg_f64(op, z128, y128, float(a))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            chk = float(prox.check_solution(xstar, z128, y128, float(a), 1.0))
            with quiet:
                one = prox(z, y, float(a), 1.0)
            torch.set_grad_enabled(True)
            chk_one = float(prox.check_solution(one.to(torch.complex128), z128, y128, float(a), 1.0))
        print(f"a = {a}: check_solution(x*) = {chk:.3e}, check_solution(one-step L2Penalty) = {chk_one:.3e}")
        out[f"cg_a{a}_xstar"] = npy(xstar)             # complex128
        out[f"cg_a{a}_check"] = np.array([chk, chk_one], dtype=np.float64)
    save("g37_cg_prox", **out)


if __name__ == "__main__":
    g37_cg_prox()
