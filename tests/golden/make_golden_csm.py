#!/usr/bin/env python3
"""Golden vectors for SENSE with COMPLEX coil sensitivity maps: g36_sense_complex_maps.npz.

Built like make_golden.py (whose reference import, mask patch and helpers it reuses): the reference runs here on the
CPU, and only data is committed.  The reference's SENSE is written for complex maps (conj_op uses sens_maps[i].conj(),
the constructor normalises with abs()**2) but generates only real ones, so RSS-normalised complex128 maps are assigned
to ``op.sens_maps`` -- the idiom its own scripts use -- and ``__call__``, ``conj_op``, ``SSOS`` and ``L2Penalty`` are
recorded unchanged.  The maps are the "exp" magnitudes times a seeded second-order polynomial phase per coil.

    python tests/golden/make_golden_csm.py
"""
import numpy as np

import make_golden as mg
from make_golden import torch, ref_uf, ref_prox, npy, quiet, MASK_PARAMS, t1_mask_patch, save


def complex_maps(real_maps, seed):
    n, H, W = real_maps.shape
    rng = np.random.RandomState(seed)
    u = np.linspace(-1.0, 1.0, H)[:, None]
    v = np.linspace(-1.0, 1.0, W)[None, :]
    maps = np.empty((n, H, W), dtype=np.complex128)
    for i in range(n):
        a = rng.randn(6)
        phase = a[0] + a[1] * u + a[2] * v + a[3] * u * v + a[4] * u * u + a[5] * v * v
        maps[i] = real_maps[i] * np.exp(1j * np.pi * 0.5 * phase)
    return maps / np.sqrt((np.abs(maps) ** 2).sum(0))


def g36_sense_complex_maps():
    out = {}
    g = torch.Generator().manual_seed(36)
    H = W = 32
    orig = ref_uf.RandomUndersamplingFourier._generate_mask
    try:
        # generate_mask needs N >= 32 and the live reference mask is T = 24: the T = 1 variant, as g04 / g05
        ref_uf.RandomUndersamplingFourier._generate_mask = t1_mask_patch(MASK_PARAMS["R8"])
        with quiet:
            op = ref_uf.SENSE("exp", 4, 8, 0.04, (1, H, W), seed=0)
    finally:
        ref_uf.RandomUndersamplingFourier._generate_mask = orig
    maps = complex_maps(npy(op.sens_maps), seed=36)
    assert maps.dtype == np.complex128 and np.allclose((np.abs(maps) ** 2).sum(0), 1.0)
    assert np.abs(maps.imag).max() > 0.3
    op.sens_maps = torch.from_numpy(maps)
    rnd = lambda *shape: torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))
    x = rnd(2, 1, H, W)
    s = rnd(4, 1, 1, H, W)                       # one sample: keeps the file under 200 KiB
    z = rnd(2, 1, H, W)
    y = op(x)
    out["maps"] = maps
    out["mask_T1"] = npy(op.random_under_fourier.mask)
    out["x"] = npy(x)
    out["Ax"] = npy(y)
    out["s"] = npy(s)
    out["AHs"] = npy(op.conj_op(s))
    out["ssos_s"] = npy(op.SSOS(s))
    out["z"] = npy(z)
    prox = ref_prox.L2Penalty(op)
    for i, (alpha, lamda) in enumerate([(3.0, 1.0), (3.0, 0.5), (9.0, 0.5)]):
        with quiet:
            xs = prox(z, y, alpha, lamda)
        torch.set_grad_enabled(True)
        assert (xs - z).abs().max() > 1e-3, (alpha, lamda, float((xs - z).abs().max()))
        out[f"l2_{i}_alpha_lamda"] = np.array([alpha, lamda], dtype=np.float64)
        out[f"l2_{i}_x"] = npy(xs)
    for k in ("Ax", "AHs", "x", "s", "z"):
        out[k] = out[k].astype(np.complex64)
    save("g36_sense_complex_maps", **out)


if __name__ == "__main__":
    g36_sense_complex_maps()
