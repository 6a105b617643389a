"""The fused iteration tails against the chain of separate kernels they stand for, bit for bit:

    fused step with Philox noise
  ==
    ops.philox_normal for plane 0 (real) and plane 1 (imaginary), ops.langevin_step on each plane with that noise injected,
    then the plain proximal of the same path.

Both sides evaluate z = x + step*g + n*noise_scale with the same Philox keying (seed, sample_offset + b, step_id, plane,
quad) and the same operand order, and the k-space sources are built without floating-point contraction, so the results
are expected to agree in every bit; they are compared as int32 patterns so that signed zeros and NaNs count.  8x16 runs the
whole-image LDS kernels, 128x256 the row / column strips.  B = 3, three coils, complex maps, a 2-D mask with a plane per
image and a non-zero sample offset."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_COILS = 3, 3
STEP, NOISE_SCALE = 0.37, float(np.sqrt(2 * 0.37))
KEY = dict(seed=20240611, sample_offset=7, step_id=5)
CG = dict(max_iter=3, tol=0.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    """read-only device tensors shared by the cases of one shape"""
    from inverseproblemwithdiffusionmodel_amd import synthetic
    rng = np.random.default_rng(H * 1000 + W)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    rnd = lambda *s: rng.standard_normal(s).astype(np.float32)
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    mask = rng.random((B, H, W)) < 0.3
    mask[:, H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = True
    return dict(x_re=dev(rnd(B, H, W)), x_im=dev(rnd(B, H, W)), g_re=dev(rnd(B, H, W)), g_im=dev(rnd(B, H, W)),
                y=dev(cplx(N_COILS, B, H, W)), y1=dev(cplx(B, H, W)), m8=dev(mask.astype(np.uint8)),
                sens=synthetic.complex_coil_maps(N_COILS, H, W, 2).to(torch.complex64).contiguous().cuda())


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _langevin_chain(ops, d):
    """z by the separate kernels: Philox normals per plane, then the plain Langevin update with them injected"""
    z = []
    for plane, (x, g) in enumerate(((d["x_re"], d["g_re"]), (d["x_im"], d["g_im"]))):
        n = ops.philox_normal(tuple(x.shape), x.device, plane=plane, **KEY)
        z.append(ops.langevin_step(x.clone(), g, step=STEP, noise_scale=NOISE_SCALE, noise=n))
    return z


@pytest.mark.parametrize("H,W", [(8, 16), (128, 256)])
@pytest.mark.parametrize("path", ["sense", "singlecoil0", "singlecoil1", "singlecoil2", "cg"])
def test_fused_step_equals_separate_chain(ops, H, W, path):
    d = _inputs(H, W)
    x_re, x_im = d["x_re"].clone(), d["x_im"].clone()
    z_re, z_im = _langevin_chain(ops, d)
    fused = dict(step=STEP, noise_scale=NOISE_SCALE, **KEY)
    if path == "sense":
        coef = 0.25
        work = ops.sense_workspace(B, N_COILS, H, W, "cuda")
        ops.ald_sense_step(x_re, x_im, d["g_re"], d["g_im"], d["y"], d["sens"], d["m8"], work, coef=coef, **fused)
        want = ops.sense_l2prox(z_re, z_im, d["y"], d["sens"], d["m8"], coef)
    elif path == "cg":
        a = 2.0
        work = ops.sense_cg_workspace(B, N_COILS, H, W, "cuda")
        iters = ops.ald_sense_cg_step(x_re, x_im, d["g_re"], d["g_im"], d["y"], d["sens"], d["m8"], work, coef=a, **fused, **CG)
        *want, want_iters = ops.sense_cgprox(z_re, z_im, d["y"], d["sens"], d["m8"], a, **CG)
        assert torch.equal(iters.cpu(), want_iters.cpu())
        assert int(iters.min()) == CG["max_iter"]                      # tol 0: every sample ran all the iterations
    else:
        mode = int(path[-1])
        coef = (0.25, 0.7, 0.3)[mode]
        ops.ald_singlecoil_step(x_re, x_im, d["g_re"], d["g_im"], d["y1"], d["m8"], mode, coef=coef, **fused)
        want = ops.singlecoil_prox(z_re, z_im, d["y1"], d["m8"], coef, mode)
    for name, got, ref, start in (("re", x_re, want[0], d["x_re"]), ("im", x_im, want[1], d["x_im"])):
        assert torch.isfinite(got).all()
        assert not torch.equal(got, start)
        differ = int((_bits(got) != _bits(ref)).sum())
        assert differ == 0, (path, (H, W), name, differ, "elements differ, max abs", float((got - ref).abs().max()))
