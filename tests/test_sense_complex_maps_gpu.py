"""SENSE with complex (measured) coil sensitivity maps on the GPU: the float2-map instantiations of the k-space kernels
through ops.py and the product classes, against the reference's outputs (g36) and the CPU oracle.  Tolerances are those
of the real-map tests of the same operators (test_kernels_gpu.py): 5e-6 / 3e-6 absolute on the 32x32 golden vectors,
3e-5 against the oracle on unit-normal inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import kspace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def cplx(re, im):
    return re.cpu().numpy() + 1j * im.cpu().numpy()


def _maps(n, H, W, seed):
    from inverseproblemwithdiffusionmodel_amd import synthetic
    return synthetic.complex_coil_maps(n, H, W, seed).numpy()


# ---- 1. golden ------------------------------------------------------------------------------------
def test_complex_maps_golden(ops, golden):
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.proximal_op import get_proximal
    g = golden("g36_sense_complex_maps")
    maps = g["maps"]
    sens = dev(maps.astype(np.complex64))
    mask = dev(g["mask_T1"].reshape(1, 32).astype(np.uint8))
    y = ops.sense_forward(dev(g["x"]), sens, mask).cpu().numpy()
    print("forward max err", np.abs(y - g["Ax"]).max())
    np.testing.assert_allclose(y, g["Ax"], atol=5e-6)
    AHs = ops.sense_adjoint(dev(g["s"]), sens).cpu().numpy()
    print("adjoint max err", np.abs(AHs - g["AHs"]).max())
    np.testing.assert_allclose(AHs, g["AHs"], atol=5e-6)
    np.testing.assert_allclose(ops.sense_ssos(dev(g["s"])).cpu().numpy(), g["ssos_s"], atol=5e-6)
    z = g["z"]
    for i in range(3):
        alpha, lamda = g[f"l2_{i}_alpha_lamda"]
        coef = 0.05 * (alpha / lamda) / (4 * 32)
        o_re, o_im = ops.sense_l2prox(dev(z.real), dev(z.imag), dev(g["Ax"]), sens, mask, coef)
        print("l2prox max err", i, np.abs(cplx(o_re, o_im) - g[f"l2_{i}_x"]).max())
        np.testing.assert_allclose(cplx(o_re, o_im), g[f"l2_{i}_x"], atol=3e-6)
    # the maps' real part alone is a different operator: what the real-map path made of complex maps before
    y_real = ops.sense_forward(dev(g["x"]), dev(maps.real.astype(np.float32)), mask).cpu().numpy()
    assert np.abs(y_real - g["Ax"]).max() > 100 * 5e-6
    # product classes: constructor with custom maps, and assignment after construction
    op = SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps, normalize=False)
    assert np.array_equal(op.random_under_fourier.mask.numpy(), g["mask_T1"])
    np.testing.assert_allclose(op(dev(g["x"])).cpu().numpy(), g["Ax"], atol=5e-6)
    np.testing.assert_allclose(op.conj_op(dev(g["s"])).cpu().numpy(), g["AHs"], atol=5e-6)
    np.testing.assert_allclose(op.SSOS(dev(g["s"])).cpu().numpy(), g["ssos_s"], atol=5e-6)
    op2 = SENSE("exp", 4, 8, 0.04, (1, 32, 32), seed=0)
    op2.sens_maps = torch.from_numpy(maps)
    prox = get_proximal("L2Penalty")(op2)
    for i in range(3):
        alpha, lamda = g[f"l2_{i}_alpha_lamda"]
        got = prox(dev(z), dev(g["Ax"]), float(alpha), float(lamda)).cpu().numpy()
        np.testing.assert_allclose(got, g[f"l2_{i}_x"], atol=3e-6)


# ---- 2. oracle sweep, adjointness, fused step ------------------------------------------------------------
# rectangular shapes and odd coil counts: where a map indexed [coil][W][H], or a coil stride taken in floats rather than
# float2, shows; (128, 256) / (256, 128) take the row / column path, the others the LDS path
@pytest.mark.parametrize("H,W,n,mask_t", [(16, 64, 5, 3), (64, 16, 12, 1), (128, 128, 5, 1), (128, 128, 1, 3),
                                          (128, 256, 5, 3), (256, 128, 12, 1)])
def test_complex_maps_vs_oracle(ops, H, W, n, mask_t):
    rng = np.random.default_rng(36)
    B = 3
    maps = _maps(n, H, W, seed=2)
    sens = dev(maps.astype(np.complex64))
    mk = rng.random((mask_t, W)) < 0.35
    mk[:, W // 2 - 2:W // 2 + 2] = True
    mask = mk.reshape(mask_t, 1, 1, W)                                       # image b uses row b % mask_t (B == 3)
    m8 = dev(mk.astype(np.uint8))
    rnd = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    x, s = rnd(B, 1, H, W), rnd(n, B, 1, H, W)
    Ax = ops.sense_forward(dev(x), sens, m8).cpu().numpy()
    err = {"forward": np.abs(Ax - kspace.sense_forward(x, maps, mask)).max()}
    got = ops.sense_adjoint(dev(s), sens).cpu().numpy()
    err["adjoint"] = np.abs(got - kspace.sense_adjoint(s, maps)).max()
    AHs = ops.sense_adjoint(dev(s), sens, m8, apply_mask=True).cpu().numpy()
    err["adjoint_masked"] = np.abs(AHs - kspace.sense_adjoint(s, maps, mask)).max()
    lhs = np.vdot(s.astype(np.complex128), Ax.astype(np.complex128))
    rhs = np.vdot(AHs.astype(np.complex128), x.astype(np.complex128))
    # L2Penalty closed form and the fused Langevin + proximal step (injected noise, device schedule)
    img = (rng.random((1, 1, H, W)) * np.exp(1j * rng.standard_normal((1, 1, H, W)))).astype(np.complex64)
    y = np.ascontiguousarray(np.repeat(kspace.sense_forward(img, maps, mask[:1]), B, axis=1))
    if mask_t > 1:
        y = kspace.sense_forward(np.repeat(img, B, axis=0), maps, mask)
    g = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    nz = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    step, ns, alpha = np.float32(0.37), np.float32(np.sqrt(2 * 0.37)), 60.0
    coef = 0.05 * alpha / (n * W)
    z = ((x.real + step * g[0] + nz[0] * ns) + 1j * (x.imag + step * g[1] + nz[1] * ns)).astype(np.complex64)
    want = kspace.l2_penalty_sense(z, y, alpha, 1.0, maps, mask)
    assert np.abs(want - z).max() > 1e-3
    o_re, o_im = ops.sense_l2prox(dev(z.real), dev(z.imag), dev(y), sens, m8, coef)
    err["l2prox"] = np.abs(cplx(o_re, o_im) - want).max()
    work = ops.sense_workspace(B, n, H, W, "cuda")
    x_re, x_im = dev(x.real), dev(x.imag)
    sched = np.zeros(1, dtype=[("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"),
                               ("rsv", "f4")])
    sched["step"], sched["ns"], sched["coef"], sched["id"] = step, ns, coef, 5
    ops.ald_sense_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(y), sens, m8, work, noise_re=dev(nz[0]), noise_im=dev(nz[1]),
                       dev_sched=dev(sched.view(np.uint8)))
    err["ald_sense_step"] = np.abs(cplx(x_re, x_im) - want).max()
    print(f"{H}x{W} n={n} mask_t={mask_t}", {k: float(v) for k, v in err.items()}, "adjointness",
          abs(lhs - rhs) / abs(lhs))
    for k, v in err.items():
        assert v < 3e-5, (k, v)
    assert abs(lhs - rhs) < 1e-4 * abs(lhs)                                  # <s, A x> = <A^H s, x>


# ---- 3. same bits across kernel forms -----------------------------------------------------------------
def test_complex_maps_coil_parallel_is_bit_identical(ops, tmp_path):
    """IPDM_SENSE_COILS=1 (one workgroup per (sample, coil) + combine) against =0 (one workgroup per sample), complex
    maps and Philox noise: the switch is read once per process, so each form runs in its own child, one after the other"""
    code = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from inverseproblemwithdiffusionmodel_amd import ops
g = torch.Generator().manual_seed(78)
B, n, H, W = 3, 4, 128, 128
x = torch.randn(2, B, H, W, generator=g).cuda(); gr = torch.randn(2, B, H, W, generator=g).cuda()
y = torch.complex(torch.randn(n, B, H, W, generator=g), torch.randn(n, B, H, W, generator=g)).cuda()
sens = torch.complex(torch.randn(n, H, W, generator=g), torch.randn(n, H, W, generator=g)).cuda()
mask = (torch.rand(1, W, generator=g) < 0.3).to(torch.uint8).cuda()
work = ops.sense_workspace(B, n, H, W, "cuda")
ops.ald_sense_step(x[0], x[1], gr[0], gr[1], y, sens, mask, work, step=0.3, noise_scale=0.7, coef=0.011, seed=5,
                   sample_offset=9, step_id=1234)
torch.save(x.cpu(), sys.argv[2])
"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for tag, val in (("coils", "1"), ("serial", "0")):
        out = str(tmp_path / f"{tag}.pt")
        r = subprocess.run([sys.executable, "-c", code, repo, out], env=dict(os.environ, IPDM_SENSE_COILS=val),
                           capture_output=True, text=True, timeout=200)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(out))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# ---- 4. real maps untouched ------------------------------------------------------------------------------
def test_real_maps_untouched_and_cache_invalidation(ops, golden):
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
    g = golden("g36_sense_complex_maps")
    op = SENSE("exp", 4, 8, 0.04, (1, 32, 32), seed=0)
    real = op.sens_maps.to(torch.float32).cuda().contiguous()
    as_c64 = torch.complex(real, torch.zeros_like(real)).contiguous()
    mask = op.mask_u8("cuda")
    x, s, z = dev(g["x"]), dev(g["s"]), g["z"]
    y_f, y_c = ops.sense_forward(x, real, mask), ops.sense_forward(x, as_c64, mask)
    np.testing.assert_allclose(y_c.cpu().numpy(), y_f.cpu().numpy(), atol=5e-6)
    assert torch.equal(y_c, y_f)                 # ... and in fact bit for bit (== : a zero's sign aside), as ipdm.h states
    a_f, a_c = ops.sense_adjoint(s, real), ops.sense_adjoint(s, as_c64)
    np.testing.assert_allclose(a_c.cpu().numpy(), a_f.cpu().numpy(), atol=5e-6)
    assert torch.equal(a_c, a_f)
    p_f = ops.sense_l2prox(dev(z.real), dev(z.imag), y_f, real, mask, 0.004)
    p_c = ops.sense_l2prox(dev(z.real), dev(z.imag), y_f, as_c64, mask, 0.004)
    np.testing.assert_allclose(cplx(*p_c), cplx(*p_f), atol=3e-6)
    assert torch.equal(p_c[0], p_f[0]) and torch.equal(p_c[1], p_f[1])
    # the float32 call and the class give the same bits
    assert op.sens_dev("cuda").dtype == torch.float32 and torch.equal(op.sens_dev("cuda"), real)
    assert torch.equal(op(x), y_f) and torch.equal(op.conj_op(s), a_f)
    # assigning new maps after first use takes effect at once (the cached device copy is dropped)
    op.sens_maps = g["maps"]
    assert op.sens_dev("cuda").dtype == torch.complex64
    y_new = op(x)
    assert not torch.equal(y_new, y_f)
    np.testing.assert_allclose(y_new.cpu().numpy(), g["Ax"], atol=5e-6)


# ---- 7. errors ------------------------------------------------------------------------------------------
def test_complex_maps_errors(ops):
    from inverseproblemwithdiffusionmodel_amd._lib import IpdmUnsupported
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
    B, n, H, W = 2, 3, 32, 32
    x = torch.zeros(B, 1, H, W, dtype=torch.complex64, device="cuda")
    s = torch.zeros(n, B, 1, H, W, dtype=torch.complex64, device="cuda")
    mask = torch.ones(1, W, dtype=torch.uint8, device="cuda")
    good = torch.ones(n, H, W, dtype=torch.complex64, device="cuda")
    planes = [torch.zeros(B, 1, H, W, device="cuda") for _ in range(4)]
    work = ops.sense_workspace(B, n, H, W, "cuda")
    bad_maps = [good.to(torch.complex128), good.real.to(torch.float64),
                torch.ones(n, H, 2 * W, dtype=torch.complex64, device="cuda")[:, :, ::2],
                torch.ones(n, W, H, device="cuda").transpose(1, 2)]
    for bad in bad_maps:
        with pytest.raises(TypeError):
            ops.sense_forward(x, bad, mask)
        with pytest.raises(TypeError):
            ops.sense_adjoint(s, bad)
        with pytest.raises(TypeError):
            ops.sense_l2prox(planes[0], planes[1], s, bad, mask, 0.01)
        with pytest.raises(TypeError):
            ops.ald_sense_step(planes[0], planes[1], planes[2], planes[3], s, bad, mask, work, step=0.1, noise_scale=0.1,
                               coef=0.01)
    op = SENSE("exp", n, 8, 0.04, (1, H, W), seed=0)
    with pytest.raises(ValueError):
        op.sens_maps = torch.ones(n, H, W + 1, dtype=torch.complex128)
    # a size without a kernel: IPDM_EUNSUPPORTED through every new entry point
    H2 = 24
    x2 = torch.zeros(B, 1, H2, W, dtype=torch.complex64, device="cuda")
    s2 = torch.zeros(n, B, 1, H2, W, dtype=torch.complex64, device="cuda")
    m2 = torch.ones(n, H2, W, dtype=torch.complex64, device="cuda")
    p2 = [torch.zeros(B, 1, H2, W, device="cuda") for _ in range(4)]
    w2 = torch.zeros(n * B * H2 * W * 2, device="cuda")
    with pytest.raises(IpdmUnsupported):
        ops.sense_forward(x2, m2, mask)
    with pytest.raises(IpdmUnsupported):
        ops.sense_adjoint(s2, m2)
    with pytest.raises(IpdmUnsupported):
        ops.sense_l2prox(p2[0], p2[1], s2, m2, mask, 0.01, work=w2)
    with pytest.raises(IpdmUnsupported):
        ops.ald_sense_step(p2[0], p2[1], p2[2], p2[3], s2, m2, mask, w2, step=0.1, noise_scale=0.1, coef=0.01)


# ---- 5. sampler ------------------------------------------------------------------------------------------
from argparse import Namespace  # noqa: E402

from conftest import state_dict_from_golden  # noqa: E402
from oracle import scorenet as oracle_net, ald as oracle_ald, map as oracle_map, metrics  # noqa: E402


def tiny_config():
    """the configuration of the tiny NCSNv2Deepest whose weights g07 holds (as the existing sampler tests)"""
    return Namespace(
        device=torch.device("cuda"),
        data=Namespace(channels=1, image_size=32, logit_transform=False, rescaled=False,
                       uniform_dequantization=False, gaussian_dequantization=False),
        model=Namespace(ngf=4, num_classes=10, sigma_begin=1.0, sigma_end=0.01, sigma_dist="geometric",
                        normalization="InstanceNorm++", nonlinearity="elu", spec_norm=False),
        recons=Namespace(sigma_dist="geometric", sigma_begin=1.0, sigma_end=0.01, num_classes=10),
        sampling=Namespace(n_steps_each=3, step_lr=9e-7, final_only=True, denoise=True))


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ALD_optimizers, proximal_op, MAP_optimizers
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier
    return Namespace(ncsnv2=ncsnv2, ald=ALD_optimizers, prox=proximal_op, map=MAP_optimizers, uf=undersampling_fourier)


@pytest.fixture(scope="module")
def tiny_net(pkg, golden):
    net = pkg.ncsnv2.NCSNv2Deepest(tiny_config())
    net.load_state_dict(state_dict_from_golden(golden("g07_layers"), "net"), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope="module")
def oracle_score(golden):
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state_dict_from_golden(golden("g07_layers"), "net").items()}

    def score(x, labels):
        with torch.no_grad():
            return oracle_net.ncsnv2_deepest(x, labels, sd)
    return score


class _Tape:
    """injected noise: the recorded arrays, one per call"""

    def __init__(self, tape):
        self.tape, self.i = tape, 0

    def __call__(self, like):
        n = torch.from_numpy(self.tape[self.i])
        self.i += 1
        return n


def _run_sampler(pkg, net, sigmas, maps, meas, noise, lr_scaled, use_graph):
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps, normalize=False)
    params = dict(n_steps_each=3, step_lr=9e-7, denoise=True, final_only=True)
    B = meas.shape[1]
    sampler = pkg.ald.ALDInvSegProximalRealImag(pkg.prox.get_proximal("L2Penalty")(op), 1.0, "linear", (B, 1, 32, 32), net,
                                                sigmas, params, tiny_config(), meas, op, seg=None,
                                                device=torch.device("cuda"))
    tape = _Tape(noise)
    x = sampler(label=None, lamda=1.0, save_dir=None, lr_scaled=lr_scaled, seg_mode="full", noise_fn=tape,
                use_graph=use_graph)[0].numpy()
    assert tape.i == 60
    return op, x


@pytest.fixture(scope="module")
def sampler_case(golden, oracle_score):
    """10 levels x 3 steps + denoise at 32x32, B = 2, the tiny NCSNv2Deepest, injected noise; the CPU oracle sampler with
    the complex maps, computed once"""
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    g8, g36 = golden("g08_ald"), golden("g36_sense_complex_maps")
    maps, mask = g36["maps"], g36["mask_T1"]
    img = torch.cat([phantom_image(32, 32, seed=s) for s in range(2)], dim=0).numpy().astype(np.complex64)
    meas = kspace.sense_forward(img, maps, mask)
    lr_scaled = float(g8["dc_visible_lr_scaled"])
    tape = _Tape(g8["noise"])
    ref = oracle_ald.ald_sense_real_imag(oracle_score, g8["sigmas"], meas, maps, mask, 9e-7, 3, lr_scaled, True, tape)
    return dict(maps=maps, mask=mask, meas=meas, ref=ref, noise=g8["noise"], sigmas=g8["sigmas"], lr_scaled=lr_scaled)


@pytest.mark.parametrize("use_graph", [False, True])
def test_sampler_with_complex_maps_vs_oracle(pkg, tiny_net, sampler_case, use_graph):
    c = sampler_case
    sigmas, meas = torch.from_numpy(c["sigmas"]).cuda(), torch.from_numpy(c["meas"]).cuda()
    op, x = _run_sampler(pkg, tiny_net, sigmas, c["maps"], meas, c["noise"], c["lr_scaled"], use_graph)
    ref = c["ref"]
    assert x.shape == ref.shape == (2, 1, 32, 32) and np.isfinite(x).all()
    x0 = op.conj_op(meas).cpu().numpy()
    for b in range(2):
        print("nrmse", metrics.nrmse(np.abs(x[b]), np.abs(ref[b])), "ssim-1", metrics.ssim(np.abs(x[b, 0]), np.abs(ref[b, 0])) - 1)
        assert metrics.nrmse(np.abs(x[b]), np.abs(ref[b])) < 1e-3
        assert abs(metrics.ssim(np.abs(x[b, 0]), np.abs(ref[b, 0])) - 1.0) < 1e-3
    print("displacement", np.linalg.norm((x - x0) - (ref - x0)) / np.linalg.norm(ref - x0))
    assert np.linalg.norm((x - x0) - (ref - x0)) <= 2e-3 * np.linalg.norm(ref - x0)
    # the phase took effect: the same run with the maps' real part lands far from both
    _, x_real = _run_sampler(pkg, tiny_net, sigmas, c["maps"].real.copy(), meas, c["noise"], c["lr_scaled"], use_graph)
    assert np.linalg.norm(x - x_real) > 10 * np.linalg.norm(x - ref)


# ---- 6. 2D+time and MAP ------------------------------------------------------------------------------------
def test_ald2dtime_with_complex_maps_vs_oracle(pkg, tiny_net, golden, oracle_score):
    """ALD2DTime(mode_T="none") on (B, T) = (1, 4) frames at 32x32: without a temporal step it is the SENSE sampler on the
    flattened batch of frames, so the oracle sampler (denoise=False) with the same complex maps and noise is the reference"""
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    g8, g36 = golden("g08_ald"), golden("g36_sense_complex_maps")
    maps, mask = g36["maps"], g36["mask_T1"]
    T = 4
    img = torch.cat([phantom_image(32, 32, seed=10 + t) for t in range(T)], dim=0).numpy().astype(np.complex64)   # (T,1,H,W)
    meas = kspace.sense_forward(img, maps, mask)                                                        # (n, T, 1, H, W)
    gen = torch.Generator().manual_seed(6)
    noise = [torch.randn(T, 1, 32, 32, generator=gen).numpy() for _ in range(60)]
    lr_scaled = float(g8["dc_visible_lr_scaled"])
    ref = oracle_ald.ald_sense_real_imag(oracle_score, g8["sigmas"], meas, maps, mask, 9e-7, 3, lr_scaled, False, _Tape(noise))
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps, normalize=False)
    sigmas = torch.from_numpy(g8["sigmas"]).cuda()
    sigmas_T = torch.from_numpy(kspace.get_sigmas(0.5, 0.01, 6)).cuda()
    no_prior = Namespace(config=Namespace(data=Namespace(channels=64)), sigmas=None)       # mode "none" never calls it
    params = dict(n_steps_each=3, step_lr=9e-7, denoise=False, final_only=True)
    sampler = pkg.ald.ALD2DTime(pkg.prox.get_proximal("L2Penalty")(op), no_prior, sigmas_T, (1, T, 1, 32, 32), tiny_net,
                                sigmas, params, tiny_config(), torch.from_numpy(meas[:, None]).cuda(), op,
                                device=torch.device("cuda"))
    tape = _Tape(noise)
    x = sampler(save_dir=None, lr_scaled=lr_scaled, mode_T="none", lamda_T=1.0, if_random_shift=False,
                noise_fn=tape)[0].numpy()
    assert tape.i == 60 and x.shape == (1, T, 1, 32, 32) and np.isfinite(x).all()
    x = x[0]
    x0 = kspace.sense_adjoint(meas, maps)
    assert np.linalg.norm(ref - x0) > 0.02 * np.linalg.norm(x0)
    for t in range(T):
        print("frame", t, "nrmse", metrics.nrmse(np.abs(x[t]), np.abs(ref[t])), "ssim-1",
              metrics.ssim(np.abs(x[t, 0]), np.abs(ref[t, 0])) - 1)
        assert metrics.nrmse(np.abs(x[t]), np.abs(ref[t])) < 1e-3
        assert abs(metrics.ssim(np.abs(x[t, 0]), np.abs(ref[t, 0])) - 1.0) < 1e-3
    print("displacement", np.linalg.norm((x - x0) - (ref - x0)) / np.linalg.norm(ref - x0))
    assert np.linalg.norm((x - x0) - (ref - x0)) <= 2e-3 * np.linalg.norm(ref - x0)


def test_map_optimizer_with_complex_maps_vs_oracle(pkg, tiny_net, golden, oracle_score):
    """MAPOptimizer (Adam on data term + score prior), 5 iterations, against oracle.map.sense_map with the oracle's forward /
    adjoint closed over the complex maps; tolerance of test_map_sense_golden_gpu: 2 % of the distance lr * n_iters travelled"""
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    g18, g36 = golden("g18_map"), golden("g36_sense_complex_maps")
    maps, mask = g36["maps"], g36["mask_T1"]
    lamda, lr, n_iters = float(g18["a_lamda"]), float(g18["a_lr"]), 5
    img = torch.cat([phantom_image(32, 32, seed=s) for s in range(2)], dim=0).numpy().astype(np.complex64)
    meas = kspace.sense_forward(img, maps, mask)
    x_init = kspace.sense_adjoint(meas, maps)

    def score_np(x, labels):
        return oracle_score(torch.from_numpy(x), torch.from_numpy(labels)).numpy()

    ref = oracle_map.sense_map(x_init, meas, score_np, lambda v: kspace.sense_forward(v, maps, mask),
                               lambda s: kspace.sense_adjoint(s, maps), lamda, lr, n_iters)
    assert np.abs(ref - x_init).max() > 0.5 * n_iters * lr                     # the optimiser moved the image
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps, normalize=False)
    cfg = tiny_config()
    cfg.MAP = Namespace(n_iters=n_iters, lr=lr, complex_inner_n_steps=20)
    opt = pkg.map.MAPOptimizer(torch.from_numpy(x_init.copy()).cuda(), torch.from_numpy(meas).cuda(), tiny_net, op, lamda, cfg,
                               logger=None, device=torch.device("cuda"))
    x = opt().cpu().numpy()
    print("map max err", np.abs(x - ref).max(), "tolerance", 0.02 * n_iters * lr)
    np.testing.assert_allclose(x, ref, atol=0.02 * n_iters * lr)
    assert metrics.nrmse(np.abs(x), np.abs(ref)) < 1e-3
    # the real part of the maps alone is another problem: the phase took effect
    op_r = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps.real.copy(), normalize=False)
    x_r = pkg.map.MAPOptimizer(torch.from_numpy(x_init.copy()).cuda(), torch.from_numpy(meas).cuda(), tiny_net, op_r, lamda,
                               cfg, logger=None, device=torch.device("cuda"))().cpu().numpy()
    assert np.abs(x_r - ref).max() > 0.02 * n_iters * lr


# ---- 8. drivers -----------------------------------------------------------------------------------------
_DRIVERS = {
    "acdc_SENSE_real_img.py": ["--R", "40", "--num_samples", "2", "--num_sens", "4", "--seed", "0", "--seg_start_time", "1.0",
                               "--n_levels", "2"],
    "acdc_SENSE_MAP.py": ["--R", "8", "--n_iters", "3", "--lamda", "0.01"],
    "acdc_SENSE_TV.py": ["--R", "5", "--num_epochs", "20", "--lr", "0.01", "--reg_weight", "0.01"],
    "cine_SENSE_real_img_2d_time.py": ["--R", "8", "--num_samples", "1", "--mode_T", "diffusion1d", "--lamda_T", "10.0",
                                       "--image_size", "64", "--start_level", "996", "--n_levels", "2"],
    "cine_SENSE_real_img_2d_time_MAP.py": ["--ds_name", "CINE127", "--R", "6", "--num_iters", "2", "--lr", "0.001", "--mode_T",
                                           "diffusion1d"],
}


def _run_driver(script, args, save_dir):
    """one fresh child process with a time limit (the arguments are those of the drivers' own script tests)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "scripts", script)] + args + ["--save_dir", save_dir],
                       capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stderr[-3000:]
    maps = torch.load(os.path.join(save_dir, "sens_maps.pt"), weights_only=False)
    rec = torch.load(os.path.join(save_dir, "reconstructions.pt"), weights_only=False)
    assert rec.dtype == torch.complex64 and torch.isfinite(torch.view_as_real(rec)).all()
    assert tuple(maps.shape[-2:]) == tuple(rec.shape[-2:])
    return maps, rec


@pytest.mark.parametrize("script", sorted(_DRIVERS))
def test_driver_with_synthetic_complex_maps(tmp_path, script):
    """--sens_phase: the driver runs on synthetic complex maps, saves them as sens_maps.pt, reconstructions are finite"""
    maps, rec = _run_driver(script, _DRIVERS[script] + ["--sens_phase"], str(tmp_path))
    assert maps.dtype == torch.complex128 and maps.shape[0] == 4 and maps.imag.abs().max() > 0.1
    np.testing.assert_allclose((maps.abs() ** 2).sum(0).numpy(), 1.0, atol=1e-12)


def test_driver_with_maps_from_a_file(tmp_path):
    """--sens_maps PATH: three measured (complex64, unnormalised, masked) coils from a .npy file set the coil count"""
    raw = (_maps(3, 128, 128, seed=5) * 7.0).astype(np.complex64)
    raw[:, :9] = 0
    np.save(tmp_path / "maps.npy", raw)
    maps, rec = _run_driver("acdc_SENSE_TV.py", _DRIVERS["acdc_SENSE_TV.py"] + ["--sens_maps", str(tmp_path / "maps.npy")],
                            str(tmp_path / "out"))
    assert maps.dtype == torch.complex128 and tuple(maps.shape) == (3, 128, 128) and not maps[:, :9].any()
    np.testing.assert_allclose((maps[:, 9:].abs() ** 2).sum(0).numpy(), 1.0, atol=1e-6)
    meas = torch.load(tmp_path / "out" / "measurement.pt", weights_only=False)
    assert meas.shape[0] == 3
