"""Non-Cartesian SENSE on the GPU: the one-off non-uniform DFT kernels, the Toeplitz normal operator, the
conjugate-gradient proximal, the fused Langevin + proximal tail and the sampler, against the float64 restatement of
tests/noncart_helpers.py.  Tolerances: ten times the largest error observed on the MI355X (the table in DESIGN.md 4.4l);
the metric of every float64 comparison is max|err| / max|ref|."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import noncart_helpers as nh
from conftest import state_dict_from_golden

pytestmark = pytest.mark.gpu

SCHED = [("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"), ("rsv", "f4")]

# 10 x the largest figure observed on the MI355X over the cases below (DESIGN.md 4.4l lists the observed figures)
TOL = dict(forward=5.7e-7, adjoint=5.6e-7, psf=7.7e-7, normal=3.2e-6, normal_vs_direct=3.5e-6, dot=1.1e-6, psf_symmetry=6.1e-7,
           cartesian_ahy=1.3e-6, cartesian_cg=4.7e-6, cg_solution=2.4e-4, cg_residual=1e-4, sampler=9.2e-5)

# image, B, coils: 16x16 and 48x80 pad to at most 16384 pixels (power of two; radix 3 and 5), 64x80 and 128x128 beyond
SHAPES = [(16, 16, 3, 4), (48, 80, 1, 5), (64, 80, 3, 1), (128, 128, 1, 2)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ALD_optimizers, proximal_op
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier, noncartesian
    return Namespace(ncsnv2=ncsnv2, ald=ALD_optimizers, prox=proximal_op, uf=undersampling_fourier, nc=noncartesian)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def cplx(re, im):
    return host(re).astype(np.complex128) + 1j * host(im)


_CASES = {}


def case(H, W, B, n, weighted):
    """inputs and float64 references of one shape, computed once: 7 spokes x 33 readouts plus the points -N/2, +N/2 and 0
    (237 samples: no multiple of 64), the float32 values the GPU gets"""
    key = (H, W, B, n, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(H * 131 + W + 7 * n)
        k = nh.edge_trajectory(7, 33, H, W)
        w = nh.ramp_weights(k, H, W).astype(np.float32) if weighted else None
        S = nh.smooth_maps(n, H, W, seed=n)
        x = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
        y = (rng.standard_normal((n, B, len(k))) + 1j * rng.standard_normal((n, B, len(k)))).astype(np.complex64)
        P = nh.toeplitz_psf(k, H, W, w)
        _CASES[key] = Namespace(H=H, W=W, B=B, n=n, k=k, w=w, S=S, x=x, y=y, P=P, Ax=nh.sense_forward(x, S, k),
                                AHy=nh.sense_adjoint(y, S, k, H, W, w), coil_imgs=nh.ndft_adjoint(y, k, H, W, w),
                                Tx=nh.toeplitz_normal(x, S, P), kd=dev(k), wd=None if w is None else dev(w), Sd=dev(S))
    return _CASES[key]


# ---- 1. kernel stages against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("H,W,B,n", SHAPES)
def test_stages_vs_float64(ops, H, W, B, n, weighted):
    c = case(H, W, B, n, weighted)
    e = {}
    e["forward"] = nh.relerr(host(ops.ndft_forward(dev(c.x), c.kd, c.Sd)), c.Ax)
    imgs = (c.S[:, None] * c.x[None]).astype(np.complex64)                     # coil images, no maps in the kernel
    e["forward_coils"] = nh.relerr(host(ops.ndft_forward(dev(imgs), c.kd)), nh.ndft_forward(imgs, c.k))
    e["adjoint"] = nh.relerr(host(ops.ndft_adjoint(dev(c.y), c.kd, H, W, c.Sd, c.wd)), c.AHy)
    e["adjoint_coils"] = nh.relerr(host(ops.ndft_adjoint(dev(c.y), c.kd, H, W, None, c.wd)), c.coil_imgs)
    psf = ops.toeplitz_psf(c.kd, H, W, c.wd)
    e["psf"] = nh.relerr(host(psf), c.P)
    e["normal"] = nh.relerr(host(ops.toeplitz_normal(dev(c.x), dev(c.P.astype(np.float32)), c.Sd)), c.Tx)
    e["normal_gpu_psf"] = nh.relerr(host(ops.toeplitz_normal(dev(c.x), psf, c.Sd)), c.Tx)
    if n == 1:                                                                 # sens None: S = 1
        one = nh.toeplitz_normal(c.x, None, c.P)
        e["normal_nomaps"] = nh.relerr(host(ops.toeplitz_normal(dev(c.x), psf)), one)
    print(f"stages {H}x{W} B={B} n={n} weighted={weighted}: " + "  ".join(f"{k} {v:.3g}" for k, v in e.items()))
    assert psf.dtype == torch.float32 and tuple(psf.shape) == (2 * H, 2 * W) and float(psf.min()) < 0
    for name, v in e.items():
        assert v <= TOL[name.split("_")[0]], (name, v)


# ---- 2. consistency without an oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("H,W,B,n", SHAPES)
def test_consistency(ops, H, W, B, n, weighted):
    c = case(H, W, B, n, weighted)
    psf = ops.toeplitz_psf(c.kd, H, W, c.wd)
    xd, yd = dev(c.x), dev(c.y)
    Ax = ops.ndft_forward(xd, c.kd, c.Sd)
    direct = host(ops.ndft_adjoint(Ax, c.kd, H, W, c.Sd, c.wd))
    e_n = nh.relerr(host(ops.toeplitz_normal(xd, psf, c.Sd)), direct)
    AHy = host(ops.ndft_adjoint(yd, c.kd, H, W, c.Sd))                          # the dot test: no weights
    lhs = np.vdot(c.y.astype(np.complex128), host(Ax).astype(np.complex128))
    rhs = np.vdot(AHy.astype(np.complex128), c.x.astype(np.complex128))
    e_d = abs(lhs - rhs) / abs(lhs)
    # P(-k) = P(k) holds when T is real, i.e. for a trajectory that holds -k with every k (equal weights): the spectrum of
    # a general trajectory is real but not symmetric (T is Hermitian in the lag, not real)
    k2 = dev(np.concatenate([c.k, -c.k]))
    w2 = None if c.w is None else dev(np.concatenate([c.w, c.w]))
    p = host(ops.toeplitz_psf(k2, H, W, w2)).astype(np.float64)
    sym = np.abs(p[1:, 1:] - p[1:, 1:][::-1, ::-1]).max() / np.abs(p).max()     # (r, c) -> (2H - r, 2W - c)
    print(f"consistency {H}x{W} weighted={weighted}: normal vs adjoint(forward) {e_n:.3g}  dot {e_d:.3g}  psf symmetry {sym:.3g}")
    assert e_n <= TOL["normal_vs_direct"] and e_d <= TOL["dot"] and sym <= TOL["psf_symmetry"]


# ---- 3. Cartesian cross-check -------------------------------------------------------------------------------------------
def _grid_trajectory(mask2d):
    H, W = mask2d.shape
    r, c = np.nonzero(mask2d)
    return np.stack([r - H / 2, c - W / 2], axis=1).astype(np.float64), r, c


@pytest.mark.parametrize("H,W,kind", [(16, 16, "line"), (64, 80, "line"), (16, 16, "2d"), (64, 80, "2d")])
def test_cartesian_cross_check(ops, H, W, kind):
    from inverseproblemwithdiffusionmodel_amd.synthetic import vd_mask_2d
    rng = np.random.default_rng(3)
    B, n = 3, 4
    if kind == "line":
        cols = rng.random(W) < 0.4
        cols[W // 2 - 2:W // 2 + 2] = True
        mask2d = np.repeat(cols[None], H, axis=0)
        m8 = dev(cols[None].astype(np.uint8))
    else:
        mask2d = vd_mask_2d(H, W, 3, seed=1).numpy()[0, 0]
        m8 = dev(mask2d[None].astype(np.uint8))
    k, r, c = _grid_trajectory(mask2d)
    S = nh.smooth_maps(n, H, W, seed=5)
    Sd, kd = dev(S), dev(k)
    img = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
    y_grid = ops.sense_forward(dev(img), Sd, m8)                                # (n, B, H, W), masked
    y_nc = y_grid[:, :, dev(r), dev(c)].contiguous()                           # the same samples as a list
    ahy_c = ops.sense_adjoint(y_grid, Sd, m8, apply_mask=True)
    ahy_n = ops.ndft_adjoint(y_nc, kd, H, W, Sd)
    e_a = nh.relerr(host(ahy_n), host(ahy_c))
    z = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
    psf = ops.toeplitz_psf(kd, H, W)
    errs = []
    for a in (1.0, 4.0):
        c_re, c_im, it_c = ops.sense_cgprox(dev(z.real), dev(z.imag), y_grid, Sd, m8, a, max_iter=40, tol=1e-5)
        n_re, n_im, it_n = ops.nc_sense_cgprox(dev(z.real), dev(z.imag), ahy_n, Sd, psf, a, max_iter=40, tol=1e-5)
        errs.append(nh.relerr(cplx(n_re, n_im), cplx(c_re, c_im)))
        assert (0 < host(it_n)).all() and (host(it_n) < 40).all()
    print(f"cartesian {H}x{W} {kind}: A^H y {e_a:.3g}  CG solutions {errs}")
    assert e_a <= TOL["cartesian_ahy"] and max(errs) <= TOL["cartesian_cg"]


# ---- 4. proximal --------------------------------------------------------------------------------------------------------
PROX_CASES = [(16, 16, 8, 32), (16, 32, 6, 40), (24, 40, 10, 64)]


def _prox_problem(H, W, spokes, readout, B=3, n=4):
    rng = np.random.default_rng(H + W)
    k = nh.radial(spokes, readout, H, W)
    S = nh.smooth_maps(n, H, W, seed=1)
    z = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
    img = (rng.random((B, H, W)) * np.exp(1j * rng.standard_normal((B, H, W)))).astype(np.complex64)
    y = nh.sense_forward(img, S, k).astype(np.complex64)
    return Namespace(H=H, W=W, B=B, n=n, k=k, S=S, z=z, y=y, kd=dev(k), Sd=dev(S))


@pytest.mark.parametrize("a", [1.0, 4.0])
@pytest.mark.parametrize("H,W,spokes,readout", PROX_CASES)
def test_cgprox_vs_float64(ops, H, W, spokes, readout, a):
    p = _prox_problem(H, W, spokes, readout)
    ahy = ops.ndft_adjoint(dev(p.y), p.kd, H, W, p.Sd)
    psf = ops.toeplitz_psf(p.kd, H, W)
    o_re, o_im, iters = ops.nc_sense_cgprox(dev(p.z.real), dev(p.z.imag), ahy, p.Sd, psf, a, max_iter=40, tol=1e-5)
    x = cplx(o_re, o_im)
    ahy64 = nh.sense_adjoint(p.y, p.S, p.k, H, W)
    P = nh.toeplitz_psf(p.k, H, W)
    ref, it64 = nh.cg_prox(p.z, ahy64, lambda v: nh.toeplitz_normal(v, p.S, P), a, 40, 1e-5)
    res = nh.prox_residual(x, p.z.astype(np.complex128), ahy64, p.S, p.k, a)
    err = nh.relerr(x, ref)
    it = host(iters)
    print(f"cgprox {H}x{W} a={a}: iters {it} float64 iters {it64}  |x - x64| {err:.3g}  residual {res}")
    assert (0 < it64).all() and (it64 < 40).all(), "the float64 reference itself must converge below the cap"
    assert (0 < it).all() and (it < 40).all()
    assert err <= TOL["cg_solution"] and res.max() <= TOL["cg_residual"]


def test_cgprox_edge_cases(ops):
    p = _prox_problem(16, 16, 8, 32)
    H = W = 16
    ahy = ops.ndft_adjoint(dev(p.y), p.kd, H, W, p.Sd)
    psf = ops.toeplitz_psf(p.kd, H, W)
    z_re, z_im = dev(p.z.real), dev(p.z.imag)
    # a = 0: z exactly, no iteration
    o_re, o_im, it = ops.nc_sense_cgprox(z_re, z_im, ahy, p.Sd, psf, 0.0, max_iter=40)
    assert torch.equal(o_re, z_re) and torch.equal(o_im, z_im) and not it.any()
    # a sample with z = 0, y = 0 freezes at once and stays finite
    z0_re, z0_im, ahy0 = z_re.clone(), z_im.clone(), ahy.clone()
    z0_re[1], z0_im[1], ahy0[1] = 0, 0, 0
    o_re, o_im, it = ops.nc_sense_cgprox(z0_re, z0_im, ahy0, p.Sd, psf, 1.0, max_iter=40)
    assert host(it)[1] == 0 and not o_re[1].any() and not o_im[1].any() and torch.isfinite(o_re).all()
    # a NaN in one sample leaves the other samples' bits unchanged
    base_re, base_im, base_it = ops.nc_sense_cgprox(z_re, z_im, ahy, p.Sd, psf, 1.0, max_iter=40)
    zn = z_re.clone()
    zn[1, 3, 5] = float("nan")
    n_re, n_im, n_it = ops.nc_sense_cgprox(zn, z_im, ahy, p.Sd, psf, 1.0, max_iter=40)
    for b in (0, 2):
        assert torch.equal(n_re[b], base_re[b]) and torch.equal(n_im[b], base_im[b]) and n_it[b] == base_it[b]
    # refusals of the wrapper
    with pytest.raises(TypeError):
        ops.nc_sense_cgprox(z_re.double(), z_im, ahy, p.Sd, psf, 1.0)
    with pytest.raises(TypeError):
        ops.nc_sense_cgprox(z_re, z_im, ahy.to(torch.complex128), p.Sd, psf, 1.0)
    with pytest.raises(TypeError):
        ops.toeplitz_normal(dev(p.z)[:, ::2], psf, p.Sd)
    with pytest.raises(ValueError, match="max_iter"):
        ops.nc_sense_cgprox(z_re, z_im, ahy, p.Sd, psf, 1.0, max_iter=0)
    with pytest.raises(ValueError, match="ahy"):
        ops.nc_sense_cgprox(z_re, z_im, None, p.Sd, psf, 1.0)


# ---- 5. fused tail ------------------------------------------------------------------------------------------------------
def _tail_problem(ops, H, W, B=3, n=4):
    p = _prox_problem(H, W, 8, 32, B=B, n=n)
    rng = np.random.default_rng(9)
    p.g = rng.standard_normal((2, B, H, W)).astype(np.float32)
    p.nz = rng.standard_normal((2, B, H, W)).astype(np.float32)
    p.ahy = ops.ndft_adjoint(dev(p.y), p.kd, H, W, p.Sd)
    p.psf = ops.toeplitz_psf(p.kd, H, W)
    p.work = ops.nc_sense_cg_workspace(B, n, H, W, "cuda")
    return p


@pytest.mark.parametrize("H,W", [(16, 16), (64, 80)])
def test_fused_tail_is_langevin_then_cgprox(ops, H, W):
    p = _tail_problem(ops, H, W)
    B = p.B
    step, ns, a, step_id = 0.37, float(np.sqrt(2 * 0.37)), 1.5, (1 << 33) + 5
    kw = dict(max_iter=12, tol=1e-5)

    def two_calls(noise, seed=11, off=4):
        x_re, x_im = dev(p.z.real), dev(p.z.imag)
        for plane, (xp, gp) in enumerate(((x_re, p.g[0]), (x_im, p.g[1]))):
            nzp = dev(p.nz[plane]) if noise else ops.philox_normal(tuple(xp.shape), "cuda", seed=seed, sample_offset=off,
                                                                   step_id=step_id, plane=plane)
            ops.langevin_step(xp, dev(gp), step, ns, noise=nzp)
        return ops.nc_sense_cgprox(x_re, x_im, p.ahy, p.Sd, p.psf, a, **kw)

    def fused(noise, seed=11, off=4, B0=0, B1=B, **extra):
        x_re, x_im = dev(p.z.real[B0:B1]), dev(p.z.imag[B0:B1])
        nkw = dict(noise_re=dev(p.nz[0][B0:B1]), noise_im=dev(p.nz[1][B0:B1])) if noise else dict(seed=seed, sample_offset=off)
        sc = dict(step=step, noise_scale=ns, coef=a, step_id=step_id) if not extra else {}
        work = p.work if B1 - B0 == B else ops.nc_sense_cg_workspace(B1 - B0, p.n, H, W, "cuda")
        it = ops.ald_nc_sense_cg_step(x_re, x_im, dev(p.g[0][B0:B1]), dev(p.g[1][B0:B1]), p.ahy[B0:B1].contiguous(), p.Sd,
                                      p.psf, work, **nkw, **sc, **extra, **kw)
        return x_re, x_im, it

    for noise in (True, False):
        r_re, r_im, r_it = two_calls(noise)
        f_re, f_im, f_it = fused(noise)
        assert torch.equal(f_re, r_re) and torch.equal(f_im, r_im) and torch.equal(f_it, r_it), f"noise injected: {noise}"
        assert (0 < host(f_it)).all()
        # a device schedule record, shared (stride 0) and one per sample (stride 1)
        rec = np.zeros(1, dtype=SCHED)
        rec["step"], rec["ns"], rec["coef"], rec["id"] = step, ns, a, step_id
        s_re, s_im, s_it = fused(noise, dev_sched=dev(rec.view(np.uint8)))
        assert torch.equal(s_re, r_re) and torch.equal(s_im, r_im) and torch.equal(s_it, r_it)
        recs = np.repeat(rec, B)
        t_re, t_im, t_it = fused(noise, sample_sched=dev(recs.view(np.uint8)))
        assert torch.equal(t_re, r_re) and torch.equal(t_im, r_im) and torch.equal(t_it, r_it)
    # row b of the B = 3 call == the B = 1 call with sample_offset = b (Philox)
    f_re, f_im, f_it = fused(False, off=0)
    for b in range(B):
        o_re, o_im, o_it = fused(False, off=b, B0=b, B1=b + 1)
        assert torch.equal(o_re[0], f_re[b]) and torch.equal(o_im[0], f_im[b]) and o_it[0] == f_it[b]


# ---- 6. sampler ---------------------------------------------------------------------------------------------------------
def tiny_config(size):
    """the configuration of the tiny NCSNv2Deepest whose weights g07 holds (as the existing CG sampler tests)"""
    return Namespace(
        device=torch.device("cuda"),
        data=Namespace(channels=1, image_size=size, logit_transform=False, rescaled=False,
                       uniform_dequantization=False, gaussian_dequantization=False),
        model=Namespace(ngf=4, num_classes=10, sigma_begin=1.0, sigma_end=0.01, sigma_dist="geometric",
                        normalization="InstanceNorm++", nonlinearity="elu", spec_norm=False),
        recons=Namespace(sigma_dist="geometric", sigma_begin=1.0, sigma_end=0.01, num_classes=10),
        sampling=Namespace(n_steps_each=3, step_lr=9e-7, final_only=True, denoise=True))


class _Tape:
    def __init__(self, tape):
        self.tape, self.i = tape, 0

    def __call__(self, like):
        n = torch.from_numpy(self.tape[self.i])
        self.i += 1
        return n


N_LEVELS, N_EACH, STEP_LR = 4, 3, 9e-7


def _sampler_case(golden, H, W):
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    B, n = 2, 4
    rng = np.random.default_rng(H)
    k = nh.radial(8, 32, H, W)
    S = nh.smooth_maps(n, H, W, seed=3)
    img = torch.cat([phantom_image(H, W, seed=s) for s in range(B)], dim=0).numpy()[:, 0].astype(np.complex64)
    y = nh.sense_forward(img, S, k).astype(np.complex64)
    sigmas = np.geomspace(1.0, 0.01, 10).astype(np.float32)[:N_LEVELS]
    noise = rng.standard_normal((2 * N_LEVELS * N_EACH, B, 1, H, W)).astype(np.float32)
    return Namespace(H=H, W=W, B=B, n=n, k=k, S=S, y=y, sigmas=sigmas, noise=noise, lr_scaled=1.0 / STEP_LR)


def _reference_sampler(golden, c):
    """the sampler's loop with the float64 restatement: the oracle's score network in float32 planes, the Langevin update,
    then the float64 CG solution of (I + a A^H A) x = z + a A^H y, a = step_lr * lr_scaled (tests/cg_helpers.py's pattern)"""
    from oracle import scorenet as oracle_net, ald as oracle_ald
    from inverseproblemwithdiffusionmodel_amd.synthetic import radial_density
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state_dict_from_golden(golden("g07_layers"), "net").items()}

    def score(x, labels):
        with torch.no_grad():
            return oracle_net.ncsnv2_deepest(x, labels, sd)
    H, W, B = c.H, c.W, c.B
    ahy = nh.sense_adjoint(c.y, c.S, c.k, H, W)
    P = nh.toeplitz_psf(c.k, H, W)
    x = nh.sense_adjoint(c.y, c.S, c.k, H, W, radial_density(c.k, H, W).numpy().astype(np.float32)).astype(np.complex64)
    x_re = torch.from_numpy(np.ascontiguousarray(x.real))[:, None]
    x_im = torch.from_numpy(np.ascontiguousarray(x.imag))[:, None]
    tape = _Tape(c.noise)
    sigmas = torch.from_numpy(c.sigmas)
    for lv in range(len(sigmas)):
        labels = torch.full((B,), lv, dtype=torch.long)
        step = oracle_ald.step_size_of(STEP_LR, sigmas[lv], sigmas[-1])
        for _ in range(N_EACH):
            g_re, g_im = score(x_re, labels), score(x_im, labels)
            x_re = x_re + step * g_re + tape(x_re) * torch.sqrt(step * 2)
            x_im = x_im + step * g_im + tape(x_im) * torch.sqrt(step * 2)
            z = (x_re.numpy() + 1j * x_im.numpy())[:, 0].astype(np.complex64)
            z, _ = nh.cg_prox(z, ahy, lambda v: nh.toeplitz_normal(v, c.S, P), STEP_LR * c.lr_scaled, 200, 1e-12)
            z = z.astype(np.complex64)
            x_re = torch.from_numpy(np.ascontiguousarray(z.real))[:, None]
            x_im = torch.from_numpy(np.ascontiguousarray(z.imag))[:, None]
    return (x_re.numpy() + 1j * x_im.numpy()).astype(np.complex64)


def _run_sampler(pkg, golden, c, use_graph, **kw):
    net = pkg.ncsnv2.NCSNv2Deepest(tiny_config(c.H))
    net.load_state_dict(state_dict_from_golden(golden("g07_layers"), "net"), strict=True)
    net = net.cuda().eval()
    op = pkg.nc.NonCartesianSENSE(c.k, (1, c.H, c.W), sens_maps=c.S, normalize=False)
    prox = pkg.prox.L2PenaltyCG(op, max_iter=30, tol=1e-6)
    meas = torch.from_numpy(c.y).cuda().reshape(c.n, c.B, 1, -1)
    params = dict(n_steps_each=N_EACH, step_lr=STEP_LR, denoise=False, final_only=True)
    sampler = pkg.ald.ALDInvSegProximalRealImag(prox, 1.0, "linear", (c.B, 1, c.H, c.W), net, torch.from_numpy(c.sigmas).cuda(),
                                                params, tiny_config(c.H), meas, op, seg=None, device=torch.device("cuda"))
    first = kw.get("start_level", 0) * 2 * N_EACH
    tape = _Tape(c.noise[first:])
    x = sampler(label=None, lamda=1.0, save_dir=None, lr_scaled=c.lr_scaled, seg_mode="full", noise_fn=tape,
                use_graph=use_graph, **kw)[0]
    return x, prox


@pytest.mark.parametrize("H,W", [(16, 16), (64, 80)])
def test_sampler(pkg, golden, H, W):
    c = _sampler_case(golden, H, W)
    x_eager, prox = _run_sampler(pkg, golden, c, False)
    x_graph, prox_g = _run_sampler(pkg, golden, c, True)
    assert torch.equal(x_eager, x_graph) and torch.equal(prox.last_iters, prox_g.last_iters)   # hipGraph == eager
    it = host(prox.last_iters)
    assert (0 < it).all() and (it < 30).all()
    # a sliced run continues the full run's bits
    x_a, _ = _run_sampler(pkg, golden, c, True, n_levels=2)
    x_b, _ = _run_sampler(pkg, golden, c, True, start_level=2, n_levels=2, x_init=x_a)
    assert torch.equal(x_b, x_graph)
    ref = _reference_sampler(golden, c)
    e = nh.relerr(x_graph.numpy(), ref)
    print(f"sampler {H}x{W}: vs the float64-proximal loop {e:.3g}  iters {it}")
    assert x_graph.shape == ref.shape and np.isfinite(x_graph.numpy()).all() and e <= TOL["sampler"]


# ---- 7. driver ----------------------------------------------------------------------------------------------------------
def _driver(*args):
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(repo, "scripts", "acdc_SENSE_real_img.py")] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


DRIVER_COMMON = ["--image_size", 16, "--num_samples", 2, "--num_sens", 4, "--seed", 0, "--seg_start_time", 1.0, "--n_levels", 2,
                 "--lr_scaled", 1.0 / 9e-7, "--cg_iters", 20]


def test_driver_radial(tmp_path):
    out = _driver("--trajectory", "radial", "--spokes", 8, "--readout", 32, "--save_dir", tmp_path, *DRIVER_COMMON)
    assert "reconstruction error" in out
    rec, k, zf, meas = (torch.load(tmp_path / f) for f in ("reconstructions.pt", "trajectory.pt", "ZF.pt", "measurement.pt"))
    assert tuple(rec.shape) == (2, 1, 16, 16) and tuple(k.shape) == (256, 2) and tuple(zf.shape) == (1, 1, 16, 16)
    assert tuple(meas.shape) == (4, 1, 1, 256) and k.dtype == torch.float64
    assert np.allclose(k.numpy(), nh.radial(8, 32, 16, 16), rtol=0, atol=1e-12)
    assert torch.isfinite(torch.view_as_real(rec)).all() and torch.isfinite(torch.view_as_real(zf)).all()
    assert not (tmp_path / "mask.pt").exists()


def test_driver_measured_samples(tmp_path):
    """--kspace / --trajectory / --sens_maps on files the test writes: samples of a phantom through the float64 transform"""
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    k, S = nh.radial(8, 32, 16, 16), nh.smooth_maps(4, 16, 16, seed=2)
    y = 37.0 * nh.sense_forward(phantom_image(16, 16, seed=0).numpy()[:, 0], S, k)[:, 0]      # arbitrary scanner units
    np.save(tmp_path / "y.npy", y.astype(np.complex64))
    np.save(tmp_path / "k.npy", k)
    np.save(tmp_path / "maps.npy", S)
    out = _driver("--kspace", tmp_path / "y.npy", "--trajectory", tmp_path / "k.npy", "--sens_maps", tmp_path / "maps.npy",
                  "--save_dir", tmp_path / "out", *DRIVER_COMMON)
    assert "k-space scale" in out and "RMSE" not in out
    rec, zf = torch.load(tmp_path / "out" / "reconstructions.pt"), torch.load(tmp_path / "out" / "ZF.pt")
    assert tuple(rec.shape) == (2, 1, 16, 16) and torch.isfinite(torch.view_as_real(rec)).all()
    assert abs(float(zf.abs().max()) - 1.0) < 1e-5                            # the automatic scale: peak |zero_filled| = 1
    assert torch.equal(torch.load(tmp_path / "out" / "trajectory.pt"), torch.from_numpy(k))
    assert not (tmp_path / "out" / "original.pt").exists()
