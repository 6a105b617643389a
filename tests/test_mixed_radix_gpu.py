"""k-space kernels at image sides 2^a 3^b 5^c (radix-3 and radix-5 Stockham stages, per-axis factor sets, strips whose
height is a divisor of the side): the transform, every SENSE / single-coil operator, the conjugate-gradient proximal, the
fused steps, the sampler and the driver at sizes that had no kernel before.

Shapes: 48 runs one radix-3 stage, 80 one radix-5 stage, 144 two radix-3 stages, 240 both in one line; 48x80 and 80x48
have another factor set per axis (the twiddle table must serve both); 16x48 mixes a power-of-two axis with a mixed one;
96x160 is the fullest LDS image (every thread's last butterfly slot is used); 80x240, 240x80 and 48x512 take the row /
column path with strips (20, 80 and 16 rows; 80, 20 and 128 columns) that are not 8192 / side; 144x160 too, with strips
that are.

Bounds: 3e-5 max abs error on unit-normal data, the bound of test_mask2d_gpu.py for these kernels (a float32 mixed-radix
FFT is 5e-7 to 9e-7 from float64 at every one of these shapes, as at power-of-two sizes); 2 tol |b| for the CG proximal
(test_cg_prox_gpu.py); the sampler bounds of the existing sampler tests.  Every case asserts that its size has a kernel,
so nothing passes through the direct-DFT fallback of fft2c."""
import functools
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import cg_helpers as cgh
from conftest import state_dict_from_golden
from oracle import kspace, scorenet as oracle_net, ald as oracle_ald, metrics

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 3e-5
TOL = 1e-5
SCHED = [("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"), ("rsv", "f4")]
LDS_SHAPES = [(48, 48), (16, 48), (48, 80), (80, 48), (96, 160)]
STRIP_SHAPES = [(80, 240), (240, 80), (144, 160), (48, 512)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd import synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ALD_optimizers, proximal_op
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier
    return Namespace(ncsnv2=ncsnv2, ald=ALD_optimizers, prox=proximal_op, uf=undersampling_fourier, syn=synthetic)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def cplx(re, im):
    return re.cpu().numpy() + 1j * im.cpu().numpy()


def _maps(kind, n, H, W, seed=2):
    if kind == "real":
        return kspace.sens_maps(n, H, W, seed)
    from inverseproblemwithdiffusionmodel_amd import synthetic
    return synthetic.complex_coil_maps(n, H, W, seed).numpy()


def _sens(maps):
    return dev(maps.astype(np.complex64 if np.iscomplexobj(maps) else np.float32))


def _mask(rng, two_d, T, H, W, frac=0.3):
    """bool (T, 1, H, W) (2-D) or (T, 1, 1, W) (line mask) with the centre sampled, and its device table"""
    if two_d:
        mk = rng.random((T, 1, H, W)) < frac
        mk[:, :, H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = True
        return mk, dev(mk.reshape(T, H, W).astype(np.uint8))
    mk = rng.random((T, 1, 1, W)) < frac
    mk[..., W // 2 - 2:W // 2 + 2] = True
    return mk, dev(mk.reshape(T, W).astype(np.uint8))


def _sched(step, ns, coef, step_id=5):
    s = np.zeros(1, dtype=SCHED)
    s["step"], s["ns"], s["coef"], s["id"] = step, ns, coef, step_id
    return dev(s.view(np.uint8))


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


# ---- 1. the transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", LDS_SHAPES + STRIP_SHAPES)
def test_fft2c_vs_numpy_float64(ops, H, W):
    assert ops.kspace_size_class(H, W) == (1 if H * W <= 16384 else 2)       # a kernel, not the DFT fallback
    rng = np.random.default_rng(H * 1000 + W)
    x = (rng.standard_normal((3, H, W)) + 1j * rng.standard_normal((3, H, W))).astype(np.complex64)
    x64 = x.astype(np.complex128)
    fwd = ops.fft2c(dev(x))
    inv = ops.fft2c(dev(x), inverse=True)
    back = ops.fft2c(fwd, inverse=True)
    e = dict(forward=np.abs(fwd.cpu().numpy() - cgh.fft2c(x64)).max(), inverse=np.abs(inv.cpu().numpy() - cgh.ifft2c(x64)).max(),
             round_trip=np.abs(back.cpu().numpy() - x64).max())
    print(f"{H}x{W}", {k: float(v) for k, v in e.items()})
    for k, v in e.items():
        assert v < BOUND, (k, v)


# ---- 2. every operator against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,n,kind,two_d,T", [
    (48, 80, 3, "real", False, 1), (80, 48, 5, "complex", True, 3), (16, 48, 2, "complex", False, 1),
    (96, 160, 2, "complex", True, 1), (80, 240, 3, "complex", True, 3), (240, 80, 3, "real", False, 1),
    (48, 512, 2, "complex", True, 1)])
def test_operators_vs_oracle(ops, H, W, n, kind, two_d, T):
    assert ops.kspace_size_class(H, W) != 0
    rng = np.random.default_rng(41)
    B = 3
    maps = _maps(kind, n, H, W)
    sens = _sens(maps)
    mask, m8 = _mask(rng, two_d, T, H, W)
    rnd = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    x, s = rnd(B, 1, H, W), rnd(n, B, 1, H, W)
    err = {}
    want = kspace.sense_forward(x, maps, mask)
    Ax = ops.sense_forward(dev(x), sens, m8).cpu().numpy()
    err["forward"] = np.abs(Ax - want).max()
    assert not Ax[:, np.broadcast_to(~mask, (B, 1, H, W))].any()             # exactly zero off the mask
    err["adjoint"] = np.abs(ops.sense_adjoint(dev(s), sens).cpu().numpy() - kspace.sense_adjoint(s, maps)).max()
    AHs = ops.sense_adjoint(dev(s), sens, m8, apply_mask=True).cpu().numpy()
    err["adjoint_masked"] = np.abs(AHs - kspace.sense_adjoint(s, maps, mask)).max()
    lhs = np.vdot(s.astype(np.complex128), Ax.astype(np.complex128))
    rhs = np.vdot(AHs.astype(np.complex128), x.astype(np.complex128))
    ssos = np.sqrt(sum(np.abs(cgh.ifft2c(s[c].astype(np.complex128))) ** 2 for c in range(n)))
    err["ssos"] = np.abs(ops.sense_ssos(dev(s)).cpu().numpy() - ssos).max()
    # L2Penalty closed form and the fused Langevin + proximal step (injected noise, device schedule)
    img = (rng.random((1, 1, H, W)) * np.exp(1j * rng.standard_normal((1, 1, H, W)))).astype(np.complex64)
    y = kspace.sense_forward(np.repeat(img, B, axis=0), maps, mask)
    g = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    nz = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    step, ns = np.float32(0.37), np.float32(np.sqrt(2 * 0.37))
    coef = 0.25                                                              # x stays of unit size: |A^H A| <= 1
    alpha = coef * n * W / 0.05                                              # L2Penalty: coef = 0.05 alpha / (n_coils W)
    z = ((x.real + step * g[0] + nz[0] * ns) + 1j * (x.imag + step * g[1] + nz[1] * ns)).astype(np.complex64)
    want = kspace.l2_penalty_sense(z, y, alpha, 1.0, maps, mask)
    o_re, o_im = ops.sense_l2prox(dev(z.real), dev(z.imag), dev(y), sens, m8, coef)
    err["l2prox"] = np.abs(cplx(o_re, o_im) - want).max()
    work = ops.sense_workspace(B, n, H, W, "cuda")
    x_re, x_im = dev(x.real), dev(x.imag)
    ops.ald_sense_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(y), sens, m8, work, noise_re=dev(nz[0]), noise_im=dev(nz[1]),
                       dev_sched=_sched(step, ns, coef))
    err["ald_sense_step"] = np.abs(cplx(x_re, x_im) - want).max()
    # single coil: L2Penalty (K = B), the 1 / (1 + a m) closed form, projection; plain and fused
    ysc = (mask * kspace.fft2c(np.repeat(img, B, axis=0))).astype(np.complex64)
    kz = kspace.fft2c(z)
    lam = 0.3
    cases = [("sc_l2penalty", ops.SC_L2PENALTY, 0.25, kspace.l2_penalty_single(z, ysc, 0.25 * B / 0.05, 1.0, mask)),
             ("sc_closed_form", ops.SC_CLOSED_FORM, 0.7, kspace.single_coil(z, ysc, 0.7, 1.0, mask)),
             ("sc_projection", ops.SC_PROJECTION, lam, kspace.ifft2c(lam * ysc + (1 - lam) * mask * kz + (1 - mask) * kz))]
    for name, mode, c, want in cases:
        o_re, o_im = ops.singlecoil_prox(dev(z.real), dev(z.imag), dev(ysc), m8, c, mode)
        err[name] = np.abs(cplx(o_re, o_im) - want).max()
        x_re, x_im = dev(x.real), dev(x.imag)
        ops.ald_singlecoil_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(ysc), m8, mode, step=float(step), noise_scale=float(ns),
                                coef=c, noise_re=dev(nz[0]), noise_im=dev(nz[1]))
        err[name + "_step"] = np.abs(cplx(x_re, x_im) - want).max()
    print(f"{H}x{W} n={n} {kind} 2d={two_d} T={T}", {k: float(v) for k, v in err.items()}, "adjointness",
          abs(lhs - rhs) / abs(lhs))
    for k, v in err.items():
        assert v < BOUND, (k, v)
    assert abs(lhs - rhs) < 1e-4 * abs(lhs)                                  # <s, A x> = <A^H s, x>


# ---- 3. the conjugate-gradient proximal ---------------------------------------------------------------------------------
def _cg_float64(z, y, a, maps, mask, iters):
    """`iters` iterations of plain CG on N x = b from x0 = z in float64 (the recurrence of kspace_cg.hip)"""
    b = cgh.rhs(z, y, a, maps, mask)
    x = np.asarray(z, dtype=np.complex128).copy()
    r = b - cgh.normal(x, a, maps, mask)
    p = r.copy()
    dot = lambda u, v: (np.conj(u) * v).real.reshape(u.shape[0], -1).sum(1).reshape(-1, 1, 1, 1)
    rr = dot(r, r)
    for _ in range(iters):
        q = cgh.normal(p, a, maps, mask)
        alpha = rr / dot(p, q)
        x, r = x + alpha * p, r - alpha * q
        rr, old = dot(r, r), rr
        p = r + (rr / old) * p
    return x


@pytest.mark.parametrize("H,W,n,T,B", [(48, 80, 4, 3, 3), (80, 240, 4, 1, 2)])
def test_cg_prox_vs_float64(ops, pkg, H, W, n, T, B):
    assert ops.kspace_size_class(H, W) != 0
    rng = np.random.default_rng(43)
    sens = _sens(_maps("complex", n, H, W))
    maps = sens.cpu().numpy()                                                # the values the GPU sees
    mk, _ = _mask(rng, True, T, H, W)
    mask = mk[np.arange(B) % T]                                              # (B, 1, H, W): image b uses plane b % T
    z = (rng.standard_normal((B, 1, H, W)) + 1j * rng.standard_normal((B, 1, H, W))).astype(np.complex64)
    img = rng.random((1, 1, H, W)) * np.exp(1j * rng.standard_normal((1, 1, H, W)))
    y = cgh.forward(np.repeat(img, B, axis=0), maps, mask).astype(np.complex64)
    op = pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=maps, normalize=False, mask_mode="custom",
                      mask=torch.from_numpy(mk))
    m8 = op.mask_u8("cuda")
    assert tuple(m8.shape) == (T, H, W)
    for a, max_iter in ((1.0, 12), (10.0, 32)):
        prox = pkg.prox.L2PenaltyCG(op, max_iter=max_iter, tol=TOL)
        x_gpu = prox(dev(z), dev(y), a, 1.0)
        x = x_gpu.cpu().numpy().astype(np.complex128)
        iters = prox.last_iters.cpu().numpy()
        b = cgh.rhs(z, y, a, maps, mask)
        bn = cgh.sample_norm(b)
        xstar = cgh.cg_solve(z, y, a, maps, mask)
        res = cgh.sample_norm(b - cgh.normal(x, a, maps, mask)) / bn
        e = cgh.sample_norm(x - xstar) / bn
        chk = float(prox.check_solution(x_gpu, dev(z), dev(y), a, 1.0))
        print(f"{H}x{W} a={a}: |b - Nx|/|b| {res} |x - x*|/|b| {e} check_solution {chk} iters {iters}")
        assert (res <= 2 * TOL).all() and (e <= 2 * TOL).all()
        assert chk <= (2 * TOL) ** 2 * float((bn ** 2).mean())
        assert abs(chk - cgh.check_solution(x, z, y, a, maps, mask)) <= (2 * TOL) ** 2 * float((bn ** 2).mean())
        assert iters.dtype == np.int32 and ((1 <= iters) & (iters < max_iter)).all(), iters
        ahy = ops.sense_adjoint(dev(y), sens, m8, apply_mask=True)
        o_re, o_im, it2 = ops.sense_cgprox(dev(z.real), dev(z.imag), dev(y), sens, m8, a, max_iter=max_iter, tol=TOL, ahy=ahy)
        assert torch.equal(torch.complex(o_re, o_im), x_gpu) and torch.equal(it2, prox.last_iters)
    # the fused tail, tol = 0: exactly 3 iterations, against 3 iterations of the same recurrence in float64
    g = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    nz = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    step, ns, a = np.float32(0.37), np.float32(np.sqrt(2 * 0.37)), 1.0
    zl = ((z.real + step * g[0] + nz[0] * ns) + 1j * (z.imag + step * g[1] + nz[1] * ns)).astype(np.complex64)
    x_re, x_im = dev(z.real), dev(z.imag)
    it = ops.ald_sense_cg_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(y), sens, m8, None, noise_re=dev(nz[0]), noise_im=dev(nz[1]),
                               dev_sched=_sched(step, ns, a), max_iter=3, tol=0.0)
    want = _cg_float64(zl, y, a, maps, mask, 3)
    e = cgh.sample_norm(cplx(x_re, x_im) - want) / cgh.sample_norm(cgh.rhs(zl, y, a, maps, mask))
    print(f"{H}x{W} fused, 3 iterations: |x - x_3|/|b| {e}")
    assert (it.cpu().numpy() == 3).all() and (e <= 2 * TOL).all()


# ---- 4. the fused step against its chain, bitwise -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_inputs(H, W):
    """read-only device tensors of one shape: B = 3, three coils, complex maps, a 2-D mask with a plane per image"""
    from inverseproblemwithdiffusionmodel_amd import synthetic
    rng = np.random.default_rng(H * 1000 + W)
    B, n = 3, 3
    rnd = lambda *s: rng.standard_normal(s).astype(np.float32)
    y = (rng.standard_normal((n, B, H, W)) + 1j * rng.standard_normal((n, B, H, W))).astype(np.complex64)
    _, m8 = _mask(rng, True, B, H, W)
    return dict(B=B, n=n, x_re=dev(rnd(B, H, W)), x_im=dev(rnd(B, H, W)), g_re=dev(rnd(B, H, W)), g_im=dev(rnd(B, H, W)),
                y=dev(y), m8=m8, sens=synthetic.complex_coil_maps(n, H, W, 2).to(torch.complex64).contiguous().cuda())


STEP_KW = dict(step=0.37, noise_scale=float(np.sqrt(2 * 0.37)), coef=0.25, seed=20240611, sample_offset=7, step_id=5)


@pytest.mark.parametrize("H,W", [(48, 80), (80, 240)])
def test_fused_step_equals_separate_chain(ops, H, W):
    """ald_sense_step with Philox noise == philox_normal + langevin_step per plane + sense_l2prox, as int32 patterns"""
    assert ops.kspace_size_class(H, W) != 0
    d = _step_inputs(H, W)
    key = {k: STEP_KW[k] for k in ("seed", "sample_offset", "step_id")}
    z = []
    for plane, (x, g) in enumerate(((d["x_re"], d["g_re"]), (d["x_im"], d["g_im"]))):
        nz = ops.philox_normal(tuple(x.shape), x.device, plane=plane, **key)
        z.append(ops.langevin_step(x.clone(), g, step=STEP_KW["step"], noise_scale=STEP_KW["noise_scale"], noise=nz))
    want = ops.sense_l2prox(z[0], z[1], d["y"], d["sens"], d["m8"], STEP_KW["coef"])
    x_re, x_im = d["x_re"].clone(), d["x_im"].clone()
    ops.ald_sense_step(x_re, x_im, d["g_re"], d["g_im"], d["y"], d["sens"], d["m8"], ops.sense_workspace(d["B"], d["n"], H, W, "cuda"),
                       **STEP_KW)
    for name, got, ref, start in (("re", x_re, want[0], d["x_re"]), ("im", x_im, want[1], d["x_im"])):
        assert torch.isfinite(got).all() and not torch.equal(got, start)
        differ = int((_bits(got) != _bits(ref)).sum())
        assert differ == 0, ((H, W), name, differ, "elements differ, max abs", float((got - ref).abs().max()))


# ---- 5. the one-workgroup-per-sample form of the step, in a fresh child --------------------------------------------------
_STEP_CODE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from inverseproblemwithdiffusionmodel_amd import ops, synthetic

H, W, B, n = 48, 80, 3, 3
g = torch.Generator().manual_seed(83)
x = torch.randn(2, B, H, W, generator=g).cuda(); gr = torch.randn(2, B, H, W, generator=g).cuda()
y = torch.complex(torch.randn(n, B, H, W, generator=g), torch.randn(n, B, H, W, generator=g)).cuda()
m8 = (torch.rand(B, H, W, generator=g) < 0.3).to(torch.uint8)
m8[:, H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = 1
for sens in (synthetic.complex_coil_maps(n, H, W, 2).to(torch.complex64).contiguous().cuda(),
             synthetic.complex_coil_maps(n, H, W, 2).abs().float().contiguous().cuda()):
    for noise in (None, torch.randn(2, B, H, W, generator=g).cuda()):
        a, b = x[0].clone(), x[1].clone()
        kw = {} if noise is None else dict(noise_re=noise[0], noise_im=noise[1])
        ops.ald_sense_step(a, b, gr[0], gr[1], y, sens, m8.cuda(), ops.sense_workspace(B, n, H, W, "cuda"), step=0.3,
                           noise_scale=0.7, coef=0.011, seed=5, sample_offset=9, step_id=1234, **kw)
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, x[0])
        sys.stdout.buffer.write(a.cpu().numpy().tobytes() + b.cpu().numpy().tobytes())
"""


def test_serial_coils_give_the_same_bits():
    """IPDM_SENSE_COILS=0 (read once per process) against the coil-parallel default at 48x80: real and complex maps,
    Philox and injected noise; the children print their outputs' bytes"""
    out = {}
    for arm in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", _STEP_CODE, REPO], env=dict(os.environ, IPDM_SENSE_COILS=arm),
                           capture_output=True, timeout=200)
        assert r.returncode == 0, r.stderr[-3000:]
        out[arm] = torch.frombuffer(bytearray(r.stdout), dtype=torch.int32)
    assert out["1"].numel() == 4 * 2 * 3 * 48 * 80
    assert torch.equal(out["0"], out["1"])


# ---- 6. a sample's bits do not depend on its batch ----------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(48, 80), (80, 240)])
def test_batch_invariance(ops, H, W):
    d = _step_inputs(H, W)
    B, n = d["B"], d["n"]
    one = lambda t, axis=0: t.narrow(axis, 1, 1).clone()                     # a copy: the shared inputs stay as they are
    m1 = one(d["m8"])
    xc = torch.complex(d["x_re"], d["x_im"]).contiguous()
    full = ops.sense_forward(xc, d["sens"], d["m8"])
    alone = ops.sense_forward(one(xc), d["sens"], m1)
    assert torch.equal(full[:, 1:2], alone)
    f_re, f_im = ops.sense_l2prox(d["x_re"], d["x_im"], d["y"], d["sens"], d["m8"], 0.25)
    a_re, a_im = ops.sense_l2prox(one(d["x_re"]), one(d["x_im"]), one(d["y"], 1), d["sens"], m1, 0.25)
    assert torch.equal(f_re[1:2], a_re) and torch.equal(f_im[1:2], a_im)
    x_re, x_im = d["x_re"].clone(), d["x_im"].clone()
    ops.ald_sense_step(x_re, x_im, d["g_re"], d["g_im"], d["y"], d["sens"], d["m8"], ops.sense_workspace(B, n, H, W, "cuda"),
                       **STEP_KW)
    s_re, s_im = one(d["x_re"]), one(d["x_im"])
    kw = dict(STEP_KW, sample_offset=STEP_KW["sample_offset"] + 1)           # the Philox key is the global sample id
    ops.ald_sense_step(s_re, s_im, one(d["g_re"]), one(d["g_im"]), one(d["y"], 1), d["sens"], m1,
                       ops.sense_workspace(1, n, H, W, "cuda"), **kw)
    assert torch.equal(x_re[1:2], s_re) and torch.equal(x_im[1:2], s_im)
    assert not torch.equal(x_re[1:2], d["x_re"][1:2])


# ---- 7. the sampler at 48x80 --------------------------------------------------------------------------------------------
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


class _Tape:
    """injected noise: the recorded arrays, one per call"""

    def __init__(self, tape):
        self.tape, self.i = tape, 0

    def __call__(self, like):
        n = torch.from_numpy(self.tape[self.i])
        self.i += 1
        return n


@pytest.fixture(scope="module")
def sampler_case(pkg, golden):
    """10 levels x 3 steps + denoise at 48x80, B = 2: the tiny NCSNv2Deepest of g07, g08's sigmas, a seeded noise tape,
    complex maps and a variable-density 2-D mask; the CPU oracle sampler, computed once"""
    H, W, B = 48, 80, 2
    g8 = golden("g08_ald")
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state_dict_from_golden(golden("g07_layers"), "net").items()}

    def score(x, labels):
        with torch.no_grad():
            return oracle_net.ncsnv2_deepest(x, labels, sd)

    net = pkg.ncsnv2.NCSNv2Deepest(tiny_config())
    net.load_state_dict(state_dict_from_golden(golden("g07_layers"), "net"), strict=True)
    maps = pkg.syn.complex_coil_maps(4, H, W, 3).numpy()
    mask_t = pkg.syn.vd_mask_2d(H, W, 4, seed=5)
    mask = mask_t.numpy()
    img = torch.cat([pkg.syn.phantom_image(H, W, seed=s) for s in range(B)], dim=0).numpy().astype(np.complex64)
    meas = kspace.sense_forward(img, maps, mask)
    noise = np.random.default_rng(48080).standard_normal((60, B, 1, H, W)).astype(np.float32)
    lr_scaled = float(g8["dc_visible_lr_scaled"])
    ref = oracle_ald.ald_sense_real_imag(score, g8["sigmas"], meas, maps, mask, 9e-7, 3, lr_scaled, True, _Tape(noise))
    return dict(H=H, W=W, B=B, net=net.cuda().eval(), maps=maps, mask_t=mask_t, meas=meas, ref=ref, noise=noise,
                sigmas=g8["sigmas"], lr_scaled=lr_scaled)


def _run_sampler(pkg, c, use_graph):
    H, W, B = c["H"], c["W"], c["B"]
    assert tuple(c["mask_t"].shape) == (1, 1, H, W)
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, H, W), seed=0, sens_maps=c["maps"], normalize=False, mask_mode="custom",
                      mask=c["mask_t"])
    params = dict(n_steps_each=3, step_lr=9e-7, denoise=True, final_only=True)
    meas = torch.from_numpy(c["meas"]).cuda()
    sampler = pkg.ald.ALDInvSegProximalRealImag(pkg.prox.get_proximal("L2Penalty")(op), 1.0, "linear", (B, 1, H, W), c["net"],
                                                torch.from_numpy(c["sigmas"]).cuda(), params, tiny_config(), meas, op, seg=None,
                                                device=torch.device("cuda"))
    tape = _Tape(c["noise"])
    x = sampler(label=None, lamda=1.0, save_dir=None, lr_scaled=c["lr_scaled"], seg_mode="full", noise_fn=tape,
                use_graph=use_graph)[0].numpy()
    assert tape.i == 60
    return op, x


def _close(x, ref, x0, what):
    for b in range(x.shape[0]):
        nr, ss = metrics.nrmse(np.abs(x[b]), np.abs(ref[b])), metrics.ssim(np.abs(x[b, 0]), np.abs(ref[b, 0])) - 1
        print(what, "nrmse", nr, "ssim-1", ss)
        assert nr < 1e-3 and abs(ss) < 1e-3
    disp = np.linalg.norm((x - x0) - (ref - x0)) / np.linalg.norm(ref - x0)
    print(what, "displacement", disp)
    assert disp <= 2e-3


def test_sampler_48x80_vs_oracle(ops, pkg, sampler_case):
    c = sampler_case
    assert ops.kspace_size_class(c["H"], c["W"]) == 1
    op, eager = _run_sampler(pkg, c, False)
    _, graph = _run_sampler(pkg, c, True)
    ref = c["ref"]
    assert eager.shape == graph.shape == ref.shape == (c["B"], 1, c["H"], c["W"])
    assert np.isfinite(eager).all() and np.isfinite(graph).all()
    x0 = op.conj_op(torch.from_numpy(c["meas"]).cuda()).cpu().numpy()
    _close(eager, ref, x0, "eager vs oracle")
    _close(graph, ref, x0, "graph vs oracle")
    _close(graph, eager, x0, "graph vs eager")


# ---- 8. sizes that still have no kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(24, 32), (40, 48), (112, 48)])
def test_sizes_still_refused(ops, H, W):
    from inverseproblemwithdiffusionmodel_amd._lib import IpdmUnsupported
    assert ops.kspace_size_class(H, W) == 0
    B, n = 2, 3
    x = torch.zeros(B, 1, H, W, dtype=torch.complex64, device="cuda")
    y = torch.zeros(n, B, 1, H, W, dtype=torch.complex64, device="cuda")
    sens = torch.ones(n, H, W, dtype=torch.complex64, device="cuda")
    mask = torch.ones(1, W, dtype=torch.uint8, device="cuda")
    p = [torch.ones(B, 1, H, W, device="cuda") for _ in range(4)]
    work = torch.zeros((n + 4) * B * H * W * 2 + 64, device="cuda")          # larger than any path would ask for
    with pytest.raises(IpdmUnsupported):
        ops.sense_forward(x, sens, mask)
    with pytest.raises(IpdmUnsupported):
        ops.sense_l2prox(p[0], p[1], y, sens, mask, 0.01, work=work)
    with pytest.raises(IpdmUnsupported):
        ops.ald_sense_step(p[0], p[1], p[2], p[3], y, sens, mask, work, step=0.1, noise_scale=0.1, coef=0.01)
    with pytest.raises(IpdmUnsupported):
        ops.sense_cgprox(p[0], p[1], y, sens, mask, 1.0, work=work)
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in p)                              # and nothing was written


# ---- 9. the driver ------------------------------------------------------------------------------------------------------
def test_driver_at_48x80(tmp_path):
    args = ["--image_size", "48", "--image_width", "80", "--n_levels", "2", "--R", "4", "--mask_2d", "--num_samples", "1",
            "--num_sens", "4", "--seed", "0", "--seg_start_time", "1.0", "--save_dir", str(tmp_path)]
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py")] + args, capture_output=True,
                       text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    load = lambda name: torch.load(os.path.join(str(tmp_path), name), weights_only=False)
    rec, mask = load("reconstructions.pt"), load("mask.pt")
    assert tuple(rec.shape[-2:]) == (48, 80) and rec.shape[0] == 1 and rec.dtype == torch.complex64
    assert torch.isfinite(torch.view_as_real(rec)).all()
    assert tuple(mask.shape) == (1, 1, 48, 80) and int(mask.sum()) == round(48 * 80 / 4)
    # a size without a kernel: refused by name of the rule, before anything is allocated
    bad = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--image_size", "40",
                          "--image_width", "48", "--save_dir", str(tmp_path / "bad")], capture_output=True, text=True,
                         timeout=120, cwd=REPO)
    assert bad.returncode != 0 and "multiple of 16" in bad.stderr and not os.path.exists(str(tmp_path / "bad"))
