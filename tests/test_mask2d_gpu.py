"""Custom and 2-D k-space sampling masks on the GPU: the uint8 [T][H][W] layout through every SENSE / single-coil kernel
path (whole image in LDS, coil-parallel and serial; row / column strips with the skip rule; the conjugate-gradient
proximal), the product classes, the sampler and the drivers, against the CPU oracle (oracle/kspace.py, oracle/ald.py) and
the float64 CG of tests/cg_helpers.py -- both multiply by whatever mask broadcasts against (B, 1, H, W).

Bounds: 3e-5 max abs error on unit-normal data, the bound of test_sense_complex_maps_gpu.py for these kernels at these
sizes; 2 tol |b| for the CG proximal (test_cg_prox_gpu.py); the sampler bounds of test_sampler_with_complex_maps_vs_oracle.
Every oracle case also shows that reading the mask's first row as a line mask gives a result more than 100 bounds away,
so a kernel that ignored the rows could not pass."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import cg_helpers as cgh
from conftest import state_dict_from_golden
from oracle import kspace, scorenet as oracle_net, ald as oracle_ald, map as oracle_map, metrics

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 3e-5
TOL = 1e-5
SCHED = [("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"), ("rsv", "f4")]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd import synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ALD_optimizers, proximal_op, MAP_optimizers
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier
    return Namespace(ncsnv2=ncsnv2, ald=ALD_optimizers, prox=proximal_op, map=MAP_optimizers, uf=undersampling_fourier,
                     syn=synthetic)


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


def random_mask_2d(rng, T, H, W, frac=0.3):
    """bool (T, 1, H, W): about `frac` of the samples plus a 4 x 4 centre block, another draw per plane"""
    mk = rng.random((T, 1, H, W)) < frac
    mk[:, :, H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = True
    return mk


def _sched(step, ns, coef, step_id=5):
    s = np.zeros(1, dtype=SCHED)
    s["step"], s["ns"], s["coef"], s["id"] = step, ns, coef, step_id
    return dev(s.view(np.uint8))


def _far(a, b, what):
    d = float(np.abs(a - b).max())
    assert d > 100 * BOUND, (what, "the 1-D reading of the mask is only", d, "away")


# ---- 1. oracle sweep ----------------------------------------------------------------------------------------------------
# the first three shapes take the LDS path, the last two the row / column path; B == 3, so with T == 3 image b uses plane b
@pytest.mark.parametrize("H,W,n,T", [(16, 64, 5, 3), (64, 16, 3, 1), (128, 128, 4, 1), (128, 256, 5, 3), (256, 128, 3, 1)])
def test_mask2d_vs_oracle(ops, H, W, n, T):
    rng = np.random.default_rng(41)
    B = 3
    maps = _maps("real" if (H, W) == (16, 64) else "complex", n, H, W)
    sens = _sens(maps)
    mask = random_mask_2d(rng, T, H, W)                                      # (T, 1, H, W)
    line = mask[:, :, :1, :]                                                 # its first row, read as a line mask
    assert (mask != line).mean() > 0.2
    m8 = dev(mask.reshape(T, H, W).astype(np.uint8))
    rnd = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    x, s = rnd(B, 1, H, W), rnd(n, B, 1, H, W)
    err = {}
    # forward, adjoint (SENSE.conj_op: no mask; the true adjoint: masked), adjointness
    want = kspace.sense_forward(x, maps, mask)
    _far(want, kspace.sense_forward(x, maps, line), "forward")
    Ax = ops.sense_forward(dev(x), sens, m8).cpu().numpy()
    err["forward"] = np.abs(Ax - want).max()
    assert not Ax[:, np.broadcast_to(~mask, (B, 1, H, W))].any()             # exactly zero off the mask
    err["adjoint"] = np.abs(ops.sense_adjoint(dev(s), sens).cpu().numpy() - kspace.sense_adjoint(s, maps)).max()
    want = kspace.sense_adjoint(s, maps, mask)
    _far(want, kspace.sense_adjoint(s, maps, line), "adjoint_masked")
    AHs = ops.sense_adjoint(dev(s), sens, m8, apply_mask=True).cpu().numpy()
    err["adjoint_masked"] = np.abs(AHs - want).max()
    lhs = np.vdot(s.astype(np.complex128), Ax.astype(np.complex128))
    rhs = np.vdot(AHs.astype(np.complex128), x.astype(np.complex128))
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
    _far(want, kspace.l2_penalty_sense(z, y, alpha, 1.0, maps, line), "l2prox")
    o_re, o_im = ops.sense_l2prox(dev(z.real), dev(z.imag), dev(y), sens, m8, coef)
    err["l2prox"] = np.abs(cplx(o_re, o_im) - want).max()
    work = ops.sense_workspace(B, n, H, W, "cuda")
    x_re, x_im = dev(x.real), dev(x.imag)
    ops.ald_sense_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(y), sens, m8, work, noise_re=dev(nz[0]), noise_im=dev(nz[1]),
                       dev_sched=_sched(step, ns, coef))
    err["ald_sense_step"] = np.abs(cplx(x_re, x_im) - want).max()
    # single coil: L2Penalty (K = B), the 1 / (1 + a m) closed form, projection
    ysc = (mask * kspace.fft2c(np.repeat(img, B, axis=0))).astype(np.complex64)
    kz = kspace.fft2c(z)
    lam = 0.3
    cases = [("sc_l2penalty", ops.SC_L2PENALTY, 0.25, lambda m: kspace.l2_penalty_single(z, ysc, 0.25 * B / 0.05, 1.0, m)),
             ("sc_closed_form", ops.SC_CLOSED_FORM, 0.7, lambda m: kspace.single_coil(z, ysc, 0.7, 1.0, m)),
             ("sc_projection", ops.SC_PROJECTION, lam, lambda m: kspace.ifft2c(lam * ysc + (1 - lam) * m * kz + (1 - m) * kz))]
    for name, mode, c, ref in cases:
        want = ref(mask)
        _far(want, ref(line), name)
        o_re, o_im = ops.singlecoil_prox(dev(z.real), dev(z.imag), dev(ysc), m8, c, mode)
        err[name] = np.abs(cplx(o_re, o_im) - want).max()
        x_re, x_im = dev(x.real), dev(x.imag)
        ops.ald_singlecoil_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(ysc), m8, mode, step=float(step), noise_scale=float(ns),
                                coef=c, noise_re=dev(nz[0]), noise_im=dev(nz[1]))
        err[name + "_step"] = np.abs(cplx(x_re, x_im) - want).max()
    print(f"{H}x{W} n={n} T={T}", {k: float(v) for k, v in err.items()}, "adjointness", abs(lhs - rhs) / abs(lhs))
    for k, v in err.items():
        assert v < BOUND, (k, v)
    assert abs(lhs - rhs) < 1e-4 * abs(lhs)                                  # <s, A x> = <A^H s, x>


# ---- 2. the skip rule of the row / column path --------------------------------------------------------------------------
def test_mask2d_strip_skip_rule(ops):
    """128 x 256: 64 columns per strip.  Strip 0 has no sample in any row (skippable); strip 1 has the single sample
    (77, 100) and must run; the rest is random.  Clearing (77, 100) must move the output as the oracle says."""
    rng = np.random.default_rng(42)
    B, n, H, W = 2, 4, 128, 256
    maps = _maps("complex", n, H, W)
    sens = _sens(maps)
    mask = rng.random((1, 1, H, W)) < 0.3
    mask[..., :128] = False
    mask[..., 77, 100] = True
    cleared = mask.copy()
    cleared[..., 77, 100] = False
    assert not mask[..., :64].any() and mask[..., 64:128].sum() == 1 and not cleared[..., :128].any()
    rnd = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    z, y_full = rnd(B, 1, H, W), rnd(n, B, 1, H, W)
    g = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    nz = rng.standard_normal((2, B, 1, H, W)).astype(np.float32)
    step, ns, coef = np.float32(0.37), np.float32(np.sqrt(2 * 0.37)), 0.25
    alpha = coef * n * W / 0.05
    zl = ((z.real + step * g[0] + nz[0] * ns) + 1j * (z.imag + step * g[1] + nz[1] * ns)).astype(np.complex64)
    got, want = {}, {}
    for tag, mk in (("with", mask), ("without", cleared)):
        m8 = dev(mk.reshape(1, H, W).astype(np.uint8))
        y = (mk * y_full).astype(np.complex64)
        want[tag] = kspace.l2_penalty_sense(zl, y, alpha, 1.0, maps, mk)
        o_re, o_im = ops.sense_l2prox(dev(zl.real), dev(zl.imag), dev(y), sens, m8, coef)
        x_re, x_im = dev(z.real), dev(z.imag)
        ops.ald_sense_step(x_re, x_im, dev(g[0]), dev(g[1]), dev(y), sens, m8, ops.sense_workspace(B, n, H, W, "cuda"),
                           noise_re=dev(nz[0]), noise_im=dev(nz[1]), dev_sched=_sched(step, ns, coef))
        got[tag] = (cplx(o_re, o_im), cplx(x_re, x_im))
        for name, v in zip(("l2prox", "ald_sense_step"), got[tag]):
            e = np.abs(v - want[tag]).max()
            print(tag, name, "max err", e)
            assert e < BOUND, (tag, name, e)
    d_want = want["with"] - want["without"]
    assert np.abs(d_want).max() > 10 * BOUND                                 # one k-space sample, visible at this coef
    for i, name in enumerate(("l2prox", "ald_sense_step")):
        d_got = got["with"][i] - got["without"][i]
        print(name, "effect of (77, 100)", np.abs(d_got).max(), "oracle", np.abs(d_want).max())
        assert np.abs(d_got - d_want).max() < 2 * BOUND and np.abs(d_got).max() > 10 * BOUND


# ---- 3. a 2-D mask with equal rows is the line mask, bit for bit --------------------------------------------------------
_BIT_CODE = r"""
import torch
from inverseproblemwithdiffusionmodel_amd import ops


def run(H, W):
    g = torch.Generator().manual_seed(79)
    B, n, T = 3, 4, 3
    x = torch.randn(2, B, H, W, generator=g).cuda(); gr = torch.randn(2, B, H, W, generator=g).cuda()
    xc = torch.complex(x[0], x[1]).contiguous()
    y = torch.complex(torch.randn(n, B, H, W, generator=g), torch.randn(n, B, H, W, generator=g)).cuda()
    sens = torch.complex(torch.randn(n, H, W, generator=g), torch.randn(n, H, W, generator=g))
    sens = (sens / sens.abs().pow(2).sum(0).sqrt()).cuda().contiguous()
    line = (torch.rand(T, W, generator=g) < 0.3).to(torch.uint8)
    line[:, W // 2 - 2:W // 2 + 2] = 1
    masks = {"line": line.cuda(), "2d": line[:, None, :].expand(T, H, W).contiguous().cuda()}
    out = {}
    for tag, m in masks.items():
        o = [ops.sense_forward(xc, sens, m), ops.sense_adjoint(y, sens, m, apply_mask=True)]
        ym = ops.sense_forward(torch.complex(gr[0], gr[1]).contiguous(), sens, m)     # a measurement of another image
        o += list(ops.sense_l2prox(x[0], x[1], ym, sens, m, 0.011))
        a, b = x[0].clone(), x[1].clone()
        ops.ald_sense_step(a, b, gr[0], gr[1], ym, sens, m, ops.sense_workspace(B, n, H, W, "cuda"), step=0.3,
                           noise_scale=0.7, coef=0.011, seed=5, sample_offset=9, step_id=1234)
        o += [a, b]
        o += list(ops.sense_cgprox(x[0], x[1], ym, sens, m, 3.0, max_iter=8, tol=1e-5))
        a, b = x[0].clone(), x[1].clone()
        it = ops.ald_sense_cg_step(a, b, gr[0], gr[1], ym, sens, m, None, step=0.3, noise_scale=0.7, coef=3.0, seed=5,
                                   sample_offset=9, step_id=1234, max_iter=8, tol=1e-5)
        o += [a, b, it]
        out[tag] = [t.cpu() for t in o]
    names = ["forward", "adjoint_masked", "l2prox_re", "l2prox_im", "step_re", "step_im", "cg_re", "cg_im", "cg_iters",
             "cgstep_re", "cgstep_im", "cgstep_iters"]
    assert len(names) == len(out["line"])
    for name, p, q in zip(names, out["line"], out["2d"]):
        f = torch.view_as_real(p) if p.is_complex() else p
        assert torch.isfinite(f.float()).all(), name
        assert torch.equal(p, q), (H, W, name)
    assert (out["line"][8] >= 1).all() and not torch.equal(out["line"][4], x[0].cpu())
"""


@pytest.mark.parametrize("H,W", [(32, 32), (128, 256)])
def test_mask2d_equal_rows_is_the_line_mask(ops, H, W):
    ns = {}
    exec(_BIT_CODE, ns)
    ns["run"](H, W)


def test_mask2d_equal_rows_is_the_line_mask_serial_coils():
    """the one-workgroup-per-sample form of the fused step (IPDM_SENSE_COILS=0): the switch is read once per process, so
    the comparison runs in a fresh child"""
    code = "import sys\nsys.path.insert(0, sys.argv[1])\n" + _BIT_CODE + "\nrun(32, 32)\nrun(128, 256)\n"
    r = subprocess.run([sys.executable, "-c", code, REPO], env=dict(os.environ, IPDM_SENSE_COILS="0"), capture_output=True,
                       text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- 4. the conjugate-gradient proximal ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,n,T,B", [(32, 32, 4, 3, 3), (128, 256, 4, 1, 2)])
def test_mask2d_cg_prox_vs_float64(ops, pkg, H, W, n, T, B):
    rng = np.random.default_rng(43)
    sens = _sens(_maps("complex", n, H, W))
    maps = sens.cpu().numpy()                                                # the values the GPU sees
    mk = random_mask_2d(rng, T, H, W)
    mask = mk[np.arange(B) % T]                                              # (B, 1, H, W): image b uses plane b % T
    line = mask[:, :, :1, :]
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
        away = cgh.sample_norm(cgh.cg_solve(z, y, a, maps, line) - xstar) / bn
        chk = float(prox.check_solution(x_gpu, dev(z), dev(y), a, 1.0))
        print(f"{H}x{W} a={a}: |b - Nx|/|b| {res} |x - x*|/|b| {e} 1-D reading {away} check_solution {chk} iters {iters}")
        assert (res <= 2 * TOL).all() and (e <= 2 * TOL).all()
        assert (away > 100 * 2 * TOL).all()
        assert chk <= (2 * TOL) ** 2 * float((bn ** 2).mean())
        assert abs(chk - cgh.check_solution(x, z, y, a, maps, mask)) <= (2 * TOL) ** 2 * float((bn ** 2).mean())
        assert iters.dtype == np.int32 and ((1 <= iters) & (iters < max_iter)).all(), iters
        ahy = ops.sense_adjoint(dev(y), sens, m8, apply_mask=True)
        o_re, o_im, it2 = ops.sense_cgprox(dev(z.real), dev(z.imag), dev(y), sens, m8, a, max_iter=max_iter, tol=TOL, ahy=ahy)
        assert torch.equal(torch.complex(o_re, o_im), x_gpu) and torch.equal(it2, prox.last_iters)


# ---- 5. product classes and the sampler ---------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def sampler_case(pkg, golden, oracle_score):
    """10 levels x 3 steps + denoise at 32x32, B = 2, the tiny NCSNv2Deepest, g08's sigmas and noise tape, g36's complex
    maps and a variable-density 2-D mask; the CPU oracle sampler, computed once"""
    g8, g36 = golden("g08_ald"), golden("g36_sense_complex_maps")
    maps = g36["maps"]
    mask_t = pkg.syn.vd_mask_2d(32, 32, 4, seed=5)
    mask = mask_t.numpy()
    img = torch.cat([pkg.syn.phantom_image(32, 32, seed=s) for s in range(2)], dim=0).numpy().astype(np.complex64)
    meas = kspace.sense_forward(img, maps, mask)
    lr_scaled = float(g8["dc_visible_lr_scaled"])
    ref = oracle_ald.ald_sense_real_imag(oracle_score, g8["sigmas"], meas, maps, mask, 9e-7, 3, lr_scaled, True,
                                         _Tape(g8["noise"]))
    return dict(maps=maps, mask=mask, mask_t=mask_t, img=img, meas=meas, ref=ref, noise=g8["noise"], sigmas=g8["sigmas"],
                lr_scaled=lr_scaled)


def _run_sampler(pkg, net, c, mask, proximal, use_graph, **prox_kw):
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=c["maps"], normalize=False, mask_mode="custom",
                      mask=mask)
    params = dict(n_steps_each=3, step_lr=9e-7, denoise=True, final_only=True)
    meas = torch.from_numpy(c["meas"]).cuda()
    prox = pkg.prox.get_proximal(proximal)(op, **prox_kw)
    sampler = pkg.ald.ALDInvSegProximalRealImag(prox, 1.0, "linear", (2, 1, 32, 32), net, torch.from_numpy(c["sigmas"]).cuda(),
                                                params, tiny_config(), meas, op, seg=None, device=torch.device("cuda"))
    tape = _Tape(c["noise"])
    x = sampler(label=None, lamda=1.0, save_dir=None, lr_scaled=c["lr_scaled"], seg_mode="full", noise_fn=tape,
                use_graph=use_graph)[0].numpy()
    assert tape.i == 60
    return op, prox, x


@pytest.mark.parametrize("use_graph", [False, True])
def test_sampler_with_2d_mask_vs_oracle(pkg, tiny_net, sampler_case, use_graph):
    c = sampler_case
    op, _, x = _run_sampler(pkg, tiny_net, c, c["mask_t"], "L2Penalty", use_graph)
    ref = c["ref"]
    assert x.shape == ref.shape == (2, 1, 32, 32) and np.isfinite(x).all()
    x0 = op.conj_op(torch.from_numpy(c["meas"]).cuda()).cpu().numpy()
    for b in range(2):
        print("nrmse", metrics.nrmse(np.abs(x[b]), np.abs(ref[b])), "ssim-1", metrics.ssim(np.abs(x[b, 0]), np.abs(ref[b, 0])) - 1)
        assert metrics.nrmse(np.abs(x[b]), np.abs(ref[b])) < 1e-3
        assert abs(metrics.ssim(np.abs(x[b, 0]), np.abs(ref[b, 0])) - 1.0) < 1e-3
    print("displacement", np.linalg.norm((x - x0) - (ref - x0)) / np.linalg.norm(ref - x0))
    assert np.linalg.norm((x - x0) - (ref - x0)) <= 2e-3 * np.linalg.norm(ref - x0)
    # the rows took effect: the same run with the mask's first row as a line mask lands further from both
    _, _, x_line = _run_sampler(pkg, tiny_net, c, c["mask_t"][:, :, :1, :], "L2Penalty", use_graph)
    assert np.linalg.norm(x - x_line) > 2 * np.linalg.norm(x - ref)


def test_sampler_cg_tail_with_2d_mask(pkg, tiny_net, sampler_case):
    c = sampler_case
    _, prox, x = _run_sampler(pkg, tiny_net, c, c["mask_t"], "L2PenaltyCG", True, max_iter=12, tol=TOL)
    assert x.shape == (2, 1, 32, 32) and np.isfinite(x).all()
    it = prox.last_iters.cpu().numpy()
    print("iters", it)
    assert it.shape == (2,) and ((1 <= it) & (it <= 12)).all()


def test_operators_follow_the_mask(pkg, sampler_case):
    """SENSE and RandomUndersamplingFourier with a 2-D mask through __call__, conj_op, projection, L2Penalty,
    L2Penalty(num_steps=k), SingleCoil and Constrained, against the oracle; `.mask = m` after first use takes effect"""
    c = sampler_case
    rng = np.random.default_rng(44)
    maps, mask = c["maps"], c["mask"]
    B, H, W = 3, 32, 32
    rnd = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    x, z, s = rnd(B, 1, H, W), rnd(B, 1, H, W), rnd(4, B, 1, H, W)
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, H, W), seed=0, sens_maps=maps, normalize=False, mask_mode="custom", mask=c["mask_t"])
    y = op(dev(x))
    np.testing.assert_allclose(y.cpu().numpy(), kspace.sense_forward(x, maps, mask), atol=BOUND)
    np.testing.assert_allclose(op.conj_op(dev(s)).cpu().numpy(), kspace.sense_adjoint(s, maps), atol=BOUND)
    alpha = 0.25 * 4 * W / 0.05
    got = pkg.prox.L2Penalty(op)(dev(z), y, alpha, 1.0).cpu().numpy()
    np.testing.assert_allclose(got, kspace.l2_penalty_sense(z, y.cpu().numpy(), alpha, 1.0, maps, mask), atol=BOUND)
    # num_steps = 3: x <- x - 0.05 [ (x - z) / B + a A^H(A x - y) / (n W) ] from x = z, in float64
    yn = y.cpu().numpy()
    xs = z.astype(np.complex128)
    for _ in range(3):
        xs = xs - 0.05 * ((xs - z) / B + alpha * cgh.adjoint(cgh.forward(xs, maps, mask) - yn, maps, mask) / (4 * W))
    got = pkg.prox.L2Penalty(op)(dev(z), y, alpha, 1.0, num_steps=3).cpu().numpy()
    np.testing.assert_allclose(got, xs, atol=BOUND)
    # assignment after first use: the operator follows the new mask at once
    other = pkg.syn.vd_mask_2d(H, W, 4, seed=6)
    assert not torch.equal(other, c["mask_t"])
    op.random_under_fourier.mask = other
    y2 = op(dev(x))
    assert not torch.equal(y2, y)
    np.testing.assert_allclose(y2.cpu().numpy(), kspace.sense_forward(x, maps, other.numpy()), atol=BOUND)
    op.random_under_fourier.mask = c["mask_t"][0, 0, 0]                      # ... and back to a line mask (W,)
    np.testing.assert_allclose(op(dev(x)).cpu().numpy(), kspace.sense_forward(x, maps, mask[:, :, :1]), atol=BOUND)
    # single coil
    sc = pkg.uf.RandomUndersamplingFourier(4, 0.04, (1, H, W), seed=0, mask_mode="custom", mask=mask)
    ysc = sc(dev(x))
    want = (mask * kspace.fft2c(x)).astype(np.complex64)
    np.testing.assert_allclose(ysc.cpu().numpy(), want, atol=BOUND)
    got = pkg.prox.L2Penalty(sc)(dev(z), ysc, 0.25 * B / 0.05, 1.0).cpu().numpy()
    np.testing.assert_allclose(got, kspace.l2_penalty_single(z, want, 0.25 * B / 0.05, 1.0, mask), atol=BOUND)
    got = pkg.prox.SingleCoil(sc)(dev(z), ysc, 0.7, 1.0).cpu().numpy()
    np.testing.assert_allclose(got, kspace.single_coil(z, want, 0.7, 1.0, mask), atol=BOUND)
    kz = kspace.fft2c(z)
    proj = kspace.ifft2c(0.3 * want + 0.7 * mask * kz + (1 - mask) * kz)
    np.testing.assert_allclose(pkg.prox.Constrained(sc)(dev(z), ysc, 0.3).cpu().numpy(), proj, atol=BOUND)
    np.testing.assert_allclose(sc.projection(dev(z), ysc, 0.3).cpu().numpy(), proj, atol=BOUND)


def test_map_optimizer_with_2d_mask_vs_oracle(pkg, tiny_net, golden, oracle_score, sampler_case):
    """MAPOptimizer, 5 iterations, against oracle.map.sense_map with the oracle's forward closed over the 2-D mask;
    tolerance of test_map_optimizer_with_complex_maps_vs_oracle: 2 % of the distance lr * n_iters travelled"""
    c = sampler_case
    g18 = golden("g18_map")
    maps, mask, meas = c["maps"], c["mask"], c["meas"]
    lamda, lr, n_iters = float(g18["a_lamda"]), float(g18["a_lr"]), 5
    x_init = kspace.sense_adjoint(meas, maps)

    def score_np(x, labels):
        return oracle_score(torch.from_numpy(x), torch.from_numpy(labels)).numpy()

    def run_oracle(m):
        return oracle_map.sense_map(x_init, meas, score_np, lambda v: kspace.sense_forward(v, maps, m),
                                    lambda s: kspace.sense_adjoint(s, maps), lamda, lr, n_iters)

    ref = run_oracle(mask)
    op = pkg.uf.SENSE("custom", 4, 8, 0.04, (1, 32, 32), seed=0, sens_maps=maps, normalize=False, mask_mode="custom",
                      mask=c["mask_t"])
    cfg = tiny_config()
    cfg.MAP = Namespace(n_iters=n_iters, lr=lr, complex_inner_n_steps=20)
    x = pkg.map.MAPOptimizer(torch.from_numpy(x_init.copy()).cuda(), torch.from_numpy(meas).cuda(), tiny_net, op, lamda, cfg,
                             logger=None, device=torch.device("cuda"))().cpu().numpy()
    print("map max err", np.abs(x - ref).max(), "tolerance", 0.02 * n_iters * lr)
    np.testing.assert_allclose(x, ref, atol=0.02 * n_iters * lr)
    assert np.abs(run_oracle(mask[:, :, :1]) - ref).max() > 0.02 * n_iters * lr       # the 1-D reading is another problem


def test_tv_map_model_with_2d_mask_vs_autograd_adam(pkg):
    """MAPModel.fit with TotalVariation, 25 epochs, against torch autograd + Adam on operators that multiply by the 2-D
    mask; data, tolerances and caveats of test_tv_map_model_vs_autograd_adam (test_kernels_gpu.py)"""
    from oracle import tv as otv
    H = W = 32
    mask_t = pkg.syn.vd_mask_2d(H, W, 4, seed=5)
    op = pkg.uf.SENSE("exp", 4, 8, 0.05, (1, H, W), seed=0, mask_mode="custom", mask=mask_t)
    gen = torch.Generator().manual_seed(11)
    img = pkg.syn.phantom_image(H, W, seed=1) + 0.2 * torch.complex(torch.randn(1, 1, H, W, generator=gen),
                                                                    torch.randn(1, 1, H, W, generator=gen))
    meas = op(img.cuda())
    x = pkg.map.MAPModel(meas, op, pkg.map.TotalVariation(), 0.01).fit(25, 1e-2).numpy()
    maps = torch.from_numpy(op.sens_maps.numpy()).to(torch.complex64)
    mask = mask_t.to(torch.float32)                                          # (1, 1, H, W)

    def fft2c(t):
        return torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(t, dim=(-1, -2)), norm="ortho"), dim=(-1, -2))

    def ifft2c(t):
        return torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(t, dim=(-1, -2)), norm="ortho"), dim=(-1, -2))

    fwd = lambda X: mask * fft2c(maps[:, None, None] * X[None])
    adj = lambda S: (torch.conj(maps[:, None, None]) * ifft2c(S)).sum(0)
    m_cpu = meas.cpu()
    assert torch.allclose(fwd(img), m_cpu, atol=1e-5)                        # the oracle operators are the op's
    want = otv.tv_map(m_cpu, fwd, adj, 0.01, 1e-2, 25).numpy()
    diff = np.abs(x - want)
    stats = (float(diff.max()), float(np.sqrt((diff ** 2).mean())), float((diff > 1e-4 * np.abs(want).max()).mean()))
    print("tv map (max, rms, outlier share)", stats)
    assert diff.max() <= 2.5 * 1e-2 and np.sqrt((diff ** 2).mean()) < 2e-3 * np.abs(want).max(), stats
    assert (diff > 1e-4 * np.abs(want).max()).mean() < 0.05, stats
    assert np.abs(want - adj(m_cpu).numpy()).max() > 0.05 * np.abs(want).max()


# ---- 6. drivers ---------------------------------------------------------------------------------------------------------
_ACDC = ["--image_size", "64", "--n_levels", "2", "--R", "8", "--num_samples", "1", "--num_sens", "4", "--seed", "0",
         "--seg_start_time", "1.0"]


def _run_acdc(args, save_dir):
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py")] + _ACDC + args +
                       ["--save_dir", save_dir], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    load = lambda name: torch.load(os.path.join(save_dir, name), weights_only=False)
    return load("mask.pt"), load("reconstructions.pt"), load("measurement.pt")


def _check_driver_output(pkg, mask, rec, meas, want_mask):
    assert tuple(mask.shape) == (1, 1, 64, 64) and mask.dtype == want_mask.dtype and torch.equal(mask, want_mask)
    assert rec.dtype == torch.complex64 and torch.isfinite(torch.view_as_real(rec)).all()
    op = pkg.uf.SENSE("exp", 4, 8, 1 / 4, (1, 64, 64), seed=0, mask_mode="custom", mask=mask)
    off = ~mask.bool().expand(4, rec.shape[0], 1, 64, 64)
    Ax = op(rec.cuda()).cpu()
    assert Ax[~off].abs().max() > 0 and not Ax[off].any()                    # A x is zero exactly where the mask is
    assert not meas[off[:, :1]].any()


def test_driver_with_synthetic_2d_mask(pkg, tmp_path):
    mask, rec, meas = _run_acdc(["--mask_2d"], str(tmp_path))
    _check_driver_output(pkg, mask, rec, meas, pkg.syn.vd_mask_2d(64, 64, 8, seed=0))


def test_driver_with_a_mask_from_a_file(pkg, tmp_path):
    want = pkg.syn.vd_mask_2d(64, 64, 6, seed=11, partial_fourier=0.75)
    torch.save(want, tmp_path / "acquired.pt")
    mask, rec, meas = _run_acdc(["--mask", str(tmp_path / "acquired.pt")], str(tmp_path / "out"))
    _check_driver_output(pkg, mask, rec, meas, want)


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def test_mask2d_errors(ops):
    B, n, H, W = 2, 3, 32, 32
    x = torch.zeros(B, 1, H, W, dtype=torch.complex64, device="cuda")
    s = torch.zeros(n, B, 1, H, W, dtype=torch.complex64, device="cuda")
    sens = torch.ones(n, H, W, dtype=torch.complex64, device="cuda")
    p = [torch.zeros(B, 1, H, W, device="cuda") for _ in range(4)]
    work = ops.sense_workspace(B, n, H, W, "cuda")
    ysc = torch.zeros(B, 1, H, W, dtype=torch.complex64, device="cuda")

    def every_entry(mask):
        return [lambda: ops.sense_forward(x, sens, mask),
                lambda: ops.sense_forward(x, None, mask),
                lambda: ops.sense_adjoint(s, sens, mask, apply_mask=True),
                lambda: ops.sense_l2prox(p[0], p[1], s, sens, mask, 0.01),
                lambda: ops.ald_sense_step(p[0], p[1], p[2], p[3], s, sens, mask, work, step=0.1, noise_scale=0.1, coef=0.01),
                lambda: ops.sense_cgprox(p[0], p[1], s, sens, mask, 1.0),
                lambda: ops.ald_sense_cg_step(p[0], p[1], p[2], p[3], s, sens, mask, None, step=0.1, noise_scale=0.1, coef=1.0),
                lambda: ops.singlecoil_prox(p[0], p[1], ysc, mask, 0.5, ops.SC_CLOSED_FORM),
                lambda: ops.ald_singlecoil_step(p[0], p[1], p[2], p[3], ysc, mask, ops.SC_L2PENALTY, step=0.1, noise_scale=0.1,
                                                coef=0.01)]

    good = torch.ones(1, H, W, dtype=torch.uint8, device="cuda")
    for bad in (torch.ones(1, H // 2, W, dtype=torch.uint8, device="cuda"),                # wrong H
                torch.ones(1, 2 * H, W, dtype=torch.uint8, device="cuda"),
                torch.ones(1, H, W + 1, dtype=torch.uint8, device="cuda"),                 # wrong W
                torch.ones(1, W + 1, dtype=torch.uint8, device="cuda"),
                torch.ones(1, 1, H, W, dtype=torch.uint8, device="cuda"),                  # not a device layout
                torch.ones(W, dtype=torch.uint8, device="cuda"),
                torch.ones(0, H, W, dtype=torch.uint8, device="cuda"),
                torch.ones(2, H, 2 * W, dtype=torch.uint8, device="cuda")[:, :, ::2]):     # strided
        for f in every_entry(bad):
            with pytest.raises(ValueError):
                f()
    for bad in (good.float(), good.bool(), good.to(torch.int32)):                          # read as bytes: never reinterpreted
        for f in every_entry(bad):
            with pytest.raises(TypeError):
                f()
    for f in every_entry(good.cpu()):
        with pytest.raises(RuntimeError):
            f()
    for f in every_entry(good):                                                            # and the good one runs
        f()
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in p)
