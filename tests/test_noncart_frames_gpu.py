"""Radial cine on the GPU: one trajectory per frame through the non-uniform DFT kernels, the Toeplitz normal
operator, the conjugate-gradient proximal, the fused tail, both samplers and the cine driver.

1. Rows {b : b % T == t} of every framed call equal, bit for bit, those rows of the one-trajectory call with trajectory t on
   the same batch: no tolerance.  2. The framed calls against the float64 restatement of tests/noncart_helpers.py, frame by
   frame; because of 1 the bounds are those of tests/test_noncart_gpu.py for the same quantity.  3., 4. the samplers.
   5. the driver.  The metric of every float64 comparison is max|err| / max|ref|."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import noncart_helpers as nh
import test_noncart_gpu as base
from conftest import state_dict_from_golden

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the first six are tests/test_noncart_gpu.py's TOL for the same quantity, copied: by the bit identity of part 1 a framed row
# IS a row of the one-trajectory call those bounds were set for.  ald2dtime: 10 x the largest error observed on the MI355X
# against the float64-proximal loop (DESIGN.md 4.4m lists the observed figures), the rule of that file.
TOL = dict(forward=5.7e-7, adjoint=5.6e-7, psf=7.7e-7, normal=3.2e-6, dot=1.1e-6, cg_solution=2.4e-4, ald2dtime=4.3e-5)

# image, T, B, coils: the padded grid within one strip; radix 3 / 5; sens=None and several strips
SHAPES = [(16, 16, 3, 6, 4), (48, 80, 2, 2, 5), (64, 80, 3, 3, 1)]

dev, host, cplx = base.dev, base.host, base.cplx


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ncsn3d, ncsn1d, ALD_optimizers, proximal_op
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import noncartesian
    return Namespace(ncsnv2=ncsnv2, ncsn3d=ncsn3d, ncsn1d=ncsn1d, ald=ALD_optimizers, prox=proximal_op, nc=noncartesian)


def frame_trajectory(T, H, W, spokes=7, readout=33, edges=True):
    """(T, M, 2): frame t = `spokes` consecutive golden-angle spokes of nh.radial(spokes * T, ...), plus (edges) the six
    bound points nh.edge_trajectory appends: M = 237, no multiple of 64"""
    whole = nh.radial(spokes * T, readout, H, W).reshape(T, spokes * readout, 2)
    if not edges:
        return np.ascontiguousarray(whole)
    extra = nh.edge_trajectory(1, 1, H, W)[1:]
    return np.ascontiguousarray(np.stack([np.concatenate([whole[t], extra]) for t in range(T)]))


_CASES = {}


def case(H, W, T, B, n, weighted):
    """inputs (the float32 values the GPU gets) and the float64 spectra of one shape, made once"""
    key = (H, W, T, B, n, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(H * 131 + W + 7 * n + T)
        k = frame_trajectory(T, H, W)
        M = k.shape[1]
        w = np.stack([nh.ramp_weights(k[t], H, W) for t in range(T)]).astype(np.float32) if weighted else None
        S = nh.smooth_maps(n, H, W, seed=n) if n > 1 else None                      # n == 1: sens=None in every call
        x = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
        y = (rng.standard_normal((n, B, M)) + 1j * rng.standard_normal((n, B, M))).astype(np.complex64)
        g = rng.standard_normal((2, B, H, W)).astype(np.float32)
        nz = rng.standard_normal((2, B, H, W)).astype(np.float32)
        P = np.stack([nh.toeplitz_psf(k[t], H, W, None if w is None else w[t]) for t in range(T)])
        _CASES[key] = Namespace(H=H, W=W, T=T, B=B, n=n, M=M, k=k, w=w, S=S, x=x, y=y, g=g, nz=nz, P=P, kd=dev(k),
                                wd=None if w is None else dev(w), Sd=None if S is None else dev(S))
    return _CASES[key]


def wt(c, t):
    return None if c.wd is None else c.wd[t].contiguous()


def test_frames_differ():
    """a kernel that ignored the set index could not pass: the float64 spectra of two frames differ by > 1e-2 of their peak"""
    for H, W, T, B, n in SHAPES:
        for weighted in (False, True):
            c = case(H, W, T, B, n, weighted)
            d = np.abs(c.P[0] - c.P[1]).max() / np.abs(c.P[0]).max()
            print(f"psf of frames 0 and 1, {H}x{W} weighted={weighted}: differ by {d:.3g} of the peak")
            assert d > 1e-2


# ---- 1. bit identity with the one-trajectory kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("H,W,T,B,n", SHAPES)
def test_rows_equal_the_single_trajectory_call(ops, H, W, T, B, n, weighted):
    c = case(H, W, T, B, n, weighted)
    xd, yd = dev(c.x), dev(c.y)
    coil_imgs = dev(np.stack([c.x] * n) if c.S is None else (c.S[:, None] * c.x[None]).astype(np.complex64))
    z_re, z_im = dev(c.x.real), dev(c.x.imag)
    g_re, g_im, nz_re, nz_im = dev(c.g[0]), dev(c.g[1]), dev(c.nz[0]), dev(c.nz[1])
    a, kw = 1.5, dict(max_iter=12, tol=1e-5)
    step = dict(step=0.37, noise_scale=float(np.sqrt(2 * 0.37)), coef=a, step_id=(1 << 33) + 5)

    def tail(psf, ahy, **noise):
        x_re, x_im = z_re.clone(), z_im.clone()
        it = ops.ald_nc_sense_cg_step(x_re, x_im, g_re, g_im, ahy, c.Sd, psf, ops.nc_sense_cg_workspace(B, n, H, W, "cuda"),
                                      **step, **noise, **kw)
        return x_re, x_im, it

    f_fwd = ops.ndft_forward(xd, c.kd, c.Sd) if c.Sd is not None else ops.ndft_forward(xd[None], c.kd)
    f_fwd_coils = ops.ndft_forward(coil_imgs, c.kd)
    f_adj = ops.ndft_adjoint(yd, c.kd, H, W, c.Sd, c.wd)
    f_adj_coils = ops.ndft_adjoint(yd, c.kd, H, W, None, c.wd)
    f_psf = ops.toeplitz_psf(c.kd, H, W, c.wd)
    assert tuple(f_psf.shape) == (T, 2 * H, 2 * W) and f_psf.dtype == torch.float32
    ahy = f_adj if c.Sd is not None else f_adj_coils[0].contiguous()
    f_nrm = ops.toeplitz_normal(xd, f_psf, c.Sd)
    f_cg = ops.nc_sense_cgprox(z_re, z_im, ahy, c.Sd, f_psf, a, **kw)
    f_philox = tail(f_psf, ahy, seed=11, sample_offset=4)
    f_inject = tail(f_psf, ahy, noise_re=nz_re, noise_im=nz_im)
    assert (0 < host(f_cg[2])).all()
    for t in range(T):
        kt, rows = c.kd[t].contiguous(), slice(t, None, T)
        r_fwd = ops.ndft_forward(xd, kt, c.Sd) if c.Sd is not None else ops.ndft_forward(xd[None], kt)
        assert torch.equal(f_fwd[:, rows], r_fwd[:, rows]), ("forward", t)
        assert torch.equal(f_fwd_coils[:, rows], ops.ndft_forward(coil_imgs, kt)[:, rows]), ("forward, coil images", t)
        assert torch.equal(f_adj[rows] if c.Sd is not None else f_adj[:, rows],
                           (lambda r: r[rows] if c.Sd is not None else r[:, rows])(ops.ndft_adjoint(yd, kt, H, W, c.Sd, wt(c, t)))), \
            ("adjoint", t)
        assert torch.equal(f_adj_coils[:, rows], ops.ndft_adjoint(yd, kt, H, W, None, wt(c, t))[:, rows]), ("adjoint, coil images", t)
        pt = ops.toeplitz_psf(kt, H, W, wt(c, t))
        assert torch.equal(f_psf[t], pt), ("psf", t)
        assert torch.equal(f_nrm[rows], ops.toeplitz_normal(xd, pt, c.Sd)[rows]), ("normal", t)
        r_cg = ops.nc_sense_cgprox(z_re, z_im, ahy, c.Sd, pt, a, **kw)
        assert all(torch.equal(f[rows], r[rows]) for f, r in zip(f_cg, r_cg)), ("cgprox", t)
        r_philox = tail(pt, ahy, seed=11, sample_offset=4)
        assert all(torch.equal(f[rows], r[rows]) for f, r in zip(f_philox, r_philox)), ("fused tail, Philox", t)
        r_inject = tail(pt, ahy, noise_re=nz_re, noise_im=nz_im)
        assert all(torch.equal(f[rows], r[rows]) for f, r in zip(f_inject, r_inject)), ("fused tail, injected noise", t)
    assert not torch.equal(f_philox[0], f_inject[0])


def test_one_frame_operator_equals_the_unframed_one(pkg):
    """(1, M, 2) is a framed operator with one frame: every call equals the (M, 2) operator's, bit for bit"""
    c = case(16, 16, 3, 6, 4, True)
    k, w = c.k[1], c.w[1]
    flat = pkg.nc.NonCartesianSENSE(k, (1, 16, 16), sens_maps=c.S, weights=w, normalize=False)
    one = pkg.nc.NonCartesianSENSE(k[None], (1, 16, 16), sens_maps=c.S, weights=w[None], normalize=False)
    assert one.framed and not flat.framed and tuple(one.psf_dev("cuda").shape) == (1, 32, 32)
    X, Y = dev(c.x)[:, None], dev(c.y)[:, :, None]
    assert torch.equal(one(X), flat(X)) and torch.equal(one.conj_op(Y), flat.conj_op(Y))
    assert torch.equal(one.adjoint_weighted(Y), flat.adjoint_weighted(Y)) and torch.equal(one.zero_filled(Y), flat.zero_filled(Y))
    assert torch.equal(one.psf_dev("cuda")[0], flat.psf_dev("cuda"))
    p1, p0 = pkg.prox.L2PenaltyCG(one, max_iter=12), pkg.prox.L2PenaltyCG(flat, max_iter=12)
    assert torch.equal(p1(X, Y, 1.5, 1.0), p0(X, Y, 1.5, 1.0)) and torch.equal(p1.last_iters, p0.last_iters)
    assert torch.equal(p1(X, Y, 1.5, 1.0, ahy=one.adjoint_weighted(Y)), p0(X, Y, 1.5, 1.0))       # ahy given: the same solve


def test_framed_refusals_with_gpu_operands(ops, pkg):
    """the host refusals hold for GPU operands too, before any launch: B % T, weights of the wrong form"""
    c = case(16, 16, 3, 6, 4, True)
    x4 = dev(c.x[:4])
    with pytest.raises(ValueError, match="do not match the 3 frames of 237 samples"):
        ops.toeplitz_psf(c.kd, 16, 16, c.wd[0].contiguous())
    with pytest.raises(ValueError, match="do not match the 3 frames of 237 samples"):
        ops.ndft_adjoint(dev(c.y), c.kd, 16, 16, c.Sd, c.wd[0].contiguous())
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.ndft_forward(x4, c.kd, c.Sd)
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.toeplitz_normal(x4, ops.toeplitz_psf(c.kd, 16, 16), c.Sd)
    op = pkg.nc.NonCartesianSENSE(c.k, (1, 16, 16), sens_maps=c.S, normalize=False)
    with pytest.raises(ValueError, match=r"B = 4 rows are not a multiple of the T = 3 frames"):
        op(x4[:, None])
    with pytest.raises(ValueError, match=r"B = 4 rows are not a multiple of the T = 3 frames"):
        op.conj_op(dev(c.y)[:, :4, None])


# ---- 2. the framed calls against float64 -----------------------------------------------------------------------------------
def _frame_err(got, ref_of_frame, T, axis):
    """max over frames t of  max|got - ref_t| on the rows of frame t  /  max|ref_t| on the whole batch: ref_t is the float64
    result of the one-trajectory call on the same batch, the quantity the copied bounds were set for"""
    worst = 0.0
    for t in range(T):
        ref = ref_of_frame(t)
        rows = (slice(None),) * axis + (slice(t, None, T),)
        worst = max(worst, float(np.abs(np.asarray(got)[rows] - ref[rows]).max() / np.abs(ref).max()))
    return worst


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("H,W,T,B,n", SHAPES)
def test_framed_calls_vs_float64(ops, pkg, H, W, T, B, n, weighted):
    c = case(H, W, T, B, n, weighted)
    w = (lambda t: None) if c.w is None else (lambda t: c.w[t])
    xd, yd = dev(c.x), dev(c.y)
    e = {}
    fwd = ops.ndft_forward(xd, c.kd, c.Sd) if c.Sd is not None else ops.ndft_forward(xd[None], c.kd)
    e["forward"] = _frame_err(host(fwd), lambda t: nh.sense_forward(c.x, c.S, c.k[t]), T, 1)
    if c.Sd is not None:
        e["adjoint"] = _frame_err(host(ops.ndft_adjoint(yd, c.kd, H, W, c.Sd, c.wd)),
                                  lambda t: nh.sense_adjoint(c.y, c.S, c.k[t], H, W, w(t)), T, 0)
    e["adjoint_coils"] = _frame_err(host(ops.ndft_adjoint(yd, c.kd, H, W, None, c.wd)),
                                    lambda t: nh.ndft_adjoint(c.y, c.k[t], H, W, w(t)), T, 1)
    psf = ops.toeplitz_psf(c.kd, H, W, c.wd)
    e["psf"] = max(nh.relerr(host(psf[t]), c.P[t]) for t in range(T))
    e["normal"] = _frame_err(host(ops.toeplitz_normal(xd, psf, c.Sd)), lambda t: nh.toeplitz_normal(c.x, c.S, c.P[t]), T, 0)
    # the dot test over the framed batch, through the operator: <y, A x> = <A^H y, x>, no weights
    op = pkg.nc.NonCartesianSENSE(c.k, (1, H, W), sens_maps=c.S, normalize=False)
    Ax = host(op(xd[:, None])).astype(np.complex128)[:, :, 0]
    AHy = host(op.conj_op(yd[:, :, None])).astype(np.complex128)[:, 0]
    lhs, rhs = np.vdot(c.y.astype(np.complex128), Ax), np.vdot(AHy, c.x.astype(np.complex128))
    e["dot"] = abs(lhs - rhs) / abs(lhs)
    print(f"framed stages {H}x{W} T={T} B={B} n={n} weighted={weighted}: " + "  ".join(f"{k} {v:.3g}" for k, v in e.items()))
    for name, v in e.items():
        assert v <= TOL[name.split("_")[0]], (name, v)


@pytest.mark.parametrize("weighted", [False, True])
def test_framed_cgprox_vs_float64(ops, weighted):
    """the framed proximal against the float64 conjugate-gradient solve with each frame's own Toeplitz operator"""
    H, W, T, B, n = SHAPES[0]
    c = case(H, W, T, B, n, weighted)
    a, cap = 1.0, 60
    ahy = ops.ndft_adjoint(dev(c.y), c.kd, H, W, c.Sd, c.wd)
    o_re, o_im, iters = ops.nc_sense_cgprox(dev(c.x.real), dev(c.x.imag), ahy, c.Sd, ops.toeplitz_psf(c.kd, H, W, c.wd), a,
                                            max_iter=cap, tol=1e-5)
    x, it = cplx(o_re, o_im), host(iters)
    ref, it64 = np.zeros_like(x), np.zeros(B, dtype=np.int64)
    for t in range(T):
        rows = slice(t, None, T)
        ahy64 = nh.sense_adjoint(c.y[:, rows], c.S, c.k[t], H, W, None if c.w is None else c.w[t])
        ref[rows], it64[rows] = nh.cg_prox(c.x[rows], ahy64, lambda v: nh.toeplitz_normal(v, c.S, c.P[t]), a, cap, 1e-5)
    err = nh.relerr(x, ref)
    print(f"framed cgprox weighted={weighted}: iters {it} float64 iters {it64}  |x - x64| {err:.3g}")
    assert (0 < it64).all() and (it64 < cap).all(), "the float64 reference itself must converge below the cap"
    assert (0 < it).all() and (it < cap).all() and err <= TOL["cg_solution"]


# ---- 3. ALDInvSegProximalRealImag: independent frames in one batch -----------------------------------------------------------
def _run_2d_sampler(pkg, golden, c, use_graph, **kw):
    net = pkg.ncsnv2.NCSNv2Deepest(base.tiny_config(c.H))
    net.load_state_dict(state_dict_from_golden(golden("g07_layers"), "net"), strict=True)
    net = net.cuda().eval()
    op = pkg.nc.NonCartesianSENSE(c.k, (1, c.H, c.W), sens_maps=c.S, normalize=False)
    prox = pkg.prox.L2PenaltyCG(op, max_iter=30, tol=1e-6)
    meas = torch.from_numpy(c.y).cuda().reshape(c.n, c.B, 1, -1)
    params = dict(n_steps_each=base.N_EACH, step_lr=base.STEP_LR, denoise=False, final_only=True)
    sampler = pkg.ald.ALDInvSegProximalRealImag(prox, 1.0, "linear", (c.B, 1, c.H, c.W), net, torch.from_numpy(c.sigmas).cuda(),
                                                params, base.tiny_config(c.H), meas, op, seg=None, device=torch.device("cuda"))
    tape = base._Tape(c.noise[kw.get("start_level", 0) * 2 * base.N_EACH:])
    x = sampler(label=None, lamda=1.0, save_dir=None, lr_scaled=c.lr_scaled, seg_mode="full", noise_fn=tape,
                use_graph=use_graph, **kw)[0]
    return x, prox


def test_2d_sampler_with_frames(pkg, golden):
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    H = W = 16
    T, B, n = 2, 4, 4
    rng = np.random.default_rng(5)
    k = frame_trajectory(T, H, W, spokes=8, readout=32, edges=False)
    S = nh.smooth_maps(n, H, W, seed=3)
    img = torch.cat([phantom_image(H, W, seed=s) for s in range(B)], dim=0).numpy()[:, 0].astype(np.complex64)
    y = np.zeros((n, B, k.shape[1]), dtype=np.complex64)
    for t in range(T):
        y[:, t::T] = nh.sense_forward(img[t::T], S, k[t])
    sigmas = np.geomspace(1.0, 0.01, 10).astype(np.float32)[:base.N_LEVELS]
    noise = rng.standard_normal((2 * base.N_LEVELS * base.N_EACH, B, 1, H, W)).astype(np.float32)
    c = Namespace(H=H, W=W, B=B, n=n, k=k, S=S, y=y, sigmas=sigmas, noise=noise, lr_scaled=1.0 / base.STEP_LR)
    x_eager, prox = _run_2d_sampler(pkg, golden, c, False)
    x_graph, prox_g = _run_2d_sampler(pkg, golden, c, True)
    assert torch.equal(x_eager, x_graph) and torch.equal(prox.last_iters, prox_g.last_iters)   # hipGraph == eager
    it = host(prox.last_iters)
    assert (0 < it).all() and (it < 30).all() and torch.isfinite(torch.view_as_real(x_graph)).all()
    x_a, _ = _run_2d_sampler(pkg, golden, c, True, n_levels=2)
    x_b, _ = _run_2d_sampler(pkg, golden, c, True, start_level=2, n_levels=2, x_init=x_a)
    assert torch.equal(x_b, x_graph)                                           # a sliced run continues the full run's bits


# ---- 4. ALD2DTime ------------------------------------------------------------------------------------------------------------
T4, H4, W4, N_LEVELS4 = 8, 32, 32, 4          # tests/test_2dtime_gpu.py's shapes and networks; a slice of its schedule


def _cine_case(golden):
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    if "cine" not in _CASES:
        k = frame_trajectory(T4, H4, W4, spokes=8, readout=32, edges=False)
        S = nh.smooth_maps(4, H4, W4, seed=3)
        base_img = phantom_image(H4, W4, seed=0).numpy()[0, 0].astype(np.complex64)
        beat = 1.0 + 0.1 * np.cos(np.arange(T4) * (2 * np.pi / T4))
        frames = (base_img[None] * beat[:, None, None]).astype(np.complex64)
        y = np.stack([nh.sense_forward(frames[t:t + 1], S, k[t])[:, 0] for t in range(T4)], axis=1).astype(np.complex64)
        g = golden("g17_ald2dtime")
        _CASES["cine"] = Namespace(k=k, S=S, y=y, sigmas=g["sigmas"], sigmas_T=g["sigmas_T"], step_lr=2e-5, lr_scaled=1.0e5,
                                   n_each=2)
    return _CASES["cine"]


class _Noise:
    """randn(like.shape) call after call from a seeded host generator; kept so that the float64 loop replays the stream"""

    def __init__(self, seed=170):
        self.g, self.calls, self.tape = torch.Generator().manual_seed(seed), 0, []

    def __call__(self, like):
        n = torch.randn(like.shape, generator=self.g, dtype=torch.float32)
        self.calls += 1
        self.tape.append(n)
        return n


def _net2d(pkg, golden):
    from test_scorenet_gpu import tiny_config
    net = pkg.ncsnv2.NCSNv2Deepest(tiny_config())
    net.load_state_dict(state_dict_from_golden(golden("g07_layers"), "net"), strict=True)
    return net.cuda().eval(), tiny_config()


def _net3d(pkg, golden):
    from test_2dtime_gpu import cfg3d
    net = pkg.ncsn3d.NCSN3DShallow(cfg3d())
    net.load_state_dict(state_dict_from_golden(golden("g16_ncsn3d"), "net3d"), strict=True)
    return net.cuda().eval()


def _run_cine(pkg, golden, c, mode, prox_cls=None, lamda_T=1.0):
    net2d, cfg = _net2d(pkg, golden)
    op = pkg.nc.NonCartesianSENSE(c.k, (1, H4, W4), sens_maps=c.S, normalize=False)
    prox = (prox_cls or pkg.prox.L2PenaltyCG)(op, max_iter=30, tol=1e-6)
    meas = torch.from_numpy(c.y).cuda().reshape(4, 1, T4, 1, -1)
    params = dict(n_steps_each=c.n_each, step_lr=c.step_lr, denoise=False, final_only=True)
    sampler = pkg.ald.ALD2DTime(prox, _net3d(pkg, golden), torch.from_numpy(c.sigmas_T).cuda(), (1, T4, 1, H4, W4), net2d,
                                torch.from_numpy(c.sigmas).cuda(), params, cfg, meas, op, device=torch.device("cuda"))
    noise = _Noise()
    x = sampler(save_dir=None, lr_scaled=c.lr_scaled, mode_T=mode, lamda_T=lamda_T, if_random_shift=False, noise_fn=noise,
                n_levels=N_LEVELS4)[0]
    return x, prox, noise, sampler


def _reference_cine(golden, c, tape, shift=0):
    """mode_T = "none" with the float64 restatement, written like tests/test_noncart_gpu.py's _reference_sampler: the
    oracle's score network on float32 planes, the Langevin update, then per frame the float64 CG solution of
    (I + a A_t^H A_t) x = z + a A_t^H y_t.  shift: frame t reconstructed with trajectory t + shift (a wrong pairing)"""
    from oracle import scorenet as oracle_net
    from inverseproblemwithdiffusionmodel_amd.synthetic import radial_density
    sd = {k: torch.from_numpy(np.array(v)) for k, v in state_dict_from_golden(golden("g07_layers"), "net").items()}
    k = np.roll(c.k, -shift, axis=0)
    P = [nh.toeplitz_psf(k[t], H4, W4) for t in range(T4)]
    ahy = np.stack([nh.sense_adjoint(c.y[:, t:t + 1], c.S, k[t], H4, W4)[0] for t in range(T4)])
    x = np.stack([nh.sense_adjoint(c.y[:, t:t + 1], c.S, k[t], H4, W4, radial_density(k[t], H4, W4).numpy().astype(np.float32))[0]
                  for t in range(T4)]).astype(np.complex64)

    def normal(v):
        return np.stack([nh.toeplitz_normal(v[t:t + 1], c.S, P[t])[0] for t in range(T4)])
    x_re = torch.from_numpy(np.ascontiguousarray(x.real))[:, None]
    x_im = torch.from_numpy(np.ascontiguousarray(x.imag))[:, None]
    sig = torch.from_numpy(c.sigmas)
    steps = c.step_lr * (sig / sig[-1]) ** 2                                   # step_schedule's float32 arithmetic
    i = 0
    for lv in range(N_LEVELS4):
        labels = torch.full((T4,), lv, dtype=torch.long)
        for _ in range(c.n_each):
            with torch.no_grad():
                g_re, g_im = oracle_net.ncsnv2_deepest(x_re, labels, sd), oracle_net.ncsnv2_deepest(x_im, labels, sd)
            x_re = x_re + steps[lv] * g_re + tape[i] * torch.sqrt(steps[lv] * 2)
            x_im = x_im + steps[lv] * g_im + tape[i + 1] * torch.sqrt(steps[lv] * 2)
            i += 2
            z = (x_re.numpy() + 1j * x_im.numpy())[:, 0].astype(np.complex64)
            z, _ = nh.cg_prox(z, ahy, normal, c.step_lr * c.lr_scaled, 200, 1e-12)
            z = z.astype(np.complex64)
            x_re = torch.from_numpy(np.ascontiguousarray(z.real))[:, None]
            x_im = torch.from_numpy(np.ascontiguousarray(z.imag))[:, None]
    return (x_re.numpy() + 1j * x_im.numpy()).astype(np.complex64)[None]      # (1, T, 1, H, W)


def test_ald2dtime_none_vs_float64_loop(pkg, golden):
    """(a) against the float64-proximal loop; the same loop with the trajectories rotated by one frame must be at least
    100 x the bound away, so that the bound tells the right frame pairing from a wrong one.  (b) the run whose proximal
    recomputes A^H W y in every call equals the run that forms it once, bit for bit.
    Observed on the MI355X: 4.25e-6 against the loop, 0.898 against the rotated one."""
    c = _cine_case(golden)
    x, prox, noise, _ = _run_cine(pkg, golden, c, "none")
    n_it = N_LEVELS4 * c.n_each
    assert noise.calls == 2 * n_it and tuple(x.shape) == (1, T4, 1, H4, W4)
    it = host(prox.last_iters)
    assert (0 < it).all() and (it < 30).all()
    e = nh.relerr(x.numpy(), _reference_cine(golden, c, noise.tape))
    e_rot = nh.relerr(x.numpy(), _reference_cine(golden, c, noise.tape, shift=1))
    print(f"ALD2DTime none: vs the float64-proximal loop {e:.3g}  vs the loop with rotated trajectories {e_rot:.3g}  iters {it}")

    class Recompute(pkg.prox.L2PenaltyCG):
        calls = 0

        def __call__(self, z, y, alpha, lamda, ahy=None):
            Recompute.calls += 1
            return super().__call__(z, y, alpha, lamda)
    x_re, _, _, _ = _run_cine(pkg, golden, c, "none", prox_cls=Recompute)
    assert Recompute.calls == n_it and torch.equal(x_re, x)
    assert e_rot >= 100 * TOL["ald2dtime"]
    assert e <= TOL["ald2dtime"]


@pytest.mark.parametrize("mode", ["diffusion1d", "tv"])
def test_ald2dtime_temporal_modes(pkg, golden, mode):
    """(c) the temporal modes finish finite with the expected number of noise calls and a converged proximal (lamda_T: the
    value tests/test_2dtime_gpu.py runs the mode with)"""
    c = _cine_case(golden)
    lamda_T = float(golden("g17_ald2dtime")[f"{mode}_lamda_T"])
    x, prox, noise, sampler = _run_cine(pkg, golden, c, mode, lamda_T=lamda_T)
    n_it = N_LEVELS4 * c.n_each
    temporal = c.n_each * int((sampler.sigmas_T[:N_LEVELS4] != -1).sum()) if mode == "diffusion1d" else 0
    assert noise.calls == 2 * n_it + 2 * temporal
    assert tuple(x.shape) == (1, T4, 1, H4, W4) and torch.isfinite(torch.view_as_real(x)).all()
    it = host(prox.last_iters)
    print(f"ALD2DTime {mode}: noise calls {noise.calls}  iters {it}")
    assert it.shape == (T4,) and (0 < it).all() and (it < 30).all()


# ---- 5. driver ---------------------------------------------------------------------------------------------------------------
def _driver(*args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "cine_SENSE_real_img_2d_time.py")] + [str(a) for a in args],
                       capture_output=True, text=True, cwd=REPO, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


DRIVER_COMMON = ["--image_size", 64, "--start_level", 996, "--n_levels", 2, "--proximal_type", "L2PenaltyCG", "--cg_iters", 6,
                 "--lr_scaled", 10000]


def test_driver_radial_cine(tmp_path):
    from inverseproblemwithdiffusionmodel_amd.synthetic import radial_trajectory
    out = _driver("--trajectory", "radial", "--spokes", 8, "--readout", 32, "--save_dir", tmp_path, *DRIVER_COMMON)
    assert "reconstruction time" in out
    rec, k, zf, meas = (torch.load(tmp_path / f, weights_only=False)
                        for f in ("reconstructions.pt", "trajectory.pt", "ZF.pt", "measurement.pt"))
    assert tuple(rec.shape) == (1, 24, 1, 64, 64) and rec.dtype == torch.complex64
    assert tuple(k.shape) == (24, 256, 2) and k.dtype == torch.float64 and tuple(zf.shape) == (24, 1, 64, 64)
    assert tuple(meas.shape) == (4, 24, 1, 256)
    assert torch.equal(k.reshape(-1, 2), radial_trajectory(24 * 8, 32, 64, 64))          # the spoke index runs on across frames
    assert torch.isfinite(torch.view_as_real(rec)).all() and torch.isfinite(torch.view_as_real(zf)).all()
    assert torch.isfinite(torch.view_as_real(meas)).all()
    assert not (tmp_path / "mask.pt").exists()


def test_driver_measured_cine_samples(tmp_path):
    """--kspace / --trajectory / --sens_maps on files the test writes: (n, T, M) samples of a pulsating phantom through the
    float64 transform, frame t on trajectory t, in arbitrary scanner units"""
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    T, H, W = 24, 64, 64
    k = frame_trajectory(T, H, W, spokes=8, readout=32, edges=False)
    S = nh.smooth_maps(4, H, W, seed=2)
    img = phantom_image(H, W, seed=0).numpy()[:, 0]
    y = np.stack([37.0 * (1.0 + 0.1 * np.cos(2 * np.pi * t / T)) * nh.sense_forward(img, S, k[t])[:, 0] for t in range(T)], axis=1)
    np.save(tmp_path / "y.npy", y.astype(np.complex64))
    np.save(tmp_path / "k.npy", k)
    np.save(tmp_path / "maps.npy", S)
    out = _driver("--kspace", tmp_path / "y.npy", "--trajectory", tmp_path / "k.npy", "--sens_maps", tmp_path / "maps.npy",
                  "--save_dir", tmp_path / "out", *DRIVER_COMMON)
    assert "k-space scale" in out
    rec, zf = (torch.load(tmp_path / "out" / f, weights_only=False) for f in ("reconstructions.pt", "ZF.pt"))
    assert tuple(rec.shape) == (1, T, 1, H, W) and torch.isfinite(torch.view_as_real(rec)).all()
    assert tuple(zf.shape) == (T, 1, H, W) and abs(float(zf.abs().max()) - 1.0) < 1e-5    # peak |zero_filled| over all frames = 1
    assert torch.equal(torch.load(tmp_path / "out" / "trajectory.pt", weights_only=False), torch.from_numpy(k))
    assert tuple(torch.load(tmp_path / "out" / "measurement.pt", weights_only=False).shape) == (4, T, 1, 256)
    assert not (tmp_path / "out" / "original.pt").exists() and not (tmp_path / "out" / "mask.pt").exists()
