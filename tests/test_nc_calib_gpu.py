"""Non-Cartesian self-calibration on the GPU: the weighted Gram matrix of the samples, the calibration
images, the maps and the compression of ``NonCartesianSENSE`` against the float64 chain of tests/nc_calib_helpers.py, the
operator ``from_measurement`` returns under both samplers, and the two drivers with --self_calibrate.

The Gram matrix is a double sum rounded once: its bound is that rounding (2^-24 of the entry) plus the float64 model's own
reordering error (1e-13 of sqrt(G_ii G_jj)), not an observation.  Every other tolerance is ten times the largest figure
observed on the MI355X (the table in DESIGN.md 4.4n); the metric is max|err| / max|ref|."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import coilcomp_helpers as cch
import csm_helpers as csm
import espirit_helpers as esp
import nc_calib_helpers as nc
import noncart_helpers as nh
import test_noncart_frames_gpu as frames
import test_noncart_gpu as base
from conftest import state_dict_from_golden

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 10 x the largest figure observed on the MI355X over the cases below (DESIGN.md 4.4n lists the observed figures)
TOL = dict(calib_images=6.2e-3, walsh_maps=4.0e-5, espirit_maps=2.1e-4, compress=6.8e-5)

dev, host = base.dev, base.host


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd import synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ncsn3d, ALD_optimizers, proximal_op
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import noncartesian
    return Namespace(ncsnv2=ncsnv2, ncsn3d=ncsn3d, ald=ALD_optimizers, prox=proximal_op, nc=noncartesian, syn=synthetic)


# ---- 1. the Gram matrix of the samples ------------------------------------------------------------------------------------------
def _weights(kind, M, rng):
    if kind == "none":
        return None
    w = np.linspace(0.0, 2.0, M, dtype=np.float32) if M > 1 else np.array([0.75], dtype=np.float32)
    if kind == "zeros":                                                      # whole runs of zero weight, across chunk borders
        w = w.copy()
        w[rng.random(M) < 0.4] = 0.0
        w[M // 3:M // 3 + 40] = 0.0
        if M == 1:
            w[:] = 0.5
    return w


def _gram_bound(ref):
    d = np.sqrt(np.abs(np.einsum("bii->bi", ref)))
    return 2.0 ** -24 * np.abs(ref) * np.sqrt(2.0) + 1e-13 * d[:, :, None] * d[:, None, :] + 1e-300


@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("M", ["1", "C-1", "C", "C+1", "3C+7"])
def test_nc_coil_gram_vs_float64(ops, M, n):
    C = ops.NC_GRAM_CHUNK
    M = {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "3C+7": 3 * C + 7}[M]
    rng = np.random.default_rng(1000 * n + M)
    y = ((rng.standard_normal((n, 3, M)) + 1j * rng.standard_normal((n, 3, M))) * rng.uniform(0.5, 2.0, (n, 1, 1))).astype(np.complex64)
    yd = dev(y)
    worst = 0.0
    for kind in ("none", "ramp", "zeros"):
        w = _weights(kind, M, rng)
        wd = None if w is None else dev(w)
        ref = nc.gram(y, w)
        G = ops.nc_coil_gram(yd, wd)
        assert tuple(G.shape) == (3, n, n) and G.dtype == torch.complex64
        g = host(G).astype(np.complex128)
        assert (np.abs(g - ref) <= _gram_bound(ref)).all(), (kind, float(np.abs(g - ref).max()))
        worst = max(worst, float((np.abs(g - ref) / _gram_bound(ref)).max()))
        assert torch.equal(G, G.conj().transpose(1, 2)) and not host(torch.diagonal(G, dim1=1, dim2=2).imag).any()   # Hermitian, exactly
        assert torch.equal(ops.nc_coil_gram(yd, wd), G)                      # two runs, the same bits
        for b in range(3):                                                   # B = 1: row b of the batch, bit for bit
            assert torch.equal(ops.nc_coil_gram(yd[:, b:b + 1].contiguous(), wd)[0], G[b])
        if kind == "zeros":                                                  # zero-weight samples are never read
            y_nan = y.copy()
            y_nan[:, :, w == 0] = np.nan + 1j * np.nan
            G_nan = ops.nc_coil_gram(dev(y_nan), wd)
            assert torch.isfinite(torch.view_as_real(G_nan)).all() and torch.equal(G_nan, G)
    print(f"nc_coil_gram n {n} M {M}: worst error / bound {worst:.2f}")


def test_nc_coil_gram_operands(ops):
    y = torch.zeros(4, 2, 50, dtype=torch.complex64, device="cuda")
    out = torch.empty(2, 4, 4, dtype=torch.complex64, device="cuda")
    work = ops.nc_coil_gram_workspace(2, 4, 50, "cuda")
    assert ops.nc_coil_gram(y, out=out, work=work) is out and not host(out).any()
    with pytest.raises(TypeError, match="complex64"):
        ops.nc_coil_gram(y.to(torch.complex128))
    with pytest.raises(TypeError, match="contiguous"):
        ops.nc_coil_gram(y.transpose(0, 1))
    with pytest.raises(ValueError, match=r"is not \[n_coils, B, M\]"):
        ops.nc_coil_gram(y[0])
    with pytest.raises(ValueError, match="do not match the 50 samples"):
        ops.nc_coil_gram(y, torch.ones(49, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        ops.nc_coil_gram(y, torch.ones(50, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.nc_coil_gram(y, out=out[:1])
    with pytest.raises(ValueError, match="work"):
        ops.nc_coil_gram(y, work=work[:4])
    with pytest.raises(NotImplementedError, match="1..64"):
        ops.nc_coil_gram(torch.zeros(65, 1, 8, dtype=torch.complex64, device="cuda"))
    assert tuple(ops.nc_coil_gram(y[:, :0].contiguous()).shape) == (0, 4, 4)   # an empty batch


# ---- 2. the calibration images --------------------------------------------------------------------------------------------------
CALIB_SHAPES = [(16, 16, 12, 32, 4, 1), (16, 32, 16, 64, 3, 1), (32, 32, 24, 64, 8, 2)]
# tol = 0 and a fixed count at which conjugate gradients have converged in both precisions: the systems have condition
# numbers of 2e3 .. 4e3 (1 / lam times the oversampling of the centre), and before convergence float32 CG lags float64 CG
# by a few iterations -- at 20 iterations the two differ by 1e-2, which says nothing about the solution
CALIB_ITERS = 200

_CASES = {}


def calib_case(H, W, spokes, readout, n, B):
    key = (H, W, spokes, readout, n, B)
    if key not in _CASES:
        acq = nc.acquisition(H, W, spokes, readout, n, seed=n, B=B)
        ah, aw, w = nc.window(acq["k"], H, W)
        _CASES[key] = Namespace(acq=acq, ah=ah, aw=aw, w=w.astype(np.float32), k=acq["k"], y=acq["y"])
    return _CASES[key]


@pytest.mark.parametrize("H,W,spokes,readout,n,B", CALIB_SHAPES)
def test_nc_calib_images_vs_float64(ops, pkg, H, W, spokes, readout, n, B):
    c = calib_case(H, W, spokes, readout, n, B)
    ah, aw, w = pkg.nc.calibration_window(c.k, H, W)
    assert (ah, aw) == (c.ah, c.aw) and np.array_equal(w.numpy().astype(np.float32), c.w)
    ref, _ = nc.calib_images(c.y, c.k, H, W, c.w, 1e-2, CALIB_ITERS, 0.0)
    x, iters = ops.nc_calib_images(dev(c.y), dev(c.k), H, W, dev(c.w), lam=1e-2, max_iter=CALIB_ITERS, tol=0.0, return_iters=True)
    assert tuple(x.shape) == (n, B, H, W) and x.dtype == torch.complex64 and tuple(iters.shape) == (n, B)
    assert (host(iters) == CALIB_ITERS).all()
    e = nh.relerr(host(x), ref)
    ks = ops.nc_calib_kspace(dev(c.y), dev(c.k), H, W, dev(c.w), lam=1e-2, max_iter=CALIB_ITERS, tol=0.0)
    e_k = nh.relerr(host(ks), nh.fft2c(ref))
    full = nc.box_of(c.acq["full"], c.ah, c.aw)
    box = nh.relerr(nc.box_of(host(ks), c.ah, c.aw), full)
    print(f"nc_calib_images {H}x{W} n {n} B {B}: box {2 * ah + 1} x {2 * aw + 1}, images {e:.3g}, k-space {e_k:.3g}; gridded box "
          f"against the Cartesian one {box:.3g}")
    assert e <= TOL["calib_images"] and e_k <= TOL["calib_images"]
    # the default tolerance stops the solve under the default cap of 40, as it stops the float64 model
    _, it64 = nc.calib_images(c.y, c.k, H, W, c.w)
    _, it32 = ops.nc_calib_images(dev(c.y), dev(c.k), H, W, dev(c.w), return_iters=True)
    print(f"    default solve: iterations float64 {it64.ravel().tolist()}  GPU {host(it32).ravel().tolist()}")
    assert it64.max() < 40 and (0 < host(it32)).all() and (host(it32) < 40).all()


def test_nc_calib_images_operands(ops):
    y = torch.zeros(2, 1, 64, dtype=torch.complex64, device="cuda")
    k = torch.zeros(64, 2, dtype=torch.float64, device="cuda")
    w = torch.ones(64, device="cuda")
    with pytest.raises(ValueError, match="is not \\(64, 2\\)"):
        ops.nc_calib_images(y, k[:63].contiguous(), 16, 16, w)
    with pytest.raises(TypeError, match="float64"):
        ops.nc_calib_images(y, k.float(), 16, 16, w)
    with pytest.raises(ValueError, match="weights"):
        ops.nc_calib_images(y, k, 16, 16, None)
    with pytest.raises(ValueError, match="lam must be positive"):
        ops.nc_calib_images(y, k, 16, 16, w, lam=0.0)
    with pytest.raises(ValueError, match="max_iter"):
        ops.nc_calib_images(y, k, 16, 16, w, max_iter=0)
    with pytest.raises(ValueError, match="all zero"):
        ops.nc_calib_images(y, k, 16, 16, torch.zeros(64, device="cuda"))
    with pytest.raises(NotImplementedError, match="2H x 2W"):
        ops.nc_calib_images(y, k, 24, 56, w)


# ---- 3. maps and compression against the float64 chain ------------------------------------------------------------------------------
SOLVER = dict(lam=1e-2, max_iter=CALIB_ITERS, tol=0.0)       # both chains solve to convergence


@pytest.fixture(scope="module")
def chain():
    """32x32, golden-angle 24 x 64, 4 coils: the float64 calibration k-space, once"""
    c = calib_case(32, 32, 24, 64, 4, 1)
    ks, _ = nc.calib_kspace(c.y, c.k, 32, 32, c.w, **SOLVER)
    return Namespace(c=c, ks=ks)


def test_estimate_sens_maps_walsh_vs_float64(pkg, chain):
    c = chain.c
    ref = csm.estimate(torch.from_numpy(chain.ks), c.ah, c.aw)
    maps = pkg.nc.NonCartesianSENSE.estimate_sens_maps(c.y[:, 0], c.k, (1, 32, 32), **SOLVER)
    assert tuple(maps.shape) == (4, 32, 32) and maps.dtype == torch.complex128 and not maps.is_cuda
    near = csm.near_threshold(ref["rss"], ref["rss_max"], 0.02)[0]
    got_sup = maps.abs().sum(0) > 0
    assert bool(((got_sup == ref["support"][0]) | near).all())
    keep = ref["support"][0] & got_sup & ~near
    e = float((maps - ref["maps"][:, 0]).abs()[:, keep].max())
    rss = (maps.abs() ** 2).sum(0).sqrt()[got_sup]
    print(f"estimate_sens_maps walsh: {int(keep.sum())} pixels, max {e:.3g}; |rss - 1| {float((rss - 1).abs().max()):.2g}")
    assert float((rss - 1).abs().max()) <= 1e-5 and float(maps[0].imag.abs().max()) <= 1e-6 and float(maps[0].real.min()) >= 0
    # for the record: the default solve (lam 1e-2, cap 40, tol 1e-4) against Walsh maps of fully sampled Cartesian k-space
    cart = csm.estimate(torch.from_numpy(c.acq["full"]), c.ah, c.aw)
    dflt = pkg.nc.NonCartesianSENSE.estimate_sens_maps(c.y[:, 0], c.k, (1, 32, 32))
    both = cart["support"][0] & (dflt.abs().sum(0) > 0) & ~csm.near_threshold(cart["rss"], cart["rss_max"], 0.02)[0]
    d = (dflt - cart["maps"][:, 0]).abs()[:, both]
    print(f"    default solve against fully sampled Cartesian Walsh maps: max {float(d.max()):.3g}, rms {float(d.pow(2).mean().sqrt()):.3g}")
    assert int(keep.sum()) > 500 and e <= TOL["walsh_maps"]


def test_estimate_sens_maps_espirit_vs_float64(pkg, chain):
    c = chain.c
    ref = esp.estimate(chain.ks[:, 0], c.ah, c.aw, k=4)
    maps, eig = pkg.nc.NonCartesianSENSE.estimate_sens_maps(c.y[:, 0], c.k, (1, 32, 32), method="espirit", ksize=4,
                                                            return_eig=True, **SOLVER)
    assert tuple(maps.shape) == (4, 32, 32) and tuple(eig.shape) == (32, 32) and eig.dtype == torch.float32
    assert ref["margin"] > 0.02                                              # no singular value on the rank threshold
    e_eig = float(np.abs(eig.numpy() - ref["eigval"]).max())
    kept = eig.numpy() > 0.8
    assert ((kept == (ref["eigval"] > 0.8)) | ref["leave_out"]).all()
    keep = kept & (ref["eigval"] > 0.8) & ~ref["leave_out"]
    e = float(np.abs(maps.numpy() - ref["maps"])[:, keep].max())
    print(f"estimate_sens_maps espirit ksize 4: rank {ref['rank']}, {int(keep.sum())} pixels, max {e:.3g}; eigenvalue map {e_eig:.3g}")
    assert int(keep.sum()) > 500 and e <= TOL["espirit_maps"]


def test_compress_measurement_vs_float64(pkg):
    c = calib_case(32, 32, 24, 64, 8, 2)
    y = c.y[:, 0]
    psi = cch.noise_cov(8, 30.0, 5)
    for noise_cov in (None, psi):
        ref = cch.matrix(nc.gram(c.y[:, :1], c.w)[0], 4, noise_cov=noise_cov)
        y_ref = np.einsum("vc,cm->vm", ref["A"][0], y.astype(np.complex128))
        out, A = pkg.nc.NonCartesianSENSE.compress_measurement(y, c.k, (1, 32, 32), 4, noise_cov=noise_cov)
        assert tuple(out.shape) == (4, y.shape[1]) and out.is_cuda and out.dtype == torch.complex64
        assert tuple(A.shape) == (4, 8) and not A.is_cuda and A.dtype == torch.complex64
        e_A, e_y = nh.relerr(A.numpy(), ref["A"][0]), nh.relerr(host(out), y_ref)
        gaps = np.diff(ref["eig"][0][:5]) / ref["eig"][0][0]
        print(f"compress_measurement 8 -> 4{' whitened' if noise_cov is not None else ''}: A {e_A:.3g}, samples {e_y:.3g}; "
              f"eigenvalue gaps {np.abs(gaps).min():.2g} of the largest")
        assert float(A[:, 0].imag.abs().max()) <= 1e-6 and float(A[:, 0].real.min()) >= 0
        assert e_A <= TOL["compress"] and e_y <= TOL["compress"]


# ---- 4. from_measurement and the samplers -------------------------------------------------------------------------------------------
def _unit_rss_on_support(maps):
    rss = (maps.abs() ** 2).sum(0).sqrt()
    sup = rss > 0
    assert int(sup.sum()) > maps.shape[-1] * maps.shape[-2] // 4
    assert float((rss[sup] - 1).abs().max()) <= 1e-5


def test_from_measurement_static(pkg, golden):
    c = calib_case(16, 16, 12, 32, 4, 1)
    cal = pkg.nc.NonCartesianSENSE.from_measurement(c.y[:, 0], c.k, (1, 16, 16))
    op = cal.op
    assert isinstance(op, pkg.nc.NonCartesianSENSE) and not op.framed and op.num_sens == 4
    assert tuple(cal.measurement.shape) == (4, 384) and cal.measurement.is_cuda and cal.measurement.dtype == torch.complex64
    assert torch.equal(cal.measurement.cpu(), torch.from_numpy(c.y[:, 0]))   # no compression: the samples as they came
    assert tuple(cal.sens_maps.shape) == (4, 16, 16) and cal.sens_maps.dtype == torch.complex128 and cal.coil_matrix is None
    assert cal.region == (c.ah, c.aw) and cal.rss_max > 0 and tuple(cal.calib_kspace.shape) == (4, 16, 16)
    assert tuple(cal.cg_iters.shape) == (4,) and int(cal.cg_iters.min()) > 0 and int(cal.cg_iters.max()) <= 40 and cal.eigval is None
    _unit_rss_on_support(cal.sens_maps)
    # the maps against the truth on the object: the estimator sees S x, so the comparison is on the body, gauged to coil 0
    truth = torch.from_numpy(esp.true_maps(c.acq["S"]))
    body = torch.from_numpy(np.abs(c.acq["obj"][0]) > 0.2) & (cal.sens_maps.abs().sum(0) > 0)
    print(f"from_measurement 16x16: maps against the true ones on the body, max {float((cal.sens_maps - truth).abs()[:, body].max()):.3g}")
    net = pkg.ncsnv2.NCSNv2Deepest(base.tiny_config(16))
    net.load_state_dict(state_dict_from_golden(golden("g07_layers"), "net"), strict=True)
    net = net.cuda().eval()
    prox = pkg.prox.L2PenaltyCG(op, max_iter=30, tol=1e-6)
    scale = 1.0 / float(op.zero_filled(cal.measurement.reshape(4, 1, 1, -1)).abs().max())
    meas = (cal.measurement * scale).reshape(4, 1, 1, -1).repeat(1, 2, 1, 1).contiguous()
    sigmas = torch.from_numpy(np.geomspace(1.0, 0.01, 10).astype(np.float32)[:2]).cuda()
    params = dict(n_steps_each=2, step_lr=base.STEP_LR, denoise=False, final_only=True)
    sampler = pkg.ald.ALDInvSegProximalRealImag(prox, 1.0, "linear", (2, 1, 16, 16), net, sigmas, params, base.tiny_config(16), meas,
                                                op, seg=None, device=torch.device("cuda"))
    x = sampler(label=None, lamda=1.0, save_dir=None, lr_scaled=1.0 / base.STEP_LR, seg_mode="full", seed=0)[0]
    assert tuple(x.shape) == (2, 1, 16, 16) and torch.isfinite(torch.view_as_real(x)).all()
    it = host(prox.last_iters)
    assert (0 < it).all() and (it <= 30).all()


def test_from_measurement_cine(pkg, golden):
    """radial_cine_trajectory(6, 4, 32, 16, 16): one frame alone has no usable window, the pool of the six has; 5 coils to 2"""
    T, H, W, n = 6, 16, 16, 5
    kc = pkg.syn.radial_cine_trajectory(T, 4, 32, H, W)
    S = nh.smooth_maps(n, H, W, seed=4).astype(np.complex128)
    beat = 1.0 + 0.1 * np.cos(np.arange(T) * (2 * np.pi / T))
    obj = nc.ellipse_phantom(H, W)
    y = np.stack([nh.ndft_forward(S * (obj * beat[t]), kc[t].numpy()) for t in range(T)], axis=1).astype(np.complex64)   # (n, T, M)
    with pytest.raises(ValueError, match="at least 5 x 5"):
        pkg.nc.NonCartesianSENSE.from_measurement(y[:, 0], kc[0], (1, H, W))
    cal = pkg.nc.NonCartesianSENSE.from_measurement(y, kc, (1, H, W), n_virtual=2)
    op = cal.op
    assert op.framed and op.n_frames == T and op.num_sens == 2 and op.n_samples == 128
    assert tuple(cal.measurement.shape) == (2, T, 128) and tuple(cal.sens_maps.shape) == (2, H, W)
    assert tuple(cal.coil_matrix.shape) == (2, n) and cal.coil_matrix.dtype == torch.complex64 and not cal.coil_matrix.is_cuda
    assert cal.region == nc.largest_box(nc.cell_occupancy(kc.numpy(), H, W)) and tuple(cal.calib_kspace.shape) == (2, H, W)
    _unit_rss_on_support(cal.sens_maps)
    # the compression acts on the samples of every frame
    want = np.einsum("vc,ctm->vtm", cal.coil_matrix.numpy().astype(np.complex128), y.astype(np.complex128))
    assert nh.relerr(host(cal.measurement), want) <= 1e-6
    net2d, cfg = frames._net2d(pkg, golden)
    g = golden("g17_ald2dtime")
    prox = pkg.prox.L2PenaltyCG(op, max_iter=30, tol=1e-6)
    scale = 1.0 / float(op.zero_filled(cal.measurement.reshape(2, T, 1, -1)).abs().max())
    meas = (cal.measurement * scale).reshape(2, 1, T, 1, -1).contiguous()
    params = dict(n_steps_each=2, step_lr=2e-5, denoise=False, final_only=True)
    sampler = pkg.ald.ALD2DTime(prox, frames._net3d(pkg, golden), torch.from_numpy(g["sigmas_T"]).cuda(), (1, T, 1, H, W), net2d,
                                torch.from_numpy(g["sigmas"]).cuda(), params, cfg, meas, op, device=torch.device("cuda"))
    x = sampler(save_dir=None, lr_scaled=1.0e5, mode_T="none", lamda_T=1.0, if_random_shift=False, seed=0, n_levels=2)[0]
    assert tuple(x.shape) == (1, T, 1, H, W) and torch.isfinite(torch.view_as_real(x)).all()
    it = host(prox.last_iters)
    assert it.shape == (T,) and (0 < it).all() and (it <= 30).all()


def test_build_problem_self_calibrate(pkg):
    from inverseproblemwithdiffusionmodel_amd import engine
    cfg = base.tiny_config(16)
    k = pkg.syn.radial_trajectory(12, 32, 16, 16)
    prob = engine.build_problem(torch.device("cuda"), 2, H=16, W=16, num_sens=6, seed=0, cfg=cfg, trajectory=k, self_calibrate=True,
                                virtual_coils=3)
    assert prob.estimated_maps and prob.op.num_sens == 3 and tuple(prob.measurement.shape) == (3, 2, 1, 384)
    assert tuple(prob.sens_maps.shape) == (3, 16, 16) and tuple(prob.coil_matrix.shape) == (3, 6)
    assert prob.calib_region == (2, 5) and tuple(prob.calib_kspace.shape) == (3, 16, 16) and prob.image is not None
    _unit_rss_on_support(prob.sens_maps)
    # the measured form: the simulated samples of 6 coils back in, no maps
    c = calib_case(16, 16, 12, 32, 4, 1)
    prob = engine.build_problem(torch.device("cuda"), 1, H=16, W=16, seed=0, cfg=cfg, trajectory=c.k, self_calibrate=True,
                                measurement=torch.from_numpy(37.0 * c.y[:, 0]))
    assert prob.image is None and prob.op.num_sens == 4 and prob.coil_matrix is None and prob.calib_region == (c.ah, c.aw)
    assert abs(float(prob.zero_filled.abs().max()) - 1.0) < 1e-5             # the automatic scale, taken after the calibration
    plain = engine.build_problem(torch.device("cuda"), 1, H=16, W=16, seed=0, cfg=cfg, trajectory=k)
    assert not plain.estimated_maps and plain.calib_region is None and plain.calib_kspace is None and plain.coil_matrix is None


# ---- 5. the drivers -----------------------------------------------------------------------------------------------------------------
def _script(name, *args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", name)] + [str(a) for a in args], capture_output=True,
                       text=True, cwd=REPO, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_driver_self_calibrate_measured(tmp_path):
    """--kspace y.npy --trajectory k.npy --self_calibrate: no maps file; 6 coils whitened and compressed to 3"""
    acq = nc.acquisition(16, 16, 12, 32, 6, seed=2)
    np.save(tmp_path / "y.npy", 37.0 * acq["y"][:, 0])
    np.save(tmp_path / "k.npy", acq["k"])
    np.save(tmp_path / "psi.npy", cch.noise_cov(6, 10.0, 1))
    out = _script("acdc_SENSE_real_img.py", "--kspace", tmp_path / "y.npy", "--trajectory", tmp_path / "k.npy", "--self_calibrate",
                  "--virtual_coils", 3, "--noise_cov", tmp_path / "psi.npy", "--save_dir", tmp_path / "out", *base.DRIVER_COMMON)
    assert "k-space scale" in out and "RMSE" not in out
    rec, maps, A, ks, meas = (torch.load(tmp_path / "out" / f, weights_only=False)
                              for f in ("reconstructions.pt", "sens_maps.pt", "coil_matrix.pt", "calib_kspace.pt", "measurement.pt"))
    assert tuple(rec.shape) == (2, 1, 16, 16) and torch.isfinite(torch.view_as_real(rec)).all()
    assert tuple(maps.shape) == (3, 16, 16) and tuple(A.shape) == (3, 6) and tuple(ks.shape) == (3, 16, 16)
    assert tuple(meas.shape) == (3, 1, 1, 384)
    _unit_rss_on_support(maps)


def test_driver_self_calibrate_cine(tmp_path):
    out = _script("cine_SENSE_real_img_2d_time.py", "--image_size", 16, "--T", 6, "--trajectory", "radial", "--spokes", 4,
                  "--readout", 32, "--self_calibrate", "--virtual_coils", 2, "--num_sens", 5, "--mode_T", "none",
                  "--start_level", 996, "--n_levels", 2, "--proximal_type", "L2PenaltyCG", "--cg_iters", 6, "--lr_scaled", 10000,
                  "--save_dir", tmp_path)
    assert "reconstruction time" in out
    rec, maps, A, ks, meas = (torch.load(tmp_path / f, weights_only=False)
                              for f in ("reconstructions.pt", "sens_maps.pt", "coil_matrix.pt", "calib_kspace.pt", "measurement.pt"))
    assert tuple(rec.shape) == (1, 6, 1, 16, 16) and torch.isfinite(torch.view_as_real(rec)).all()
    assert tuple(maps.shape) == (2, 16, 16) and tuple(A.shape) == (2, 5) and tuple(ks.shape) == (2, 16, 16)
    assert tuple(meas.shape) == (2, 6, 1, 128)
    _unit_rss_on_support(maps)
