"""Non-Cartesian SENSE, host side (no GPU): the C ABI's new entries, the size rule, every host refusal, the trajectory
helpers, and self-checks of the float64 restatement (tests/noncart_helpers.py) that the GPU tests compare against."""
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import noncart_helpers as nh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["ipdm_nc_supported", "ipdm_ndft_forward_c64", "ipdm_ndft_adjoint_c64", "ipdm_toeplitz_psf_f32",
               "ipdm_toeplitz_normal_c64", "ipdm_nc_sense_cg_workspace_bytes", "ipdm_nc_sense_cgprox_f32",
               "ipdm_ald_nc_sense_cg_step_f32", "ipdm_ndft_workspace_bytes", "ipdm_toeplitz_psf_workspace_bytes",
               "ipdm_toeplitz_workspace_bytes"]
DRIVER = os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py")


@pytest.fixture(scope="module")
def pkg():
    from inverseproblemwithdiffusionmodel_amd import _lib, ops, engine, synthetic
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import proximal_op, ALD_optimizers, MAP_optimizers
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import noncartesian
    return Namespace(lib=_lib, ops=ops, prox=proximal_op, nc=noncartesian, engine=engine, syn=synthetic, load=load_data,
                     ald=ALD_optimizers, map=MAP_optimizers)


def _header_args(name):
    text = open(os.path.join(REPO, "include", "ipdm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/ipdm.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_abi_entries(pkg, name):
    assert name in pkg.lib.SIGNATURES
    assert len(pkg.lib.SIGNATURES[name]) == _header_args(name)
    assert hasattr(pkg.lib.lib, name)                                        # exported by the built library


def test_abi_is_additive(pkg):
    sig = pkg.lib.SIGNATURES
    assert pkg.lib.lib.ipdm_abi_version() == 4
    # the fused tail: ipdm_pc_sense_cg_step_f32's list with (sens, psf) in place of (y, sens, sens_complex, sens_sets, mask, mask_t)
    assert len(sig["ipdm_ald_nc_sense_cg_step_f32"]) == len(sig["ipdm_pc_sense_cg_step_f32"]) - 4
    assert sig["ipdm_ald_nc_sense_cg_step_f32"][:13] == sig["ipdm_pc_sense_cg_step_f32"][:13]      # ..., dev_sched, sched_stride
    for n in ("ipdm_nc_sense_cg_workspace_bytes", "ipdm_ndft_workspace_bytes", "ipdm_toeplitz_psf_workspace_bytes",
              "ipdm_toeplitz_workspace_bytes"):
        assert getattr(pkg.lib.lib, n).restype is pkg.lib.c_int64


def test_size_rule_and_workspaces(pkg):
    ops = pkg.ops
    for H, W in [(16, 16), (48, 80), (1024, 1024), (64, 80), (128, 128), (16, 1024)]:
        assert ops.nc_supported(H, W) and ops.kspace_size_class(2 * H, 2 * W) != ops.KSPACE_NONE, (H, W)
    for H, W in [(24, 56), (1040, 1040), (16, 1040), (15, 16), (16, 17), (2048, 2048), (0, 16), (-4, 16), (4, 1000)]:
        assert not ops.nc_supported(H, W), (H, W)
    for H in range(1, 200):
        for W in (16, 40, 1000):
            assert ops.nc_supported(H, W) == (ops.kspace_size_class(2 * H, 2 * W) != ops.KSPACE_NONE), (H, W)
    f = pkg.lib.lib.ipdm_nc_sense_cg_workspace_bytes
    # the Toeplitz chain's n * B * H * 2W values + (T v, r, p) + 16 bytes of state per sample
    assert f(3, 4, 16, 32) == (2 * 4 + 3) * 3 * 16 * 32 * 8 + 3 * 16
    assert f(3, 4, 24, 56) == 0 and f(0, 4, 16, 16) == 0
    assert pkg.lib.lib.ipdm_toeplitz_workspace_bytes(3, 4, 16, 32) == 4 * 3 * 16 * 64 * 8
    assert pkg.lib.lib.ipdm_ndft_workspace_bytes(100, 16, 32) == (16 + 64) * 100 * 8
    assert "2H x 2W" in ops.NC_SIZE_RULE


# ---- refusals, all on the host ---------------------------------------------------------------------------------------------
def test_operator_refusals(pkg):
    NC = pkg.nc.NonCartesianSENSE
    k = pkg.syn.radial_trajectory(4, 16, 16, 16)
    maps = np.ones((3, 16, 16), dtype=np.complex64)
    with pytest.raises(ValueError, match=r"not \(M, 2\)"):
        NC(k.T.contiguous(), (1, 16, 16))
    with pytest.raises(ValueError, match=r"not \(M, 2\)"):
        NC(k[:, :1], (1, 16, 16))
    bad = k.clone()
    bad[3, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        NC(bad, (1, 16, 16))
    bad = k.clone()
    bad[3, 1] = 8.5
    with pytest.raises(ValueError, match=r"leaves \[-N/2, N/2\]"):
        NC(bad, (1, 16, 16))
    edge = k.clone()
    edge[0], edge[1] = torch.tensor([-8.0, 8.0]), torch.tensor([8.0, -8.0])
    NC(edge, (1, 16, 16))                                                    # the bounds themselves are served
    with pytest.raises(ValueError, match="not negative"):
        NC(k, (1, 16, 16), weights=-torch.ones(len(k)))
    with pytest.raises(ValueError, match="do not match the 64 samples"):
        NC(k, (1, 16, 16), weights=torch.ones(len(k) + 1))
    with pytest.raises(ValueError, match=r"do not match \(n_coils, 16, 16\)"):
        NC(k, (1, 16, 16), sens_maps=np.ones((3, 16, 32)))
    with pytest.raises(ValueError, match="map sets .* out of scope"):
        NC(k, (1, 16, 16), sens_maps=np.ones((2, 3, 16, 16)))
    with pytest.raises(pkg.lib.IpdmUnsupported, match="2H x 2W must be a served k-space size"):
        NC(pkg.syn.radial_trajectory(4, 16, 24, 56), (1, 24, 56))
    op = NC(k, (1, 16, 16), sens_maps=maps)
    assert op.num_sens == 3 and op.n_samples == 64 and op.trajectory.dtype == torch.float64
    assert torch.allclose((op.sens_maps.abs() ** 2).sum(0), torch.ones(16, 16, dtype=torch.float64))    # normalize=True
    with pytest.raises(NotImplementedError, match="L2PenaltyCG"):
        op.projection(None, None, 1.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        op(torch.zeros(1, 1, 16, 16, dtype=torch.complex64))
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import LinearTransform
    assert type(op).log_lh_grad is LinearTransform.log_lh_grad               # the ABC's concrete gradient


def test_proximal_and_optimiser_refusals(pkg):
    op = pkg.nc.NonCartesianSENSE(pkg.syn.radial_trajectory(4, 16, 16, 16), (1, 16, 16))
    with pytest.raises(NotImplementedError, match="L2Penalty: .* use L2PenaltyCG"):
        pkg.prox.L2Penalty(op)
    with pytest.raises(NotImplementedError, match="SingleCoil: .* use L2PenaltyCG"):
        pkg.prox.SingleCoil(op)
    cg = pkg.prox.L2PenaltyCG(op, max_iter=7)
    assert cg.max_iter == 7 and cg.coef(3.0, 0.5) == 6.0
    with pytest.raises(NotImplementedError, match="MAPModel: NonCartesianSENSE"):
        pkg.map.MAPModel(torch.zeros(1, 1, 1, 64, dtype=torch.complex64), op, None, 0.1, device="cpu")
    with pytest.raises(NotImplementedError, match="SENSEMAP: NonCartesianSENSE"):
        pkg.map.SENSEMAP(None, None, None, op, 1.0, Namespace(MAP=Namespace(n_iters=1, lr=0.1)))
    with pytest.raises(NotImplementedError, match="MAPOptimizer2DTime: NonCartesianSENSE"):
        pkg.map.MAPOptimizer2DTime(None, None, None, Namespace(config=Namespace(data=Namespace(channels=64))), op, None, {})
    sampler = pkg.ald.ALDInvSegProximalRealImag(pkg.prox.Constrained(op), 1.0, "linear", (1, 1, 16, 16), None,
                                                torch.ones(2), {}, None, None, op, device="cpu")
    with pytest.raises(NotImplementedError, match="takes L2PenaltyCG"):
        sampler._check_fast_path({})
    sampler.proximal = cg
    assert sampler._check_fast_path({}) is None
    with pytest.raises(NotImplementedError, match="ALD2DTime: NonCartesianSENSE"):
        pkg.ald.ALD2DTime(cg, None, torch.ones(2), (1, 1, 1, 16, 16), None, torch.ones(2), {}, None, None, op, device="cpu")


def test_ops_refuse_before_the_gpu(pkg):
    ops = pkg.ops
    z = torch.zeros(1, 16, 16)
    with pytest.raises(ValueError, match="max_iter"):
        ops.nc_sense_cgprox(z, z, None, None, None, 1.0, max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        ops.ald_nc_sense_cg_step(z, z, z, z, None, None, None, None, tol=-1.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.nc_sense_cgprox(z, z, None, None, None, 1.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.ndft_forward(torch.zeros(1, 16, 16, dtype=torch.complex64), torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.toeplitz_psf(torch.zeros(4, 2, dtype=torch.float64), 16, 16)


def test_build_problem_refusals(pkg):
    bp = pkg.engine.build_problem
    k = pkg.syn.radial_trajectory(4, 16, 16, 16)
    kw = dict(H=16, W=16, trajectory=k)
    for extra, msg in ((dict(estimate_maps=True), "estimate_maps="), (dict(coil_compress=2), "coil_compress="),
                       (dict(n_slices=2), "n_slices="), (dict(mask=np.ones(16)), "mask=")):
        with pytest.raises(ValueError, match=msg + " does not go with trajectory="):
            bp("cpu", 1, **kw, **extra)
    with pytest.raises(ValueError, match="takes L2PenaltyCG"):
        bp("cpu", 1, proximal="SingleCoil", **kw)
    with pytest.raises(ValueError, match="pass sens_maps="):
        bp("cpu", 1, measurement=torch.zeros(4, 64, dtype=torch.complex64), **kw)
    with pytest.raises(ValueError, match=r"complex \(n_coils, M = 64\)"):
        bp("cpu", 1, measurement=torch.zeros(4, 63, dtype=torch.complex64), sens_maps=np.ones((4, 16, 16)), **kw)
    with pytest.raises(ValueError, match="4 coil signals, 3 coil maps"):
        bp("cpu", 1, measurement=torch.zeros(4, 64, dtype=torch.complex64), sens_maps=np.ones((3, 16, 16)), **kw)
    with pytest.raises(pkg.lib.IpdmUnsupported, match="2H x 2W"):
        bp("cpu", 1, H=24, W=56, trajectory=pkg.syn.radial_trajectory(4, 16, 24, 56))
    with pytest.raises(ValueError, match="traj_weights= goes with trajectory="):
        bp("cpu", 1, H=16, W=16, traj_weights=torch.ones(4))


def _driver(*args):
    r = subprocess.run([sys.executable, DRIVER, *args], capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr)


@pytest.mark.parametrize("args,msg", [
    (["--trajectory", "radial"], "--trajectory radial needs --spokes N"),
    (["--trajectory", "radial", "--spokes", "8", "--proximal_type", "L2Penalty"], "takes --proximal_type L2PenaltyCG, not L2Penalty"),
    (["--trajectory", "radial", "--spokes", "8", "--mask_2d"], "--trajectory does not go with --mask_2d"),
    (["--trajectory", "radial", "--spokes", "8", "--estimate_maps"], "--trajectory does not go with --estimate_maps"),
    (["--trajectory", "radial", "--spokes", "8", "--n_slices", "2"], "--trajectory does not go with --n_slices"),
    (["--trajectory", "radial", "--spokes", "8", "--image_size", "24", "--image_width", "56"], "no non-Cartesian kernel for 24x56"),
    (["--trajectory", "radial", "--spokes", "8", "--kspace", "y.npy"], "--kspace PATH needs --trajectory PATH"),
    (["--spokes", "8"], "--spokes / --readout go with --trajectory radial"),
    (["--trajectory", "nowhere.txt"], "a .npy or .pt file"),
])
def test_driver_refuses_before_the_network(args, msg):
    """each refusal is the process' exit message; none of them reaches the GPU (this test runs without one)"""
    rc, out = _driver("--image_size", "16", *args) if "--image_size" not in args else _driver(*args)
    assert rc != 0 and msg in out, out[-600:]


def test_driver_measured_form_checks(tmp_path):
    k = nh.radial(4, 16, 16, 16)
    np.save(tmp_path / "k.npy", k)
    np.save(tmp_path / "y.npy", np.zeros((4, 63), dtype=np.complex64))
    np.save(tmp_path / "far.npy", k * 3)
    rc, out = _driver("--image_size", "16", "--trajectory", str(tmp_path / "k.npy"), "--kspace", str(tmp_path / "y.npy"))
    assert rc != 0 and "needs --sens_maps PATH" in out
    rc, out = _driver("--image_size", "16", "--trajectory", str(tmp_path / "k.npy"), "--kspace", str(tmp_path / "y.npy"),
                      "--sens_maps", str(tmp_path / "maps.npy"))
    assert rc != 0 and "(n_coils, 64) expected" in out
    rc, out = _driver("--image_size", "16", "--trajectory", str(tmp_path / "far.npy"))
    assert rc != 0 and "leaves [-N/2, N/2]" in out


# ---- trajectory helpers and loaders ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("golden_angle", [True, False])
@pytest.mark.parametrize("H,W,spokes,readout", [(16, 16, 8, 32), (16, 32, 6, 40), (24, 40, 10, 64), (128, 128, 32, 256)])
def test_radial_trajectory_and_density(pkg, H, W, spokes, readout, golden_angle):
    k = pkg.syn.radial_trajectory(spokes, readout, H, W, golden_angle=golden_angle)
    assert k.dtype == torch.float64 and tuple(k.shape) == (spokes * readout, 2)
    assert float(k[:, 0].abs().max()) <= H / 2 and float(k[:, 1].abs().max()) <= W / 2
    assert np.allclose(k.numpy(), nh.radial(spokes, readout, H, W, golden=golden_angle), rtol=0, atol=1e-12)
    assert float(k[readout // 2].abs().max()) == 0.0                          # every spoke runs through the centre
    w = pkg.syn.radial_density(k, H, W)
    assert tuple(w.shape) == (len(k),) and float(w.min()) > 0 and abs(float(w.sum()) - H * W) < 1e-9 * H * W
    pkg.nc.check_trajectory(k, H, W)


def test_loaders(pkg, tmp_path):
    k = nh.radial(4, 16, 16, 16)
    np.save(tmp_path / "k.npy", k.astype(np.float32))
    torch.save(torch.from_numpy(k), tmp_path / "k.pt")
    for name in ("k.npy", "k.pt"):
        t = pkg.load.load_trajectory(str(tmp_path / name))
        assert t.dtype == torch.float64 and tuple(t.shape) == (64, 2)
    np.save(tmp_path / "bad.npy", k.T)
    with pytest.raises(ValueError, match=r"\(M, 2\)"):
        pkg.load.load_trajectory(str(tmp_path / "bad.npy"))
    np.save(tmp_path / "int.npy", np.zeros((4, 2), dtype=np.int64))
    with pytest.raises(TypeError, match="real floating"):
        pkg.load.load_trajectory(str(tmp_path / "int.npy"))
    with pytest.raises(ValueError, match=".npy or .pt"):
        pkg.load.load_trajectory(str(tmp_path / "k.txt"))
    np.save(tmp_path / "y.npy", np.zeros((4, 64), dtype=np.complex128))
    y = pkg.load.load_kspace(str(tmp_path / "y.npy"), noncartesian=True)
    assert y.dtype == torch.complex64 and tuple(y.shape) == (4, 64)
    np.save(tmp_path / "cube.npy", np.zeros((2, 3, 4), dtype=np.complex64))
    with pytest.raises(ValueError, match=r"\(n_coils, M\)"):
        pkg.load.load_kspace(str(tmp_path / "cube.npy"), noncartesian=True)
    with pytest.raises(ValueError, match="neither cine=True nor slices=True"):
        pkg.load.load_kspace(str(tmp_path / "y.npy"), noncartesian=True, slices=True)


# ---- self-checks of the float64 restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("H,W,spokes,readout", [(16, 16, 8, 32), (16, 32, 6, 40), (24, 40, 10, 64)])
def test_restatement_toeplitz_is_the_normal_operator(H, W, spokes, readout, weighted):
    rng = np.random.default_rng(0)
    k = nh.radial(spokes, readout, H, W)
    w = nh.ramp_weights(k, H, W) if weighted else None
    S = nh.smooth_maps(3, H, W)
    x = rng.standard_normal((2, H, W)) + 1j * rng.standard_normal((2, H, W))
    Pc = nh.toeplitz_psf_complex(k, H, W, w)
    assert np.abs(Pc.imag).max() <= 1e-12 * np.abs(Pc).max()
    assert Pc.real.min() < 0                                                 # a spectrum, not a density: it changes sign
    assert nh.relerr(nh.toeplitz_normal(x, S, Pc.real), nh.normal_direct(x, S, k, w)) <= 1e-12
    T = nh.toeplitz_T(k, H, W, w)
    assert not T[0].any() and not T[:, 0].any()
    assert np.abs(T[1:, 1:] - T[1:, 1:][::-1, ::-1].conj()).max() <= 1e-12 * np.abs(T).max()     # Hermitian in the lag
    assert abs(T[H, W] - (len(k) if w is None else w.sum())) <= 1e-9 * len(k)


@pytest.mark.parametrize("H,W", [(16, 16), (16, 32), (24, 40)])
def test_restatement_on_grid_is_the_centred_fft(H, W):
    rng = np.random.default_rng(1)
    mask = rng.random((H, W)) < 0.4
    mask[0, 0] = mask[H - 1, W - 1] = True
    r, c = np.nonzero(mask)
    k = np.stack([r - H / 2, c - W / 2], axis=1)
    x = rng.standard_normal((2, H, W)) + 1j * rng.standard_normal((2, H, W))
    full = np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(x, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))
    assert nh.relerr(nh.ndft_forward(x, k), full[:, r, c]) <= 1e-12
    y = rng.standard_normal((2, len(k))) + 1j * rng.standard_normal((2, len(k)))
    lhs, rhs = np.vdot(y, nh.ndft_forward(x, k)), np.vdot(nh.ndft_adjoint(y, k, H, W), x)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_restatement_cg_converges_below_the_cap():
    H, W = 16, 16
    rng = np.random.default_rng(2)
    k = nh.radial(8, 32, H, W)
    S = nh.smooth_maps(4, H, W, seed=1)
    z = rng.standard_normal((2, H, W)) + 1j * rng.standard_normal((2, H, W))
    ahy = nh.sense_adjoint(nh.sense_forward(0.7 * z, S, k), S, k, H, W)
    P = nh.toeplitz_psf(k, H, W)
    for a in (1.0, 4.0):
        x, it = nh.cg_prox(z, ahy, lambda v: nh.toeplitz_normal(v, S, P), a, 40, 1e-5)
        assert (0 < it).all() and (it < 40).all()
        assert nh.prox_residual(x, z, ahy, S, k, a).max() <= 2e-5
    x, it = nh.cg_prox(z, ahy, lambda v: nh.toeplitz_normal(v, S, P), 0.0, 40, 1e-5)
    assert not it.any() and (x == z).all()
