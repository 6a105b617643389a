"""Radial cine, host side (no GPU): the framed NonCartesianSENSE operator (one trajectory per frame), the
C ABI's `_sets` entries, the host refusals of ops, ALD2DTime and the cine driver, the cine trajectory helper and loaders."""
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
DRIVER = os.path.join(REPO, "scripts", "cine_SENSE_real_img_2d_time.py")
SETS_ENTRIES = {"ipdm_ndft_forward_sets_c64": "ipdm_ndft_forward_c64", "ipdm_ndft_adjoint_sets_c64": "ipdm_ndft_adjoint_c64",
                "ipdm_toeplitz_psf_sets_f32": "ipdm_toeplitz_psf_f32", "ipdm_toeplitz_normal_sets_c64": "ipdm_toeplitz_normal_c64",
                "ipdm_nc_sense_cgprox_sets_f32": "ipdm_nc_sense_cgprox_f32",
                "ipdm_ald_nc_sense_cg_step_sets_f32": "ipdm_ald_nc_sense_cg_step_f32"}


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


@pytest.mark.parametrize("name", sorted(SETS_ENTRIES))
def test_abi_sets_entries(pkg, name):
    """every `_sets` entry is declared, exported and is its one-set entry's list plus the set count"""
    sig = pkg.lib.SIGNATURES
    assert len(sig[name]) == _header_args(name) == len(sig[SETS_ENTRIES[name]]) + 1
    assert hasattr(pkg.lib.lib, name)
    assert [t for t in sig[name] if t is not pkg.lib.c_int] == [t for t in sig[SETS_ENTRIES[name]] if t is not pkg.lib.c_int]
    assert pkg.lib.lib.ipdm_abi_version() == 4                                # additive: the six one-set entries are unchanged


def test_sets_entries_refuse_on_the_host(pkg):
    """B % T != 0 and T < 1 are IPDM_EINVAL before any pointer is looked at (NULL operands here: no GPU is touched)"""
    L = pkg.lib.lib
    EINVAL = L.ipdm_ndft_forward_sets_c64(None, None, None, 0, None, None, 4, 1, 8, 16, 16, None)
    assert EINVAL != 0
    assert L.ipdm_ndft_forward_sets_c64(None, None, None, 3, None, None, 4, 1, 8, 16, 16, None) == EINVAL
    assert L.ipdm_ndft_adjoint_sets_c64(None, None, None, 3, None, None, None, 4, 1, 8, 16, 16, None) == EINVAL
    assert L.ipdm_toeplitz_psf_sets_f32(None, 0, None, None, None, 8, 16, 16, None) == EINVAL
    assert L.ipdm_toeplitz_normal_sets_c64(None, None, None, 3, None, None, 4, 1, 16, 16, None) == EINVAL
    assert L.ipdm_nc_sense_cgprox_sets_f32(None, None, None, None, 3, 1.0, None, 5, 0.0, None, None, None, None, 4, 1, 16, 16,
                                           None) == EINVAL
    # B == 0 with T dividing it: nothing to do
    assert L.ipdm_toeplitz_normal_sets_c64(None, None, None, 3, None, None, 0, 1, 16, 16, None) == 0


# ---- the framed operator ------------------------------------------------------------------------------------------------------
def test_framed_operator_construction(pkg):
    NC = pkg.nc.NonCartesianSENSE
    T, spf, ro = 3, 4, 16
    k = pkg.syn.radial_cine_trajectory(T, spf, ro, 16, 16)
    M = spf * ro
    op = NC(k, (1, 16, 16), sens_maps=np.ones((3, 16, 16), dtype=np.complex64))
    assert op.framed and op.n_frames == T and op.n_samples == M and op.num_sens == 3
    assert tuple(op.trajectory.shape) == (T, M, 2) and op.trajectory.dtype == torch.float64 and op.weights is None
    flat = NC(k[1], (1, 16, 16))
    assert not flat.framed and flat.n_frames == 1 and flat.n_samples == M
    one = NC(k[:1], (1, 16, 16))
    assert one.framed and one.n_frames == 1 and tuple(one.trajectory.shape) == (1, M, 2)
    # weights: (M,) is every frame's, (T, M) is per frame
    w = torch.rand(M, dtype=torch.float64)
    assert torch.equal(NC(k, (1, 16, 16), weights=w).weights, w[None].expand(T, M))
    wt = torch.rand(T, M, dtype=torch.float64)
    assert torch.equal(NC(k, (1, 16, 16), weights=wt).weights, wt)
    with pytest.raises(ValueError, match=r"match neither the 64 samples nor \(3, 64\)"):
        NC(k, (1, 16, 16), weights=torch.ones(T, M + 1))
    with pytest.raises(ValueError, match="not negative"):
        NC(k, (1, 16, 16), weights=-torch.ones(T, M))
    # bounds and finiteness per frame, the frame named
    bad = k.clone()
    bad[2, 5, 1] = 8.5
    with pytest.raises(ValueError, match=r"frame 2 of the trajectory leaves \[-N/2, N/2\]"):
        NC(bad, (1, 16, 16))
    bad = k.clone()
    bad[1, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="frame 1 of the trajectory holds non-finite"):
        NC(bad, (1, 16, 16))
    with pytest.raises(ValueError, match=r"not \(M, 2\)"):
        NC(torch.zeros(T, M, 3, dtype=torch.float64), (1, 16, 16))
    with pytest.raises(ValueError, match=r"not \(M, 2\)"):
        NC(torch.zeros(2, T, M, 2, dtype=torch.float64), (1, 16, 16))
    with pytest.raises(ValueError, match="map sets .* out of scope"):
        NC(k, (1, 16, 16), sens_maps=np.ones((2, 3, 16, 16)))
    # the row rule is checked on the host, before the GPU check
    with pytest.raises(RuntimeError, match="GPU tensor"):
        op(torch.zeros(3, 1, 16, 16, dtype=torch.complex64))
    # the out-of-scope consumers keep refusing the operator, framed or not
    with pytest.raises(NotImplementedError, match="MAPOptimizer2DTime: NonCartesianSENSE"):
        pkg.map.MAPOptimizer2DTime(None, None, None, Namespace(config=Namespace(data=Namespace(channels=64))), op, None, {})
    with pytest.raises(NotImplementedError, match="MAPModel: NonCartesianSENSE"):
        pkg.map.MAPModel(torch.zeros(1, 1, 1, 64, dtype=torch.complex64), op, None, 0.1, device="cpu")
    with pytest.raises(ValueError, match=r"a 2-D problem takes \(M, 2\)"):
        pkg.engine.build_problem("cpu", 1, H=16, W=16, trajectory=k)


def test_ald2dtime_accepts_framed_only(pkg):
    NC, ALD = pkg.nc.NonCartesianSENSE, pkg.ald.ALD2DTime
    k = pkg.syn.radial_cine_trajectory(3, 4, 16, 16, 16)
    op = NC(k, (1, 16, 16))
    cg = pkg.prox.L2PenaltyCG(op, max_iter=7)
    net_T = Namespace(config=Namespace(data=Namespace(channels=64)), sigmas=None)
    smp = ALD(cg, net_T, torch.ones(2), (1, 3, 1, 16, 16), None, torch.ones(2), {}, None, None, op, device="cpu")
    assert smp.proximal is cg and smp.win_size == 8
    with pytest.raises(ValueError, match=r"holds 3 frames.* T = 4"):
        ALD(cg, net_T, torch.ones(2), (1, 4, 1, 16, 16), None, torch.ones(2), {}, None, None, op, device="cpu")
    with pytest.raises(NotImplementedError, match="no proximal Constrained for NonCartesianSENSE"):
        ALD(pkg.prox.Constrained(op), net_T, torch.ones(2), (1, 3, 1, 16, 16), None, torch.ones(2), {}, None, None, op,
            device="cpu")
    flat = NC(k[0], (1, 16, 16))                                              # one trajectory for all frames: still refused
    with pytest.raises(NotImplementedError, match="ALD2DTime: NonCartesianSENSE"):
        ALD(pkg.prox.L2PenaltyCG(flat), net_T, torch.ones(2), (1, 1, 1, 16, 16), None, torch.ones(2), {}, None, None, flat,
            device="cpu")
    # the 2-D sampler takes the framed operator with L2PenaltyCG as it takes the unframed one
    s2 = pkg.ald.ALDInvSegProximalRealImag(cg, 1.0, "linear", (3, 1, 16, 16), None, torch.ones(2), {}, None, None, op, device="cpu")
    assert s2._check_fast_path({}) is None


def test_ops_refuse_frames_before_the_gpu(pkg):
    ops = pkg.ops
    z = torch.zeros(4, 16, 16)
    c = torch.zeros(4, 16, 16, dtype=torch.complex64)
    k3 = torch.zeros(3, 5, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.nc_sense_cgprox(z, z, None, None, torch.zeros(3, 32, 32), 1.0)
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.ald_nc_sense_cg_step(z, z, z, z, None, None, torch.zeros(3, 32, 32), None)
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.toeplitz_normal(c, torch.zeros(3, 32, 32))
    with pytest.raises(ValueError, match=r"psf \(2, 32, 30\) is neither \[32, 32\] nor \[T, 32, 32\]"):
        ops.toeplitz_normal(c, torch.zeros(2, 32, 30))
    with pytest.raises(ValueError, match=r"neither \[32, 32\] nor \[T, 32, 32\]"):
        ops.nc_sense_cgprox(z, z, None, None, torch.zeros(1, 2, 32, 32), 1.0)
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.ndft_forward(c, k3, torch.zeros(2, 16, 16, dtype=torch.complex64))
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.ndft_forward(c[None], k3)                                          # coil images [n, B, H, W]
    with pytest.raises(ValueError, match=r"B = 4 .* T = 3"):
        ops.ndft_adjoint(torch.zeros(2, 4, 5, dtype=torch.complex64), k3, 16, 16)
    # a batch the frames divide passes the shape checks and stops at the GPU check, as the one-set forms do
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.toeplitz_normal(c, torch.zeros(2, 32, 32))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.toeplitz_psf(torch.zeros(2, 4, 2, dtype=torch.float64), 16, 16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.ndft_forward(c[:3], k3, torch.zeros(2, 16, 16, dtype=torch.complex64))


# ---- helpers and loaders ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,T,spf,ro", [(16, 16, 3, 4, 16), (48, 80, 2, 7, 33), (128, 128, 24, 32, 256)])
def test_radial_cine_trajectory(pkg, H, W, T, spf, ro):
    k = pkg.syn.radial_cine_trajectory(T, spf, ro, H, W)
    assert k.dtype == torch.float64 and tuple(k.shape) == (T, spf * ro, 2) and k.is_contiguous()
    whole = pkg.syn.radial_trajectory(T * spf, ro, H, W).numpy()               # the golden-angle spoke index runs on
    for t in range(T):
        assert np.allclose(k[t].numpy(), whole[t * spf * ro:(t + 1) * spf * ro], rtol=0, atol=1e-12)
    if T * spf <= 32:                                                          # the restatement, where the existing tests compare
        assert np.allclose(k.reshape(-1, 2).numpy(), nh.radial(T * spf, ro, H, W), rtol=0, atol=1e-12)
    if T > 1:
        assert float((k[0] - k[1]).abs().max()) > 0.1                         # the golden angle runs on: no two frames alike
    w = pkg.syn.radial_density(k, H, W)
    assert tuple(w.shape) == (T, spf * ro) and float(w.min()) > 0
    for t in range(T):
        assert torch.equal(w[t], pkg.syn.radial_density(k[t], H, W)) and abs(float(w[t].sum()) - H * W) < 1e-9 * H * W
    pkg.nc.check_trajectory(k, H, W)
    with pytest.raises(ValueError, match="n_frames"):
        pkg.syn.radial_cine_trajectory(0, spf, ro, H, W)


def test_cine_loaders(pkg, tmp_path):
    k = pkg.syn.radial_cine_trajectory(3, 4, 16, 16, 16)
    np.save(tmp_path / "k.npy", k.numpy().astype(np.float32))
    torch.save(k, tmp_path / "k.pt")
    for name in ("k.npy", "k.pt"):
        t = pkg.load.load_trajectory(str(tmp_path / name), cine=True)
        assert t.dtype == torch.float64 and tuple(t.shape) == (3, 64, 2)
    with pytest.raises(ValueError, match=r"\(M, 2\)"):
        pkg.load.load_trajectory(str(tmp_path / "k.npy"))                      # without cine=True: the 2-D form, as before
    np.save(tmp_path / "flat.npy", k[0].numpy())
    with pytest.raises(ValueError, match=r"\(T, M, 2\)"):
        pkg.load.load_trajectory(str(tmp_path / "flat.npy"), cine=True)
    np.save(tmp_path / "y.npy", np.zeros((4, 3, 64), dtype=np.complex128))
    y = pkg.load.load_kspace(str(tmp_path / "y.npy"), noncartesian=True, cine=True)
    assert y.dtype == torch.complex64 and tuple(y.shape) == (4, 3, 64)
    with pytest.raises(ValueError, match=r"\(n_coils, M\)"):
        pkg.load.load_kspace(str(tmp_path / "y.npy"), noncartesian=True)
    np.save(tmp_path / "y2.npy", np.zeros((4, 64), dtype=np.complex64))
    with pytest.raises(ValueError, match=r"\(n_coils, T, M\)"):
        pkg.load.load_kspace(str(tmp_path / "y2.npy"), noncartesian=True, cine=True)


# ---- the cine driver's refusals -------------------------------------------------------------------------------------------------
def _driver(*args):
    r = subprocess.run([sys.executable, DRIVER, *args], capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr)


CG = ["--proximal_type", "L2PenaltyCG"]


@pytest.mark.parametrize("args,msg", [
    (["--trajectory", "radial", "--spokes", "8"], "takes --proximal_type L2PenaltyCG, not L2Penalty"),
    (["--trajectory", "radial", *CG], "--trajectory radial needs --spokes N"),
    (["--trajectory", "radial", "--spokes", "8", "--mask", "m.npy", *CG], "--trajectory does not go with --mask"),
    (["--trajectory", "radial", "--spokes", "8", "--mask_2d", *CG], "--trajectory does not go with --mask_2d"),
    (["--trajectory", "radial", "--spokes", "8", "--estimate_maps", *CG], "--trajectory does not go with --estimate_maps"),
    (["--trajectory", "radial", "--spokes", "8", "--coil_compress", "2", *CG], "--trajectory does not go with --coil_compress"),
    (["--trajectory", "radial", "--spokes", "8", "--image_size", "24", "--image_width", "56", *CG],
     "no non-Cartesian kernel for 24x56"),
    (["--trajectory", "radial", "--spokes", "8", "--kspace", "y.npy", *CG], "--kspace PATH needs --trajectory PATH"),
    (["--spokes", "8"], "--spokes / --readout go with --trajectory radial"),
    (["--trajectory", "nowhere.txt", *CG], "a .npy or .pt file"),
])
def test_driver_refuses_before_the_network(args, msg):
    """each refusal is the process' exit message; none of them reaches the GPU (this test runs without one)"""
    rc, out = _driver("--image_size", "16", *args) if "--image_size" not in args else _driver(*args)
    assert rc != 0 and msg in out, out[-600:]


def test_driver_measured_form_checks(tmp_path):
    k = nh.radial(3 * 4, 16, 16, 16).reshape(3, 64, 2)
    np.save(tmp_path / "k.npy", k)
    np.save(tmp_path / "flat.npy", k[0])
    np.save(tmp_path / "y.npy", np.zeros((4, 3, 63), dtype=np.complex64))
    np.save(tmp_path / "far.npy", k * 3)
    np.save(tmp_path / "maps.npy", np.ones((5, 16, 16), dtype=np.complex64))
    base = ["--image_size", "16", *CG]
    rc, out = _driver(*base, "--trajectory", str(tmp_path / "flat.npy"))
    assert rc != 0 and "(T, M, 2)" in out
    rc, out = _driver(*base, "--trajectory", str(tmp_path / "far.npy"))
    assert rc != 0 and "frame 0 of the trajectory leaves [-N/2, N/2]" in out
    rc, out = _driver(*base, "--trajectory", str(tmp_path / "k.npy"), "--kspace", str(tmp_path / "y.npy"))
    assert rc != 0 and "needs --sens_maps PATH" in out
    rc, out = _driver(*base, "--trajectory", str(tmp_path / "k.npy"), "--kspace", str(tmp_path / "y.npy"),
                      "--sens_maps", str(tmp_path / "maps.npy"))
    assert rc != 0 and "(n_coils, 3, 64) expected" in out
    np.save(tmp_path / "y.npy", np.zeros((4, 3, 64), dtype=np.complex64))
    rc, out = _driver(*base, "--trajectory", str(tmp_path / "k.npy"), "--kspace", str(tmp_path / "y.npy"),
                      "--sens_maps", str(tmp_path / "maps.npy"))
    assert rc != 0 and "(4, 16, 16) expected" in out
