"""Time-averaged calibration of 2D+time k-space, host side: the composite calibration region and the union mask against
the float64 helper (tests/cine_helpers.py), the C entry's argument checks that need no GPU, the refusals of the Python
front ends before any launch, load_kspace(cine=True), and that both cine drivers refuse bad arguments before anything is
built.  (The refusals of ops.kspace_time_average that need a GPU tensor to be reached -- dtype, strides, rank, mask -- are
in test_cine_calib_gpu.py: the device check comes first, as in ops._csm_measurement.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cine_helpers as cineh
import csm_helpers as csmh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CINE_DRIVERS = ["cine_SENSE_real_img_2d_time.py", "cine_SENSE_real_img_2d_time_MAP.py"]


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, ops, synthetic
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
    return Namespace(lib=_lib, ops=ops, load=load_data, uf=uf, syn=synthetic)


def cine_mask(pkg, W, seed=0):
    """the cine drivers' generated T = 24 line mask, (24, 1, 1, W)"""
    return pkg.uf.RandomUndersamplingFourier(8, 0.05, (1, W, W), seed, mask_T=24).mask


# ---- calibration_region ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,aw", [(64, 5), (128, 10)])
def test_composite_region_of_the_generated_cine_mask(pkg, W, aw):
    """the frames share only the column W // 2; their union is fully sampled on 2 aw + 1 columns (numpy restatement of
    generate_mask, seed 0: aw = 5 at W = 64, 10 at W = 128)"""
    H = W
    mask = cine_mask(pkg, W)
    assert tuple(mask.shape) == (24, 1, 1, W)
    with pytest.raises(ValueError, match=r"calibration region.*25 x 1 samples.*composite=True"):
        pkg.uf.calibration_region(mask, H, W)
    ah = min(H // 2, H - 1 - H // 2, 12)
    assert pkg.uf.calibration_region(mask, H, W, composite=True) == (ah, aw)
    assert pkg.uf.calibration_region(mask, H, W, calib_max=7, composite=True) == (7, min(aw, 7))
    assert pkg.uf.calibration_region(mask, 48, W, calib_max=30, composite=True) == (23, aw)        # a line mask: ah from H alone
    # the helper on the union agrees
    assert csmh.calibration_region(cineh.union_mask(mask, H, W), H, W) == (ah, aw)
    assert pkg.uf.calibration_region(pkg.uf.composite_mask(mask, H, W), H, W) == (ah, aw)


def test_composite_region_of_one_plane_is_the_plain_region(pkg):
    H, W = 40, 48
    for mask in (pkg.syn.vd_mask_2d(H, W, 4, center_frac=0.2, seed=3), torch.ones(W), torch.ones(1, 1, H, W)):
        assert pkg.uf.calibration_region(mask, H, W, composite=True) == pkg.uf.calibration_region(mask, H, W)
    line = torch.zeros(W, dtype=torch.bool)
    line[::3] = True
    line[W // 2 - 4:W // 2 + 5] = True
    assert pkg.uf.calibration_region(line, H, W, composite=True) == pkg.uf.calibration_region(line, H, W) == (12, 4)


def test_composite_region_of_2d_frames(pkg):
    """per-frame 2-D masks whose union holds a 7 x 9 box that no frame holds"""
    H, W, T = 32, 32, 4
    m = torch.zeros(T, 1, H, W, dtype=torch.bool)
    for t in range(T):
        m[t, 0, H // 2 - 3:H // 2 + 4, W // 2 - 4 + t:W // 2 + 5:T] = True
        m[t, 0, H // 2, W // 2] = True
    assert pkg.uf.calibration_region(m, H, W, composite=True) == (3, 4)
    assert csmh.calibration_region(cineh.union_mask(m, H, W), H, W) == (3, 4)
    with pytest.raises(ValueError, match="composite=True"):
        pkg.uf.calibration_region(m, H, W)


def test_composite_region_still_refuses_a_small_union(pkg):
    H = W = 32
    m = torch.zeros(3, 1, 1, W, dtype=torch.bool)
    m[0, ..., W // 2], m[1, ..., W // 2 - 1], m[2, ..., W // 2 + 1] = True, True, True            # union: 3 columns, aw = 1
    with pytest.raises(ValueError, match=r"calibration region.*25 x 3 samples") as e:
        pkg.uf.calibration_region(m, H, W, composite=True)
    assert "composite=True" not in str(e.value)
    with pytest.raises(ValueError, match="calibration region") as e:                            # nor is a hint given without a use
        pkg.uf.calibration_region(m, H, W)
    assert "composite=True" not in str(e.value)
    with pytest.raises(ValueError, match="not sampled in any frame"):
        pkg.uf.calibration_region(torch.zeros(3, 1, 1, W), H, W, composite=True)
    with pytest.raises(ValueError):
        pkg.uf.calibration_region(cine_mask(pkg, 64), 64, 64, calib_max=-1, composite=True)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int64, torch.float32, torch.float64])
def test_composite_mask(pkg, dtype):
    H, W = 12, 20
    rng = np.random.default_rng(0)
    line = torch.from_numpy(rng.random((5, 1, 1, W)) < 0.3)
    full = torch.from_numpy(rng.random((4, 1, H, W)) < 0.2)
    for m, shape in ((line, (W,)), (full, (H, W)), (line[0, 0, 0], (W,)), (full[0, 0], (H, W))):
        scaled = (m.to(torch.float64) * 2.5).to(dtype) if dtype.is_floating_point else m.to(dtype)
        got = pkg.uf.composite_mask(scaled, H, W)
        assert got.dtype == torch.bool and tuple(got.shape) == shape and not got.is_cuda
        want = cineh.union_mask(m, H, W)
        assert np.array_equal(got.numpy(), want if len(shape) == 2 else want[0])
    with pytest.raises(TypeError):
        pkg.uf.composite_mask(torch.zeros(W, dtype=torch.complex64), H, W)
    with pytest.raises(ValueError):
        pkg.uf.composite_mask(torch.zeros(W + 1), H, W)


def test_helper_composite():
    """the helper itself: the plane rule, the count, zeros, and that unsampled input is never touched"""
    rng = np.random.default_rng(1)
    n, B, T, H, W = 2, 2, 3, 4, 5
    y = rng.standard_normal((n, B, T, H, W)) + 1j * rng.standard_normal((n, B, T, H, W))
    mask = rng.random((2, 1, H, W)) < 0.5
    ybar, count = cineh.composite(y, mask)
    m = cineh.planes(mask, H, W)
    for b in range(B):
        for p in np.ndindex(H, W):
            ts = [t for t in range(T) if m[(b * T + t) % 2][p]]
            assert count[b][p] == len(ts)
            want = sum(y[:, b, t][(slice(None),) + p] for t in ts) / len(ts) if ts else np.zeros(n)
            assert np.abs(ybar[:, b][(slice(None),) + p] - want).max() <= 1e-15
    poisoned = np.where(cineh.frame_planes(mask, B, T, H, W)[None], y, np.nan)
    assert np.array_equal(cineh.composite(poisoned, mask)[0], ybar)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declaration_and_answers_without_a_gpu(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    i, P = pkg.lib.c_int, pkg.lib.P
    m = re.search(r"\b(\w+)\s+ipdm_kspace_tavg_c64\s*\(([^;]*)\)\s*;", header)
    assert m, "ipdm_kspace_tavg_c64 is not declared in include/ipdm.h"
    args = [P, P, i, P, P, i, i, i, i, i, P]
    assert m.group(1) == "int" and len(m.group(2).split(",")) == len(args)
    fn = pkg.lib.lib.ipdm_kspace_tavg_c64
    assert pkg.lib.SIGNATURES["ipdm_kspace_tavg_c64"] == args and fn.argtypes == args and fn.restype is i
    assert "#define IPDM_ABI_VERSION 4" in header and pkg.lib.lib.ipdm_abi_version() == 4   # an entry point added, none changed
    EINVAL, EUNSUP = pkg.lib.IPDM_EINVAL, pkg.lib.IPDM_EUNSUPPORTED
    #           y    mask  mask_t ybar count B  T  n  H  W  stream
    assert fn(None, None, 1, None, None, 1, 0, 1, 4, 4, None) == EINVAL                      # T = 0
    assert fn(None, None, 1, None, None, 1, 2, 1, 0, 4, None) == EINVAL                      # H = 0
    assert fn(None, None, 1, None, None, 1, 2, 1, 4, 0, None) == EINVAL
    assert fn(None, None, 1, None, None, 1, 2, 0, 4, 4, None) == EINVAL
    assert fn(None, None, 1, None, None, -1, 2, 1, 4, 4, None) == EINVAL
    assert fn(None, None, 0, None, None, 1, 2, 1, 4, 4, None) == EINVAL                      # mask_t = 0
    assert fn(None, None, 1, None, None, 1, 4097, 1, 4, 4, None) == EUNSUP
    assert fn(None, None, -3, None, None, 1, 4097, 1, 4, 4, None) == EUNSUP
    assert fn(None, None, 1, None, None, 0, 2, 1, 4, 4, None) == 0                           # an empty batch: nothing launched
    assert fn(None, None, -2, None, None, 0, 4096, 64, 1, 1, None) == 0
    assert fn(None, None, 1, None, None, 1, 2, 1, 4, 4, None) == EINVAL                      # the sizes are fine, the tensors NULL


# ---- Python front ends ------------------------------------------------------------------------------------------------------
def test_ops_refuses_a_cpu_tensor(pkg):
    y = torch.zeros(2, 3, 4, 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pkg.ops.kspace_time_average(y, torch.ones(1, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pkg.ops.kspace_time_average(y.numpy(), torch.ones(1, 4, dtype=torch.uint8))


def test_sense_front_ends_refuse_before_the_gpu(pkg):
    """nothing here may reach a kernel: on a machine without a GPU a launch, or a .to("cuda"), would raise something else"""
    S = pkg.uf.SENSE
    T, H, W = 24, 64, 64
    mask = cine_mask(pkg, W)
    y = torch.zeros(4, T, H, W, dtype=torch.complex64)
    for fn in (S.time_average, S.from_cine_measurement):
        with pytest.raises(ValueError, match="planes"):
            fn(y, mask[:5])                                                  # 5 planes for 24 frames
        with pytest.raises(ValueError, match="planes"):
            fn(y[:, :12], mask)
        with pytest.raises(ValueError, match="planes"):
            fn(y, torch.ones(5, H, W))                                       # (T', H, W) -> (T', 1, H, W)
        with pytest.raises(TypeError):
            fn(y.real, mask)
        with pytest.raises(TypeError):
            fn([1, 2], mask)
        with pytest.raises(TypeError):
            fn(y, [True] * W)
        with pytest.raises(ValueError):
            fn(y[0, 0], mask)                                                # (H, W)
        with pytest.raises(ValueError):
            fn(y, mask[..., :W - 1])
    with pytest.raises(ValueError, match="n_virtual"):
        S.from_cine_measurement(y, mask, noise_cov=np.eye(4))
    for nv in (0, 5, 2.5):
        with pytest.raises(ValueError, match="n_virtual"):
            S.from_cine_measurement(y, mask, n_virtual=nv)
    with pytest.raises(pkg.lib.IpdmUnsupported):
        S.from_cine_measurement(torch.zeros(65, T, H, W, dtype=torch.complex64), mask, n_virtual=8)
    with pytest.raises(ValueError, match="positive definite"):
        S.from_cine_measurement(y, mask, n_virtual=2, noise_cov=-np.eye(4))
    with pytest.raises(ValueError, match="shape"):
        S.from_cine_measurement(y, mask, n_virtual=2, noise_cov=np.eye(3))
    with pytest.raises(ValueError, match="calibration region"):
        S.from_cine_measurement(y, torch.tensor([True, False] * (W // 2)))   # every other line: no 5 x 5 centre
    with pytest.raises(ValueError, match="calibration region"):
        S.from_cine_measurement(y, mask, calib_max=1)


def test_load_kspace_cine(pkg, tmp_path):
    rng = np.random.default_rng(0)
    y = (rng.standard_normal((3, 5, 8, 8)) + 1j * rng.standard_normal((3, 5, 8, 8))).astype(np.complex64)
    torch.save(torch.from_numpy(y), tmp_path / "y.pt")
    np.save(tmp_path / "y.npy", y.astype(np.complex128))
    np.save(tmp_path / "single.npy", y[:, 0])
    np.save(tmp_path / "real.npy", y.real)
    for name in ("y.pt", "y.npy"):
        got = pkg.load.load_kspace(str(tmp_path / name), cine=True)
        assert got.dtype == torch.complex64 and tuple(got.shape) == (3, 5, 8, 8) and np.array_equal(got.numpy(), y)
    with pytest.raises(ValueError, match=r"\(n_coils, T, H, W\)"):
        pkg.load.load_kspace(str(tmp_path / "single.npy"), cine=True)        # a 3-D file
    with pytest.raises(ValueError, match="complex"):
        pkg.load.load_kspace(str(tmp_path / "real.npy"), cine=True)
    # the default is unchanged
    assert tuple(pkg.load.load_kspace(str(tmp_path / "single.npy")).shape) == (3, 8, 8)
    with pytest.raises(ValueError, match=r"\(n_coils, H, W\)"):
        pkg.load.load_kspace(str(tmp_path / "y.npy"))


# ---- drivers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script", CINE_DRIVERS)
def test_cine_drivers_refuse_before_anything_is_built(script, tmp_path):
    size = 64 if script == CINE_DRIVERS[0] else 128                          # the MAP driver runs at its networks' size
    rng = np.random.default_rng(0)
    y = torch.from_numpy((rng.standard_normal((4, 24, size, size)) + 0j).astype(np.complex64))
    torch.save(y, tmp_path / "kspace.pt")
    torch.save(y[:, 0].clone(), tmp_path / "single.pt")
    torch.save(torch.tensor([True, False] * (size // 2)), tmp_path / "alternate.pt")
    torch.save(torch.ones(5, 1, 1, size, dtype=torch.bool), tmp_path / "five.pt")
    np.save(tmp_path / "psi.npy", -np.eye(4))
    p = lambda name: str(tmp_path / name)                                    # noqa: E731
    base = [sys.executable, os.path.join(REPO, "scripts", script), "--save_dir", p("out")]
    if script == CINE_DRIVERS[0]:
        base += ["--image_size", "64", "--n_levels", "1"]
    cases = [(["--kspace", p("kspace.pt")], "--kspace PATH needs --mask PATH"),
             (["--kspace", p("single.pt"), "--mask", p("five.pt"), "--estimate_maps"], "(n_coils, T, H, W)"),
             (["--kspace", p("kspace.pt"), "--mask", p("five.pt"), "--estimate_maps"], "planes"),
             (["--kspace", p("kspace.pt"), "--mask", p("alternate.pt"), "--estimate_maps"], "calibration region"),
             (["--estimate_maps", "--calib_max", "1"], "calibration region"),
             (["--noise_cov", p("psi.npy")], "--noise_cov PATH goes with --coil_compress N"),
             (["--estimate_maps", "--coil_compress", "5"], "n_virtual")]
    for extra, word in cases:
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr[-2000:])
        assert "Traceback" not in r.stderr, (extra, r.stderr[-2000:])
        assert not (tmp_path / "out").exists()
