"""Coil-map estimation, host side: the calibration box found in a sampling mask (calibration_region), the window, the
C ABI's declarations and its GPU-free answers, load_kspace, and the driver's refusal of a mask without a usable centre
before anything is built or written."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import csm_helpers as csmh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, ops, synthetic
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
    return Namespace(lib=_lib, ops=ops, syn=synthetic, load=load_data, uf=uf)


def line_mask(W, centre=17, every=3):
    """bool (W,): every `every`-th line plus `centre` lines around W // 2"""
    m = torch.zeros(W, dtype=torch.bool)
    m[::every] = True
    m[W // 2 - centre // 2:W // 2 + centre // 2 + 1] = True
    return m


# ---- calibration_region -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (16, 64), (128, 80), (9, 65)])
def test_region_of_a_line_mask(pkg, H, W):
    m = line_mask(W)
    want = (min(H // 2, H - 1 - H // 2, 12), 8)
    for shaped in (m, m[None], m[None, None], m[None, None, None], m.float(), m.numpy().astype(np.int32)):
        assert pkg.uf.calibration_region(shaped, H, W) == want
    assert csmh.calibration_region(m, H, W) == want


def test_region_of_a_2d_mask(pkg):
    H = W = 64
    m = pkg.syn.vd_mask_2d(H, W, 4, center_frac=0.3, seed=1)                 # a 19 x 19 block: rows and columns 23 .. 41
    ah, aw = pkg.uf.calibration_region(m, H, W)
    assert (ah, aw) == csmh.calibration_region(m, H, W) and 9 <= ah <= 12 and 9 <= aw <= 12
    assert m[0, 0, H // 2 - ah:H // 2 + ah + 1, W // 2 - aw:W // 2 + aw + 1].all()
    assert pkg.uf.calibration_region(m[0, 0], H, W) == (ah, aw)
    # an off-centre block: the box is symmetric about DC, so the shorter side decides
    m2 = torch.zeros(H, W, dtype=torch.bool)
    m2[H // 2 - 3:H // 2 + 8, W // 2 - 9:W // 2 + 5] = True
    assert pkg.uf.calibration_region(m2, H, W) == (3, 4)


def test_region_is_the_intersection_of_the_frames(pkg):
    H, W = 32, 64
    frames = torch.zeros(2, 1, 1, W, dtype=torch.bool)
    frames[0, ..., W // 2 - 6:W // 2 + 7] = True
    frames[1, ..., W // 2 - 4:W // 2 + 10] = True
    assert pkg.uf.calibration_region(frames[:1], H, W) == (12, 6)
    assert pkg.uf.calibration_region(frames[1:], H, W) == (12, 4)
    assert pkg.uf.calibration_region(frames, H, W) == (12, 4) == csmh.calibration_region(frames, H, W)
    planes = torch.zeros(2, 1, H, W, dtype=torch.bool)
    planes[0, 0, H // 2 - 5:H // 2 + 6, W // 2 - 7:W // 2 + 8] = True
    planes[1, 0, H // 2 - 3:H // 2 + 9, W // 2 - 9:W // 2 + 6] = True
    assert pkg.uf.calibration_region(planes, H, W) == (3, 5) == csmh.calibration_region(planes, H, W)


def test_region_calib_max_caps_both_sides(pkg):
    full = torch.ones(40, 48, dtype=torch.bool)
    assert pkg.uf.calibration_region(full, 40, 48) == (12, 12)
    assert pkg.uf.calibration_region(full, 40, 48, calib_max=5) == (5, 5)
    assert pkg.uf.calibration_region(full, 40, 48, calib_max=30) == (19, 23)   # min(N // 2, N - 1 - N // 2)
    assert pkg.uf.calibration_region(torch.ones(16, 9), 16, 9, calib_max=30) == (7, 4)
    with pytest.raises(ValueError):
        pkg.uf.calibration_region(full, 40, 48, calib_max=1)
    with pytest.raises(ValueError):
        pkg.uf.calibration_region(full, 40, 48, calib_max=-1)


def _boxes(H, W, boxes):
    m = torch.zeros(H, W, dtype=torch.bool)
    for ah, aw in boxes:
        m[H // 2 - ah:H // 2 + ah + 1, W // 2 - aw:W // 2 + aw + 1] = True
    return m


def test_region_tie_rule(pkg):
    """four fully sampled boxes of 45 samples: the smaller |ah - aw| wins, then the larger aw"""
    H = W = 32
    m = _boxes(H, W, [(1, 7), (7, 1), (2, 4), (4, 2)])
    assert pkg.uf.calibration_region(m, H, W) == (2, 4) == csmh.calibration_region(m, H, W)
    assert pkg.uf.calibration_region(m.T.contiguous(), H, W) == (2, 4)
    # the largest area wins before the tie rule is asked: 3 x 17 = 51 samples beat the 5 x 9, and that box is refused
    with pytest.raises(ValueError, match="3 x 17"):
        pkg.uf.calibration_region(_boxes(H, W, [(1, 8), (2, 4)]), H, W)


def test_region_refuses_a_centre_too_small(pkg):
    op = pkg.uf.SENSE("exp", 4, 40, 0.04, (1, 128, 128), seed=0)             # the default mask: centre lines 63 and 64 -> aw = 0
    with pytest.raises(ValueError, match=r"calibration region.*25 x \d samples"):
        pkg.uf.calibration_region(op.random_under_fourier.mask, 128, 128)
    with pytest.raises(ValueError, match="calibration region"):
        pkg.uf.calibration_region(pkg.syn.vd_mask_2d(64, 64, 8, center_frac=0.04), 64, 64)
    with pytest.raises(ValueError, match="not sampled"):
        pkg.uf.calibration_region(torch.zeros(32), 32, 32)
    with pytest.raises(ValueError):                                          # _mask_u8's shape rules
        pkg.uf.calibration_region(torch.ones(31), 32, 32)


# ---- window -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,a", [(16, 7), (17, 8), (64, 8), (9, 2), (8, 3)])
def test_window_formula(N, a):
    """the helper's window, which the GPU window is held to through the calibration images (test_csm_gpu.py)"""
    w = csmh.window(N, a)
    want = np.zeros(N)
    for k in range(N):
        if abs(k - N // 2) <= a:
            want[k] = 0.5 + 0.5 * np.cos(np.pi * (k - N // 2) / (a + 1))
    assert np.abs(w - want).max() < 1e-15
    assert w[N // 2] == 1.0 and w[N // 2 - a] > 0 and np.allclose(w[N // 2 - a], w[N // 2 + a], atol=1e-15)
    assert not w[:N // 2 - a].any() and not w[N // 2 + a + 1:].any()
    assert csmh.window(N, a, np.float32).dtype == np.float32


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_abi_declarations(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    i = pkg.lib.c_int
    P = pkg.lib.P
    want = {"ipdm_csm_workspace_bytes": ("size_t", [i] * 4),
            "ipdm_csm_supported": ("int", [i] * 4),
            "ipdm_csm_calib_images_c64": ("int", [P, i, i, P, i, i, i, i, P]),
            "ipdm_csm_walsh_c64": ("int", [P, i, i, i, i, pkg.lib.c_float, P, P, P, P, i, i, i, i, P])}
    for name, (ret, args) in want.items():
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ipdm.h"
        params = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        assert m.group(1) == ret and len(params.split(",")) == len(args)
        assert pkg.lib.SIGNATURES[name] == args and hasattr(pkg.lib.lib, name)
    assert pkg.lib.lib.ipdm_csm_workspace_bytes.restype is __import__("ctypes").c_size_t
    assert "#define IPDM_ABI_VERSION 4" in header and pkg.lib.lib.ipdm_abi_version() == 4


def test_abi_answers_without_a_gpu(pkg):
    lib = pkg.lib.lib
    for n, want in ((1, 1), (32, 1), (33, 0), (0, 0)):
        assert lib.ipdm_csm_supported(n, 2, 32, 32) == want
        assert pkg.ops.csm_supported(n, 2, 32, 32) == bool(want)
    for r, want in ((0, 0), (1, 1), (4, 1), (5, 0)):
        assert lib.ipdm_csm_supported(4, r, 32, 32) == want
    for (H, W), want in (((24, 32), 0), ((32, 24), 0), ((48, 80), 1), ((144, 128), 1), ((8, 8), 1), ((2048, 16), 0)):
        assert lib.ipdm_csm_supported(4, 2, H, W) == want
        assert want == (pkg.ops.kspace_size_class(H, W) != pkg.ops.KSPACE_NONE and max(H, W) <= 1024)
    # calibration images (8 bytes per coil and pixel) + the RSS plane (4 bytes per pixel)
    assert lib.ipdm_csm_workspace_bytes(3, 5, 48, 80) == 3 * 48 * 80 * (5 * 8 + 4)
    assert lib.ipdm_csm_workspace_bytes(1, 32, 16, 16) == 16 * 16 * (32 * 8 + 4)
    for args in ((1, 33, 16, 16), (1, 4, 24, 32), (0, 4, 16, 16), (1, 0, 16, 16)):
        assert lib.ipdm_csm_workspace_bytes(*args) == 0


# ---- load_kspace --------------------------------------------------------------------------------------------------------
def test_load_kspace(pkg, tmp_path):
    y = (torch.randn(3, 8, 16, dtype=torch.float64) + 1j * torch.randn(3, 8, 16, dtype=torch.float64))
    torch.save(y, tmp_path / "y.pt")
    np.save(tmp_path / "y.npy", y.numpy())
    for name in ("y.pt", "y.npy"):
        got = pkg.load.load_kspace(str(tmp_path / name))
        assert got.dtype == torch.complex64 and tuple(got.shape) == (3, 8, 16) and torch.equal(got, y.to(torch.complex64))
    torch.save(y[0], tmp_path / "rank2.pt")
    torch.save(y[:, None], tmp_path / "rank4.pt")
    np.save(tmp_path / "real.npy", y.real.numpy())
    torch.save({"y": y}, tmp_path / "dict.pt")
    np.save(tmp_path / "y.dat.npy", y.numpy())
    os.rename(tmp_path / "y.dat.npy", tmp_path / "y.dat")
    for name in ("rank2.pt", "rank4.pt", "real.npy", "dict.pt", "y.dat"):
        with pytest.raises(ValueError):
            pkg.load.load_kspace(str(tmp_path / name))


# ---- driver -------------------------------------------------------------------------------------------------------------
def test_driver_refuses_the_default_mask_before_anything_is_written(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--estimate_maps",
                        "--image_size", "64", "--n_levels", "1", "--save_dir", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode != 0
    assert "calibration region" in r.stderr and "needs at least 5 x 5" in r.stderr
    assert not out.exists()
