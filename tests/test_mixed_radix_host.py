"""Image sizes of the k-space kernels, host side: `ops.kspace_size_class` (the C ABI's `ipdm_kspace_size_class`) and the
workspace-size functions at sides 2^a 3^b 5^c.  A side is served when it is a power of two from 4, or a multiple of 16 of
that form between 16 and 2048; H*W <= 16384 takes the whole-image LDS kernels (class 1), larger pairs the row / column
strips (class 2), everything else has no kernel (class 0).  Loads the library; needs no GPU."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, ops
    return Namespace(lib=_lib, ops=ops)


@pytest.mark.parametrize("H,W,want", [
    (48, 48, 1), (16, 48, 1), (48, 80, 1), (80, 48, 1), (96, 160, 1), (128, 128, 1),
    (80, 240, 2), (240, 80, 2), (144, 160, 2), (48, 512, 2), (256, 256, 2),
    (24, 32, 0), (40, 48, 0), (48, 50, 0), (112, 48, 0), (49, 48, 0), (2064, 16, 0)])
def test_size_class(pkg, H, W, want):
    assert pkg.ops.kspace_size_class(H, W) == want
    assert pkg.lib.lib.ipdm_kspace_size_class(H, W) == want


def test_size_class_edges(pkg):
    f = pkg.ops.kspace_size_class
    assert (pkg.ops.KSPACE_NONE, pkg.ops.KSPACE_LDS, pkg.ops.KSPACE_STRIPS) == (0, 1, 2)
    # powers of two are served from 4, as before; the other sides from 16
    assert f(4, 4) == 1 and f(8, 16) == 1 and f(4, 4096) == 1 and f(2, 8) == 0 and f(12, 16) == 0
    assert f(2048, 2048) == 2 and f(4096, 8) == 0 and f(4096, 4096) == 0
    # the largest sides with a factor 3 or 5, and the first past the limit
    assert f(1920, 2000) == 2 and f(1536, 16) == 2 and f(2048, 1536) == 2 and f(2160, 16) == 0 and f(2400, 16) == 0
    assert f(960, 16) == 1 and f(16, 1024) == 1 and f(16, 1040) == 0                      # 1040 = 16 * 5 * 13
    # 96x160 = 15360 pixels is the fullest LDS image with a factor 3 or 5; a multiple of 8 that is no multiple of 16 is no size
    assert f(96, 160) == 1 and f(120, 128) == 0 and f(0, 16) == 0 and f(-16, 16) == 0
    # a power-of-two side of 4 or 8 beside a mixed side: served, except the one pair past the radix-3 / 5 stages' 15360 elements
    assert f(8, 1920) == 1 and f(1920, 8) == 1 and f(4, 2000) == 1 and f(8, 48) == 1 and f(8, 2000) == 0 and f(2000, 8) == 0
    assert "multiple of 16" in pkg.ops.KSPACE_SIZE_RULE


def test_real_matrix_sizes_are_served(pkg):
    for n in (96, 144, 160, 192, 240, 288, 320, 384):
        assert pkg.ops.kspace_size_class(n, n) == (1 if n * n <= 16384 else 2), n


def test_workspace_bytes(pkg):
    lib = pkg.lib.lib
    assert lib.ipdm_sense_workspace_bytes(2, 3, 48, 80) == 2 * 3 * 48 * 80 * 8
    assert lib.ipdm_sense_workspace_bytes(2, 3, 80, 240) == 2 * 3 * 80 * 240 * 8 > 0
    assert lib.ipdm_sense_cg_workspace_bytes(2, 3, 48, 80) == (3 + 4) * 2 * 48 * 80 * 8 + 2 * 16 > 0
    assert lib.ipdm_sense_cg_workspace_bytes(2, 3, 80, 240) == (3 + 4) * 2 * 80 * 240 * 8 + 2 * 16 > 0
    assert lib.ipdm_fft2c_workspace_bytes(2, 48, 80) == 0                                 # served: no DFT fallback
    assert lib.ipdm_fft2c_workspace_bytes(2, 80, 240) == 0
    # sizes without a kernel keep their answers: only fft2c falls back (and asks for its scratch)
    assert lib.ipdm_sense_workspace_bytes(2, 3, 24, 32) == 0 and lib.ipdm_sense_cg_workspace_bytes(2, 3, 40, 48) == 0
    assert lib.ipdm_fft2c_workspace_bytes(2, 40, 48) == 2 * 40 * 48 * 8


def test_c_abi_declares_the_size_class(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    assert re.search(r"\bint\s+ipdm_kspace_size_class\s*\(\s*int\s+H\s*,\s*int\s+W\s*\)\s*;", header)
    for name, val in (("IPDM_KSPACE_NONE", 0), ("IPDM_KSPACE_LDS", 1), ("IPDM_KSPACE_STRIPS", 2)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", header)
    assert pkg.lib.SIGNATURES["ipdm_kspace_size_class"] == [pkg.lib.c_int, pkg.lib.c_int]
    assert pkg.lib.lib.ipdm_abi_version() == 4                                            # an entry point added, none changed


@pytest.mark.parametrize("script", ["acdc_SENSE_real_img.py", "cine_SENSE_real_img_2d_time.py"])
def test_drivers_refuse_a_size_without_a_kernel(script, tmp_path):
    """both SENSE drivers name the rule and stop before anything is allocated (no GPU is touched, nothing is written)"""
    import subprocess
    import sys
    for size in (["--image_size", "40", "--image_width", "48"], ["--image_size", "24"], ["--image_size", "48", "--image_width", "50"]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", script)] + size + ["--save_dir", str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=120, cwd=REPO)
        assert r.returncode != 0 and "multiple of 16" in r.stderr and "no k-space kernel" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(str(tmp_path / "out"))
