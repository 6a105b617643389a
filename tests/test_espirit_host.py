"""Host-side tests of the ESPIRiT estimator: the float64 helper (tests/espirit_helpers.py) against the true maps, the
helper's own mutations, the coverage answers of the C ABI, its declarations, and the refusals that happen on the host."""
import os
import re

import numpy as np
import pytest
import torch

import csm_helpers as csmh
import espirit_helpers as eh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W, n, k, ah, aw, seed, sv_thresh): the margin to the rank threshold is 11 % and 10 %
TRUTH_CASES = [(32, 32, 4, 4, 8, 8, 7, 0.0225), (32, 32, 4, 4, 8, 8, 1, 0.02)]
TRUTH_BOUND = 0.017                                                          # 2 x the larger median measured below


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, ops, synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier
    return Namespace(lib=_lib, ops=ops, syn=synthetic, uf=undersampling_fourier)


_TRUTH = {}


def median_error(case, **mut):
    """median over kept pixels inside the object of the 2-norm over the coils of (helper map - true unit-RSS, coil-0-gauged
    map); the data are computed once per case"""
    H, W, n, k, ah, aw, seed, sv = case
    if case not in _TRUTH:
        y, maps, objs = csmh.make_data(H, W, n, B=1, seed=seed, scales=(1.0,))
        obj = np.abs(objs[0].numpy())
        _TRUTH[case] = (y.to(torch.complex64).numpy()[:, 0], eh.true_maps(maps.numpy()), obj > 0.05 * obj.max())
    y, truth, support = _TRUTH[case]
    out = eh.estimate(y, ah, aw, k, sv, **mut)
    sel = (out["eigval"] > 0.8) & support
    assert out["margin"] >= 0.05 and sel.sum() >= 200
    err = np.sqrt((np.abs(out["maps"] - truth) ** 2).sum(0))
    return float(np.median(err[sel]))


@pytest.mark.parametrize("case", TRUTH_CASES)
def test_helper_recovers_the_true_maps(case):
    """synthetic.complex_coil_maps times phantom_image, 4 coils at 32 x 32, k = 4, a 17 x 17 box: median error 0.0071 (seed 7)
    and 0.0085 (seed 1) of unit-norm maps, measured in float64 on the CPU; asserted with a 2 x margin"""
    err = median_error(case)
    print(f"helper against the truth {case}: median error {err:.4f}")
    assert err <= TRUTH_BOUND


@pytest.mark.parametrize("mut", [dict(exp_sign=+1), dict(conj=False)])
def test_the_truth_check_catches_both_mutations(mut):
    """the other exponent sign and the missing conjugate give errors of order 1 (measured: 0.81 and 1.42)"""
    err = median_error(TRUTH_CASES[0], **mut)
    print(f"mutation {mut}: median error {err:.4f}")
    assert err > 20 * TRUTH_BOUND


def test_helper_properties():
    median_error(TRUTH_CASES[0])                                             # (cached) builds the data
    y = _TRUTH[TRUTH_CASES[0]][0]
    out = eh.estimate(y, 8, 8, 4, 0.0225)
    Gm = out["gram"]
    assert np.abs(Gm - Gm.conj().T).max() <= 1e-12 * np.abs(Gm).max() and out["n_patches"] == 14 * 14
    K = out["K"]                                                             # K[c'][c][-d] = conj(K[c][c'][d])
    assert np.abs(K - K.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1].conj()).max() <= 1e-12
    assert out["lam1"].max() <= 1 + 1e-9 and out["lam2"].min() >= -1e-9       # G(x) has its eigenvalues in [0, 1]
    kept = out["eigval"] > 0.8
    m = out["maps"]
    assert np.abs(np.sqrt((np.abs(m) ** 2).sum(0))[kept] - 1).max() <= 1e-12 and not m[:, ~kept].any()
    assert np.abs(m[0].imag).max() <= 1e-12 and m[0].real.min() >= 0
    clear = kept & (out["lam2"] < 0.7 * out["lam1"])                          # (lam2 / lam1)^62 < 3e-10 there
    assert clear.sum() > 100 and np.abs(out["eigval"] - out["lam1"])[clear].max() <= 1e-6


def test_supported_grid(pkg):
    sup = pkg.ops.espirit_supported
    for n, want in ((0, False), (1, True), (16, True), (17, False)):
        assert sup(n, 3, 64, 64) is want
    for k, want in ((2, False), (3, True), (8, True), (9, False)):
        assert sup(1, k, 64, 64) is want
    assert sup(12, 6, 64, 64) and not sup(13, 6, 64, 64)                      # n k^2 = 432 is the cap (lowered from 576: the
    assert sup(16, 5, 64, 64) and not sup(16, 6, 64, 64)                      # Jacobi stage took 2.8 s there)
    assert not sup(16, 7, 64, 64) and sup(6, 8, 64, 64) and not sup(7, 8, 64, 64)
    assert sup(4, 6, 24, 56) and sup(4, 6, 1024, 1000) and not sup(4, 6, 1025, 64) and not sup(4, 6, 64, 0)
    lib = pkg.lib.lib
    assert lib.ipdm_espirit_workspace_bytes(3, 12, 6) == 3 * 2 * 432 * 432 * 16
    assert lib.ipdm_espirit_workspace_bytes(1, 16, 6) == 0 and lib.ipdm_espirit_workspace_bytes(0, 4, 4) == 0
    assert lib.ipdm_espirit_workspace_bytes(65536, 4, 4) == 0


def test_abi_declarations(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    want = {"ipdm_espirit_supported": ("int", 4), "ipdm_espirit_workspace_bytes": ("size_t", 3), "ipdm_espirit_gram_c64": ("int", 10),
            "ipdm_espirit_kernels_c64": ("int", 16), "ipdm_espirit_pixel_c64": ("int", 12), "ipdm_espirit_c64": ("int", 19)}
    for name, (ret, nargs) in want.items():
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ipdm.h"
        params = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        assert m.group(1) == ret and len(params.split(",")) == nargs == len(pkg.lib.SIGNATURES[name])
        assert hasattr(pkg.lib.lib, name)
    assert pkg.lib.lib.ipdm_espirit_workspace_bytes.restype is __import__("ctypes").c_size_t
    assert "#define IPDM_ABI_VERSION 4" in header and pkg.lib.lib.ipdm_abi_version() == 4


def test_c_entries_check_their_arguments_without_a_gpu(pkg):
    """IPDM_EINVAL first, then IPDM_EUNSUPPORTED; every one of these returns before a pointer is looked at"""
    lib, P = pkg.lib.lib, pkg.lib.P
    z = P(0)
    gram = lambda ah, aw, k, B, n, H, W: lib.ipdm_espirit_gram_c64(z, ah, aw, k, z, B, n, H, W, z)
    assert gram(8, 8, 6, 1, 4, 32, 32) == pkg.lib.IPDM_EINVAL                 # NULL tensors
    assert gram(8, 8, 6, 0, 4, 32, 32) == 0                                   # an empty batch launches nothing
    assert gram(2, 8, 6, 1, 4, 32, 32) == pkg.lib.IPDM_EINVAL                 # a box side of 5 below ksize 6
    assert gram(16, 8, 6, 1, 4, 32, 32) == pkg.lib.IPDM_EINVAL                # the box leaves the image
    assert gram(8, 8, 6, 1, 17, 32, 32) == pkg.lib.IPDM_EUNSUPPORTED
    assert gram(8, 8, 7, 1, 16, 32, 32) == pkg.lib.IPDM_EUNSUPPORTED
    assert gram(8, 8, 6, 65536, 4, 32, 32) == pkg.lib.IPDM_EUNSUPPORTED
    assert gram(2, 8, 9, 1, 4, 32, 32) == pkg.lib.IPDM_EINVAL                 # both: IPDM_EINVAL wins
    full = lambda sv, crop, it: lib.ipdm_espirit_c64(z, 8, 8, 6, sv, crop, it, z, z, z, z, z, z, z, 1, 17, 32, 32, z)
    assert full(0.02, 0.8, 30) == pkg.lib.IPDM_EUNSUPPORTED
    for bad in ((-0.1, 0.8, 30), (float("nan"), 0.8, 30), (1.0, 0.8, 30), (0.02, float("nan"), 30), (0.02, 0.8, -1)):
        assert full(*bad) == pkg.lib.IPDM_EINVAL
    assert lib.ipdm_espirit_pixel_c64(z, z, 6, 0.8, 30, z, z, 1, 17, 32, 32, z) == pkg.lib.IPDM_EUNSUPPORTED
    assert lib.ipdm_espirit_pixel_c64(z, z, 6, 0.8, 30, z, z, 1, 4, 32, 32, z) == pkg.lib.IPDM_EINVAL


def line_mask(W, centre=17):
    m = torch.zeros(W, dtype=torch.bool)
    m[::3] = True
    m[W // 2 - centre // 2:W // 2 + centre // 2 + 1] = True
    return m


def test_host_refusals_happen_before_any_launch(pkg, monkeypatch):
    def launched(*a, **k):
        raise AssertionError("a kernel entry was reached")
    monkeypatch.setattr(pkg.lib, "call", launched)
    monkeypatch.setattr(pkg.ops, "call", launched)
    est = pkg.uf.SENSE.estimate_sens_maps
    y = torch.zeros(4, 32, 32, dtype=torch.complex64)
    with pytest.raises(ValueError, match=r"calibration box 25 x 5 .* ksize = 6"):       # 5 centre lines
        est(y, line_mask(32, 5), method="espirit")
    with pytest.raises(ValueError, match=r"calibration box 7 x 7 .* ksize = 8"):
        est(y, line_mask(32), calib_max=3, method="espirit", ksize=8)
    for n, k in ((17, 3), (16, 6), (24, 6)):
        with pytest.raises(pkg.lib.IpdmUnsupported, match="n_virtual"):
            est(torch.zeros(n, 32, 32, dtype=torch.complex64), line_mask(32), method="espirit", ksize=k)
        with pytest.raises(pkg.lib.IpdmUnsupported, match="n_virtual"):
            pkg.uf.SENSE.from_measurement(torch.zeros(n, 32, 32, dtype=torch.complex64), line_mask(32), method="espirit", ksize=k)
    with pytest.raises(pkg.lib.IpdmUnsupported, match="n_virtual"):             # compressed to 12 coils, k = 7: 588 columns > 432
        pkg.uf.SENSE.from_measurement(torch.zeros(24, 32, 32, dtype=torch.complex64), line_mask(32), n_virtual=12,
                                      method="espirit", ksize=7)
    with pytest.raises(TypeError, match="radius"):                            # Walsh's keyword
        est(y, line_mask(32), method="espirit", radius=2)
    with pytest.raises(ValueError, match="method"):
        est(y, line_mask(32), method="grappa")
    with pytest.raises(ValueError, match="integer"):
        est(y, line_mask(32), method="espirit", ksize=4.5)
    cine = torch.zeros(4, 3, 32, 32, dtype=torch.complex64)
    with pytest.raises(ValueError, match="ksize = 6"):
        pkg.uf.SENSE.from_cine_measurement(cine, line_mask(32, 5), method="espirit")


def test_a_failed_decomposition_names_the_image(pkg, monkeypatch):
    """status != 0 (the kernel's report of no convergence or a non-finite value) becomes a RuntimeError naming the images"""
    def fake(y, ah, aw, **kw):
        return y, torch.zeros(3, 8, 8), torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 1], dtype=torch.int32)
    monkeypatch.setattr(pkg.ops, "espirit_maps", fake)
    with pytest.raises(RuntimeError, match=r"image\(s\) \[1, 2\]"):
        pkg.uf.SENSE._espirit_maps(torch.zeros(4, 3, 8, 8, dtype=torch.complex64), 2, 2, "estimate_sens_maps")


def test_driver_flag_checks(pkg):
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    base = dict(maps_method="espirit", espirit_kernel=6, espirit_thresh=0.02, espirit_crop=0.8)
    assert load_data.driver_maps_method(dict(base, maps_method="walsh"), False, 64, 32, 32, None) == ("walsh", {})
    assert load_data.driver_maps_method(base, True, 4, 32, 32, (12, 8)) == ("espirit", dict(ksize=6, sv_thresh=0.02, crop=0.8))
    for bad, n, region, word in ((base, 4, (2, 8), "calibration box 5 x 17"), (base, 24, (12, 8), "coil_compress"),
                                 (dict(base, espirit_kernel=9), 4, (12, 8), "3..8"), (dict(base, espirit_thresh=1.5), 4, (12, 8), "thresh"),
                                 (dict(base, espirit_crop=float("nan")), 4, (12, 8), "crop")):
        with pytest.raises(SystemExit) as e:
            load_data.driver_maps_method(bad, True, n, 32, 32, region)
        assert word in str(e.value)
    with pytest.raises(SystemExit, match="estimate_maps"):
        load_data.driver_maps_method(base, False, 4, 32, 32, None)
