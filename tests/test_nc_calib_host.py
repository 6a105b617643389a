"""Non-Cartesian self-calibration, host side: the C entries' declarations and the answers they give without
a GPU, ``calibration_window`` on the trajectories the design lists, the method itself in float64 (tests/nc_calib_helpers.py:
maps and compression from the windowed samples against the same estimators on fully sampled Cartesian k-space of the
same object), and every new refusal of ``build_problem`` and of the two drivers, reached before a network is built."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import coilcomp_helpers as cch
import csm_helpers as csm
import espirit_helpers as esp
import nc_calib_helpers as nc
import noncart_helpers as nh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACDC = os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py")
CINE = os.path.join(REPO, "scripts", "cine_SENSE_real_img_2d_time.py")


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, engine, ops, synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import noncartesian
    return Namespace(lib=_lib, ops=ops, engine=engine, syn=synthetic, nc=noncartesian)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_declarations(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    i, P = pkg.lib.c_int, pkg.lib.P
    want = {"ipdm_nc_coil_gram_c64": ("int", [P, P, P, P, i, i, i, P]),
            "ipdm_nc_coil_gram_workspace_bytes": ("size_t", [i, i, i])}
    for name, (ret, args) in want.items():
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ipdm.h"
        assert m.group(1) == ret and len(m.group(2).split(",")) == len(args)
        assert pkg.lib.SIGNATURES[name] == args and hasattr(pkg.lib.lib, name)
    assert pkg.lib.lib.ipdm_nc_coil_gram_workspace_bytes.restype is ctypes.c_size_t
    assert "#define IPDM_ABI_VERSION 4" in header and pkg.lib.lib.ipdm_abi_version() == 4      # two entries added, none changed


def test_abi_answers_without_a_gpu(pkg):
    lib = pkg.lib.lib
    EINVAL, EUNSUP = pkg.lib.IPDM_EINVAL, pkg.lib.IPDM_EUNSUPPORTED
    gram = lib.ipdm_nc_coil_gram_c64
    assert gram(None, None, None, None, 1, 4, 100, None) == EINVAL           # NULL tensors
    assert gram(None, None, None, None, 1, 65, 100, None) == EUNSUP          # the range of ipdm_coilcomp_supported
    assert gram(None, None, None, None, 1, 64, 100, None) == EINVAL
    assert gram(None, None, None, None, 1, 0, 100, None) == EINVAL
    assert gram(None, None, None, None, 1, 4, 0, None) == EINVAL             # M < 1
    assert gram(None, None, None, None, -1, 4, 100, None) == EINVAL
    assert gram(None, None, None, None, 0, 4, 100, None) == 0                # an empty batch
    assert gram(None, None, None, None, 65536, 4, 100, None) == EUNSUP       # images ride on grid.z
    for n in (1, 64):
        assert bool(lib.ipdm_coilcomp_supported(n, 1)) and gram(None, None, None, None, 0, n, 1, None) == 0


def test_workspace_grows_with_the_chunk_count(pkg):
    ws, C = pkg.lib.lib.ipdm_nc_coil_gram_workspace_bytes, pkg.ops.NC_GRAM_CHUNK
    for n in (1, 5, 64):
        pairs = n * (n + 1) // 2
        for M, chunks in ((1, 1), (C - 1, 1), (C, 1), (C + 1, 2), (3 * C + 7, 4)):
            assert ws(1, n, M) == chunks * pairs * 16, (n, M)                # double2 partials [B][chunks][pairs]
            assert ws(3, n, M) == 3 * ws(1, n, M)
    for args in ((0, 4, 10), (1, 65, 10), (1, 0, 10), (1, 4, 0), (65536, 4, 10)):
        assert ws(*args) == 0


def test_ops_refuse_before_the_gpu(pkg):
    ops = pkg.ops
    y = torch.zeros(4, 1, 64, dtype=torch.complex64)
    k = torch.zeros(64, 2, dtype=torch.float64)
    w = torch.ones(64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.nc_coil_gram(y)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.nc_calib_images(y, k, 16, 16, w)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.nc_calib_kspace(y, k, 16, 16, w)
    with pytest.raises(pkg.lib.IpdmUnsupported, match="no k-space kernel for 24x24"):
        ops.nc_calib_kspace(y, k, 24, 24, w)
    assert ops.nc_coil_gram_workspace(1, 65, 10, "cpu") is None


# ---- calibration_window -----------------------------------------------------------------------------------------------------------
def largest_square(occ, calib_max=12):
    """half-width of the largest square about the centre that the samples cover"""
    H, W = occ.shape
    a = -1
    while a + 1 <= min(H // 2, H - 1 - H // 2, W // 2, W - 1 - W // 2, calib_max) and \
            occ[H // 2 - a - 1:H // 2 + a + 2, W // 2 - a - 1:W // 2 + a + 2].all():
        a += 1
    return a


@pytest.mark.parametrize("spokes,readout,size,square,box", [
    (4, 32, 16, 1, None),              # refused: a 3 x 3 square, and no box of 5 x 5
    (12, 32, 16, 2, (2, 5)),
    (13, 256, 128, 2, (2, 5)),
    (32, 256, 128, 6, (5, 11)),
    (24, 64, 32, 6, (6, 6)),           # the 13 x 13 box of the accuracy table
])
def test_window_of_the_listed_trajectories(pkg, spokes, readout, size, square, box):
    """the covered square the design quotes per trajectory, and the box the largest-box rule of calibration_region makes of
    the same occupancy (largest area first, so a radial pattern at a low spoke count gives a box wider than it is high)"""
    k = pkg.syn.radial_trajectory(spokes, readout, size, size)
    occ = nc.cell_occupancy(k.numpy(), size, size)
    assert largest_square(occ) == square
    if box is None:
        with pytest.raises(ValueError, match=r"ah = \d+, aw = \d+.*at least 5 x 5"):
            pkg.nc.calibration_window(k, size, size)
        return
    ah, aw, w = pkg.nc.calibration_window(k, size, size)
    assert (ah, aw) == box == nc.largest_box(occ)
    assert isinstance(w, torch.Tensor) and w.dtype == torch.float64 and tuple(w.shape) == (spokes * readout,)
    assert np.array_equal(w.numpy(), nc.window_weights(k.numpy(), ah, aw))


def test_window_weights_shape(pkg):
    H, W = 16, 32
    k = pkg.syn.radial_trajectory(16, 64, H, W)
    ah, aw, w = pkg.nc.calibration_window(k, H, W, taper=2.0)
    assert (ah, aw) == (2, 8) == nc.largest_box(nc.cell_occupancy(k.numpy(), H, W))      # a rectangular box
    d = np.maximum(np.abs(k[:, 0].numpy()) - ah, np.abs(k[:, 1].numpy()) - aw)
    w = w.numpy()
    assert (w[d <= 0.5] == 1.0).all() and (d <= 0.5).sum() > 25
    assert (w[d >= 0.5 + 2.0] == 0.0).all() and (d >= 2.5).sum() > 0
    ramp = (d > 0.5) & (d < 2.5)
    assert ramp.sum() > 10 and ((w[ramp] > 0) & (w[ramp] < 1)).all()
    order = np.argsort(d)
    assert (np.diff(w[order]) <= 0).all()                                    # monotone in the distance from the box
    assert np.abs(w[ramp] - 0.5 * (1 + np.cos(np.pi * (d[ramp] - 0.5) / 2.0))).max() <= 1e-15
    hard = pkg.nc.calibration_window(k, H, W, taper=0.0)[2].numpy()
    assert set(np.unique(hard)) == {0.0, 1.0} and np.array_equal(hard == 1.0, d <= 0.5)
    capped = pkg.nc.calibration_window(k, H, W, calib_max=4)[:2]             # the half-widths stop at calib_max
    assert max(capped) <= 4 and capped == nc.largest_box(nc.cell_occupancy(k.numpy(), H, W), 4)
    with pytest.raises(ValueError, match="calib_max"):
        pkg.nc.calibration_window(k, H, W, calib_max=-1)
    with pytest.raises(ValueError, match="taper"):
        pkg.nc.calibration_window(k, H, W, taper=-1.0)
    with pytest.raises(ValueError, match="leaves"):
        pkg.nc.calibration_window(k * 3, H, W)
    with pytest.raises(ValueError, match="rounds to the k-space centre"):    # nothing near the centre
        pkg.nc.calibration_window(k[k.abs().max(dim=1).values > 2.0], H, W)


def test_window_pools_the_frames_of_a_cine_trajectory(pkg):
    kc = pkg.syn.radial_cine_trajectory(6, 4, 32, 16, 16)
    assert largest_square(nc.cell_occupancy(kc[0].numpy(), 16, 16)) == 1
    with pytest.raises(ValueError, match="at least 5 x 5"):
        pkg.nc.calibration_window(kc[0], 16, 16)                              # one frame alone is refused
    occ = nc.cell_occupancy(kc.numpy(), 16, 16)
    assert largest_square(occ) == 5
    ah, aw, w = pkg.nc.calibration_window(kc, 16, 16)
    assert (ah, aw) == nc.largest_box(occ) == (6, 5) and tuple(w.shape) == (6 * 128,)
    assert np.array_equal(w.numpy(), nc.window_weights(kc.numpy(), ah, aw))


# ---- the method, in float64 ---------------------------------------------------------------------------------------------------------
H32 = 32
# what this model gave when the test was written (the accuracy table); the bounds below are 3 x these
WALSH_SEEN, ESPIRIT_SEEN = 3.5e-3, 5.7e-3


@pytest.fixture(scope="module")
def model():
    """32x32, golden-angle 24 x 64, 4 coils: the gridded calibration k-space with the default lam, cap and tolerance"""
    acq = nc.acquisition(H32, H32, 24, 64, 4)
    ah, aw, w = nc.window(acq["k"], H32, H32)
    w = w.astype(np.float32).astype(np.float64)
    ks, iters = nc.calib_kspace(acq["y"], acq["k"], H32, H32, w, lam=1e-2, max_iter=40, tol=1e-4)
    return dict(acq=acq, ah=ah, aw=aw, w=w, ks=ks, iters=iters)


def test_model_gridded_box_against_cartesian(model):
    ah, aw = model["ah"], model["aw"]
    assert (ah, aw) == (6, 6)
    assert 15 <= model["iters"].min() and model["iters"].max() <= 30        # the tolerance stops it well under the cap of 40
    full = nc.box_of(model["acq"]["full"][:, 0], ah, aw)
    err = np.abs(nc.box_of(model["ks"][:, 0], ah, aw) - full).max() / np.abs(full).max()
    print(f"iterations {model['iters'].ravel().tolist()}, box error {err:.2e} of the peak")
    assert err <= 1.5e-2


def test_model_walsh_maps_against_cartesian(model):
    ah, aw = model["ah"], model["aw"]
    ref = csm.estimate(torch.from_numpy(model["acq"]["full"]), ah, aw)
    got = csm.estimate(torch.from_numpy(model["ks"]), ah, aw)
    near = csm.near_threshold(ref["rss"], ref["rss_max"], 0.02) | csm.near_threshold(got["rss"], got["rss_max"], 0.02)
    assert bool(((got["support"] == ref["support"]) | near).all())
    sup = (ref["support"] & got["support"] & ~near)[None].expand_as(ref["maps"])
    d = (got["maps"] - ref["maps"]).abs()[sup]
    print(f"Walsh: support {int(ref['support'].sum())} pixels, max {float(d.max()):.2e}, rms {float(d.pow(2).mean().sqrt()):.2e}")
    assert int(ref["support"].sum()) > 500 and float(d.max()) <= 3 * WALSH_SEEN


def test_model_espirit_maps_against_cartesian(model):
    ah, aw = model["ah"], model["aw"]
    ref = esp.estimate(model["acq"]["full"][:, 0], ah, aw, k=4)
    got = esp.estimate(model["ks"][:, 0], ah, aw, k=4)
    assert got["rank"] == ref["rank"] and min(got["margin"], ref["margin"]) > 0.02
    leave = ref["leave_out"] | got["leave_out"]
    kept_ref, kept_got = ref["eigval"] > 0.8, got["eigval"] > 0.8
    assert ((kept_ref == kept_got) | leave).all()
    keep = kept_ref & kept_got & ~leave
    d = np.abs(got["maps"] - ref["maps"])[:, keep]
    print(f"ESPIRiT ksize 4: rank {got['rank']}, support {int(kept_ref.sum())} pixels, max {d.max():.2e}")
    assert keep.sum() > 500 and d.max() <= 3 * ESPIRIT_SEEN


def test_model_compression_against_the_box_pca():
    """4 virtual coils of 8 from the windowed Gram matrix of the samples keep the energy of the Cartesian calibration box
    that the box's own PCA keeps, within 1e-3"""
    acq = nc.acquisition(H32, H32, 24, 64, 8, seed=1)
    ah, aw, w = nc.window(acq["k"], H32, H32)
    G = nc.gram(acq["y"], w)
    assert np.array_equal(G, G.conj().transpose(0, 2, 1)) and not np.diagonal(G, axis1=1, axis2=2).imag.any()
    direct = np.einsum("m,im,jm->ij", w, acq["y"][:, 0].astype(np.complex128), acq["y"][:, 0].astype(np.complex128).conj())
    assert np.abs(G[0] - direct).max() <= 1e-12 * np.abs(direct).max()
    box = nc.box_of(acq["full"][:, 0], ah, aw).reshape(8, -1)
    A = cch.matrix(G[0], 4)["A"][0]
    A_box = cch.matrix(cch.hermitian(box @ box.conj().T), 4)["A"][0]
    kept, kept_box = nc.energy_kept(A, box), nc.energy_kept(A_box, box)
    print(f"energy kept by 4 of 8 virtual coils: sample Gram {kept:.5f}, box PCA {kept_box:.5f}")
    assert kept_box > 0.98 and abs(kept - kept_box) <= 1e-3
    y_nan = acq["y"].copy()
    y_nan[:, :, w == 0] = np.nan                                             # zero-weight samples are never looked at
    assert np.array_equal(nc.gram(y_nan, w), G)


# ---- build_problem ----------------------------------------------------------------------------------------------------------------
def test_build_problem_new_refusals(pkg):
    bp = pkg.engine.build_problem
    k = pkg.syn.radial_trajectory(12, 32, 16, 16)
    kw = dict(H=16, W=16, trajectory=k)
    y = torch.zeros(4, 384, dtype=torch.complex64)
    with pytest.raises(ValueError, match="self_calibrate=True estimates the coil maps; it does not go with sens_maps="):
        bp("cpu", 1, self_calibrate=True, sens_maps=np.ones((4, 16, 16)), **kw)
    with pytest.raises(ValueError, match="self_calibrate= and virtual_coils= go with trajectory="):
        bp("cpu", 1, H=16, W=16, self_calibrate=True)
    with pytest.raises(ValueError, match="self_calibrate= and virtual_coils= go with trajectory="):
        bp("cpu", 1, H=16, W=16, virtual_coils=2)
    with pytest.raises(ValueError, match="virtual_coils= goes with self_calibrate=True"):
        bp("cpu", 1, virtual_coils=2, **kw)
    with pytest.raises(ValueError, match="at least 5 x 5"):                  # the window, before the network is built
        bp("cpu", 1, H=16, W=16, trajectory=pkg.syn.radial_trajectory(4, 32, 16, 16), self_calibrate=True)
    with pytest.raises(ValueError, match="n_virtual = 5 outside 1..n_coils = 4"):
        bp("cpu", 1, measurement=y, self_calibrate=True, virtual_coils=5, **kw)
    with pytest.raises(ValueError, match="noise_cov= goes with n_virtual="):
        bp("cpu", 1, measurement=y, self_calibrate=True, noise_cov=np.eye(4), **kw)
    with pytest.raises(ValueError, match="not positive definite"):
        bp("cpu", 1, measurement=y, self_calibrate=True, virtual_coils=2, noise_cov=-np.eye(4), **kw)
    with pytest.raises(ValueError, match="'walsh' or 'espirit'"):
        bp("cpu", 1, measurement=y, self_calibrate=True, maps_method="sake", **kw)
    with pytest.raises(ValueError, match="smaller than ksize = 6"):         # the 5 x 11 box of 12 spokes
        bp("cpu", 1, measurement=y, self_calibrate=True, maps_method="espirit", **kw)
    y40 = torch.zeros(40, 384, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match="n_virtual="):            # more than 32 coils: compress first
        bp("cpu", 1, measurement=y40, self_calibrate=True, **kw)
    with pytest.raises(NotImplementedError, match="n_virtual="):            # ESPIRiT past its caps
        bp("cpu", 1, measurement=y40, self_calibrate=True, virtual_coils=20, maps_method="espirit",
           maps_kwargs=dict(ksize=4), **kw)
    with pytest.raises(ValueError, match=r"complex \(n_coils, M = 384\)"):
        bp("cpu", 1, measurement=torch.zeros(4, 383, dtype=torch.complex64), self_calibrate=True, **kw)
    with pytest.raises(ValueError, match=r"a 2-D problem takes \(M, 2\)"):
        bp("cpu", 1, H=16, W=16, trajectory=pkg.syn.radial_cine_trajectory(6, 4, 32, 16, 16), self_calibrate=True)


def test_build_problem_old_refusals_hold(pkg):
    bp = pkg.engine.build_problem
    k = pkg.syn.radial_trajectory(12, 32, 16, 16)
    kw = dict(H=16, W=16, trajectory=k)
    for extra, msg in ((dict(estimate_maps=True), "estimate_maps="), (dict(coil_compress=2), "coil_compress="),
                       (dict(noise_cov=np.eye(4)), "noise_cov=")):
        with pytest.raises(ValueError, match=msg + " does not go with trajectory="):
            bp("cpu", 1, **kw, **extra)
        if "noise_cov" not in extra:                                         # ... and the new argument does not lift them
            with pytest.raises(ValueError, match=msg + " does not go with trajectory="):
                bp("cpu", 1, self_calibrate=True, **kw, **extra)
    with pytest.raises(ValueError, match="pass sens_maps="):
        bp("cpu", 1, measurement=torch.zeros(4, 384, dtype=torch.complex64), **kw)


def test_class_methods_refuse_on_the_host(pkg):
    N = pkg.nc.NonCartesianSENSE
    k = pkg.syn.radial_trajectory(12, 32, 16, 16)
    y = np.zeros((4, 384), dtype=np.complex64)
    with pytest.raises(TypeError, match="complex samples"):
        N.estimate_sens_maps(np.zeros((4, 384)), k, (1, 16, 16))
    with pytest.raises(ValueError, match=r"\(n_coils,\) \+ \(384,\) expected"):
        N.estimate_sens_maps(y[:, :383], k, (1, 16, 16))
    with pytest.raises(ValueError, match=r"\(n_coils,\) \+ \(6, 128\) expected"):
        N.from_measurement(y, pkg.syn.radial_cine_trajectory(6, 4, 32, 16, 16), (1, 16, 16))
    with pytest.raises(ValueError, match="'walsh' or 'espirit'"):
        N.estimate_sens_maps(y, k, (1, 16, 16), method="sake")
    with pytest.raises(TypeError, match="method='espirit' takes"):
        N.estimate_sens_maps(y, k, (1, 16, 16), method="espirit", radius=2)
    with pytest.raises(ValueError, match="n_virtual = 0 outside"):
        N.compress_measurement(y, k, (1, 16, 16), 0)
    with pytest.raises(ValueError, match="Hermitian"):
        N.compress_measurement(y, k, (1, 16, 16), 2, noise_cov=np.triu(np.ones((4, 4))))
    with pytest.raises(ValueError, match="is not \\(1, H, W\\)"):
        N.from_measurement(y, k, (2, 16, 16))
    with pytest.raises(ValueError, match="weights"):
        N.from_measurement(y, k, (1, 16, 16), weights=np.ones(5))
    with pytest.raises(ValueError, match="at least 5 x 5"):
        N.from_measurement(np.zeros((4, 128), dtype=np.complex64), pkg.syn.radial_trajectory(4, 32, 16, 16), (1, 16, 16))


# ---- the drivers ------------------------------------------------------------------------------------------------------------------
def _run(script, *args):
    r = subprocess.run([sys.executable, script, *args], capture_output=True, text=True, timeout=120)
    return r.returncode, (r.stdout + r.stderr)


RADIAL = ["--image_size", "16", "--trajectory", "radial", "--readout", "32"]
CG = ["--proximal_type", "L2PenaltyCG"]


@pytest.mark.parametrize("script,extra", [(ACDC, []), (CINE, CG)])
@pytest.mark.parametrize("args,msg", [
    (["--self_calibrate"], "--self_calibrate goes with --trajectory"),
    (["--virtual_coils", "2"], "--virtual_coils N goes with --self_calibrate"),
    ([*RADIAL, "--spokes", "12", "--virtual_coils", "2"], "--virtual_coils N goes with --self_calibrate"),
    ([*RADIAL, "--spokes", "12", "--self_calibrate", "--sens_phase"], "it does not go with --sens_maps / --sens_phase"),
    ([*RADIAL, "--spokes", "12", "--self_calibrate", "--noise_cov", "psi.npy"], "--noise_cov PATH goes with --virtual_coils N"),
    ([*RADIAL, "--spokes", "12", "--self_calibrate", "--virtual_coils", "5"], "n_virtual = 5 outside 1..n_coils = 4"),
    ([*RADIAL, "--spokes", "12", "--self_calibrate", "--calib_max", "3", "--maps_method", "espirit", "--espirit_kernel", "8"],
     "smaller than ksize = 8"),
    ([*RADIAL, "--spokes", "12", "--self_calibrate", "--estimate_maps"], "--trajectory does not go with --estimate_maps"),
    ([*RADIAL, "--spokes", "12", "--self_calibrate", "--coil_compress", "2"], "--trajectory does not go with --coil_compress"),
])
def test_drivers_refuse_before_the_network(script, extra, args, msg):
    """each refusal is the process' exit message; none of them reaches the GPU (this test runs without one)"""
    rc, out = _run(script, *args, *extra) if "--image_size" in args else _run(script, "--image_size", "16", *args, *extra)
    assert rc != 0 and msg in out, out[-600:]


def test_driver_window_is_checked_before_the_network():
    rc, out = _run(ACDC, *RADIAL, "--spokes", "4", "--self_calibrate")
    assert rc != 0 and "--self_calibrate: calibration window" in out and "at least 5 x 5" in out, out[-600:]
    rc, out = _run(CINE, *RADIAL, "--spokes", "1", "--T", "3", "--self_calibrate", *CG)       # 3 spokes in the pool
    assert rc != 0 and "--self_calibrate: calibration window" in out and "at least 5 x 5" in out, out[-600:]


def test_drivers_measured_form(tmp_path):
    """--kspace --trajectory: without --self_calibrate the maps file is still asked for; with it the shapes are checked and
    more than 32 coils are sent to --virtual_coils"""
    k = nh.radial(12, 32, 16, 16)
    np.save(tmp_path / "k.npy", k)
    np.save(tmp_path / "kc.npy", k.reshape(3, 128, 2))
    np.save(tmp_path / "y.npy", np.zeros((4, 384), dtype=np.complex64))
    np.save(tmp_path / "yc.npy", np.zeros((4, 3, 128), dtype=np.complex64))
    np.save(tmp_path / "y40.npy", np.zeros((40, 384), dtype=np.complex64))
    np.save(tmp_path / "short.npy", np.zeros((4, 383), dtype=np.complex64))
    np.save(tmp_path / "maps.npy", np.ones((4, 16, 16), dtype=np.complex64))
    p = lambda name: str(tmp_path / name)
    rc, out = _run(ACDC, "--image_size", "16", "--trajectory", p("k.npy"), "--kspace", p("y.npy"))
    assert rc != 0 and "needs --sens_maps PATH" in out
    rc, out = _run(CINE, "--image_size", "16", *CG, "--trajectory", p("kc.npy"), "--kspace", p("yc.npy"))
    assert rc != 0 and "needs --sens_maps PATH" in out
    rc, out = _run(ACDC, "--image_size", "16", "--trajectory", p("k.npy"), "--kspace", p("short.npy"), "--self_calibrate")
    assert rc != 0 and "(n_coils, 384) expected" in out
    rc, out = _run(ACDC, "--image_size", "16", "--trajectory", p("k.npy"), "--kspace", p("y.npy"), "--self_calibrate",
                   "--sens_maps", p("maps.npy"))
    assert rc != 0 and "it does not go with --sens_maps" in out
    rc, out = _run(ACDC, "--image_size", "16", "--trajectory", p("k.npy"), "--kspace", p("y40.npy"), "--self_calibrate")
    assert rc != 0 and "n_virtual=" in out
    rc, out = _run(CINE, "--image_size", "16", *CG, "--trajectory", p("kc.npy"), "--kspace", p("yc.npy"), "--self_calibrate",
                   "--virtual_coils", "9")
    assert rc != 0 and "n_virtual = 9 outside 1..n_coils = 4" in out
