"""Host side of the predictor-corrector SENSE sampler (sde/inverse.py): the float64 schedule table against the formulas
evaluated through sde_lib.VESDE's own methods, the denoising record, the Philox step ids of sliced runs, every refusal
(raised with no GPU present) and the C ABI of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import pc_helpers as pch

from inverseproblemwithdiffusionmodel_amd import _lib, ops            # a package that does not import fails this file
from inverseproblemwithdiffusionmodel_amd.sde import inverse, sde_lib
from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE, RandomUndersamplingFourier

N, SNR, EPS = 8, 0.16, 1e-5


@pytest.mark.parametrize("predictor", inverse.PREDICTORS)
@pytest.mark.parametrize("corrector", inverse.CORRECTORS)
def test_schedule_table_against_float64(predictor, corrector):
    sde = pch.vesde64(N=N)
    got = inverse.pc_schedule(sde, predictor, corrector, SNR, EPS, denoise=True)
    want = pch.schedule64(sde, predictor, corrector, SNR, EPS, denoise=True)
    # VESDE.sde builds sqrt(2 log(sigma_max / sigma_min)) as a float32 tensor: that constant alone carries 2^-24
    rtol = 2.0 ** -22 if predictor == "euler_maruyama" else 1e-12
    for k in ("t", "sigma", "corr_step", "corr_noise"):
        if want[k] is None:
            assert got[k] is None, k
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    for k in ("pred_step", "pred_noise"):
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].dtype == np.float64
            np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=0, err_msg=k)
    if predictor != "none":
        assert got["pred_noise"][-1] == 0.0 and (got["pred_noise"][:-1] > 0).all()      # denoise: the returned x_mean
        assert (got["pred_step"] > 0).all()
        keep = inverse.pc_schedule(sde, predictor, corrector, SNR, EPS, denoise=False)
        assert keep["pred_noise"][-1] > 0 or predictor == "ancestral_sampling"           # (ancestral: sigma_{-1} = 0 there)
    if corrector == "ald":
        np.testing.assert_allclose(got["corr_step"], 2 * (SNR * got["sigma"]) ** 2, rtol=1e-15)


def test_schedule_uses_the_modules_own_sigmas():
    """the table of a plain VESDE (float32 discrete sigmas) is the float64 table of those float32 values"""
    a = inverse.pc_schedule(sde_lib.VESDE(0.01, 50.0, N), "reverse_diffusion", "ald", SNR, EPS, True)
    b = inverse.pc_schedule(pch.vesde64(N=N), "reverse_diffusion", "ald", SNR, EPS, True)
    for k in ("pred_step", "pred_noise", "corr_step"):
        assert np.array_equal(a[k], b[k])
    sig = sde_lib.VESDE(0.01, 50.0, N).discrete_sigmas.double().numpy()
    np.testing.assert_allclose(a["pred_step"][0], sig[-1] ** 2 - sig[-2] ** 2, rtol=1e-15)
    np.testing.assert_allclose(a["pred_step"][-1], sig[0] ** 2, rtol=1e-15)              # below the first sigma: 0


@pytest.mark.parametrize("n_steps,predictor,corrector", [(1, "reverse_diffusion", "langevin"), (3, "ancestral_sampling", "ald"),
                                                         (2, "none", "langevin"), (0, "euler_maruyama", "none")])
def test_records_and_step_ids_of_a_sliced_run(n_steps, predictor, corrector):
    sde = sde_lib.VESDE(0.01, 50.0, N)
    sched = inverse.pc_schedule(sde, predictor, corrector, SNR, EPS, True)
    slots = inverse.pc_slots(predictor, corrector, n_steps)
    assert len(slots) == (n_steps if corrector != "none" else 0) + (predictor != "none")
    full = inverse.pc_records(sched, slots, n_steps, 0.7, 0, N)
    assert full.dtype.itemsize == 32 and full.shape == (N, len(slots))
    for i in range(N):
        for j, (kind, s) in enumerate(slots):
            assert full["step_id"][i, j] == i * (n_steps + 1) + s
            assert s == (n_steps if kind == "predictor" else j)
    assert len(np.unique(full["step_id"])) == full.size and full["step_id"].min() >= 0 != inverse.INIT_STEP_ID
    a, b = inverse.pc_records(sched, slots, n_steps, 0.7, 0, 3), inverse.pc_records(sched, slots, n_steps, 0.7, 3, N)
    assert np.array_equal(np.concatenate([a, b]).view(np.uint8), full.view(np.uint8))      # a split run: the same records
    assert (full["coef"] == np.float32(0.7)).all() and (full["seg_scale"] == 0).all()
    np.testing.assert_array_equal(full["sigma"][:, 0], sched["sigma"].astype(np.float32))
    for j, (kind, _) in enumerate(slots):
        if kind == "predictor":
            np.testing.assert_array_equal(full["step"][:, j], sched["pred_step"].astype(np.float32))
            np.testing.assert_array_equal(full["noise_scale"][:, j], sched["pred_noise"].astype(np.float32))
            assert full["noise_scale"][-1, j] == 0.0
        elif kind == "ald":
            np.testing.assert_array_equal(full["step"][:, j], sched["corr_step"].astype(np.float32))
        else:                                                    # langevin: formed on the device
            assert (full["step"][:, j] == 0).all() and (full["noise_scale"][:, j] == 0).all()


def _sense(H=16, W=16, n=2):
    maps = torch.rand(n, H, W, dtype=torch.float64) + 0.1
    mask = torch.zeros(W, dtype=torch.bool)
    mask[::2] = True
    return SENSE("custom", n, 2, 0.04, (1, H, W), seed=0, sens_maps=maps, mask_mode="custom", mask=mask)


def _single(H=16, W=16):
    mask = torch.zeros(W, dtype=torch.bool)
    mask[::2] = True
    return RandomUndersamplingFourier(2, 0.04, (1, H, W), seed=0, mask_mode="custom", mask=mask)


def test_refusals_without_a_gpu():
    sde = sde_lib.VESDE(0.01, 50.0, N)
    op, sc = _sense(), _single()
    y = torch.zeros(2, 3, 1, 16, 16, dtype=torch.complex64)
    ysc = torch.zeros(3, 1, 16, 16, dtype=torch.complex64)
    get = inverse.get_pc_inverse_sampler
    with pytest.raises(NotImplementedError, match="VESDE"):
        get(sde_lib.VPSDE(0.1, 20.0, N), op, y)
    with pytest.raises(NotImplementedError, match="VESDE"):
        get(sde_lib.subVPSDE(0.1, 20.0, N), op, y)
    with pytest.raises(NotImplementedError, match="probability_flow"):
        get(sde, op, y, probability_flow=True)
    with pytest.raises(ValueError, match="predictor"):
        get(sde, op, y, predictor="heun")
    with pytest.raises(ValueError, match="corrector"):
        get(sde, op, y, corrector="mala")
    with pytest.raises(ValueError, match="dc"):
        get(sde, op, y, dc="admm")
    with pytest.raises(ValueError, match="not served"):
        get(sde, op, y, dc="projection")
    with pytest.raises(ValueError, match="not served"):
        get(sde, sc, ysc, dc="cg")
    for dc, w in (("gradient", 1.5), ("gradient", -0.1), ("cg", -1.0), ("cg", float("inf")), ("cg", float("nan"))):
        with pytest.raises(ValueError, match="dc_weight"):
            get(sde, op, y, dc=dc, dc_weight=w)
    for dc, w in (("projection", 1.01), ("closed_form", -2.0)):
        with pytest.raises(ValueError, match="dc_weight"):
            get(sde, sc, ysc, dc=dc, dc_weight=w)
    with pytest.raises(ValueError, match="n_steps"):
        get(sde, op, y, n_steps=-1)
    with pytest.raises(ValueError, match="n_steps"):
        get(sde, op, y, n_steps=0)
    with pytest.raises(ValueError, match="n_steps"):
        get(sde, op, y, n_steps=1.5)
    with pytest.raises(ValueError, match="max_iter"):
        get(sde, op, y, dc="cg", cg_iters=0)
    with pytest.raises(ValueError, match="measurement"):
        get(sde, op, torch.zeros(3, 3, 1, 16, 16, dtype=torch.complex64))                 # 3 coil images, 2 maps
    # a k-space size of class 0: the operator's IpdmUnsupported, before any network forward (no model exists here)
    assert ops.kspace_size_class(16, 24) == ops.KSPACE_NONE
    bad = RandomUndersamplingFourier(2, 0.04, (1, 16, 24), seed=0, mask_mode="custom", mask=torch.ones(24, dtype=torch.bool))
    with pytest.raises(_lib.IpdmUnsupported, match="16x24"):
        get(sde, bad, torch.zeros(1, 1, 16, 24, dtype=torch.complex64))
    # the legal choices build without a GPU; dc=None picks the operator's first
    assert get(sde, op, y).dc == "gradient" and get(sde, sc, ysc).dc == "projection"
    assert get(sde, op, y, n_steps=0, corrector="none").slots == [("predictor", 0)]
    assert get(sde, sc, ysc.unsqueeze(0), dc="closed_form", dc_weight=3.0).dc == "closed_form"


def test_engine_and_driver_exist():
    from inverseproblemwithdiffusionmodel_amd import engine
    assert callable(engine.build_pc_sampler)
    assert os.path.exists(os.path.join(REPO, "scripts", "acdc_SENSE_pc.py"))
    assert os.path.exists(os.path.join(REPO, "scripts", "bench_pc_sense.py"))


def test_abi_of_the_new_entry_points():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ipdm.h")).read(), flags=re.S)
    i, P, f, d, u64, i64 = _lib.c_int, _lib.P, _lib.c_float, _lib.c_double, _lib.c_uint64, _lib.c_int64
    head = [P, P, P, P, P, P, f, f, u64, i64, i64, P, i]                                    # ..., dev_sched, sched_stride
    want = {"ipdm_pc_langevin_coef_workspace_bytes": ("int64_t", [i]),
            "ipdm_pc_langevin_coef_f32": ("int", [P, P, P, P, d, d, u64, i64, i64, P, f, f, P, P, i, i64, P]),
            "ipdm_pc_sense_step_f32": ("int", head + [P, P, i, i, P, i, f, P, i, i, i, i, P]),
            "ipdm_pc_sense_cg_step_f32": ("int", head + [P, P, i, i, P, i, f, P, P, i, f, P, i, i, i, i, P]),
            "ipdm_pc_singlecoil_step_f32": ("int", head + [P, P, i, f, i, P, i, i, i, P])}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, args) in want.items():
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ipdm.h"
        assert m.group(1) == ret and len(m.group(2).split(",")) == len(args), name
        assert _lib.SIGNATURES[name] == args and hasattr(lib, name), name
    # the per-sample tails: the shared-record entry points' lists plus `int sched_stride` after dev_sched
    for new, old in (("ipdm_pc_sense_step_f32", "ipdm_ald_sense_step_sets_f32"),
                     ("ipdm_pc_sense_cg_step_f32", "ipdm_ald_sense_cg_step_sets_f32"),
                     ("ipdm_pc_singlecoil_step_f32", "ipdm_ald_singlecoil_step_f32")):
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old][:12] + [i] + _lib.SIGNATURES[old][12:]
    assert _lib.lib.ipdm_pc_langevin_coef_workspace_bytes.restype is i64
    assert _lib.lib.ipdm_pc_langevin_coef_workspace_bytes(3) >= 3 * 2 * 8 and _lib.lib.ipdm_pc_langevin_coef_workspace_bytes(0) == 0
    assert "#define IPDM_ABI_VERSION 4" in header and _lib.lib.ipdm_abi_version() == 4
    assert ctypes.sizeof(ctypes.c_float) * 6 + 8 == 32 == pch.SCHED.itemsize                # ipdm_sched_t stays 32 bytes
    # NULL operands and bad strides are refused by the library itself, before any launch (no GPU needed)
    z = _lib.P(0)
    assert _lib.lib.ipdm_pc_langevin_coef_f32(z, z, z, z, 0.1, 1.0, 0, 0, 0, z, 0.0, 0.0, z, z, 1, 16, z) == _lib.IPDM_EINVAL
    assert _lib.lib.ipdm_pc_singlecoil_step_f32(z, z, z, z, z, z, 0.0, 0.0, 0, 0, 0, z, 2, z, z, 1, 0.0, 0, z, 1, 16, 16,
                                                z) == _lib.IPDM_EINVAL
    assert _lib.lib.ipdm_pc_singlecoil_step_f32(z, z, z, z, z, z, 0.0, 0.0, 0, 0, 0, z, 1, z, z, 1, 0.0, 0, z, 1, 16, 16,
                                                z) == _lib.IPDM_EINVAL                      # stride 1 without records
    for name in ("pc_langevin_coef", "pc_sense_step", "pc_sense_cg_step", "pc_singlecoil_step"):
        assert callable(getattr(ops, name))
