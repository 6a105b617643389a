"""Per-slice coil maps (a stack of slices in one SENSE batch), host side: the operator's (S, n, H, W) maps, the six
`_sets_` entries of the C ABI (header, ctypes table, exported symbols), the stack loader, and every refusal that has to
come before any GPU work -- build_problem's shape checks, the 2D+time classes, the driver under more than one rank."""
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import multislice_helpers as msh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS_ENTRIES = {"ipdm_sense_forward_sets_c64": "ipdm_sense_forward_c64",
                "ipdm_sense_adjoint_sets_c64": "ipdm_sense_adjoint_c64",
                "ipdm_sense_l2prox_sets_f32": "ipdm_sense_l2prox_f32",
                "ipdm_ald_sense_step_sets_f32": "ipdm_ald_sense_step_f32",
                "ipdm_sense_cgprox_sets_f32": "ipdm_sense_cgprox_f32",
                "ipdm_ald_sense_cg_step_sets_f32": "ipdm_ald_sense_cg_step_f32"}


@pytest.fixture(scope="module")
def pkg():
    from inverseproblemwithdiffusionmodel_amd import _lib, engine, ops
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ALD_optimizers, MAP_optimizers, proximal_op
    return Namespace(lib=_lib, ops=ops, engine=engine, load_data=load_data, uf=uf, ald=ALD_optimizers, map=MAP_optimizers,
                     prox=proximal_op)


# ---- the operator ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("complex_maps", [False, True])
def test_operator_takes_one_map_set_per_slice(pkg, complex_maps):
    S, n, H, W = 3, 4, 16, 32
    unit = msh.map_sets(S, n, H, W, complex_maps, seed=1)
    raw = unit * (1.0 + np.arange(S * H).reshape(S, 1, H, 1))              # another scale per set and row
    raw[1, :, :3] = 0                                                       # no support there, in set 1 alone
    op = pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=raw)
    assert op.n_map_sets == S and tuple(op.sens_maps.shape) == (S, n, H, W)
    assert op.sens_maps.dtype == (torch.complex128 if complex_maps else torch.float64)
    got = op.sens_maps.numpy()
    energy = (np.abs(got) ** 2).sum(1)                                      # over each set's OWN coils
    assert not got[1, :, :3].any()
    energy[1, :3] = 1.0
    np.testing.assert_allclose(energy, 1.0, atol=1e-12)
    keep = np.ones((S, 1, H, 1), dtype=bool)
    keep[1, :, :3] = False
    np.testing.assert_allclose(got, np.where(keep, unit, 0), atol=1e-13)
    dev = op.sens_dev("cpu")
    assert tuple(dev.shape) == (S, n, H, W) and dev.is_contiguous()
    assert dev.dtype == (torch.complex64 if complex_maps else torch.float32) and op.sens_dev("cpu") is dev
    # assignment after construction; three dims are the single set they always were
    op.sens_maps = unit[:2]
    assert op.n_map_sets == 2 and op.sens_dev("cpu").shape[0] == 2
    op.sens_maps = unit[0]
    assert op.n_map_sets == 1 and tuple(op.sens_maps.shape) == (n, H, W)
    one = pkg.uf.SENSE("exp", n, 8, 0.04, (1, H, W), seed=0)
    assert one.n_map_sets == 1
    for bad in (msh.map_sets(S, n + 1, H, W, complex_maps, 2), unit[None], unit[:, :, :8], unit[:, :, :, :16], unit[:0]):
        with pytest.raises(ValueError):
            pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=bad)
        with pytest.raises(ValueError):
            op.sens_maps = bad
    assert op.n_map_sets == 1                                               # a refused assignment changes nothing


def test_coil_count_is_read_from_the_coil_axis(pkg):
    """L2Penalty's K = n_coils * W must not become S * W"""
    S, n, H, W = 2, 5, 16, 16
    op = pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=msh.map_sets(S, n, H, W, True, 3))
    one = pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=msh.map_sets(1, n, H, W, True, 3)[0])
    prox, prox1 = pkg.prox.get_proximal("L2Penalty")(op), pkg.prox.get_proximal("L2Penalty")(one)
    assert prox.coef(2.0, 0.5, (4, 1, H, W)) == prox1.coef(2.0, 0.5, (4, 1, H, W)) == 0.05 * 4.0 / (n * W)


# ---- C ABI -----------------------------------------------------------------------------------------------
def _header_params(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ipdm.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/ipdm.h"
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", sorted(SETS_ENTRIES))
def test_sets_entries(pkg, name):
    sig, base = pkg.lib.SIGNATURES, SETS_ENTRIES[name]
    assert name in sig and hasattr(pkg.lib.lib, name)                       # in the table, exported by the built library
    params, base_params = _header_params(name), _header_params(base)
    assert len(sig[name]) == len(params) == len(base_params) + 2
    # `int sens_complex, int sens_sets` directly after sens; everything else is the single-set argument list
    i = params.index("const float* sens")
    assert params[i + 1:i + 3] == ["int sens_complex", "int sens_sets"]
    assert params[:i + 1] + params[i + 3:] == base_params
    assert sig[name][:i + 1] + sig[name][i + 3:] == sig[base]
    assert sig[name][i + 1:i + 3] == [pkg.lib.c_int, pkg.lib.c_int]


def test_abi_version_and_documentation(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    assert re.search(r"#define\s+IPDM_ABI_VERSION\s+4\b", header) and pkg.lib.lib.ipdm_abi_version() == 4   # additive
    assert "[sens_sets][n_coils][H][W]" in header and "b % sens_sets" in header


# ---- loader ----------------------------------------------------------------------------------------------
def test_load_kspace_stack(pkg, tmp_path):
    rng = np.random.default_rng(0)
    y = (rng.standard_normal((3, 4, 16, 16)) + 1j * rng.standard_normal((3, 4, 16, 16))).astype(np.complex64)
    np.save(tmp_path / "stack.npy", y)
    torch.save(torch.from_numpy(y), tmp_path / "stack.pt")
    np.save(tmp_path / "slice.npy", y[0])
    for name in ("stack.npy", "stack.pt"):
        got = pkg.load_data.load_kspace(str(tmp_path / name), slices=True)
        assert got.dtype == torch.complex64 and got.is_contiguous() and np.array_equal(got.numpy(), y)
    with pytest.raises(ValueError):
        pkg.load_data.load_kspace(str(tmp_path / "slice.npy"), slices=True)          # a 3-D file is no stack
    with pytest.raises(ValueError):
        pkg.load_data.load_kspace(str(tmp_path / "stack.npy"))                       # and a stack no single slice
    with pytest.raises(ValueError):
        pkg.load_data.load_kspace(str(tmp_path / "stack.npy"), cine=True, slices=True)
    np.save(tmp_path / "real.npy", np.abs(y))
    with pytest.raises(ValueError):
        pkg.load_data.load_kspace(str(tmp_path / "real.npy"), slices=True)
    assert np.array_equal(pkg.load_data.load_kspace(str(tmp_path / "slice.npy")).numpy(), y[0])       # as before


# ---- refusals before any GPU work ------------------------------------------------------------------------------
def test_build_problem_refuses_on_the_host(pkg, monkeypatch):
    """every shape, mask and calibration-region check of a stack comes before the score network is built"""
    def no_gpu_work(*a, **k):
        raise AssertionError("the score network was built before the host-side checks had finished")
    monkeypatch.setattr(pkg.engine, "build_scorenet", no_gpu_work)
    monkeypatch.setattr(pkg.engine, "acdc_config", no_gpu_work)
    dev, H, W = torch.device("cuda"), 16, 16
    rng = np.random.default_rng(1)
    y = torch.from_numpy((rng.standard_normal((3, 4, H, W)) + 1j * rng.standard_normal((3, 4, H, W))).astype(np.complex64))
    mask = torch.zeros(1, 1, W, dtype=torch.bool)
    mask[..., 5:11] = True
    maps = msh.map_sets(3, 4, H, W, True, 0)
    bp = lambda **kw: pkg.engine.build_problem(dev, 2, H=H, W=W, **kw)
    for bad in (y[0, 0], y[None], y[..., :8], y.real):                      # wrong rank, wrong side, not complex
        with pytest.raises(ValueError):
            bp(measurement=bad, mask=mask, sens_maps=maps)
    for bad_maps in (maps[:2], maps[:, :3], msh.map_sets(3, 4, H, 8, True, 0), maps[None]):
        with pytest.raises(ValueError):
            bp(measurement=y, mask=mask, sens_maps=bad_maps)
    with pytest.raises(ValueError):
        bp(measurement=y, mask=mask, sens_maps=maps, n_slices=3)            # n_slices simulates; the stack has its own S
    with pytest.raises(ValueError):
        bp(measurement=y[0], mask=mask, sens_maps=maps[0], n_slices=1)
    with pytest.raises(ValueError):
        bp(measurement=y, sens_maps=maps)                                   # no mask
    with pytest.raises(ValueError):
        bp(measurement=y, mask=mask)                                        # no maps and none to be estimated
    with pytest.raises(ValueError):
        bp(measurement=y, mask=mask, sens_maps=maps, estimate_maps=True)
    no_centre = torch.zeros(1, 1, W, dtype=torch.bool)
    no_centre[..., ::4] = True
    with pytest.raises(ValueError):
        bp(measurement=y, mask=no_centre, estimate_maps=True)               # no calibration region
    with pytest.raises(ValueError):
        bp(measurement=y, mask=mask, estimate_maps=True, coil_compress=5)   # more virtual than physical coils
    for bad_n in (0, -2, 1.5, True):
        with pytest.raises(ValueError):
            bp(n_slices=bad_n)
    with pytest.raises(ValueError):
        bp(n_slices=2, sens_maps=maps)                                      # three sets for two slices


def test_2dtime_classes_refuse_a_multi_set_operator(pkg):
    S, n, H, W, T = 2, 4, 16, 16, 3
    op = pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=msh.map_sets(S, n, H, W, True, 0))
    one = pkg.uf.SENSE("custom", n, 8, 0.04, (1, H, W), seed=0, sens_maps=msh.map_sets(1, n, H, W, True, 0)[0])
    sigmas, sigmas_T = torch.linspace(1.0, 0.01, 10), torch.linspace(0.5, 0.01, 6)
    prior = lambda: Namespace(config=Namespace(data=Namespace(channels=64)), sigmas=None)
    params = dict(n_steps_each=3, step_lr=9e-7, denoise=False, final_only=True)
    meas = torch.zeros(n, 1, T, 1, H, W, dtype=torch.complex64)
    make = lambda o: pkg.ald.ALD2DTime(pkg.prox.get_proximal("L2Penalty")(o), prior(), sigmas_T, (1, T, 1, H, W), None, sigmas,
                                       params, None, meas, o, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="coil-map sets"):
        make(op)
    assert make(one).linear_tfm is one                                      # one set: as before
    mp = dict(lr=1e-3, num_iters=1, win_size=8, prior_weight=1.0, spatial_step_weight=1.0, temporal_step_weight=1.0,
              mode_T="tv", if_random_shift=False, device=torch.device("cpu"))
    x0 = torch.zeros(1, T, 1, H, W, dtype=torch.complex64)
    with pytest.raises(ValueError, match="coil-map sets"):
        pkg.map.MAPOptimizer2DTime(x0, meas, None, prior(), op, None, mp)
    assert pkg.map.MAPOptimizer2DTime(x0, meas, None, prior(), one, None, mp).linear_tfm is one


@pytest.mark.parametrize("flags", [["--n_slices", "2"], ["--kspace", "stack.npy", "--slices", "--mask", "mask.npy",
                                                         "--estimate_maps"]])
def test_driver_refuses_a_stack_under_more_than_one_rank(tmp_path, flags):
    """RANK / WORLD_SIZE of a two-rank launch: the refusal comes up front -- no file is read, no GPU touched"""
    env = dict(os.environ, RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533",
               HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--image_size", "32",
                        "--num_samples", "2", "--save_dir", str(tmp_path / "out")] + flags,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode != 0 and "one process" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "out").exists()


def test_driver_flag_pairs(tmp_path):
    """--slices without --kspace, and --n_slices beside --kspace, end the driver at once"""
    np.save(tmp_path / "maps64.npy", msh.map_sets(1, 4, 64, 64, True, 0)[0])          # maps of another image size
    for flags in (["--slices"], ["--n_slices", "2", "--kspace", "x.npy", "--mask", "m.npy", "--estimate_maps"],
                  ["--n_slices", "0"], ["--n_slices", "2", "--image_size", "32", "--sens_maps", str(tmp_path / "maps64.npy")]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--save_dir",
                            str(tmp_path / "out")] + flags, capture_output=True, text=True, timeout=300, cwd=str(tmp_path),
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
        assert r.returncode != 0 and "slices" in r.stderr, (flags, r.stderr[-2000:])
        assert not (tmp_path / "out").exists()
