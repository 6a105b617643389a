"""The SENSE drivers with --proximal_type: L2PenaltyCG runs end to end and fits the measurement better than the one-step
L2Penalty of the same command; an unknown name is refused before any GPU work.  Sizes and level counts are those of
tests/test_scripts_gpu.py; children are fresh processes."""
import os
import pickle
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_script(name, args, timeout=900):
    """scripts/<name> with `args` as one fresh process -> (returncode, stdout, stderr)"""
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", name)] + [str(a) for a in args], capture_output=True,
                       text=True, cwd=REPO, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def _data_error(out):
    m = re.search(r"data error \|\|A x - y\|\|\^2 = ([0-9.eE+-]+)", out)
    assert m, out[-1500:]
    return float(m.group(1))


def test_acdc_driver_honours_proximal_type(tmp_path):
    common = ["--R", 40, "--num_samples", 2, "--num_sens", 4, "--seed", 0, "--seg_start_time", 1.0, "--n_levels", 2,
              "--lr_scaled", 1111111]
    d_cg, d_l2 = str(tmp_path / "cg"), str(tmp_path / "l2")
    rc, out_cg, err = run_script("acdc_SENSE_real_img.py", common + ["--proximal_type", "L2PenaltyCG", "--cg_iters", 8,
                                                                    "--save_dir", d_cg])
    assert rc == 0, err[-3000:]
    rc, out_l2, err = run_script("acdc_SENSE_real_img.py", common + ["--proximal_type", "L2Penalty", "--save_dir", d_l2])
    assert rc == 0, err[-3000:]
    for d in (d_cg, d_l2):
        for n in ("original.pt", "measurement.pt", "reconstructions.pt", "ZF.pt", "mask.pt", "args_dict.pkl"):
            assert os.path.exists(os.path.join(d, n)), (d, n)
    rec = torch.load(os.path.join(d_cg, "reconstructions.pt"), weights_only=False)
    assert rec.shape == (2, 1, 128, 128) and rec.dtype == torch.complex64 and torch.isfinite(torch.view_as_real(rec)).all()
    with open(os.path.join(d_cg, "args_dict.pkl"), "rb") as f:
        a = pickle.load(f)
    assert a["proximal_type"] == "L2PenaltyCG" and a["cg_iters"] == 8 and a["cg_tol"] == 1e-5
    with open(os.path.join(d_l2, "args_dict.pkl"), "rb") as f:
        a = pickle.load(f)
    assert a["proximal_type"] == "L2Penalty" and a["cg_iters"] == 10 and a["cg_tol"] == 1e-5       # the defaults, recorded
    e_cg, e_l2 = _data_error(out_cg), _data_error(out_l2)
    print("data error: L2PenaltyCG", e_cg, "L2Penalty", e_l2)
    assert e_cg < e_l2
    assert not torch.equal(rec, torch.load(os.path.join(d_l2, "reconstructions.pt"), weights_only=False))


def test_cine_driver_runs_with_cg(tmp_path):
    d = str(tmp_path)
    rc, out, err = run_script("cine_SENSE_real_img_2d_time.py",
                              ["--R", 8, "--num_samples", 1, "--mode_T", "diffusion1d", "--lamda_T", 10.0, "--image_size", 64,
                               "--start_level", 996, "--n_levels", 2, "--proximal_type", "L2PenaltyCG", "--cg_iters", 6,
                               "--lr_scaled", 10000, "--save_dir", d])
    assert rc == 0, err[-3000:]
    assert "reconstruction time" in out
    rec = torch.load(os.path.join(d, "reconstructions.pt"), weights_only=False)
    assert rec.shape == (1, 24, 1, 64, 64) and rec.dtype == torch.complex64 and torch.isfinite(torch.view_as_real(rec)).all()
    with open(os.path.join(d, "args_dict.pkl"), "rb") as f:
        a = pickle.load(f)
    assert a["proximal_type"] == "L2PenaltyCG" and a["cg_iters"] == 6 and a["cg_tol"] == 1e-5


@pytest.mark.parametrize("script", ["acdc_SENSE_real_img.py", "cine_SENSE_real_img_2d_time.py"])
def test_bogus_proximal_type_is_refused(tmp_path, script):
    rc, out, err = run_script(script, ["--proximal_type", "L2PenaltyGC", "--save_dir", str(tmp_path)], timeout=120)
    assert rc != 0 and "proximal_type" in err
    assert not os.listdir(str(tmp_path))                                     # refused by argparse, before any work
