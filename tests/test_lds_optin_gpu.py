"""The dynamic-LDS opt-in (csrc/launch.h): hipFuncSetAttribute is called once per (kernel instantiation, device, size above what
was granted before) and never again, counted by `ipdm_debug_lds_optin_count` in ONE fresh process (the count is per process, and
any other test of the session may have launched these kernels already).  Run as a script (`python tests/test_lds_optin_gpu.py
OUT.json`) this file is the child: it makes the calls below in order and writes, per call, the counter after it, the error against
float64 on the CPU and the bound.  The parent asserts:
  * `ops.fft2c`, B = 2, at 64x64, 64x128, 128x128, 64x128, 128x128 (one instantiation; image + twiddles: under 64 KiB, over it,
    larger, smaller than granted, as granted): the counter reads 0, 1, 2, 2, 2; every result within test_kernels_gpu.
    test_fft2c_sizes' bound, max(2e-5 * sqrt(H W) / 32, 5e-6);
  * the 1-D Winograd convolution at test_wino1d_gpu's smallest shape, one output: +1 (not one per instantiation of the family),
    a repeat +0; within that file's 1e-6 * max|ref|;
  * `conv2d_wino_bx3` at 16x16, 256 -> 256 (the HALF form): +1, a repeat +0; within test_wino16_gpu's 4e-6 * max|ref| per image;
  * with a second device visible, the 1-D Winograd call again on device 1: +1 (the attribute is per device), same bound.
A child that dies by signal, exits 134 / 139 / 124 / 137 or times out fails the module without a retry."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
CHILD_TIMEOUT = 60
FFT_SIZES = [(64, 64), (64, 128), (128, 128), (64, 128), (128, 128)]
WINO1D_SHAPE = (1, 32, 128, 8, 32)                  # test_wino1d_gpu.SHAPES[0]


def _fft2c_ref(x):
    k = torch.fft.fftn(torch.fft.ifftshift(x.to(torch.complex128), dim=(-1, -2)), dim=(-1, -2), norm="ortho")
    return torch.fft.fftshift(k, dim=(-1, -2))


def _child(out_path):
    sys.path.insert(0, REPO)
    from inverseproblemwithdiffusionmodel_amd import _lib, ops
    count = _lib.lib.ipdm_debug_lds_optin_count
    res = dict(start=int(count()), fft=[], devices=torch.cuda.device_count())
    gen = torch.Generator().manual_seed(4)
    for H, W in FFT_SIZES:
        x = torch.complex(torch.randn(2, H, W, generator=gen), torch.randn(2, H, W, generator=gen))
        k = ops.fft2c(x.cuda()).cpu()
        res["fft"].append(dict(count=int(count()), err=float((k.to(torch.complex128) - _fft2c_ref(x)).abs().max()),
                               bound=max(2e-5 * (H * W) ** 0.5 / 32, 5e-6)))

    def wino1d(device):
        B, Cin, Cout, H, W = WINO1D_SHAPE
        gen = torch.Generator().manual_seed(7)                              # test_wino1d_gpu._case
        x = torch.randn(B, Cin, H, W, generator=gen)
        w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (3 * Cin ** 0.5)
        b = torch.randn(Cout, generator=gen)
        r = torch.randn(B, Cout, H, W, generator=gen)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + r.double()
        with torch.cuda.device(device):
            xd, bd, rd = x.cuda(), b.cuda(), r.cuda()
            U = ops.conv_wino1d_weight(w.cuda())
            out = []
            for _ in range(2):
                y = ops.conv2d_wino_bx3(xd, U, bd, rd).cpu()
                out.append(dict(count=int(count()), err=float((y.double() - ref).abs().max() / ref.abs().max()), bound=1e-6))
        return out
    res["wino1d"] = wino1d(0)

    gen = torch.Generator().manual_seed(16)                                 # inputs as test_wino16_gpu._inputs
    x = F.elu(torch.randn(3, 256, 16, 16, generator=gen)) * (10.0 ** torch.linspace(-3, 3, 3)).view(3, 1, 1, 1)
    w = torch.randn(256, 256, 3, 3, generator=gen) / (9 * 256) ** 0.5
    b = torch.randn(256, generator=gen)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert ops.wino_hx2_form(256, 256, 16, 16, 1) == ops.WINO_FORM_HALF
    xd, bd, U = x.cuda(), b.cuda(), ops.conv_wino_bx3_weight(w.cuda(), fmt="hx2")
    res["half"] = []
    for _ in range(2):
        y = ops.conv2d_wino_bx3(xd, U, bd, dilation=1, in_amax=True).cpu()
        err = (y.double() - ref).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))
        res["half"].append(dict(count=int(count()), err=float(err.max()), bound=4e-6))
    if res["devices"] >= 2:
        res["wino1d_dev1"] = wino1d(1)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lds_optin") / "out.json")
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=REPO, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"child: timeout after {CHILD_TIMEOUT} s")
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        pytest.fail(f"child: exit status {p.returncode}\n" + p.stderr[-3000:])
    assert p.returncode == 0, p.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    print(json.dumps(res))
    return res


def _within(entries):
    for e in entries:
        assert e["err"] <= e["bound"], e


def test_fft2c_asks_once_per_larger_size(child):
    assert child["start"] == 0
    assert [e["count"] for e in child["fft"]] == [0, 1, 2, 2, 2]
    _within(child["fft"])


def test_wino1d_asks_for_the_launched_instantiation_only(child):
    before = child["fft"][-1]["count"]
    assert [e["count"] - before for e in child["wino1d"]] == [1, 1]
    _within(child["wino1d"])


def test_wino_bx3_half_asks_once(child):
    before = child["wino1d"][-1]["count"]
    assert [e["count"] - before for e in child["half"]] == [1, 1]
    _within(child["half"])


def test_second_device_asks_again(child):
    if child["devices"] < 2:
        pytest.skip("one device visible")
    before = child["half"][-1]["count"]
    assert [e["count"] - before for e in child["wino1d_dev1"]] == [1, 1]
    _within(child["wino1d_dev1"])


if __name__ == "__main__":
    _child(sys.argv[1])
