"""The starved 16 x 16 layers of the score network on the persistent 2-D Winograd kernel (csrc/conv_wino_bx3.hip, f16x2 family):
the undilated 256 -> 256 and 512 -> 256 layers as (image, upper / lower eight rows, 64 channels) workgroups (HALF) and the
dilated ones on the polyphase form (POLY), with plain / residual / two-output epilogues, dynamic input range and per-image maxima:
  (i)   against a float64 convolution: max error <= 4e-6 of max |reference| (the bound test_kernels_gpu.py sets for these kernels);
  (ii)  bit-identical to the path `IPDM_WBX3_HALF=0` selects (32-channel workgroups, CO32), computed in a child process;
  (iii) a sample's bits do not depend on the batch around it (B = 1, 5, 28 and slices);
  (iv)  the per-image maxima of what was stored are exact;
  (v)   the dispatch rule (ops.wino_hx2_form) returns HALF for exactly the undilated 16 x 16 layers with fewer than 512 output
        channels, and what it returned before everywhere else.
Run as a script (`python tests/test_wino16_gpu.py OUTDIR`) it is that child: it writes every case's results to OUTDIR."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, B, Cin, Cout, dilation): the six 16 x 16 shapes of NCSNv2Deepest's census, and the production batch on the commonest one
CASES = [("c256_256_d1", 5, 256, 256, 1), ("c512_512_d4", 5, 512, 512, 4), ("c512_512_d2", 5, 512, 512, 2),
         ("c256_512_d2", 5, 256, 512, 2), ("c512_256_d1", 5, 512, 256, 1), ("c256_256_d2", 5, 256, 256, 2),
         ("ragged_256_256_d1", 28, 256, 256, 1)]
EPILOGUES = ["plain", "residual", "two_output"]
# (Cin, Cout, H, W, dilation) -> form name, with the switches at their defaults
FORMS = [((256, 256, 16, 16, 1), "HALF"), ((512, 256, 16, 16, 1), "HALF"), ((64, 64, 16, 16, 1), "HALF"),
         ((32, 448, 16, 16, 1), "HALF"), ((128, 128, 8, 16, 1), "CO32"), ((256, 128, 16, 12, 1), "CO32"),
         ((256, 256, 16, 8, 1), "CO32"), ((256, 512, 16, 16, 1), "OTHER"), ((512, 512, 16, 16, 1), "OTHER"),
         ((16, 64, 16, 16, 1), "OTHER"), ((256, 256, 32, 32, 1), "OTHER"), ((128, 128, 128, 128, 1), "OTHER"),
         ((256, 256, 16, 16, 2), "POLY"), ((256, 512, 16, 16, 2), "POLY"), ((512, 512, 16, 16, 2), "POLY"),
         ((512, 512, 16, 16, 4), "POLY"), ((64, 64, 24, 16, 2), "OTHER")]


def _inputs(name, B, Cin, Cout):
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = F.elu(torch.randn(B, Cin, 16, 16, generator=gen)) * (10.0 ** torch.linspace(-3, 3, B)).view(B, 1, 1, 1)   # every image its own range
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=gen)
    r = torch.randn(B, Cout, 16, 16, generator=gen)
    return x.cuda(), w.cuda(), b.cuda(), r.cuda()


def _run(ops, U, x, b, r, dil, epi):
    """-> {out[, act], amax_out[, amax_act]} on the GPU"""
    kw = dict(dilation=dil, in_amax=True, want_amax=True)
    if epi == "two_output":
        out, act = ops.conv2d_wino_bx3(x, U, b, r, act_out=ops.ACT_ELU, **kw)
        return dict(out=out, act=act, amax_out=ops.amax_value(ops.amax_of(out)), amax_act=ops.amax_value(ops.amax_of(act)))
    out = ops.conv2d_wino_bx3(x, U, b, r if epi == "residual" else None, **kw)
    return dict(out=out, amax_out=ops.amax_value(ops.amax_of(out)))


def _form_names(ops):
    names = {ops.WINO_FORM_OTHER: "OTHER", ops.WINO_FORM_CO32: "CO32", ops.WINO_FORM_HALF: "HALF", ops.WINO_FORM_POLY: "POLY"}
    return {",".join(map(str, shape)): names.get(ops.wino_hx2_form(*shape)) for shape, _ in FORMS}


def _child(outdir):
    sys.path.insert(0, REPO)
    from inverseproblemwithdiffusionmodel_amd import ops
    for name, B, Cin, Cout, dil in CASES:
        x, w, b, r = _inputs(name, B, Cin, Cout)
        U = ops.conv_wino_bx3_weight(w, fmt="hx2")
        for epi in EPILOGUES:
            got = _run(ops, U, x, b, r, dil, epi)
            np.savez(os.path.join(outdir, f"{name}_{epi}.npz"), **{k: v.cpu().numpy() for k, v in got.items()})
    with open(os.path.join(outdir, "forms.json"), "w") as f:
        json.dump(_form_names(ops), f)


@pytest.fixture(scope="module")
def ops():
    from inverseproblemwithdiffusionmodel_amd import ops as o
    assert os.environ.get("IPDM_WBX3_HALF", "1") != "0" and o.WBX3_CO32, "this module tests the default dispatch"
    return o


@pytest.fixture(scope="module")
def old_path(tmp_path_factory):
    """every case through the path IPDM_WBX3_HALF=0 selects, from a fresh process (the switch is read once per process)"""
    outdir = str(tmp_path_factory.mktemp("wino16_old"))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), outdir], env=dict(os.environ, IPDM_WBX3_HALF="0"), cwd=REPO,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return outdir


@pytest.fixture(scope="module")
def layer():
    """(inputs, weights) of a case, built once per module"""
    cache = {}

    def get(ops, name, B, Cin, Cout):
        if name not in cache:
            cache.clear()                                      # one case resident at a time
            x, w, b, r = _inputs(name, B, Cin, Cout)
            cache[name] = (x, w, b, r, ops.conv_wino_bx3_weight(w, fmt="hx2"))
        return cache[name]
    return get


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("name,B,Cin,Cout,dil", CASES)
def test_wino16_layers(ops, old_path, layer, name, B, Cin, Cout, dil, epi):
    x, w, b, r, U = layer(ops, name, B, Cin, Cout)
    got = _run(ops, U, x, b, r, dil, epi)
    out = got["out"]
    # (i) float64 reference, image by image (each image has its own range: its own bound)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil)
    if epi != "plain":
        ref = ref + r.double()
    err = (out.double() - ref).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))
    print(f"{name} {epi}: max error / max |reference| per image: worst {err.max().item():.3e}")
    assert err.max().item() <= 4e-6
    if epi == "two_output":
        erra = (got["act"].double() - F.elu(ref)).abs().amax(dim=(1, 2, 3)) / ref.abs().amax(dim=(1, 2, 3))
        print(f"{name} {epi}: activated copy: worst {erra.max().item():.3e}")
        assert erra.max().item() <= 4e-6
    # (ii) the same bits as the path the switch restores
    old = np.load(os.path.join(old_path, f"{name}_{epi}.npz"))
    assert sorted(old.files) == sorted(got)
    for k, v in got.items():
        assert np.array_equal(v.cpu().numpy(), old[k]), f"{k} differs from the IPDM_WBX3_HALF=0 path"
    # (iii) a sample's bits do not depend on its batch
    for lo, hi in sorted({(0, 1), (B - 1, B), (0, min(5, B)), (1, 3)}):
        part = _run(ops, U, x[lo:hi].contiguous(), b, r[lo:hi].contiguous(), dil, epi)
        for k, v in part.items():
            assert torch.equal(v, got[k][lo:hi]), f"{k} of images {lo}:{hi} depends on the batch"
    # (iv) per-image maxima of what was stored, exactly
    assert torch.equal(got["amax_out"], out.abs().amax(dim=(1, 2, 3)))
    if epi == "two_output":
        assert torch.equal(got["amax_act"], got["act"].abs().amax(dim=(1, 2, 3)))


def test_wino16_dispatch_rule(ops, old_path):
    """(v) HALF for the undilated 16 x 16 layers with fewer than 512 output channels and at least two chunks, nothing else moved;
    with the switch off those layers are CO32 again; the host's split-K rule and its CO32 switch keep their meaning"""
    now = _form_names(ops)
    with open(os.path.join(old_path, "forms.json")) as f:
        off = json.load(f)
    for shape, want in FORMS:
        key = ",".join(map(str, shape))
        assert now[key] == want, (shape, now[key])
        assert off[key] == ("CO32" if want == "HALF" else want), (shape, off[key])
    assert ops.wino_hx2_form(256, 256, 16, 16) == ops.wino_hx2_form(256, 256, 16, 16, 1) == ops.WINO_FORM_HALF
    assert ops.wino_hx2_form(256, 256, 15, 16) is None          # odd image: no Winograd kernel
    assert ops.wino_bx3_splitk(256, 256, 16, 16) == 2 and ops.wino_bx3_splitk(512, 256, 16, 16) == 2
    assert ops.wino_bx3_splitk(256, 512, 16, 16) == 1 and ops.wino_bx3_splitk(256, 256, 16, 16, 2) == 1


if __name__ == "__main__":
    _child(sys.argv[1])
