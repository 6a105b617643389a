"""Every arm of the 2-D Winograd launcher's `switch (plan.form)` (csrc/conv_wino_bx3.hip, csrc/wino_plan.h) once, through
ops.conv2d_wino_bx3 at the smallest shape that selects it, against the float64 convolution within 4e-6 * max |reference| -- the
bound tests/test_kernels_gpu.py sets for these kernels in both operand families (test_wino_bx3_split_k,
test_wino_bx3_dilated_16px_polyphase, test_conv_wino_bx3_pooled_epilogue).  Each case first asserts what the library's shape
queries say about it, so that a shape that selects another form fails there.  The queries tell POLY / HALF / CO32 / the rest
(_hx2_form), split-K (_splitk) and the statistics epilogue (_stats_partials; 0 on every small form and on the
one-workgroup-per-tile form) apart; that 160 (image, channel tile) pairs is where the 8 x 8 block form takes over from the
register-staged one, and that an input off a 16-byte boundary gets the dword forms, is the plan's rule, swept on the host by
tests/host/wino_plan_main.cpp.  One process, no children; the switches are at their defaults."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert not [k for k in os.environ if k.startswith("IPDM_WBX3_")], "this module tests the default switches"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    assert _ops.WBX3_CO32
    return _ops


@functools.lru_cache(maxsize=None)
def _layer(B, Cin, Cout, H, W, dil):
    """inputs and the float64 convolution (+ bias) of one layer shape, shared read-only by the cases that use it"""
    gen = torch.Generator().manual_seed(B * 1000 + Cin + H + 3 * W + dil)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=gen)
    r = torch.randn(B, Cout, H, W, generator=gen)
    return x, w, b, r, F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil)


def _off16(t, k=1):
    """a contiguous GPU copy of t that starts k floats past a 16-byte boundary, inside a larger buffer"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    lead = (-buf.data_ptr() % 16) // 4 + k
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k and v.is_contiguous()
    return v


def _close(name, got, want):
    err, top = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
    print(f"{name}: max error {err:.3e} = {err / top:.2e} of max |reference| (bound 4e-6)")
    assert err <= 4e-6 * top, (name, err, top)


# form, fmt, B, Cin, Cout, H, W, dilation, input offset (floats past a 16-byte boundary)
PLAIN = [
    ("POLY", "hx2", 2, 32, 64, 16, 16, 2, 0), ("POLY", "bx3", 2, 32, 64, 16, 16, 2, 0),
    ("HALF", "hx2", 2, 32, 64, 16, 16, 1, 0),
    ("CO32", "hx2", 2, 32, 64, 8, 16, 1, 0),
    ("SMALL_DMA", "bx3", 160, 32, 64, 16, 16, 1, 0), ("SMALL_DMA", "bx3", 160, 32, 64, 16, 16, 1, 1),     # 16-byte / dword DMA
    ("SMALL_REG", "bx3", 2, 32, 64, 16, 16, 1, 0),
    ("SMALL_REG", "hx2", 2, 32, 64, 32, 32, 2, 0), ("SMALL_REG", "bx3", 2, 32, 64, 32, 32, 2, 0),
    ("TILE", "hx2", 2, 16, 64, 32, 32, 1, 0), ("TILE", "bx3", 2, 16, 64, 32, 32, 1, 0),
    ("WIDE", "hx2", 2, 32, 64, 32, 32, 1, 0), ("WIDE", "bx3", 2, 32, 64, 32, 32, 1, 0),                   # 16-byte DMA
    ("WIDE", "hx2", 2, 32, 64, 32, 34, 1, 0), ("WIDE", "bx3", 2, 32, 64, 32, 34, 1, 0),                   # W % 4: dword DMA
    ("KSPLIT", "bx3", 2, 64, 64, 16, 16, 1, 0),
]


def _assert_queries(ops, form, fmt, Cin, Cout, H, W, dil):
    from inverseproblemwithdiffusionmodel_amd import _lib
    assert ops.conv_wino_bx3_supported(Cin, Cout, H, W, dil)
    hx_form = {"POLY": ops.WINO_FORM_POLY, "HALF": ops.WINO_FORM_HALF, "CO32": ops.WINO_FORM_CO32}
    if fmt == "hx2" or form == "POLY":                          # (POLY comes first for both families)
        assert ops.wino_hx2_form(Cin, Cout, H, W, dil) == hx_form.get(form, ops.WINO_FORM_OTHER)
    assert ops.wino_bx3_splitk(Cin, Cout, H, W, dil) == (2 if form == "KSPLIT" else 1)
    partials = [int(_lib.lib.ipdm_conv2d_wino_bx3_stats_partials(Cin, Cout, H, W, dil, p)) for p in (0, 1)]
    wide4 = form == "WIDE" and W % 4 == 0
    assert partials == ([2 * ((W + 31) // 32) * ((H + 7) // 8)] * 2 if wide4 else [0, 0]), partials


@pytest.mark.parametrize("form,fmt,B,Cin,Cout,H,W,dil,off", PLAIN)
def test_plain_forms(ops, form, fmt, B, Cin, Cout, H, W, dil, off):
    _assert_queries(ops, form, fmt, Cin, Cout, H, W, dil)
    x, w, b, r, conv = _layer(B, Cin, Cout, H, W, dil)
    U = ops.conv_wino_bx3_weight(w.cuda(), fmt=fmt)
    xd = _off16(x, off) if off else x.cuda()
    assert xd.data_ptr() % 16 == 4 * off
    out, act = ops.conv2d_wino_bx3(xd, U, b.cuda(), r.cuda(), act_out=ops.ACT_ELU, dilation=dil)
    _close(f"{form} {fmt} raw", out, conv + r.double())
    _close(f"{form} {fmt} act", act, F.elu(conv + r.double()))


@pytest.mark.parametrize("W", [32, 34])
@pytest.mark.parametrize("fmt", ["hx2", "bx3"])
def test_wide_pooled(ops, fmt, W):
    B, Cin, Cout, H = 2, 32, 64, 32
    _assert_queries(ops, "WIDE", fmt, Cin, Cout, H, W, 1)
    x, w, b, r, conv = _layer(B, Cin, Cout, H, W, 1)
    rp = r[..., :H // 2, :W // 2].contiguous()
    U = ops.conv_wino_bx3_weight(w.cuda(), fmt=fmt)
    out, act = ops.conv2d_wino_bx3(x.cuda(), U, b.cuda(), rp.cuda(), act_out=ops.ACT_ELU, pool2=True)
    want = F.avg_pool2d(conv, 2) + rp.double()
    _close(f"WIDE pooled {fmt} W={W} raw", out, want)
    _close(f"WIDE pooled {fmt} W={W} act", act, F.elu(want))


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("fmt", ["hx2", "bx3"])
def test_wide_statistics(ops, fmt, pool):
    B, Cin, Cout, H, W = 2, 32, 64, 32, 32
    _assert_queries(ops, "WIDE", fmt, Cin, Cout, H, W, 1)
    x, w, b, r, conv = _layer(B, Cin, Cout, H, W, 1)
    rp = r[..., :H // 2, :W // 2].contiguous() if pool else r
    U = ops.conv_wino_bx3_weight(w.cuda(), fmt=fmt)
    out = ops.conv2d_wino_bx3(x.cuda(), U, b.cuda(), rp.cuda(), pool2=pool, want_stats=True)
    assert hasattr(out, "_ipdm_partials"), "the statistics epilogue did not run"
    part = out._ipdm_partials[0]
    oh, ow = (H // 2, W // 2) if pool else (H, W)
    assert tuple(part.shape) == (B, Cout, 8, 3) and float(part[..., 0].sum(dim=2).min()) == oh * ow == float(part[..., 0].sum(dim=2).max())
    _close(f"WIDE stats {fmt} pool={pool}", out, (F.avg_pool2d(conv, 2) if pool else conv) + rp.double())
