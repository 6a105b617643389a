"""Custom and 2-D k-space sampling masks, host side: the synthetic variable-density pattern, the broadcasting rules of
ops._mask_u8 (the reference's `mask * i2k_complex(X)` against a (B, 1, H, W) stack), the validating `.mask` property,
load_mask, and the C ABI's announcement of the [T][H][W] layout."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, ops, synthetic, engine
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
    return Namespace(lib=_lib, ops=ops, syn=synthetic, load=load_data, uf=uf, engine=engine)


# ---- vd_mask_2d ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,R", [(32, 32, 4), (16, 64, 8), (128, 128, 40)])
def test_vd_mask_2d(pkg, H, W, R):
    m = pkg.syn.vd_mask_2d(H, W, R, seed=3)
    assert m.dtype == torch.bool and tuple(m.shape) == (1, 1, H, W)
    assert int(m.sum()) == round(H * W / R)                                  # exactly, not on average
    bh, bw = max(2, round(0.04 * H)), max(2, round(0.04 * W))
    assert m[0, 0, H // 2 - bh // 2:H // 2 - bh // 2 + bh, W // 2 - bw // 2:W // 2 - bw // 2 + bw].all()
    assert torch.equal(m, pkg.syn.vd_mask_2d(H, W, R, seed=3))               # the seed decides
    assert not torch.equal(m, pkg.syn.vd_mask_2d(H, W, R, seed=4))
    # the density falls with the distance from the centre: the inner half of the rows holds most of the samples
    assert int(m[0, 0, H // 4:3 * H // 4].sum()) > 0.6 * int(m.sum())
    pf = pkg.syn.vd_mask_2d(H, W, R, seed=3, partial_fourier=0.75)
    cut = round(0.75 * H)
    assert not pf[0, 0, cut:].any() and torch.equal(pf[0, 0, :cut], m[0, 0, :cut])


def test_vd_mask_2d_block_larger_than_the_budget(pkg):
    m = pkg.syn.vd_mask_2d(32, 32, 4, center_frac=0.75)                      # 24 x 24 block > 256 samples
    assert int(m.sum()) == 24 * 24 and m[0, 0, 4:28, 4:28].all()


# ---- ops._mask_u8 -------------------------------------------------------------------------------------------------------
def _parent_mask_u8(mask, W):
    """what the package made of a line mask before it knew 2-D masks"""
    return (mask.reshape(-1, W) != 0).to(torch.uint8).contiguous()


def test_mask_u8_line_masks_map_as_before(pkg):
    H, W, T = 8, 16, 3
    g = torch.Generator().manual_seed(0)
    for shape in ((W,), (1, W), (1, 1, W), (T, 1, 1, W), (1, 1, 1, W)):
        for m in (torch.rand(shape, generator=g) < 0.4, (torch.rand(shape, generator=g) < 0.4).float(),
                  (torch.rand(shape, generator=g) < 0.4).to(torch.int64) * 7):
            got = pkg.ops._mask_u8(m, H, W, "cpu")
            want = _parent_mask_u8(m, W)
            assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (shape[0] if len(shape) == 4 else 1, W)
            assert torch.equal(got, want)
    # every mask the package generates
    for kw in (dict(), dict(mask_mode="uniform"), dict(mask_T=24)):
        op = pkg.uf.RandomUndersamplingFourier(8, 0.04, (1, 32, 32), seed=0, **kw)
        assert torch.equal(op.mask_u8("cpu"), _parent_mask_u8(op.mask, 32))
        assert op.mask_u8("cpu").dim() == 2


def test_mask_u8_2d_masks(pkg):
    H, W, T = 8, 16, 3
    g = torch.Generator().manual_seed(1)
    for shape in ((H, W), (1, H, W), (1, 1, H, W), (T, 1, H, W)):
        m = torch.rand(shape, generator=g) < 0.4
        got = pkg.ops._mask_u8(m, H, W, "cpu")
        t = shape[0] if len(shape) == 4 else 1
        assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (t, H, W)
        assert torch.equal(got.bool(), m.reshape(t, H, W))
    assert torch.equal(pkg.ops._mask_u8(np.ones((H, W), dtype=np.float64), H, W, "cpu"), torch.ones(1, H, W, dtype=torch.uint8))


@pytest.mark.parametrize("shape", [(3, 16), (5, 16), (1, 1, 7, 16), (1, 1, 9, 16), (3, 1, 4, 16),      # dim -2 neither 1 nor H
                                   (1, 2, 8, 16), (3, 2, 1, 16), (2, 8, 16), (3, 8, 16),               # channel dim != 1
                                   (8, 15), (1, 1, 17), (1, 1, 8, 1), (8,),                            # last dim != W
                                   (1, 1, 1, 8, 16), (0, 1, 8, 16), ()])
def test_mask_u8_refuses_what_does_not_broadcast(pkg, shape):
    with pytest.raises(ValueError):
        pkg.ops._mask_u8(torch.ones(shape, dtype=torch.bool), 8, 16, "cpu")


def test_mask_u8_refuses_complex(pkg):
    with pytest.raises(TypeError):
        pkg.ops._mask_u8(torch.ones(8, 16, dtype=torch.complex64), 8, 16, "cpu")


# ---- the operators ------------------------------------------------------------------------------------------------------
def test_mask_property(pkg):
    H, W = 16, 32
    op = pkg.uf.SENSE("exp", 3, 8, 0.04, (1, H, W), seed=0)
    ruf = op.random_under_fourier
    line = ruf.mask_u8("cpu")
    assert tuple(line.shape) == (1, W) and "cpu" in ruf._dev
    m = pkg.syn.vd_mask_2d(H, W, 4, seed=1)
    ruf.mask = m                                                             # after first use: the cached copy goes
    assert ruf._dev == {} and torch.equal(ruf.mask, m) and ruf.mask.dtype == torch.bool
    assert torch.equal(op.mask_u8("cpu"), m.reshape(1, H, W).to(torch.uint8))
    for good in (m.numpy(), m.float(), m.to(torch.int32), m[0, 0], torch.ones(W), torch.ones(5, 1, 1, W),
                 torch.ones(5, 1, H, W, dtype=torch.bool)):
        ruf.mask = good
        assert isinstance(ruf.mask, torch.Tensor) and tuple(ruf.mask.shape) == tuple(good.shape) and ruf._dev == {}
    ruf.mask = m
    for bad in (torch.ones(1, 1, H + 1, W), torch.ones(1, 1, H, W + 1), torch.ones(1, 2, H, W), torch.ones(3, W),
                np.ones((H // 2, W))):
        with pytest.raises(ValueError):
            ruf.mask = bad
    for bad in (torch.ones(H, W, dtype=torch.complex64), [[1] * W] * H, None):
        with pytest.raises(TypeError):
            ruf.mask = bad
    assert torch.equal(ruf.mask, m)                                          # a refused assignment changes nothing


def test_mask_mode_custom(pkg):
    H, W = 16, 32
    m = pkg.syn.vd_mask_2d(H, W, 4, seed=2)
    sc = pkg.uf.RandomUndersamplingFourier(4, 0.04, (1, H, W), seed=0, mask_mode="custom", mask=m)
    assert torch.equal(sc.mask, m) and tuple(sc.mask_u8("cpu").shape) == (1, H, W)
    op = pkg.uf.SENSE("exp", 3, 4, 0.04, (1, H, W), seed=0, mask_mode="custom", mask=m.numpy())
    assert torch.equal(op.random_under_fourier.mask, m)
    # R without generated-mask parameters is fine when the mask is given
    assert pkg.uf.RandomUndersamplingFourier(13, 0.04, (1, H, W), mask_mode="custom", mask=m).R == 13
    with pytest.raises(ValueError):
        pkg.uf.RandomUndersamplingFourier(4, 0.04, (1, H, W), seed=0, mask_mode="custom")
    with pytest.raises(ValueError):
        pkg.uf.SENSE("exp", 3, 4, 0.04, (1, H, W), seed=0, mask_mode="custom")
    with pytest.raises(ValueError):
        pkg.uf.RandomUndersamplingFourier(4, 0.04, (1, H, W), seed=0, mask=m)                 # mask= without the mode
    with pytest.raises(ValueError):
        pkg.uf.RandomUndersamplingFourier(4, 0.04, (1, H, W), seed=0, mask_mode="custom", mask=m[..., :-1])
    with pytest.raises(ValueError):
        pkg.uf.RandomUndersamplingFourier(4, 0.04, (1, H, W), seed=0, mask_mode="2d")


# ---- load_mask ----------------------------------------------------------------------------------------------------------
def test_load_mask_round_trip(pkg, tmp_path):
    m = pkg.syn.vd_mask_2d(16, 32, 4, seed=7)
    np.save(tmp_path / "m.npy", m.numpy())
    torch.save(m, tmp_path / "m.pt")
    torch.save(m[0, 0].float(), tmp_path / "f.pt")
    for name, want in (("m.npy", m), ("m.pt", m), ("f.pt", m[0, 0].float())):
        got = pkg.load.load_mask(str(tmp_path / name))
        assert got.dtype == want.dtype and torch.equal(got, want)
    with pytest.raises(ValueError):
        pkg.load.load_mask(str(tmp_path / "m.txt"))
    np.save(tmp_path / "c.npy", np.ones((16, 32), dtype=np.complex64))
    with pytest.raises(TypeError):
        pkg.load.load_mask(str(tmp_path / "c.npy"))
    # the drivers' flags
    assert pkg.load.driver_mask(None, False, 16, 32, 4, 0) is None
    assert torch.equal(pkg.load.driver_mask(None, True, 16, 32, 4, 7), m)
    assert torch.equal(pkg.load.driver_mask(str(tmp_path / "m.npy"), False, 16, 32, 4, 0), m)
    np.save(tmp_path / "t.npy", np.ones((3, 16, 32), dtype=bool))                             # per-frame (T, H, W)
    assert tuple(pkg.load.driver_mask(str(tmp_path / "t.npy"), False, 16, 32, 4, 0).shape) == (3, 1, 16, 32)
    with pytest.raises(ValueError):
        pkg.load.driver_mask(str(tmp_path / "m.npy"), True, 16, 32, 4, 0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------
MASK_ENTRIES = ["ipdm_sense_forward_c64", "ipdm_sense_adjoint_c64", "ipdm_sense_l2prox_f32", "ipdm_ald_sense_step_f32",
                "ipdm_sense_forward_csm_c64", "ipdm_sense_adjoint_csm_c64", "ipdm_sense_l2prox_csm_f32",
                "ipdm_ald_sense_step_csm_f32", "ipdm_sense_cgprox_f32", "ipdm_sense_cgprox_csm_f32",
                "ipdm_ald_sense_cg_step_f32", "ipdm_ald_sense_cg_step_csm_f32", "ipdm_singlecoil_prox_f32",
                "ipdm_ald_singlecoil_step_f32"]


def _header():
    return open(os.path.join(REPO, "include", "ipdm.h")).read()


def test_abi_announces_the_2d_layout(pkg):
    """the fourteen (mask, mask_t) entry points keep their signatures (a negative mask_t carries the layout), so the
    version stays; ipdm_mask_layouts() is how a caller of the C ABI learns that the library takes [T][H][W] masks"""
    header = _header()
    assert re.search(r"#define\s+IPDM_ABI_VERSION\s+4\b", header) and pkg.lib.lib.ipdm_abi_version() == 4
    assert re.search(r"#define\s+IPDM_MASK_LINES\s+1\b", header) and re.search(r"#define\s+IPDM_MASK_2D\s+2\b", header)
    assert re.search(r"\bint\s+ipdm_mask_layouts\s*\(\s*void\s*\)\s*;", header)
    assert pkg.lib.SIGNATURES["ipdm_mask_layouts"] == [] and hasattr(pkg.lib.lib, "ipdm_mask_layouts")
    assert pkg.lib.lib.ipdm_mask_layouts() == 3
    assert "[T][H][W]" in header and "mask_t = -T" in header


@pytest.mark.parametrize("name", MASK_ENTRIES)
def test_abi_mask_entries_unchanged(pkg, name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    i = args.index("const uint8_t* mask")
    assert args[i + 1] == "int mask_t"
    sig = pkg.lib.SIGNATURES[name]
    assert len(sig) == len(args) and sig[i] is pkg.lib.P and sig[i + 1] is pkg.lib.c_int and hasattr(pkg.lib.lib, name)


def test_build_problem_takes_a_mask():
    import inspect
    from inverseproblemwithdiffusionmodel_amd import engine
    assert inspect.signature(engine.build_problem).parameters["mask"].default is None
