"""Kernel forms chosen by pointer alignment.  The C ABI accepts any contiguous tensor on its element's natural boundary;
16-byte alignment only selects faster forms (float4 rows, 16-byte LDS-DMA, the 1-D Winograd kernel, statistics epilogues).  Every
operation here is handed a contiguous view that starts 4, 8 or 12 bytes past a 16-byte boundary, inside a buffer whose slack is
NaN on both sides:
  * a kernel that rounds the pointer down, or reads a vector across the end, poisons its result instead of passing by luck;
  * for operands a kernel WRITES (`out=`, in-place state) the slack must still be all NaN afterwards (no out-of-bounds store).
One operand is misaligned at a time, then all together.  Bounds are the ones the existing test of the same operation asserts on
its aligned path (named at each test); where the misaligned form is the same per-element arithmetic the result must be
bit-identical to the aligned call, where it is another kernel (another summation order) the bits are only printed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import state_dict_from_golden
from oracle import kspace, resample, scorenet

pytestmark = pytest.mark.gpu
SLACK = 64                                                  # elements of NaN on each side (a multiple of every 16 / itemsize)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


class Mis:
    """a contiguous GPU copy of `t` that starts k elements past a 16-byte boundary, NaN all around"""

    def __init__(self, t, k=1):
        t = torch.as_tensor(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
        n, item = t.numel(), t.element_size()
        fill = complex(float("nan"), float("nan")) if t.is_complex() else float("nan")
        self.buf = torch.full((n + 2 * SLACK,), fill, dtype=t.dtype, device="cuda")
        lead = (-self.buf.data_ptr() % 16) // item          # elements up to the first 16-byte boundary of the buffer
        assert (self.buf.data_ptr() + lead * item) % 16 == 0
        self.lo, self.hi = lead + 16 // item + k, lead + 16 // item + k + n
        self.t = self.buf[self.lo:self.hi].view(t.shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (item * k) % 16 != 0, (self.t.data_ptr() % 16, item, k)
        self.t.copy_(t)

    def slack_untouched(self):
        return bool(torch.isnan(torch.view_as_real(self.buf[:self.lo]) if self.buf.is_complex() else self.buf[:self.lo]).all()
                    and torch.isnan(torch.view_as_real(self.buf[self.hi:]) if self.buf.is_complex() else self.buf[self.hi:]).all())


def mis(t, k=1):
    return Mis(t, k).t


def variants(names):
    """one operand at a time, then all together"""
    return [frozenset([n]) for n in names] + ([frozenset(names)] if len(names) > 1 else [])


def test_helper_really_misaligns(ops):
    for dt, ks in ((torch.float32, (1, 2, 3)), (torch.float16, (2, 4, 6)), (torch.float64, (1,)), (torch.complex64, (1,))):
        for k in ks:
            src = torch.arange(24, dtype=torch.float32).to(dt).view(2, 3, 4)
            m = Mis(src, k)
            assert m.t.data_ptr() % 16 == (k * src.element_size()) % 16 and m.t.data_ptr() % 16 != 0
            assert torch.equal(m.t.cpu(), src) and m.slack_untouched()
            m.buf[m.hi] = 0
            assert not m.slack_untouched()


# ---- element-wise: the same arithmetic per element, so the same bits ------------------------------------------------------
@pytest.mark.parametrize("n_extra", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_elementwise_bit_identical(ops, n_extra, k):
    """affine_act, act, add, scale_shift, axpby, sample_axpy2, div_sigma, axpy_sched on planes of 4k and 4k+1..3 elements:
    bit-identical to the aligned call whichever operand (inputs, `out=`) is off the boundary; the slack of `out` stays NaN"""
    gen = torch.Generator().manual_seed(100 + n_extra)
    B, C, HW = 3, 2, 4 * 37 + n_extra
    x = (torch.randn(B, C, 1, HW, generator=gen) * 2).cuda()
    y = torch.randn(B, C, 1, HW, generator=gen).cuda()
    z = torch.randn(B, C, 1, HW, generator=gen).cuda()
    coef = torch.randn(B, C, 3, generator=gen).cuda()
    a, c = torch.randn(B, generator=gen).cuda(), torch.randn(B, generator=gen).cuda()
    sig = torch.tensor(kspace.get_sigmas(20, 0.01, 50)).cuda()
    labels = torch.tensor([0, 19, 7]).cuda()
    cases = {
        "affine_act": (lambda x_, o: ops.affine_act(x_["x"], x_["coef"], ops.ACT_ELU, out=o), dict(x=x, coef=coef)),
        "act": (lambda x_, o: ops.act(x_["x"], ops.ACT_SWISH, out=o), dict(x=x)),
        "add": (lambda x_, o: ops.add(x_["x"], x_["y"], out=o), dict(x=x, y=y)),
        "scale_shift": (lambda x_, o: ops.scale_shift(x_["x"], 2.0, -1.0, out=o), dict(x=x)),
        "axpby": (lambda x_, o: ops.axpby(x_["x"], x_["y"], 0.3, -1.7, out=o), dict(x=x, y=y)),
        "sample_axpy2": (lambda x_, o: ops.sample_axpy2(x_["x"], x_["y"], x_["a"], x_["z"], x_["c"], out=o), dict(x=x, y=y, z=z, a=a, c=c)),
        "div_sigma": (lambda x_, o: ops.div_sigma(x_["x"], x_["sig"], labels, out=o), dict(x=x, sig=sig)),
    }
    for name, (fn, operands) in cases.items():
        want = fn(operands, None)
        for which in variants(list(operands) + ["out"]):
            args = {n: (mis(t, k) if n in which else t) for n, t in operands.items()}
            if "out" in which:
                o = Mis(torch.zeros_like(x), k)
                got = fn(args, o.t)
                assert got.data_ptr() == o.t.data_ptr() and o.slack_untouched(), (name, sorted(which))
            else:
                got = fn(args, None)
            assert torch.equal(got, want), (name, sorted(which), k)
    # axpy_sched: in place on y
    want = ops.axpy_sched(y.clone(), x, 0.37)
    for which in variants(["y", "x"]):
        ym = Mis(y, k) if "y" in which else None
        yt = ym.t if ym else y.clone()
        ops.axpy_sched(yt, mis(x, k) if "x" in which else x, 0.37)
        assert torch.equal(yt, want) and (ym is None or ym.slack_untouched()), sorted(which)


# ---- statistics / normalisation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 128, 128, 128), (3, 512, 16, 16), (1, 7, 9, 5), (2, 256, 32, 32), (5, 3, 4, 4), (2, 6, 8, 20)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_instnorm_plus_coef(ops, shape, k):
    """test_kernels_gpu.test_instnorm_plus_sizes' shapes and bound (max(2e-5, 2 x the fp32 CPU oracle's error) against float64);
    the conditional form on the same tensor (test_ncsn1_gpu.test_cond_instnorm_coef_kernel: 2e-5 * max(1, max|ref|))"""
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(shape, generator=gen) * 3 + 50.0
    C = shape[1]
    p = {"alpha": 1 + 0.1 * torch.randn(C, generator=gen), "gamma": 1 + 0.1 * torch.randn(C, generator=gen),
         "beta": 0.1 * torch.randn(C, generator=gen)}
    want = scorenet.instance_norm_plus(x, p)
    exact = scorenet.instance_norm_plus(x.double(), {n: v.double() for n, v in p.items()})
    xm = mis(x, k)
    coef = ops.instnorm_plus_coef(xm, p["alpha"].cuda(), p["gamma"].cuda(), p["beta"].cuda())
    got = ops.affine_act(xm, coef, ops.ACT_NONE).cpu()
    err_gpu, err_cpu = (got.double() - exact).abs().max(), (want.double() - exact).abs().max()
    aligned = ops.instnorm_plus_coef(x.cuda(), p["alpha"].cuda(), p["gamma"].cuda(), p["beta"].cuda())
    print(f"instnorm {shape} k={k}: err {float(err_gpu):.3e} (cpu fp32 {float(err_cpu):.3e}); coefficients bit-equal to aligned: "
          f"{torch.equal(coef, aligned)}")
    assert err_gpu < max(2e-5, 2 * float(err_cpu)), (float(err_gpu), float(err_cpu))
    if k == 1:
        from test_ncsn1_gpu import _apply, _embed, _ref_cond_norm
        embed, labels = _embed(5, C, True, gen), torch.randint(0, 5, (shape[0],), generator=gen)
        xs = torch.randn(shape, generator=gen)
        ref = _ref_cond_norm(xs, embed, labels, True)
        cc = ops.cond_instnorm_plus_coef(mis(xs, k), embed.cuda(), labels.cuda(), True)
        err = float((_apply(xs.cuda().double(), cc.double()).cpu() - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), err


@pytest.mark.parametrize("B,C,G,H,W", [(2, 32, 8, 16, 16), (1, 16, 4, 5, 7), (3, 64, 16, 32, 32), (2, 8, 8, 3, 3), (2, 24, 4, 9, 6)])
def test_groupnorm_coef_and_cat(ops, B, C, G, H, W):
    """GroupNorm + swish (bound of test_score_sde_gpu.test_groupnorm_swish_vs_torch: 2e-5 * max(1, max|ref|) against float64), on
    planes with HW % 4 == 0 and != 0; the two-source form with either or both sources misaligned"""
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(B, C, H, W, generator=gen) * 2 + 1
    wt, bs = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    want = F.silu(F.group_norm(x.double(), G, wt.double(), bs.double(), eps=1e-6))
    for k in (1, 2, 3):
        xm = mis(x, k)
        got = ops.affine_act(xm, ops.groupnorm_coef(xm, wt.cuda(), bs.cuda(), G), ops.ACT_SWISH).cpu().double()
        assert (got - want).abs().max() < 2e-5 * max(1.0, float(want.abs().max())), k
        coef, am = ops.groupnorm_coef(xm, wt.cuda(), bs.cuda(), G, want_amax=True)
        assert torch.equal(ops.amax_value(am).cpu(), x.abs().amax(dim=(1, 2, 3)))
    x1, x2 = x[:, :C // 2].contiguous(), x[:, C // 2:].contiguous()
    for which in variants(["x1", "x2"]):
        got = ops.groupnorm_act_cat(mis(x1) if "x1" in which else x1.cuda(), mis(x2) if "x2" in which else x2.cuda(), wt.cuda(),
                                    bs.cuda(), G, act=ops.ACT_SWISH).cpu().double()
        assert (got - want).abs().max() < 2e-5 * max(1.0, float(want.abs().max())), sorted(which)


@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (2, 3, 5, 7), (5, 1, 1, 1), (2, 64, 32, 32)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_absmax_per_image_exact(ops, shape, k):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)) * 10.0 ** torch.linspace(-3, 3, shape[0]).view(-1, 1, 1, 1)
    got = ops.amax_value(ops.absmax_per_image(mis(x, k)))
    assert torch.equal(got.cpu(), x.abs().amax(dim=(1, 2, 3)))          # a maximum has no rounding order


# ---- pooling / resizing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (1, 4, 128, 128), (2, 2, 37, 70), (1, 1, 3, 2)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_maxpool5_and_meanpool2(ops, shape, k):
    """per-output gathers: bit-identical to torch (as test_maxpool5 / test_meanpool2 assert on the aligned path)"""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(10))
    xm = mis(x, k)
    assert torch.equal(ops.maxpool5(xm).cpu(), F.max_pool2d(x, 5, 1, 2))
    if shape[2] % 2 == 0 and shape[3] % 2 == 0:
        assert torch.equal(ops.meanpool2(xm).cpu(), scorenet.mean_pool2(x))
    xe = torch.randn(2, 5, 12, 10, generator=torch.Generator().manual_seed(11))
    assert torch.equal(ops.meanpool2(mis(xe, k)).cpu(), scorenet.mean_pool2(xe))


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (2, 5, 7, 9), (1, 8, 32, 32), (3, 16, 12, 10)])
def test_affine_avgpool5(ops, shape):
    """bound of test_ncsn1_gpu.test_affine_avgpool5_kernel (1e-5 * max(1, max|ref|) against float64), k = 1, 2, 3"""
    gen = torch.Generator().manual_seed(12)
    x, coef = torch.randn(shape, generator=gen), torch.randn(shape[0], shape[1], 3, generator=gen)
    xa = (x.double() - coef[..., 0, None, None].double()) * coef[..., 1, None, None].double() + coef[..., 2, None, None].double()
    ref = F.avg_pool2d(xa, 5, 1, 2, count_include_pad=True)
    for k in (1, 2, 3):
        y = ops.affine_avgpool5(mis(x, k), coef.cuda()).cpu()
        assert float((y.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), k
    y = ops.affine_avgpool5(mis(x), mis(coef)).cpu()
    assert float((y.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("ish,osh", [((6, 5), (12, 10)), ((16, 16), (32, 32)), ((64, 64), (128, 128)), ((16, 16), (16, 16)),
                                     ((5, 7), (11, 9)), ((1, 1), (4, 4)), ((32, 32), (64, 64)), ((20, 24), (52, 60)),
                                     ((8, 128), (24, 256)), ((12, 16), (12, 32))])
def test_bilinear(ops, ish, osh):
    """test_kernels_gpu.test_bilinear's shapes and bound (2e-6 against torch), plain / out= / accumulate / act, x and out
    misaligned in turn and together; the slack of `out` untouched"""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 3, *ish, generator=gen)
    acc = torch.randn(2, 3, *osh, generator=gen)
    want = F.interpolate(x, size=osh, mode="bilinear", align_corners=True)
    for k in (1, 2, 3):
        got = ops.bilinear(mis(x, k), osh).cpu()
        assert (got - want).abs().max() < 2e-6
        if ish == osh:
            assert torch.equal(got, x)
    for which in variants(["x", "out"]):
        o = Mis(acc, 1) if "out" in which else None
        out = o.t if o else acc.clone().cuda()
        ops.bilinear(mis(x) if "x" in which else x.cuda(), osh, out=out, accumulate=True, act=ops.ACT_ELU)
        assert (out.cpu() - F.elu(acc + want)).abs().max() < 2e-6, sorted(which)
        assert o is None or o.slack_untouched()
        with ops.amax_scope():
            r = ops.bilinear(mis(x) if "x" in which else x.cuda(), osh, out=out, want_amax=True)
            assert torch.equal(ops.amax_value(ops.amax_of(r)), r.abs().amax(dim=(1, 2, 3)))
        assert (out.cpu() - want).abs().max() < 2e-6 and (o is None or o.slack_untouched())


@pytest.mark.parametrize("ish,osh", [((3, 4, 5), (6, 8, 10)), ((8, 8, 12), (8, 8, 24)), ((4, 4, 6), (4, 4, 6)), ((2, 5, 7), (5, 11, 9)),
                                     ((1, 1, 1), (2, 3, 4)), ((8, 8, 24), (8, 8, 12))])
def test_trilinear(ops, ish, osh):
    """test_kernels_gpu.test_trilinear's shapes and bounds (2e-5 against float64)"""
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, *ish, generator=gen)
    acc = torch.randn(2, 3, *osh, generator=gen)
    want = F.interpolate(x.double(), size=osh, mode="trilinear", align_corners=True)
    for k in (1, 2, 3):
        assert (ops.trilinear(mis(x, k), osh).cpu().double() - want).abs().max() < 2e-5
    for which in variants(["x", "out"]):
        o = Mis(acc, 1) if "out" in which else None
        out = o.t if o else acc.clone().cuda()
        ops.trilinear(mis(x) if "x" in which else x.cuda(), osh, out=out, accumulate=True, act=ops.ACT_ELU)
        assert (out.cpu().double() - F.elu(acc.double() + want)).abs().max() < 2e-5, sorted(which)
        assert o is None or o.slack_untouched()


# ---- StyleGAN2 resampling ops -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,atol", [(torch.float32, 2e-6), (torch.float16, None), (torch.float64, 1e-12)])
@pytest.mark.parametrize("name", ["down2", "up2", "down2_nonsq", "up2_nonsq", "up3_down2_k5", "negpad_k3", "up1_down3_k2x4",
                                  "up2_down1_k6"])
def test_upfirdn2d_golden(ops, golden, name, dtype, atol):
    """g09 cases against the golden outputs: float32 at test_upfirdn2d_golden's 2e-6; float16 / float64 against the float64 oracle at
    the bounds of test_upfirdn2d_golden_half_and_double (half: one rounding of the result, 2^-10 relative + 1e-3; double: 1e-12)"""
    g = golden("g09_upfirdn")
    x, kk = g[f"{name}_x"], g[f"{name}_k"]
    up, down, p0, p1 = (int(v) for v in g[f"{name}_udp"])
    N, C, H, W = x.shape
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(N * C, H, W, 1)
    for k in ((1, 2, 3) if dtype == torch.float32 else (2,) if dtype == torch.float16 else (1,)):
        y = ops.upfirdn2d_raw(mis(xt, k), torch.from_numpy(kk).cuda(), up, up, down, down, p0, p1, p0, p1)
        y = y.reshape(N, C, y.shape[1], y.shape[2]).cpu()
        assert tuple(y.shape) == g[f"{name}_y"].shape
        if dtype == torch.float32:
            np.testing.assert_allclose(y.numpy(), g[f"{name}_y"], atol=atol)
        else:
            ref = resample.upfirdn2d(xt.reshape(N, C, H, W).double().numpy(), kk.astype(np.float64) if dtype == torch.float64
                                     else kk.astype(np.float16).astype(np.float64), up, up, down, down, p0, p1, p0, p1)
            if dtype == torch.float64:
                np.testing.assert_allclose(y.numpy(), ref, atol=atol)
            else:
                assert (np.abs(y.double().numpy() - ref) <= 2.0 ** -10 * np.abs(ref) + 1e-3).all()


@pytest.mark.parametrize("shape,mode,ksize,pad1", [
    ((3, 5, 12, 20), "down", (4, 4), 1), ((3, 5, 12, 24), "down", (4, 4), 1), ((2, 7, 9, 8), "down", (4, 4), 1),
    ((2, 3, 16, 16), "down", (3, 2), 1), ((2, 3, 16, 16), "down", (4, 4), 3), ((2, 3, 16, 16), "down", (4, 4), -1),
    ((3, 5, 6, 4), "up", (4, 4), 1), ((3, 5, 7, 12), "up", (4, 4), 1), ((2, 3, 8, 8), "up", (2, 3), 1), ((2, 3, 8, 6), "up", (4, 4), 1),
    ((40, 16, 64, 64), "down", (4, 4), 1), ((40, 16, 32, 32), "up", (4, 4), 1)])
def test_upfirdn2d_stream_shapes(ops, shape, mode, ksize, pad1):
    """the shapes of test_upfirdn2d_stream_kernel (the streaming kernel needs 16-byte rows: a misaligned input takes the tiled
    kernel) at that test's bound, 1e-5 against the oracle"""
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape).astype(np.float32)
    kk = rng.standard_normal(ksize).astype(np.float32)
    args = (1, 1, 2, 2, 1, pad1, 1, pad1) if mode == "down" else (2, 2, 1, 1, 2, pad1, 2, pad1)
    ref = resample.upfirdn2d(x, kk, *args)
    N, C, H, W = shape
    for k in (1, 2, 3):
        y = ops.upfirdn2d_raw(mis(torch.from_numpy(x).reshape(N * C, H, W, 1), k), torch.from_numpy(kk).cuda(), *args)
        np.testing.assert_allclose(y.reshape(ref.shape).cpu().numpy(), ref, atol=1e-5)


def test_fused_bias_act(ops, golden):
    """g10 goldens and the oracle at test_fused_bias_act's 1e-6 (float32), x and ref misaligned in turn and together; float16 /
    float64 storage on that test's cases at the bounds of test_fused_bias_act_half_and_double, x and ref in turn and together"""
    g = golden("g10_biasact")
    for k in (1, 2, 3):
        y = ops.fused_bias_act_raw(mis(g["x"], k), torch.from_numpy(g["b"]).cuda(), None, 3, 0, 0.2, 2 ** 0.5).cpu().numpy()
        np.testing.assert_allclose(y, g["y_default"], atol=1e-6)
        y = ops.fused_bias_act_raw(mis(g["x2"], k), torch.from_numpy(g["b2"]).cuda(), None, 3, 0, 0.2, 2 ** 0.5).cpu().numpy()
        np.testing.assert_allclose(y, g["y2"], atol=1e-6)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 6, 8, 8)).astype(np.float32)
    b = rng.standard_normal(6).astype(np.float32)
    ref = rng.standard_normal(x.shape).astype(np.float32)
    for act, grad in [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)]:
        want = resample.bias_act(x, b, ref, act, grad, 0.3, 1.7)
        for which in variants(["x", "ref"]):
            got = ops.fused_bias_act_raw(mis(x) if "x" in which else torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda(),
                                         mis(ref) if "ref" in which else torch.from_numpy(ref).cuda(), act, grad, 0.3, 1.7)
            np.testing.assert_allclose(got.cpu().numpy(), want, atol=1e-6, err_msg=f"act={act} grad={grad} {sorted(which)}")
    # half / double storage (bias_act_any_kernel): test_fused_bias_act_half_and_double's cases and bounds -- against the float64
    # oracle of the operands as stored, 2e-3 (half) / 2e-6 (double) * max(1, max|want|), and half against the fp32 golden at 4e-3;
    # half at 2, 4 and 6 bytes past a boundary, double at 8
    for dtype, tol, ks in ((torch.float16, 2e-3, (1, 2, 3)), (torch.float64, 2e-6, (1,))):
        for xk, bk, yk in (("x", "b", "y_default"), ("x2", "b2", "y2")):
            xt, bt = torch.from_numpy(g[xk]).to(dtype), torch.from_numpy(g[bk]).to(dtype)
            want = resample.bias_act(xt.double().numpy(), bt.double().numpy(), None, 3, 0, 0.2, 2 ** 0.5)
            for k in ks:
                xm = mis(xt, k)
                assert xm.data_ptr() % 16 == k * xt.element_size()
                y = ops.fused_bias_act_raw(xm, bt.cuda(), None, 3, 0, 0.2, 2 ** 0.5)
                assert y.dtype == dtype
                np.testing.assert_allclose(y.cpu().double().numpy(), want, atol=tol * max(1.0, np.abs(want).max()))
                if dtype == torch.float16:
                    np.testing.assert_allclose(y.cpu().float().numpy(), g[yk], atol=4e-3 * np.abs(g[yk]).max())
        rng = np.random.default_rng(3)
        xt = torch.from_numpy(rng.standard_normal((2, 6, 8, 8))).to(dtype)
        bt = torch.from_numpy(rng.standard_normal(6)).to(dtype)
        rt = torch.from_numpy(rng.standard_normal(tuple(xt.shape))).to(dtype)
        for act, grad in [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)]:
            want = resample.bias_act(xt.double().numpy(), bt.double().numpy(), rt.double().numpy(), act, grad, 0.3, 1.7)
            aligned = ops.fused_bias_act_raw(xt.cuda(), bt.cuda(), rt.cuda(), act, grad, 0.3, 1.7)
            for which in variants(["x", "ref"]):
                for k in ks:
                    got = ops.fused_bias_act_raw(mis(xt, k) if "x" in which else xt.cuda(), bt.cuda(),
                                                 mis(rt, k) if "ref" in which else rt.cuda(), act, grad, 0.3, 1.7)
                    np.testing.assert_allclose(got.cpu().double().numpy(), want, atol=tol * max(1.0, np.abs(want).max()),
                                               err_msg=f"{dtype} act={act} grad={grad} {sorted(which)} k={k}")
                    assert torch.equal(got, aligned)                 # one scalar kernel for these storage types: the same bits


# ---- Langevin / k-space -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 1, 33, 31), (3, 1, 32, 32), (2, 2, 128, 128)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_langevin_step(ops, shape, k):
    """injected noise and Philox (keyed by the index inside the sample, not by the address): bit-identical to the aligned call
    whichever of x, g, noise is off the boundary; value against numpy at test_langevin_and_philox's 1e-6; x's slack stays NaN"""
    rng = np.random.default_rng(7)
    x, g, n = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    step, ns = np.float32(0.011), np.float32(np.sqrt(0.022))
    xd, gd, nd = (torch.from_numpy(a).cuda() for a in (x, g, n))
    want = ops.langevin_step(xd.clone(), gd, float(step), float(ns), noise=nd)
    np.testing.assert_allclose(want.cpu().numpy(), x + step * g + n * ns, atol=1e-6)
    want_p = ops.langevin_step(xd.clone(), gd, float(step), float(ns), seed=3, sample_offset=2, step_id=9)
    for which in variants(["x", "g", "noise"]):
        xm = Mis(xd, k) if "x" in which else None
        xt = xm.t if xm else xd.clone()
        ops.langevin_step(xt, mis(gd, k) if "g" in which else gd, float(step), float(ns), noise=mis(nd, k) if "noise" in which else nd)
        assert torch.equal(xt, want) and (xm is None or xm.slack_untouched()), sorted(which)
        if "noise" not in which or len(which) > 1:
            xm = Mis(xd, k) if "x" in which else None
            xt = xm.t if xm else xd.clone()
            ops.langevin_step(xt, mis(gd, k) if "g" in which else gd, float(step), float(ns), seed=3, sample_offset=2, step_id=9)
            assert torch.equal(xt, want_p) and (xm is None or xm.slack_untouched()), sorted(which)


def _sched(step, ns, coef, sid):
    s = np.zeros(1, dtype=[("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"), ("rsv", "f4")])
    s["step"], s["ns"], s["coef"], s["id"] = step, ns, coef, sid
    return torch.from_numpy(s.view(np.uint8)).cuda()


@pytest.mark.parametrize("H,W", [(128, 128), (256, 256)])
def test_ald_steps(ops, H, W):
    """the fused Langevin + proximal steps (SENSE and single coil; 128 x 128: one kernel per image, 256 x 256: the strip kernels with
    the planar Langevin update): every float plane (state, gradient, noise) and the complex measurement off the boundary in turn
    and together -- bit-identical to the aligned call, injected and Philox noise; the state's slack stays NaN.  The aligned call
    itself is held to the oracle by test_ald_sense_step_matches_oracle / test_large_image_kspace_ops_vs_oracle."""
    rng = np.random.default_rng(25)
    B, n = 3, 4
    x = (rng.standard_normal((B, 1, H, W)) + 1j * rng.standard_normal((B, 1, H, W))).astype(np.complex64)
    maps = kspace.sens_maps(n, H, W, 0)
    mask = kspace.generate_mask(1, W, seed=0, **kspace.MASK_PARAMS["R20"])
    sens, m8 = torch.from_numpy(maps.astype(np.float32)).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda()
    img = (rng.random((1, 1, H, W)) * np.exp(1j * rng.standard_normal((1, 1, H, W)))).astype(np.complex64)
    y = torch.from_numpy(np.repeat(kspace.sense_forward(img, maps, mask[None]), B, axis=1)).cuda()
    ysc = torch.from_numpy(np.repeat((mask * kspace.fft2c(img)).astype(np.complex64), B, axis=0)).cuda()
    g = torch.from_numpy(rng.standard_normal((2, B, 1, H, W)).astype(np.float32)).cuda()
    nz = torch.from_numpy(rng.standard_normal((2, B, 1, H, W)).astype(np.float32)).cuda()
    step, ns, coef = 0.37, float(np.sqrt(2 * 0.37)), 0.05 * 60.0 / (n * W)
    work = ops.sense_workspace(B, n, H, W, "cuda")
    planes = dict(x_re=torch.from_numpy(np.ascontiguousarray(x.real)).cuda(), x_im=torch.from_numpy(np.ascontiguousarray(x.imag)).cuda(),
                  g_re=g[0].contiguous(), g_im=g[1].contiguous(), n_re=nz[0].contiguous(), n_im=nz[1].contiguous())

    def run(which, philox, single):
        held = {nm: Mis(t) for nm, t in planes.items() if nm in which}
        a = {nm: (held[nm].t if nm in held else t.clone()) for nm, t in planes.items()}
        yy = ysc if single else y
        yy = mis(yy) if "y" in which else yy                                 # complex64: 8 bytes past the boundary
        noise = dict(seed=9, sample_offset=4, step_id=77) if philox else dict(noise_re=a["n_re"], noise_im=a["n_im"])
        if single:
            ops.ald_singlecoil_step(a["x_re"], a["x_im"], a["g_re"], a["g_im"], yy, m8, ops.SC_L2PENALTY, step=step, noise_scale=ns,
                                    coef=0.05 * 30.0 / B, **noise)
        elif philox:
            ops.ald_sense_step(a["x_re"], a["x_im"], a["g_re"], a["g_im"], yy, sens, m8, work, step=step, noise_scale=ns, coef=coef, **noise)
        else:
            ops.ald_sense_step(a["x_re"], a["x_im"], a["g_re"], a["g_im"], yy, sens, m8, work, dev_sched=_sched(step, ns, coef, 5), **noise)
        for nm in ("x_re", "x_im"):
            assert nm not in held or held[nm].slack_untouched(), (nm, sorted(which))
        return a["x_re"].clone(), a["x_im"].clone()

    for single in (False, True):
        for philox in (False, True):
            want = run(frozenset(), philox, single)
            assert all(bool(torch.isfinite(t).all()) for t in want)
            for which in variants(["x_re", "x_im", "g_re", "g_im", "n_re", "n_im", "y"]):
                if philox and which <= {"n_re", "n_im"}:
                    continue
                got = run(which, philox, single)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (sorted(which), philox, single)


def test_kspace_operators(ops, golden):
    """fft2c, SENSE forward / adjoint, the L2Penalty proximal and the single-coil proximal at 128 x 128 with complex operands 8 bytes
    past a boundary and real planes 4: bit-identical to the aligned call (complex64 is accessed as pairs, planes as scalars: the same
    kernels), and fft2c against the oracle at test_fft2c_sizes' bound"""
    rng = np.random.default_rng(26)
    B, n, H, W = 2, 4, 128, 128
    x = (rng.standard_normal((B, 1, H, W)) + 1j * rng.standard_normal((B, 1, H, W))).astype(np.complex64)
    xd = torch.from_numpy(x).cuda()
    k0 = ops.fft2c(xd)
    np.testing.assert_allclose(k0.cpu().numpy(), kspace.fft2c(x), atol=2e-5)
    assert torch.equal(ops.fft2c(mis(xd)), k0) and torch.equal(ops.fft2c(mis(k0), inverse=True), ops.fft2c(k0, inverse=True))
    g = golden("g03_fft")
    for shape in ("2x1x8x8", "1x2x7x9", "1x1x32x32", "1x1x6x5"):                 # test_fft2c_golden: 3e-6
        xs = torch.from_numpy(np.ascontiguousarray(g[f"x_{shape}"])).to(torch.complex64)
        np.testing.assert_allclose(ops.fft2c(mis(xs)).cpu().numpy(), g[f"i2k_{shape}"], atol=3e-6)
        np.testing.assert_allclose(ops.fft2c(mis(xs), inverse=True).cpu().numpy(), g[f"k2i_{shape}"], atol=3e-6)
    maps = kspace.sens_maps(n, H, W, 0)
    mask = kspace.generate_mask(1, W, seed=0, **kspace.MASK_PARAMS["R20"])
    sens, m8 = torch.from_numpy(maps.astype(np.float32)).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda()
    Ax = ops.sense_forward(xd, sens, m8)
    np.testing.assert_allclose(Ax.cpu().numpy(), kspace.sense_forward(x, maps, mask[None]), atol=3e-5)
    for which in variants(["x", "sens"]):
        assert torch.equal(ops.sense_forward(mis(xd) if "x" in which else xd, mis(sens) if "sens" in which else sens, m8), Ax), sorted(which)
    AH = ops.sense_adjoint(Ax, sens, m8, apply_mask=True)
    for which in variants(["s", "sens"]):
        assert torch.equal(ops.sense_adjoint(mis(Ax) if "s" in which else Ax, mis(sens) if "sens" in which else sens, m8,
                                             apply_mask=True), AH), sorted(which)
    z_re, z_im = xd.real.contiguous(), xd.imag.contiguous()
    coef = 0.05 * 60.0 / (n * W)
    o_re, o_im = ops.sense_l2prox(z_re, z_im, Ax, sens, m8, coef)
    want = kspace.l2_penalty_sense(x, Ax.cpu().numpy(), 60.0, 1.0, maps, mask[None])
    np.testing.assert_allclose(o_re.cpu().numpy() + 1j * o_im.cpu().numpy(), want, atol=2e-5)
    for which in variants(["z_re", "z_im", "y", "out_re", "out_im"]):
        outs = {nm: Mis(torch.zeros_like(z_re)) for nm in ("out_re", "out_im") if nm in which}
        r_re, r_im = ops.sense_l2prox(mis(z_re) if "z_re" in which else z_re, mis(z_im) if "z_im" in which else z_im,
                                      mis(Ax) if "y" in which else Ax, sens, m8, coef,
                                      out_re=outs["out_re"].t if "out_re" in outs else None, out_im=outs["out_im"].t if "out_im" in outs else None)
        assert torch.equal(r_re, o_re) and torch.equal(r_im, o_im) and all(o.slack_untouched() for o in outs.values()), sorted(which)
    ysc = ops.fft2c(xd).reshape(B, 1, H, W) * m8.view(1, 1, 1, W)
    for mode, c in ((ops.SC_L2PENALTY, 0.05 * 30.0 / B), (ops.SC_CLOSED_FORM, 0.7), (ops.SC_PROJECTION, 0.3)):
        o_re, o_im = ops.singlecoil_prox(z_re, z_im, ysc, m8, c, mode)
        for which in variants(["z_re", "z_im", "y", "out_re"]):
            o = Mis(torch.zeros_like(z_re)) if "out_re" in which else None
            r_re, r_im = ops.singlecoil_prox(mis(z_re) if "z_re" in which else z_re, mis(z_im) if "z_im" in which else z_im,
                                             mis(ysc) if "y" in which else ysc, m8, c, mode, out_re=o.t if o else None)
            assert torch.equal(r_re, o_re) and torch.equal(r_im, o_im) and (o is None or o.slack_untouched()), (mode, sorted(which))


def test_kspace_goldens(ops, golden):
    """the reference's own vectors on misaligned operands: SENSE forward / adjoint (without the mask) / SSOS and the T = 24 per-image
    mask form (g04; test_sense_ops_golden: 5e-6), the L2Penalty SENSE proximal (g05; test_l2prox_golden: 3e-6) and the single-coil
    operators and proximals through the product classes and the raw planar kernel (g05 sc_*; test_singlecoil_ops_golden: 5e-6,
    3e-6 for the L2Penalty branch).  Complex operands sit 8 bytes past a boundary, real planes 4, 8 and 12."""
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import RandomUndersamplingFourier
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.proximal_op import get_proximal
    g, p = golden("g04_sense"), golden("g05_prox")
    maps = kspace.sens_maps(4, 32, 32, 0)
    sens = torch.from_numpy(maps.astype(np.float32)).cuda()
    mask = torch.from_numpy(g["mask_T1"].reshape(1, 32).astype(np.uint8)).cuda()
    m24 = torch.from_numpy(g["mask_T24"].reshape(24, 32).astype(np.uint8)).cuda()
    for which in variants(["x", "sens"]):
        sn = mis(sens) if "sens" in which else sens
        xs = (lambda t: mis(t)) if "x" in which else (lambda t: torch.from_numpy(t).cuda())
        np.testing.assert_allclose(ops.sense_forward(xs(g["x"]), sn, mask).cpu().numpy(), g["Ax"], atol=5e-6)
        np.testing.assert_allclose(ops.sense_adjoint(xs(g["s"]), sn).cpu().numpy(), g["AHs"], atol=5e-6)
        np.testing.assert_allclose(ops.sense_ssos(xs(g["s"])).cpu().numpy(), g["ssos_s"], atol=5e-6)
        np.testing.assert_allclose(ops.sense_forward(xs(g["x24"]), sn, m24).cpu().numpy(), g["Ax24"], atol=5e-6)
    z = p["z"]
    z_re, z_im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    for i in range(3):
        alpha, lamda = p[f"l2_sense_{i}_alpha_lamda"]
        coef = 0.05 * (alpha / lamda) / (4 * 32)
        for which in variants(["z_re", "z_im", "y", "out"]):
            for k in ((1, 2, 3) if len(which) == 1 and "y" not in which else (1,)):
                o = (Mis(torch.zeros(z_re.shape), k), Mis(torch.zeros(z_re.shape), k)) if "out" in which else None
                o_re, o_im = ops.sense_l2prox(mis(z_re, k) if "z_re" in which else torch.from_numpy(z_re).cuda(),
                                              mis(z_im, k) if "z_im" in which else torch.from_numpy(z_im).cuda(),
                                              mis(p["y"]) if "y" in which else torch.from_numpy(p["y"]).cuda(), sens, mask, coef,
                                              out_re=o[0].t if o else None, out_im=o[1].t if o else None)
                np.testing.assert_allclose(o_re.cpu().numpy() + 1j * o_im.cpu().numpy(), p[f"l2_sense_{i}_x"], atol=3e-6,
                                           err_msg=f"{sorted(which)} k={k}")
                assert o is None or (o[0].slack_untouched() and o[1].slack_untouched())
    # single coil, through the product classes (they hand the measurement / image to the kernels as given)
    sc = RandomUndersamplingFourier(8, 0.04, (1, 32, 32), seed=2)
    assert np.array_equal(sc.mask.numpy(), p["sc_mask"])
    np.testing.assert_allclose(sc(mis(g["x"])).cpu().numpy(), p["sc_y"], atol=5e-6)
    np.testing.assert_allclose(sc.conj_op(mis(p["sc_y"])).cpu().numpy(), p["sc_Ax_adj"], atol=5e-6)
    a, l = p["singlecoil_alpha_lamda"]
    for which in variants(["z", "y"]):
        zz = mis(z) if "z" in which else torch.from_numpy(z).cuda()
        yy = mis(p["sc_y"]) if "y" in which else torch.from_numpy(p["sc_y"]).cuda()
        np.testing.assert_allclose(get_proximal("L2Penalty")(sc)(zz, yy, 0.9, 1.0).cpu().numpy(), p["l2_sc_x"], atol=3e-6)
        np.testing.assert_allclose(get_proximal("SingleCoil")(sc)(zz, yy, float(a), float(l)).cpu().numpy(), p["singlecoil_x"], atol=5e-6)
    # ... and the raw planar kernel in place (out aliases z), planes and measurement off the boundary
    m8 = torch.from_numpy(p["sc_mask"].reshape(1, 32).astype(np.uint8)).cuda()
    want = kspace.single_coil(z, p["sc_y"], a, l, p["sc_mask"])
    for k in (1, 2, 3):
        zr, zi = Mis(z_re, k), Mis(z_im, k)
        ops.singlecoil_prox(zr.t, zi.t, mis(p["sc_y"]), m8, float(a / l), ops.SC_CLOSED_FORM, out_re=zr.t, out_im=zi.t)
        np.testing.assert_allclose(zr.t.cpu().numpy() + 1j * zi.t.cpu().numpy(), want, atol=5e-6)
        np.testing.assert_allclose(zr.t.cpu().numpy() + 1j * zi.t.cpu().numpy(), p["singlecoil_x"], atol=5e-6)
        assert zr.slack_untouched() and zi.slack_untouched()


# ---- convolutions ----------------------------------------------------------------------------------------------------------
def _rel64(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


WINO_LAYERS = [  # name, B, Cin, Cout, H, W, dilation: the six 16 x 16 census shapes (test_wino16_gpu.CASES) at B = 3, and the larger layers
    ("c256_256_d1", 3, 256, 256, 16, 16, 1), ("c512_512_d4", 3, 512, 512, 16, 16, 4), ("c512_512_d2", 3, 512, 512, 16, 16, 2),
    ("c256_512_d2", 3, 256, 512, 16, 16, 2), ("c512_256_d1", 3, 512, 256, 16, 16, 1), ("c256_256_d2", 3, 256, 256, 16, 16, 2),
    ("l128_64", 2, 128, 128, 64, 64, 1), ("l32_40x36", 3, 32, 64, 40, 36, 1), ("l256_32", 2, 256, 256, 32, 32, 1),
    ("l128_32_d2", 2, 128, 128, 32, 32, 2)]


@pytest.mark.parametrize("fmt", ["hx2", "bx3"])
@pytest.mark.parametrize("name,B,Cin,Cout,H,W,dil", WINO_LAYERS)
def test_conv2d_wino_bx3(ops, name, B, Cin, Cout, H, W, dil, fmt):
    """the 2-D Winograd kernel with x and / or the residual off the boundary (x: k = 1, 2, 3, the operand its launcher keys on):
    every epilogue (plain, residual, two-output, res_second) within 4e-6 * max|float64 reference| per image, the bound of
    test_kernels_gpu.py / test_wino16_gpu.py for these kernels; want_stats on a misaligned x: no partials and the plain call's bits;
    a sample's bits do not depend on its batch; a misaligned residual is re-homed, so it gives the aligned call's bits exactly"""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = F.elu(torch.randn(B, Cin, H, W, generator=gen)) * (10.0 ** torch.linspace(-3, 3, B)).view(B, 1, 1, 1)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5
    b, r = torch.randn(Cout, generator=gen), torch.randn(B, Cout, H, W, generator=gen)
    U = ops.conv_wino_bx3_weight(w.cuda(), fmt=fmt)
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil)
    ref_r = conv + r.double()
    xa, ra, bd = x.cuda(), r.cuda(), b.cuda()
    kw = dict(dilation=dil, in_amax=True)

    def bound(got, ref, scale=None):
        err = (got.double().cpu() - ref).abs().amax(dim=(1, 2, 3)) / (ref if scale is None else scale).abs().amax(dim=(1, 2, 3))
        return float(err.max())
    for k in (1, 2, 3):
        xm = mis(xa, k)
        plain = ops.conv2d_wino_bx3(xm, U, bd, **kw)
        e = bound(plain, conv)
        print(f"{name} {fmt} k={k} plain: {e:.3e}; bit-equal to the aligned launch: {torch.equal(plain, ops.conv2d_wino_bx3(xa, U, bd, **kw))}")
        assert e <= 4e-6
        st = ops.conv2d_wino_bx3(xm, U, bd, want_stats=True, **kw)
        assert not hasattr(st, "_ipdm_partials") and torch.equal(st, plain)
        one = ops.conv2d_wino_bx3(xm[B - 1:], U, bd, **kw)
        assert xm[B - 1:].data_ptr() % 16 == 4 * k and torch.equal(one, plain[B - 1:])
    for which in variants(["x", "residual"]):
        xx = mis(xa) if "x" in which else xa
        rr = mis(ra) if "residual" in which else ra
        out, act = ops.conv2d_wino_bx3(xx, U, bd, rr, act_out=ops.ACT_ELU, **kw)
        assert bound(out, ref_r) <= 4e-6 and bound(act, F.elu(ref_r), ref_r) <= 4e-6, sorted(which)
        path, both = ops.conv2d_wino_bx3(xx, U, bd, rr, act_out=ops.ACT_COPY, res_second=True, **kw)
        assert bound(path, conv) <= 4e-6 and bound(both, ref_r) <= 4e-6, sorted(which)
        same_x = ops.conv2d_wino_bx3(xx, U, bd, ra, act_out=ops.ACT_ELU, **kw)
        assert torch.equal(out, same_x[0]) and torch.equal(act, same_x[1])          # where the residual lies changes no bit
        one = ops.conv2d_wino_bx3(xx[B - 1:], U, bd, rr[B - 1:], **kw)
        assert torch.equal(one, out[B - 1:])


@pytest.mark.parametrize("fmt", ["hx2", "bx3"])
@pytest.mark.parametrize("B,Cin,Cout,H,W,res", [(2, 64, 128, 64, 32, True), (3, 128, 256, 64, 64, False)])
def test_conv2d_wino_bx3_pooled(ops, B, Cin, Cout, H, W, res, fmt):
    """the ConvMeanPool epilogue (test_conv_wino_bx3_pooled_epilogue's layers; 4e-6 * max|ref| against the float64 2x2 mean of the
    convolution) with x / the pooled-size residual off the boundary; with statistics asked on a misaligned x: none, same bits"""
    gen = torch.Generator().manual_seed(44)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.1
    b = torch.randn(Cout, generator=gen)
    r = (torch.randn(B, Cout, H // 2, W // 2, generator=gen) * 2 + 3) if res else None
    U = ops.conv_wino_bx3_weight(w.cuda(), fmt=fmt)
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = (conv[..., ::2, ::2] + conv[..., 1::2, ::2] + conv[..., ::2, 1::2] + conv[..., 1::2, 1::2]) / 4
    if res:
        ref = ref + r.double()
    aligned = ops.conv2d_wino_bx3(x.cuda(), U, b.cuda(), None if r is None else r.cuda(), pool2=True, in_amax=True)
    for which in variants(["x", "residual"] if res else ["x"]):
        for k in ((1, 2, 3) if which == {"x"} else (1,)):
            xx = mis(x, k) if "x" in which else x.cuda()
            rr = None if r is None else (mis(r, k) if "residual" in which else r.cuda())
            y = ops.conv2d_wino_bx3(xx, U, b.cuda(), rr, pool2=True, in_amax=True)
            assert _rel64(y, ref) <= 4e-6, (sorted(which), k)
            print(f"pooled {fmt} {sorted(which)} k={k}: {_rel64(y, ref):.3e}; bit-equal to aligned: {torch.equal(y, aligned)}")
            ys = ops.conv2d_wino_bx3(xx, U, b.cuda(), rr, pool2=True, want_stats=True, in_amax=True)
            assert torch.equal(ys, y) and ("x" not in which or not hasattr(ys, "_ipdm_partials"))


W1D_SHAPES = [(1, 32, 128, 8, 32), (2, 64, 128, 16, 64), (3, 128, 256, 40, 36), (2, 32, 128, 10, 44), (1, 64, 384, 24, 96),
              (2, 128, 128, 128, 128)]


@pytest.mark.parametrize("B,Cin,Cout,H,W", W1D_SHAPES)
def test_wino1d_blob_on_misaligned_input(ops, B, Cin, Cout, H, W):
    """the 1-D Winograd kernel moves 16-byte row pieces: handed a misaligned x with its own weight blob it must refuse
    (IpdmUnsupported) or be right (1e-6 of the range, test_wino1d_against_float64's bound) -- never silently wrong; a misaligned
    RESIDUAL with an aligned x runs the kernel and gives the aligned call's bits; and the module-level dispatch picks the 2-D blob
    for the misaligned input and stays within the 2-D kernel's 4e-6"""
    from inverseproblemwithdiffusionmodel_amd import _lib
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers
    from inverseproblemwithdiffusionmodel_amd.models import layers as pp_layers
    from test_wino1d_gpu import _case
    x, w, b, r = _case(B, Cin, Cout, H, W)
    U = ops.conv_wino1d_weight(w)
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1) + r.double().cpu()
    want = ops.conv2d_wino_bx3(x, U, b, r)
    assert torch.equal(ops.conv2d_wino_bx3(x, U, b, mis(r)), want)
    for k in (1, 2, 3):
        try:
            y = ops.conv2d_wino_bx3(mis(x, k), U, b, r)
            assert _rel64(y, ref) <= 1e-6
            print(f"wino1d blob, misaligned x (k={k}): ran, {_rel64(y, ref):.3e}")
        except _lib.IpdmUnsupported:
            print(f"wino1d blob, misaligned x (k={k}): IpdmUnsupported")
    for make in (lambda: layers.Conv2d(Cin, Cout, 3), lambda: pp_layers.Conv(Cin, Cout, 3)):
        conv = make().cuda()
        conv.weight.data.copy_(w)
        conv.bias.data.copy_(b)
        for xin in (x, mis(x)):
            ops.CONV_TRACE = []
            try:
                with torch.no_grad():
                    y = conv(xin, residual=r)
                trace = ops.CONV_TRACE
            finally:
                ops.CONV_TRACE = None
            assert _rel64(y, ref) <= 4e-6
            if xin.data_ptr() % 16:
                assert trace and not any(t.get("wino1d") or t.get("thin") for t in trace), trace
    cmp_ = layers.ConvMeanPool(Cin, Cout, 3).cuda()
    cmp_.conv.weight.data.copy_(w)
    cmp_.conv.bias.data.copy_(b)
    conv = F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
    pooled = (conv[..., ::2, ::2] + conv[..., 1::2, ::2] + conv[..., ::2, 1::2] + conv[..., 1::2, 1::2]) / 4
    ops.CONV_TRACE = []
    try:
        with torch.no_grad():
            y = cmp_.fused(mis(x))
        trace = ops.CONV_TRACE
    finally:
        ops.CONV_TRACE = None
    if y is None:                                            # "not built for this layer": the caller runs conv + meanpool2
        with torch.no_grad():
            y = cmp_(mis(x))
    y = y[0] if isinstance(y, tuple) else y
    assert _rel64(y, pooled) <= 4e-6 and not any(t.get("wino1d") for t in trace)


CONV_CASES = [  # test_kernels_gpu.CONV_CASES + the three extra cases of test_conv_bx3
    (2, 16, 32, 32, 32, 3, 1, False, "none", False), (2, 128, 128, 64, 64, 3, 1, True, "elu", True),
    (1, 128, 256, 32, 32, 3, 1, False, "elu", False), (3, 256, 256, 16, 16, 3, 1, True, "elu", True),
    (2, 256, 512, 16, 16, 3, 2, True, "elu", False), (2, 512, 512, 16, 16, 3, 4, False, "elu", True),
    (2, 1, 128, 32, 32, 3, 1, False, "none", False), (2, 128, 1, 32, 32, 3, 1, True, "elu", False),
    (2, 128, 256, 32, 32, 1, 1, False, "none", False), (1, 6, 5, 12, 10, 3, 1, True, "elu", True),
    (1, 7, 9, 19, 45, 3, 1, False, "relu", False), (2, 24, 40, 8, 8, 3, 2, False, "none", False),
    (3, 32, 96, 40, 70, 3, 1, False, "none", True), (2, 48, 64, 16, 16, 3, 4, False, "none", False),
    (2, 20, 33, 9, 16, 1, 1, True, "elu", True)]


@pytest.mark.parametrize("fam", ["hx2", "bx3", "f32"])
@pytest.mark.parametrize("B,Cin,Cout,H,W,k,dil,norm,actname,res", CONV_CASES)
def test_direct_conv2d(ops, B, Cin, Cout, H, W, k, dil, norm, actname, res, fam):
    """the direct kernels (split-operand families: test_conv_bx3's bound, 4e-6 or 2e-5 with a fused norm / activation; f32 family:
    test_conv2d's 2e-5; both times max(1, max|float64 reference|)) with x, residual, out=, coef off the boundary in turn and
    together; scalar accesses throughout, so the bits must equal the aligned call's; `out`'s slack stays NaN"""
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=gen)
    resid = torch.randn(B, Cout, H, W, generator=gen) if res else None
    p = {"alpha": 1 + 0.1 * torch.randn(Cin, generator=gen), "gamma": 1 + 0.1 * torch.randn(Cin, generator=gen),
         "beta": 0.1 * torch.randn(Cin, generator=gen)}
    fn = {"none": lambda t: t, "elu": F.elu, "relu": F.relu}[actname]
    h = scorenet.instance_norm_plus(x.double(), {a: v.double() for a, v in p.items()}) if norm else x.double()
    want = F.conv2d(fn(h), w.double(), bias.double(), padding=(k // 2) * dil, dilation=dil)
    if res:
        want = want + resid.double()
    xd = x.cuda()
    coef = ops.instnorm_plus_coef(xd, p["alpha"].cuda(), p["gamma"].cuda(), p["beta"].cuda()) if norm else None
    wq = ops.conv_pack_weight(w.cuda()) if fam == "f32" else ops.conv_bx3_weight(w.cuda(), fmt=fam)
    tol = (2e-5 if fam == "f32" or norm or actname != "none" else 4e-6) * max(1.0, float(want.abs().max()))
    operands = dict(x=xd, residual=None if resid is None else resid.cuda(), coef=coef)
    aligned = ops.conv2d(xd, wq, bias.cuda(), coef, ops.ACT_CODES[actname], operands["residual"], dil)
    assert float((aligned.cpu().double() - want).abs().max()) < tol
    names = [n for n, t in operands.items() if t is not None] + ["out"]
    for which in variants(names):
        for kk in ((1, 2, 3) if which == {"x"} else (1,)):
            a = {n: (mis(t, kk) if n in which and t is not None else t) for n, t in operands.items()}
            o = Mis(torch.zeros(B, Cout, H, W), kk) if "out" in which else None
            got = ops.conv2d(a["x"], wq, bias.cuda(), a["coef"], ops.ACT_CODES[actname], a["residual"], dil, out=o.t if o else None)
            assert float((got.cpu().double() - want).abs().max()) < tol, (sorted(which), kk)
            assert torch.equal(got, aligned), (sorted(which), kk)
            assert o is None or (got.data_ptr() == o.t.data_ptr() and o.slack_untouched())


@pytest.mark.parametrize("fam", ["hx2", "bx3", "f32"])
@pytest.mark.parametrize("B,Cin,Cout,D,Hh,Ww", [(2, 128, 128, 8, 8, 12), (1, 64, 128, 5, 8, 12), (1, 128, 256, 3, 6, 16), (3, 8, 16, 8, 8, 24)])
def test_direct_conv3d(ops, B, Cin, Cout, D, Hh, Ww, fam):
    """3-D direct kernels (the lists of test_conv3d_two_slices_per_workgroup and test_conv3d_vs_torch; 4e-6 * max(1, max|ref|) for the
    split-operand families, 2e-5 for the f32 family, as their 2-D forms) with x / residual off the boundary, and with a fused
    input affine + ELU (`coef`; 2e-5, test_conv_bx3's bound where a prologue leads) with x / residual / coef off it: the aligned
    call's bits"""
    gen = torch.Generator().manual_seed(20)
    x = torch.randn(B, Cin, D, Hh, Ww, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=gen) / (Cin * 27) ** 0.5
    b, r = torch.randn(Cout, generator=gen), torch.randn(B, Cout, D, Hh, Ww, generator=gen)
    coef = torch.stack([0.3 * torch.randn(B, Cin, generator=gen), 1 + 0.1 * torch.randn(B, Cin, generator=gen),
                        0.1 * torch.randn(B, Cin, generator=gen)], dim=-1)
    want = F.conv3d(x.double(), w.double(), b.double(), padding=1) + r.double()
    c = coef.double()[..., None, None, None]
    want_c = F.conv3d(F.elu((x.double() - c[:, :, 0]) * c[:, :, 1] + c[:, :, 2]), w.double(), b.double(), padding=1) + r.double()
    wq = ops.conv_pack_weight(w.cuda()) if fam == "f32" else ops.conv_bx3_weight(w.cuda(), fmt=fam)
    aligned = ops.conv3d(x.cuda(), wq, b.cuda(), residual=r.cuda())
    tol = (2e-5 if fam == "f32" else 4e-6) * max(1.0, float(want.abs().max()))
    assert float((aligned.cpu().double() - want).abs().max()) < tol
    aligned_c = ops.conv3d(x.cuda(), wq, b.cuda(), coef.cuda(), ops.ACT_ELU, residual=r.cuda())
    assert float((aligned_c.cpu().double() - want_c).abs().max()) < 2e-5 * max(1.0, float(want_c.abs().max()))
    for which in variants(["x", "residual", "coef"]):
        for k in ((1, 2, 3) if which == {"x"} else (1,)):
            xx = mis(x, k) if "x" in which else x.cuda()
            rr = mis(r, k) if "residual" in which else r.cuda()
            if "coef" not in which or len(which) > 1:
                assert torch.equal(ops.conv3d(xx, wq, b.cuda(), residual=rr), aligned), (sorted(which), k)
            got = ops.conv3d(xx, wq, b.cuda(), mis(coef, k) if "coef" in which else coef.cuda(), ops.ACT_ELU, residual=rr)
            assert torch.equal(got, aligned_c), (sorted(which), k)


@pytest.mark.parametrize("B,Cin,Cout,H,W,res,dil", [(2, 64, 64, 32, 32, True, 1), (1, 128, 128, 64, 64, False, 1), (3, 64, 64, 16, 16, True, 1),
                                                     (2, 64, 128, 16, 16, True, 2), (1, 16, 64, 32, 32, True, 2)])
def test_conv2d_wino_f32(ops, B, Cin, Cout, H, W, res, dil):
    """the f32 family's Winograd kernel (dword buffer loads of x: any alignment) at test_conv2d_winograd's 4e-5 * max(1, max|ref|):
    the aligned call's bits with x off the boundary, and with a (re-homed) misaligned residual"""
    gen = torch.Generator().manual_seed(15)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (Cin * 9) ** 0.5
    bias = torch.randn(Cout, generator=gen)
    resid = torch.randn(B, Cout, H, W, generator=gen) if res else None
    want = F.conv2d(x.double(), w.double(), bias.double(), padding=dil, dilation=dil) + (resid.double() if res else 0)
    U = ops.conv_wino_weight(w.cuda())
    aligned = ops.conv2d_wino(x.cuda(), U, bias.cuda(), None if resid is None else resid.cuda(), act_out=ops.ACT_ELU, dilation=dil)
    assert float((aligned[0].cpu().double() - want).abs().max()) < 4e-5 * max(1.0, float(want.abs().max()))
    for which in variants(["x", "residual"] if res else ["x"]):
        for k in ((1, 2, 3) if which == {"x"} else (1,)):
            got = ops.conv2d_wino(mis(x, k) if "x" in which else x.cuda(), U, bias.cuda(),
                                  None if resid is None else (mis(resid, k) if "residual" in which else resid.cuda()),
                                  act_out=ops.ACT_ELU, dilation=dil)
            assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1]), (sorted(which), k)


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(3, 1, 128, 32, 32), (2, 2, 20, 12, 16), (2, 3, 128, 16, 32), (1, 1, 5, 1, 4), (3, 128, 1, 32, 32),
                                            (2, 24, 2, 12, 16), (2, 128, 3, 16, 32), (1, 7, 1, 1, 4), (2, 1, 1, 8, 8), (2, 3, 3, 9, 12),
                                            (2, 16, 1, 6, 512), (1, 16, 2, 5, 24)])
def test_first_and_last_layer(ops, B, Cin, Cout, H, W):
    """test_conv3x3_thin's list.  The streaming kernels move float4 rows: on a misaligned input the low-level entry says
    IpdmUnsupported (never "invalid argument"), the shape-and-tensor rule says no, and Conv2d.forward of both model families routes
    the same input to the matrix-core kernels: float64 bound 4e-6 * max(1, max|ref|), the one test_conv3x3_thin sets for that path"""
    from inverseproblemwithdiffusionmodel_amd import _lib
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers
    from inverseproblemwithdiffusionmodel_amd.models import layers as pp_layers
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.2
    b = torch.randn(Cout, generator=gen)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert ops.conv3x3_thin_ok(Cin, Cout, H, W) and ops.conv3x3_thin_ok(Cin, Cout, H, W, x.cuda())
    for k in (1, 2, 3):
        xm = mis(x, k)
        assert not ops.conv3x3_thin_ok(Cin, Cout, H, W, xm)
        with pytest.raises(_lib.IpdmUnsupported):
            ops.conv3x3_thin(xm, w.cuda(), b.cuda())
        for conv in (layers.Conv2d(Cin, Cout, 3, full_range=Cin <= 3), pp_layers.Conv(Cin, Cout, 3)):
            conv = conv.cuda()
            conv.weight.data.copy_(w)
            conv.bias.data.copy_(b)
            for xin, thin in ((x.cuda(), True), (xm, False)):
                ops.CONV_TRACE = []
                try:
                    with torch.no_grad():
                        y = conv(xin)
                    trace = ops.CONV_TRACE
                finally:
                    ops.CONV_TRACE = None
                assert len(trace) == 1 and bool(trace[0].get("thin")) == thin, trace
                assert float((y.cpu().double() - want).abs().max()) <= 4e-6 * max(1.0, float(want.abs().max())), (type(conv), thin)


# ---- whole networks on a misaligned input batch -----------------------------------------------------------------------------
def _forward_traced(ops, net, *args):
    """-> (output, CONV_TRACE records, [(entry, x.data_ptr() % 16, uses 16-byte rows)] of every convolution entry called)"""
    seen, saved = [], {}

    def spy(name, rows16):
        saved[name] = getattr(ops, name)

        def f(x, *a, **kw):
            seen.append((name, x.data_ptr() % 16, rows16(a)))
            return saved[name](x, *a, **kw)
        setattr(ops, name, f)
    spy("conv3x3_thin", lambda a: True)
    spy("conv2d_wino_bx3", lambda a: a[0].kk == 12)              # a conv_wino1d_weight blob
    spy("conv3d_wino1d", lambda a: True)
    spy("conv2d", lambda a: False)                               # the direct kernels: scalar accesses
    spy("conv3d", lambda a: False)
    ops.CONV_TRACE = []
    try:
        with torch.no_grad():
            y = net(*args)
        return y.cpu().numpy(), ops.CONV_TRACE, seen
    finally:
        ops.CONV_TRACE = None
        for name, fn in saved.items():
            setattr(ops, name, fn)


def _check_net(ops, net, x, rest, ref, rel, first_is_thin=True, reaches_conv=True):
    y0, t0, s0 = _forward_traced(ops, net, torch.from_numpy(x).cuda(), *rest)
    assert np.abs(y0 - ref).max() <= rel * np.abs(ref).max()
    thin0 = sum(1 for t in t0 if t.get("thin"))
    assert thin0 >= 1 or not first_is_thin                       # the aligned input does take the streaming kernels
    for k in (1, 2, 3):
        y, t, s = _forward_traced(ops, net, mis(x, k), *rest)
        err = np.abs(y - ref).max() / np.abs(ref).max()
        thin = sum(1 for r in t if r.get("thin"))
        print(f"{type(net).__name__} k={k}: {err:.3e} of max|golden| (aligned {np.abs(y0 - ref).max() / np.abs(ref).max():.3e}); "
              f"bit-equal to the aligned forward: {np.array_equal(y, y0)}; thin layers {thin} (aligned {thin0}); "
              f"convolution entries that saw the misaligned tensor: {[e for e in s if e[1]]}")
        assert err <= rel
        assert not any(e[1] and e[2] for e in s), s                # no 16-byte-row kernel was handed a misaligned tensor
        saw = [e for e in s if e[1]]
        assert saw or not reaches_conv, s                          # the network hands its input to a convolution as it came ...
        if saw and first_is_thin:
            assert thin == thin0 - 1                               # ... which is then the one layer that left the streaming kernel
        assert len(t) == len(t0)


def test_tiny_ncsnv2_deepest(ops, golden):
    """bound of test_scorenet_gpu.test_tiny_ncsnv2_deepest: 1e-4 * max|golden|"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2
    from test_scorenet_gpu import tiny_config
    g = golden("g07_layers")
    net = ncsnv2.NCSNv2Deepest(tiny_config())
    net.load_state_dict(state_dict_from_golden(g, "net"), strict=True)
    _check_net(ops, net.cuda().eval(), g["net_x"], (torch.from_numpy(g["net_labels"]).cuda(),), g["net_y"], 1e-4)


def test_tiny_ncsnpp(ops, golden):
    """bound of test_score_sde_gpu.test_ncsnpp_forward_golden: 2e-4 * max|golden|"""
    from inverseproblemwithdiffusionmodel_amd.models import ncsnpp
    from test_score_sde_gpu import tiny_cfg
    g = golden("g14_ncsnpp")
    m = ncsnpp.NCSNpp(tiny_cfg())
    m.load_state_dict(state_dict_from_golden(g, "pp"), strict=True)
    # (NCSN++ rescales its input to [-1, 1] first: its convolutions read that fresh tensor, whatever the batch's alignment)
    _check_net(ops, m.cuda().eval(), g["pp_x"], (torch.from_numpy(g["pp_sigma"]).cuda(),), g["pp_y"], 2e-4, reaches_conv=False)


@pytest.mark.parametrize("name", ["n32", "n28"])
def test_tiny_ncsn1(ops, golden, name):
    """bound of test_ncsn1_gpu.test_tiny_ncsn_networks: 1e-4 * max|golden|"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsn
    from test_ncsn1_gpu import NETS, tiny_config
    g = golden("g31_ncsn1")
    cls, kw = NETS[name]
    net = getattr(ncsn, cls)(tiny_config(**kw))
    net.load_state_dict(state_dict_from_golden(g, name), strict=True)
    _check_net(ops, net.cuda().eval(), g[name + "_x"], (torch.from_numpy(g[name + "_labels"]).cuda(),), g[name + "_y"], 1e-4)


def test_tiny_ncsn3d(ops, golden):
    """NCSN3DShallow on a misaligned volume batch: its first convolution reads the batch as given (a reshaped view, `2x - 1` folded
    into the layer's input coefficients) and must be seen doing so, on a scalar-access kernel (no streaming first layer in 3-D; the 1-D Winograd volume form needs 16-byte
    rows): bound of test_2dtime_gpu.test_ncsn3d_shallow_forward_golden, 2e-4 * max|golden|"""
    import test_2dtime_gpu as t3
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ncsn3d import NCSN3DShallow
    g = golden("g16_ncsn3d")
    m = NCSN3DShallow(t3.cfg3d())
    m.load_state_dict(state_dict_from_golden(g, "net3d"), strict=True)
    m = m.cuda().eval()
    _check_net(ops, m, g["x"], (torch.from_numpy(g["labels"]).cuda(),), g["y"], 2e-4, first_is_thin=False, reaches_conv=True)
