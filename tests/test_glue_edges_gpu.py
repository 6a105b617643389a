"""The glue kernels behind the baselines and the reporting at their edges: csrc/tv.hip, csrc/metrics.hip, csrc/seg_ops.hip,
adam_ascent (csrc/nn_extra.hip), maxpool3d5 and temporal_taps (csrc/volume.hip).

What the cases are for.  (1) ipdm_ew_grid caps an elementwise launch at 2048 workgroups of 256, so a grid-stride loop takes a
second trip only past 524 288 work items: every elementwise kernel runs once "past the cap" (a size above it that is no multiple
of 256 and no power of two; 3 x 419 x 419 = 526 683 where the op leaves the shape free), where the (plane, row, column) decoded
from the flat index inside that loop must still be right.  (2) The block reductions (nrmse, ssim, tv_value, in_prelu_*,
maxpool3d5) run below one wave, below the block, one past the block and at their smallest legal input.  (3) The scalar formulas
run off unit scale: Adam's bias correction at steps 1-5 and 1000-1004 with both beta pairs the project uses, softmax with logits
of +-150, atan2 on its branch cut, constant planes in InstanceNorm, TV from 1e-30 to 1e30.

References are float64 on the CPU (numpy / torch, written here or taken from oracle/); inputs are rounded to float32 / complex64
first, so both sides see the same values.  Bounds, and where each comes from:
  tv_value rtol 1e-6, tv_grad atol 2e-6         test_kernels_gpu.test_tv_value_and_gradient_vs_autograd (oracle/tv.py + autograd)
  nrmse rtol 1e-6, ssim abs 1e-8,               test_kernels_gpu.test_device_metrics_match_host_definitions; SSIM against a per-window
  magnitude rtol 1e-6                           float64 evaluation (sliding_window_view, two-pass moments), not uniform_filter
  posterior planes / n: 1e-6 (|x|, |x|^2, Re,   the same test's atol for the magnitude mean (1e-6) and the phase mean (2e-6); the
  Im), 2e-6 (angle, angle^2, |angle|)           reference is numpy's float32 np.abs / np.angle of the complex64 samples, float64 sums
  in_prelu y 2e-6, gx 5e-6 * max|grad|          test_seg_guidance_gpu.test_seg_glue_kernels_vs_torch, planes of order one (x * 3 + 1)
  seg_loglh_grad 2e-6                           the same test
  zero_insert2, subsample2, maxpool3d5,         no arithmetic: torch.equal.  axpy_sched: torch.equal against the fp32 torch
  temporal_taps, axpy_sched                     expression, as in its existing test (the library is built with -ffp-contract=off)
  adam_ascent; in_prelu on offset / constant    no bound of their own exists: the idiom of test_launch_geometry_gpu part 4 -- the same
  planes and its rstd                           formula in fp32 torch on the CPU, both judged against float64,
                                                err_gpu <= max(2e-5 * max(1, max|want|), 2 * err_cpu), both errors printed
The in_prelu backward on the offset planes is judged on the kernel's own operands: its header formula takes (gy, xhat, rstd), so
the float64 reference is evaluated on the xhat / rstd the forward kernel stored (on a constant plane xhat is rounding noise around
zero, and PReLU's branch on its sign is not a property of x).  On planes of order one it is also judged end to end, as today.
HW = 2 is the exception: there the gradient is eps * rstd^2 of the terms of the formula, the fp32 xhat no longer holds it (fp32
torch misses 5e-6 * max|grad| by a factor of 17) and the kernel takes the closed form +-eps rstd^3 (g0 - g1) / 2, so both
in_prelu tests judge HW = 2 against float64 from x.

The last test of each family shows on the references alone that a plausible wrong kernel would miss by more than 100 bounds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from numpy.lib.stride_tricks import sliding_window_view

from oracle import tv as otv

pytestmark = pytest.mark.gpu

CAP = 2048 * 256                       # work items one launch covers without a second trip of the grid-stride loop
BIG = (3, 419, 419)                    # 526 683 = 3 * 419^2: past the cap, odd, no multiple of 256, the stride crosses planes
assert BIG[0] * BIG[1] * BIG[2] > CAP and (BIG[0] * BIG[1] * BIG[2]) % 256


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


def dev(t):
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).cuda()


def _idiom(got, want32, exact, what):
    """err_gpu <= max(2e-5 * max(1, max|want|), 2 * err_cpu), both errors printed (test_launch_geometry_gpu part 4)"""
    err_gpu = float((got.double() - exact).abs().max())
    err_cpu = float((want32.double() - exact).abs().max())
    top = float(exact.abs().max())
    print(f"{what}: err_gpu {err_gpu:.3e} err_cpu {err_cpu:.3e} (max|want| {top:.3e})")
    assert torch.isfinite(got).all(), what
    assert err_gpu <= max(2e-5 * max(1.0, top), 2 * err_cpu), (what, err_gpu, err_cpu)
    return err_gpu, err_cpu


def _cabs_err(a, b):
    return float(torch.view_as_real(a.to(torch.complex128) - b.to(torch.complex128)).abs().max())


# ---- TV -------------------------------------------------------------------------------------------------------------------------
def _cimg(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g))


def _tv_ref(x):
    """oracle/tv.py and its float64 autograd on the complex64 values of x -> (value [n] float64, gradient complex128)"""
    xp = x.to(torch.complex128).requires_grad_(True)
    val = otv.total_variation(xp)
    val.sum().backward()
    return val.detach(), (torch.zeros_like(xp) if xp.grad is None else xp.grad)


def _tv_check(ops, x, what, ref=None):
    val, grad = _tv_ref(x) if ref is None else ref
    got_v = ops.tv_value(dev(x)).cpu()
    got_g = ops.tv_grad(dev(x)).cpu()
    assert got_g.shape == x.shape and torch.isfinite(torch.view_as_real(got_g)).all()
    err = _cabs_err(got_g, grad)
    rel = float(((got_v - val.reshape(-1)).abs() / val.reshape(-1).abs().clamp_min(1e-300)).max()) if val.numel() else 0.0
    print(f"tv {what}: grad err {err:.3e} (bound 2e-6), value rel err {rel:.3e} (bound 1e-6)")
    np.testing.assert_allclose(got_v.numpy(), val.reshape(-1).numpy(), rtol=1e-6, atol=0)
    assert err <= 2e-6, (what, err)
    return got_v, got_g


@pytest.mark.parametrize("H,W", [(1, 1), (1, 37), (37, 1), (2, 2), (7, 300), (257, 3)])
def test_tv_small_shapes(ops, H, W):
    """fewer pixels than a wave, than the 256-thread block of tv_value, one column, one row; three images with their own data"""
    _tv_check(ops, _cimg((3, H, W), seed=H * 1000 + W), f"{H}x{W}")


def test_tv_past_the_cap(ops):
    """3 images of 419 x 419: the second trip of the grid-stride loop starts inside image 2; the last row of an image must not see
    the first row of the next (the reference is per image), and an image alone has the bits it has in the batch"""
    x = _cimg(BIG, seed=419)
    _, got_g = _tv_check(ops, x, "3 x 419x419")
    for b in range(3):
        assert torch.equal(ops.tv_grad(dev(x[b:b + 1].contiguous())).cpu(), got_g[b:b + 1]), b


def test_tv_zero_differences(ops):
    """a flat image gives exactly 0 everywhere and a value of exactly 0; a flat patch is exactly 0 inside; two equal neighbours
    contribute nothing (s(0) = 0, no NaN)"""
    flat = torch.full((2, 5, 7), 0.7 - 0.2j, dtype=torch.complex64)
    assert not torch.view_as_real(ops.tv_grad(dev(flat)).cpu()).any()
    assert torch.equal(ops.tv_value(dev(flat)).cpu(), torch.zeros(2, dtype=torch.float64))
    x = _cimg((2, 20, 28), seed=6)
    x[0, 4:9, 5:11] = 0.7 - 0.2j
    x[1, 3, 8] = x[1, 3, 7]                                            # equal along W
    x[1, 11, 2] = x[1, 10, 2]                                          # equal along H
    _, got_g = _tv_check(ops, x, "flat patch, equal neighbours")
    assert not torch.view_as_real(got_g[0, 5:8, 6:10]).any()


TV_SCALES = [1e-12, 1e-3, 1e3, 1e12, 1e-21, 1e-30, 1e19, 1e30]
TV_SEED = 30


@pytest.fixture(scope="module")
def tv_unit():
    """one 20 x 28 image and its unit-scale reference, shared by every scale.  Rounding s * x to complex64 moves a difference d
    of two neighbours by 2^-24 |x|, which turns its unit vector by 2^-24 |x| / |d|: the float64 gradient at s * x is not the
    unit-scale one.  Seed 30 is the one of 0..39 where the two agree best over TV_SCALES (4.3e-7; min |d| = 0.075; the worst seed
    parts them by 3.7e-6); test_tv_can_tell holds it to 5e-7"""
    x = _cimg((1, 20, 28), seed=TV_SEED)
    return x, _tv_ref(x)


@pytest.mark.parametrize("s", TV_SCALES)
def test_tv_scale(ops, tv_unit, s):
    """s(z) = z / |z| has no scale: the gradient of s * x is within 2e-6 of the float64 gradient at s * x AND of the unit-scale
    reference, from 1e-30 to 1e30 (the fp32 squares of the differences underflow / overflow outside 1e-19 ... 1e19; before
    unit_of took hypotf the kernel lost the whole gradient, error 4.0, at 1e-23 and 1e19).  tv_value (float64 squares) likewise."""
    x, (_, grad1) = tv_unit
    xs = (x.to(torch.complex128) * s).to(torch.complex64)
    assert torch.isfinite(torch.view_as_real(xs)).all() and float(xs.abs().min()) > 1e-37       # ordinary floats
    ref = _tv_ref(xs)
    moved = _cabs_err(ref[1], grad1)
    _, got_g = _tv_check(ops, xs, f"scale {s:g}", ref)
    err1 = _cabs_err(got_g, grad1)
    print(f"tv scale {s:g}: against the unit-scale reference {err1:.3e} (the two references differ by {moved:.3e})")
    assert err1 <= 2e-6, (s, err1)


def _tv_grad_wrapping(x):
    """the wrong kernel: the batch as one tall image (no row test at the image border)"""
    n, H, W = x.shape
    return _tv_ref(x.reshape(1, n * H, W))[1].reshape(n, H, W)


def test_tv_can_tell():
    x = _cimg((3, 7, 9), seed=2)
    away = _cabs_err(_tv_grad_wrapping(x), _tv_ref(x)[1])
    print(f"tv gradient wrapping across the image border: {away:.3e} = {away / 2e-6:.0f} bounds")
    assert away > 100 * 2e-6
    x1 = _cimg((1, 20, 28), seed=TV_SEED)
    g1 = _tv_ref(x1)[1]
    d = torch.cat([(x1[..., 1:, :] - x1[..., :-1, :]).abs().flatten(), (x1[..., :, 1:] - x1[..., :, :-1]).abs().flatten()])
    print(f"tv scale image: min |difference| {float(d.min()):.3e}, max |x| {float(x1.abs().max()):.3e}")
    for s in TV_SCALES:                                                # the two references of test_tv_scale agree far inside 2e-6
        moved = _cabs_err(_tv_ref((x1.to(torch.complex128) * s).to(torch.complex64))[1], g1)
        assert moved <= 5e-7, (s, moved)


# ---- metrics --------------------------------------------------------------------------------------------------------------------
def _nrmse_ref(a, b, by="image"):
    a, b = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt(((a - b) ** 2).sum(axis=1) / ((a if by == "image" else b) ** 2).sum(axis=1))


@pytest.mark.parametrize("elems", [1, 63, 65, 1023, 1025, 128 * 128 + 1])
@pytest.mark.parametrize("n", [1, 300])
def test_nrmse_sizes(ops, n, elems):
    """fewer elements than a wave, one more, either side of the 1024-thread block, one past a 128 x 128 image; one reference for
    all images and one per image"""
    rng = np.random.default_rng(n + elems)
    ref1 = rng.random((1, elems), dtype=np.float32) + 0.1
    img = (ref1 * (1 + 0.1 * rng.standard_normal((n, 1))) + 0.05 * rng.standard_normal((n, elems))).astype(np.float32)
    refn = (ref1 * (1 + 0.2 * rng.random((n, 1)))).astype(np.float32)
    for ref in (ref1, refn):
        got = ops.nrmse(dev(img), dev(ref)).cpu().numpy()
        want = _nrmse_ref(img, ref)
        assert got.shape == (n,) and got.dtype == np.float64
        print(f"nrmse n{n} elems{elems} ref{ref.shape[0]}: rel err {np.abs(got / want - 1).max():.3e} (bound 1e-6)")
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_nrmse_large_values_and_zero_images(ops):
    """values near 1e4 whose differences are one or two ulps (1e-3): float64 accumulation keeps them; an all-zero image gives
    the non-finite class of np.sqrt(num / den) in float64 (inf against a non-zero reference, NaN against a zero one)"""
    rng = np.random.default_rng(8)
    img = (1e4 + rng.random((4, 1025))).astype(np.float32)
    ref = (img.astype(np.float64) + 1e-3 * rng.choice([-1.0, 1.0], size=img.shape)).astype(np.float32)
    assert 0 < np.abs(img.astype(np.float64) - ref).max() < 3e-3
    got = ops.nrmse(dev(img), dev(ref)).cpu().numpy()
    print(f"nrmse near 1e4: {got}, rel err {np.abs(got / _nrmse_ref(img, ref) - 1).max():.3e}")
    np.testing.assert_allclose(got, _nrmse_ref(img, ref), rtol=1e-6, atol=0)
    img = rng.random((4, 65), dtype=np.float32)
    ref = rng.random((4, 65), dtype=np.float32)
    img[1] = 0
    img[2] = 0
    ref[2] = 0
    got, want = ops.nrmse(dev(img), dev(ref)).cpu().numpy(), _nrmse_ref(img, ref)
    assert np.isposinf(want[1]) and np.isnan(want[2])
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    np.testing.assert_allclose(got[[0, 3]], want[[0, 3]], rtol=1e-6, atol=0)


def _ssim_ref(a, b, data_range, ddof=1):
    """mean SSIM of two [H][W] images, float64, every 7 x 7 window on its own: window means, two-pass (co)variances over
    49 - ddof, K1 0.01, K2 0.03 (skimage's defaults are the sample covariance, ddof = 1)"""
    wa = sliding_window_view(a.astype(np.float64), (7, 7))
    wb = sliding_window_view(b.astype(np.float64), (7, 7))
    ux, uy = wa.mean(axis=(-2, -1)), wb.mean(axis=(-2, -1))
    da, db = wa - ux[..., None, None], wb - uy[..., None, None]
    k = 49.0 - ddof
    vx, vy, vxy = (da * da).sum(axis=(-2, -1)) / k, (db * db).sum(axis=(-2, -1)) / k, (da * db).sum(axis=(-2, -1)) / k
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return float(S.mean())


def _ssim_check(ops, img, ref, data_range, what):
    got = ops.ssim(dev(img), dev(ref), data_range).cpu().numpy()
    want = np.array([_ssim_ref(img[i], ref[0 if ref.shape[0] == 1 else i], data_range) for i in range(img.shape[0])])
    err = float(np.abs(got - want).max())
    print(f"ssim {what} range {data_range}: err {err:.3e} (bound 1e-8), values {want.min():.4f} .. {want.max():.4f}")
    assert got.shape == (img.shape[0],) and err <= 1e-8, (what, err)
    return got


@pytest.mark.parametrize("H,W", [(7, 7), (7, 300), (300, 7), (13, 9), (128, 128)])
@pytest.mark.parametrize("data_range", [1.0, 2.0])
def test_ssim_sizes(ops, H, W, data_range):
    """one window (1023 of the 1024 threads sum nothing), one row / one column of windows, 21 windows, 122 x 122 windows"""
    rng = np.random.default_rng(H * 1000 + W)
    ref1 = rng.random((1, H, W), dtype=np.float32)
    img = (ref1 + 0.05 * rng.standard_normal((3, H, W))).astype(np.float32)
    refn = (ref1 * (1 + 0.1 * np.arange(3, dtype=np.float32))[:, None, None]).astype(np.float32)
    _ssim_check(ops, img, ref1, data_range, f"{H}x{W} broadcast")
    _ssim_check(ops, img, refn, data_range, f"{H}x{W} per image")


def test_ssim_special_images(ops):
    rng = np.random.default_rng(77)
    img = rng.random((3, 13, 40), dtype=np.float32)
    got = ops.ssim(dev(img), dev(img.copy()), 2.0).cpu().numpy()
    print(f"ssim identical images: 1 - ssim {1 - got}")
    assert np.abs(got - 1).max() <= 1e-12
    const_a = np.stack([np.full((9, 11), v, dtype=np.float32) for v in (0.3, 0.3, 0.0)])
    const_b = np.stack([np.full((9, 11), v, dtype=np.float32) for v in (0.3, 0.8, 0.5)])
    for r in (1.0, 2.0):
        _ssim_check(ops, const_a, const_b, r, "constant images")
    a = (1000 + rng.standard_normal((2, 20, 23))).astype(np.float32)
    b = (a + 0.3 * rng.standard_normal(a.shape)).astype(np.float32)
    for r in (1.0, 2.0):
        _ssim_check(ops, a, b, r, "mean 1000, unit texture")


def test_ssim_rejects_images_smaller_than_the_window(ops):
    from inverseproblemwithdiffusionmodel_amd._lib import IpdmError
    for (H, W) in [(6, 9), (9, 6)]:
        x = torch.rand(2, H, W)
        with pytest.raises(IpdmError):
            ops.ssim(dev(x), dev(x), 2.0)


SPECIAL = [(0.0, 0.0), (-1.5, 0.0), (-1.5, -0.0), (0.0, 0.7), (0.0, -0.7), (-0.0, 0.0), (0.9, -0.0)]


def _samples(n, HW, seed):
    """[n][HW] complex64 with moduli below 1.3 and phases all around the circle; where there is room, pixels at exactly 0, on the
    negative real axis with imaginary part +0.0 and -0.0 (angle +pi and -pi) and on the imaginary axis"""
    rng = np.random.default_rng(seed)
    s = np.empty((n, HW), dtype=np.complex64)
    mag, ph = rng.random((n, HW)), rng.uniform(-np.pi, np.pi, (n, HW))
    s.real, s.imag = (mag * np.cos(ph)).astype(np.float32), (mag * np.sin(ph)).astype(np.float32)
    for j, (re, im) in enumerate(SPECIAL):
        if j < n * HW:
            k, p = (j % n, (j * 37) % HW) if HW > 1 else (j, 0)
            s.real[k, p], s.imag[k, p] = np.float32(re), np.float32(im)
    return s


def _moments_ref(s):
    """numpy on the complex64 samples: np.abs and np.angle in float32 (as the reference's panels), the sums in float64"""
    mag, ang = np.abs(s), np.angle(s)
    assert mag.dtype == np.float32 and ang.dtype == np.float32
    mag, ang = mag.astype(np.float64), ang.astype(np.float64)
    return np.stack([mag.sum(0), (mag * mag).sum(0), ang.sum(0), (ang * ang).sum(0), s.real.astype(np.float64).sum(0),
                     s.imag.astype(np.float64).sum(0), np.abs(ang).sum(0)])


PLANE_NAMES = ["|x|", "|x|^2", "angle", "angle^2", "Re", "Im", "|angle|"]
PLANE_BOUND = [1e-6, 1e-6, 2e-6, 2e-6, 1e-6, 1e-6, 2e-6]


@pytest.mark.parametrize("n,HW", [(n, hw) for n in (1, 2, 33) for hw in (1, 255, 257)] + [(2, 725 * 725)])
def test_posterior_moment_planes(ops, n, HW):
    """every plane on its own, divided by n; 725 x 725 = 525 625 pixels is past the cap"""
    s = _samples(n, HW, seed=n * 10 + HW % 1000)
    got = ops.posterior_moment_planes(dev(s)).cpu().numpy()
    want = _moments_ref(s)
    assert got.shape == (7, HW) and got.dtype == np.float64 and np.isfinite(got).all()
    errs = np.abs(got - want).max(axis=1) / n
    print(f"posterior planes n{n} HW{HW}: " + ", ".join(f"{nm} {e:.2e}" for nm, e in zip(PLANE_NAMES, errs)))
    for nm, e, bound in zip(PLANE_NAMES, errs, PLANE_BOUND):
        assert e <= bound, (nm, e, bound)
    if n * HW >= len(SPECIAL):                                           # the branch cut itself: +pi and -pi, not one of them twice
        ang = np.angle(s)
        assert (ang == np.float32(np.pi)).any() and (ang == -np.float32(np.pi)).any()


def test_posterior_std_of_identical_samples(ops):
    from inverseproblemwithdiffusionmodel_amd.helpers import metrics as hm
    one = _samples(1, 13 * 17, seed=3).reshape(1, 1, 13, 17)
    mm, pm, ms, ps = (t.cpu() for t in hm.compute_mean_and_std_device(dev(np.repeat(one, 4, axis=0))))
    print(f"identical samples: max mag_std {float(ms.max()):.3e}, max phase_std {float(ps.max()):.3e} (bound 1e-6)")
    for t in (mm, pm, ms, ps):
        assert torch.isfinite(t).all()
    assert float(ms.max()) <= 1e-6 and float(ps.max()) <= 1e-6
    assert float((mm.double().numpy() - np.abs(one[0]).astype(np.float64)).max()) <= 1e-6


def test_magnitude(ops):
    one = torch.complex(torch.tensor([3.0]), torch.tensor([-4.0]))
    assert torch.equal(ops.magnitude(dev(one)).cpu(), torch.tensor([5.0]))
    x = _cimg(BIG, seed=12)
    x[0, 0, :4] = torch.tensor([1e-30 + 1e-30j, 1e30 - 1e30j, 1e-30 + 0j, 3e30 + 1e-30j])
    x[2, -1, -4:] = torch.tensor([-1e-30 + 2e-30j, 1e30 + 2e30j, 0j, -1e30j])
    got = ops.magnitude(dev(x)).cpu().numpy().astype(np.float64)
    want = np.abs(x.numpy().astype(np.complex128))
    assert np.isfinite(got).all()
    print(f"magnitude 3 x 419x419 with 1e-30 / 1e30 components: rel err {np.abs(got / np.where(want > 0, want, 1) - 1)[want > 0].max():.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_metrics_can_tell():
    rng = np.random.default_rng(5)
    ref = rng.random((1, 13, 9), dtype=np.float32)
    img = (1.5 * ref + 0.3 * rng.standard_normal((1, 13, 9))).astype(np.float32)
    want = _nrmse_ref(img.reshape(1, -1), ref.reshape(1, -1))
    away = abs(float(_nrmse_ref(img.reshape(1, -1), ref.reshape(1, -1), by="reference")[0] - want[0])) / float(want[0])
    print(f"nrmse normalised by the reference: relative {away:.3e} = {away / 1e-6:.0f} bounds")
    assert away > 100 * 1e-6
    # noise of 0.3 on a 13 x 9 image: the covariance normalisation only shows through C2, more so the less the images agree
    away = abs(_ssim_ref(img[0], ref[0], 2.0, ddof=0) - _ssim_ref(img[0], ref[0], 2.0))
    print(f"ssim with the population covariance: {away:.3e} = {away / 1e-8:.0f} bounds")
    assert away > 100 * 1e-8
    s = _samples(5, 64, seed=1)
    m = _moments_ref(s)
    std_abs = np.sqrt(np.maximum(m[3] / 5 - (m[6] / 5) ** 2, 0))
    std_signed = np.sqrt(np.maximum(m[3] / 5 - (m[2] / 5) ** 2, 0))
    assert np.abs(std_abs - np.std(np.abs(np.angle(s).astype(np.float64)), axis=0)).max() < 1e-12
    away = float(np.abs(std_abs - std_signed).max())
    print(f"std(angle) instead of std(|angle|): {away:.3e} = {away / 2e-6:.0f} bounds")
    assert away > 100 * 2e-6


# ---- guidance glue ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,H,W", [(3, 1, 1), (3, 1, 9), (3, 5, 1), (3, 7, 13), (5, 181, 183)])
def test_zero_insert2(ops, P, H, W):
    """(5, 181, 183) writes 5 x 362 x 366 = 662 460 outputs: past the cap"""
    assert H != 181 or (P * 4 * H * W > CAP and (P * 4 * H * W) % 256)
    x = torch.randn(P, H, W, generator=torch.Generator().manual_seed(H + W)) + 3.0      # no zero in x: a zero is an inserted one
    want = torch.zeros(P, 2 * H, 2 * W)
    want[:, ::2, ::2] = x
    assert torch.equal(ops.zero_insert2(dev(x)).cpu(), want)


@pytest.mark.parametrize("P,H,W", [(3, 7, 13), (2, 33, 35), (3, 839, 841)])
def test_subsample2(ops, P, H, W):
    """odd H and W, every offset with its default size; (3, 839, 841) writes 3 x 420 x 421 = 530 460 outputs: past the cap"""
    x = torch.randn(P, H, W, generator=torch.Generator().manual_seed(H))
    xg = dev(x)
    for oy in (0, 1):
        for ox in (0, 1):
            assert torch.equal(ops.subsample2(xg, (oy, ox)).cpu(), x[:, oy::2, ox::2]), (oy, ox)
    assert H != 839 or (x[:, ::2, ::2].numel() > CAP and x[:, ::2, ::2].numel() % 256)


def test_subsample2_explicit_size(ops):
    """the size conv2d_stride2_valid passes for k = 3 at 33 x 35: offset (1, 1), (16, 17); one row or one column more would
    read past the plane and is refused before the launch (the wrapper allocates the output itself, so only the raise shows)"""
    from inverseproblemwithdiffusionmodel_amd._lib import IpdmError
    x = torch.randn(2, 3, 33, 35, generator=torch.Generator().manual_seed(1))
    size = ((33 - 3) // 2 + 1, (35 - 3) // 2 + 1)
    got = ops.subsample2(dev(x), (1, 1), size).cpu()
    assert got.shape == (2, 3, 16, 17) and torch.equal(got, x[..., 1:32:2, 1:34:2])
    for bad in [(17, 17), (16, 18)]:
        with pytest.raises(IpdmError):
            ops.subsample2(dev(x), (1, 1), bad)


def _in_prelu(x, slope, eps=1e-5):
    """the forward kernel's header formula in x's precision on [P, HW]: biased variance, eps inside the root -> xhat, y, rstd"""
    mean = x.mean(dim=1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=1, keepdim=True) + eps)
    h = d * rstd
    a = 1.0 if slope is None else slope
    return h, torch.where(h > 0, h, a * h), rstd[:, 0]


def _in_prelu_bwd(gy, h, rstd, slope):
    """the backward kernel's header formula in gy's precision on [P, HW] from (gy, xhat, rstd)"""
    a = 1.0 if slope is None else slope
    g = gy * torch.where(h > 0, torch.ones_like(h), a * torch.ones_like(h))
    return rstd[:, None] * (g - g.mean(dim=1, keepdim=True) - h * (g * h).mean(dim=1, keepdim=True))


IN_PRELU_HW = [1, 2, 63, 64, 255, 256, 257, 4097, 128 * 128]
CONST_PLANE = 7


def _order_one(HW):
    """-> (x, gy) [15, HW]: planes of order one, x * 3 + 1 as in test_seg_guidance_gpu"""
    g = torch.Generator().manual_seed(HW)
    gy = torch.randn(15, HW, generator=g)
    return torch.randn(15, HW, generator=g) * 3 + 1, gy


@pytest.mark.parametrize("slope", [0.17, 0.0, None])
@pytest.mark.parametrize("HW", IN_PRELU_HW)
def test_in_prelu_order_one(ops, HW, slope):
    """B * C = 3 * 5 planes of order one (x * 3 + 1, as the existing test): xhat and y within 2e-6 of the float64 formula, rstd by
    the fp32-CPU idiom; HW = 1 gives xhat = 0 and rstd = eps^-1/2"""
    x, _ = _order_one(HW)
    h64, y64, r64 = _in_prelu(x.double(), slope)
    xhat, y, rstd = ops.in_prelu_fwd(dev(x.view(3, 5, 1, HW)), None if slope is None else dev(torch.tensor([slope])))
    assert xhat.shape == y.shape == (3, 5, 1, HW) and rstd.shape == (15,)
    err_y = float((y.cpu().view(15, HW).double() - y64).abs().max())
    err_h = float((xhat.cpu().view(15, HW).double() - h64).abs().max())
    print(f"in_prelu HW{HW} slope {slope} order one: y {err_y:.3e} xhat {err_h:.3e} (bound 2e-6)")
    assert err_y <= 2e-6 and err_h <= 2e-6
    _idiom(rstd.cpu(), _in_prelu(x, slope)[2], r64, f"in_prelu HW{HW} slope {slope} order one rstd")


@pytest.mark.parametrize("slope", [0.17, 0.0, None])
@pytest.mark.parametrize("HW", IN_PRELU_HW)
def test_in_prelu_bwd_order_one_end_to_end(ops, HW, slope):
    """forward + backward kernels against the float64 formulas from x, as the existing test: gx within 5e-6 * max|grad|.
    At HW = 2 xhat = +-(1 - eps / 2 var) whatever x is, and gx = rstd (g0 - g1) / 2 * eps / (var + eps) is what is left when terms
    of order one cancel: the header formula in fp32 (torch on the CPU: 5.4e-7, 5.1e-7, 3.7e-7 for the three slopes, against bounds
    of 3.0e-8, 2.6e-8, 5.0e-8) cannot hold the bound from an fp32 xhat; the kernel's closed form for two pixels does (1e-9)"""
    x, gy = _order_one(HW)
    sl = None if slope is None else dev(torch.tensor([slope]))
    h64, _, r64 = _in_prelu(x.double(), slope)
    xhat, _, rstd = ops.in_prelu_fwd(dev(x.view(3, 5, 1, HW)), sl)
    gx = ops.in_prelu_bwd(dev(gy.view(3, 5, 1, HW)), xhat, rstd, sl).cpu().view(15, HW)
    want = _in_prelu_bwd(gy.double(), h64, r64, slope)
    w32 = _in_prelu_bwd(gy, *_in_prelu(x, slope)[::2], slope)
    err, err_cpu, top = float((gx.double() - want).abs().max()), float((w32.double() - want).abs().max()), float(want.abs().max())
    print(f"in_prelu_bwd HW{HW} slope {slope} end to end: gx err {err:.3e} (fp32 torch on the CPU {err_cpu:.3e}), "
          f"bound {5e-6 * top:.3e} = 5e-6 * max|grad| {top:.3e}")
    assert torch.isfinite(gx).all() and err <= 5e-6 * top


@pytest.mark.parametrize("slope", [0.17, 0.0, None])
@pytest.mark.parametrize("HW", IN_PRELU_HW)
def test_in_prelu_offset_and_constant_planes(ops, HW, slope):
    """every plane its own mean in +-50 and width in [0.5, 3], plane 7 exactly constant: xhat, y, rstd by the fp32-CPU idiom (the
    constant plane also on its own: float64 gives exactly 0 there), gx by the idiom on the operands the forward kernel stored
    (HW = 2: end to end, see the module docstring)"""
    B, C = 3, 5
    P = B * C
    g = torch.Generator().manual_seed(HW + 1)
    sl = None if slope is None else dev(torch.tensor([slope]))
    gy = torch.randn(P, HW, generator=g)
    off = (torch.rand(P, 1, generator=g) * 2 - 1) * 50
    x = torch.randn(P, HW, generator=g) * (0.5 + 2.5 * torch.rand(P, 1, generator=g)) + off
    x[CONST_PLANE] = off[CONST_PLANE]
    h64, y64, r64 = _in_prelu(x.double(), slope)
    h32, y32, r32 = _in_prelu(x, slope)
    assert not h64[CONST_PLANE].any() and abs(float(r64[CONST_PLANE]) - 1e-5 ** -0.5) < 1e-9
    xhat, y, rstd = ops.in_prelu_fwd(dev(x.view(B, C, 1, HW)), sl)
    xh, yk, rk = xhat.cpu().view(P, HW), y.cpu().view(P, HW), rstd.cpu()
    tag = f"in_prelu HW{HW} slope {slope} offset planes"
    _idiom(xh, h32, h64, tag + " xhat")
    _idiom(yk, y32, y64, tag + " y")
    _idiom(rk, r32, r64, tag + " rstd")
    _idiom(yk[CONST_PLANE], y32[CONST_PLANE], y64[CONST_PLANE], tag + " y of the constant plane")
    gx = ops.in_prelu_bwd(dev(gy.view(B, C, 1, HW)), xhat, rstd, sl).cpu().view(P, HW)
    if HW == 2:                     # closed form from (gy, the sign of xhat, rstd, eps): the float64 formula from x is the reference
        _idiom(gx, _in_prelu_bwd(gy, h32, r32, slope), _in_prelu_bwd(gy.double(), h64, r64, slope), tag + " gx (from x)")
    else:
        _idiom(gx, _in_prelu_bwd(gy, xh, rk, slope), _in_prelu_bwd(gy.double(), xh.double(), rk.double(), slope), tag + " gx")


def _seg_case(B, C, HW, seed):
    """logits normal * 4; image 1 (where there is one) normal * 40; image 2 with two exactly equal maxima at every pixel; labels
    (p + b) % C: every class, and the first and the last pixel of every image carry a label of their own"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, HW, generator=g) * 4
    if B > 1:
        logits[1] *= 10
    if B > 2 and C > 1:
        top = logits[2].argmax(dim=0, keepdim=True)
        logits[2].scatter_(0, (top + 1) % C, logits[2].gather(0, top))
        srt = logits[2].sort(dim=0).values
        assert torch.equal(srt[-1], srt[-2])
    label = (torch.arange(HW)[None, :] + torch.arange(B)[:, None]) % C
    return logits, label.view(B, 1, HW)


def _seg_ref(logits, label):
    ld = logits.double()
    return torch.zeros_like(ld).scatter_(1, label, 1.0) - torch.softmax(ld, dim=1)


@pytest.mark.parametrize("C,B,HW", [(C, B, HW) for C in (1, 2, 4) for (B, HW) in [(1, 1), (2, 255), (3, 257)]]
                         + [(4, 3, 419 * 419)])
def test_seg_loglh_grad(ops, C, B, HW):
    """one class gives exactly 0; 3 x 419 x 419 pixels are past the cap"""
    logits, label = _seg_case(B, C, HW, seed=C * 1000 + HW % 997)
    got = ops.seg_loglh_grad(dev(logits.view(B, C, 1, HW)), dev(label.view(B, 1, 1, HW))).cpu().view(B, C, HW)
    if C == 1:
        assert not got.any()
        return
    want = _seg_ref(logits, label)
    assert set(label.unique().tolist()) == set(range(min(C, HW))) or HW < C
    err = float((got.double() - want).abs().max())
    print(f"seg_loglh_grad B{B} C{C} HW{HW}: err {err:.3e} (bound 2e-6), max|logit| {float(logits.abs().max()):.0f}")
    assert torch.isfinite(got).all() and err <= 2e-6


def _sched(seg_scale):
    s = np.zeros(1, dtype=[("step", "f4"), ("ns", "f4"), ("coef", "f4"), ("sigma", "f4"), ("id", "i8"), ("seg", "f4"), ("rsv", "f4")])
    s["seg"] = seg_scale
    assert s.nbytes == 32
    return dev(torch.from_numpy(s.view(np.uint8)))


@pytest.mark.parametrize("shape,period", [((1,), None), ((255,), None), ((257,), None), ((37, 7), 7), (BIG, 419 * 419),
                                          ((75241, 7), 7)])
def test_axpy_sched(ops, shape, period):
    """bits against the fp32 torch expression y + (x * mask) * scale, host scale and the device schedule's seg_scale; the
    419 x 419 mask wraps three times past the cap, the period-7 mask at 259 and at 526 687 elements"""
    g = torch.Generator().manual_seed(len(shape) + shape[0])
    y, x = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    scale = torch.tensor(0.3712, dtype=torch.float32)
    masks = [None]
    if period is not None:
        masks.append(torch.randint(0, 2, (period,), generator=g))
        assert masks[1].min() == 0 and masks[1].max() == 1
    for m in masks:
        v = x if m is None else (x.reshape(-1, period) * m.float()).reshape(shape)
        want = y + v * scale
        mg = None if m is None else dev(m)
        assert torch.equal(ops.axpy_sched(dev(y.clone()), dev(x), scale=float(scale), mask=mg).cpu(), want)
        assert torch.equal(ops.axpy_sched(dev(y.clone()), dev(x), dev_sched=_sched(float(scale)), mask=mg).cpu(), want)


def test_axpy_sched_rejects_a_mask_that_does_not_tile(ops):
    y = dev(torch.zeros(257))
    with pytest.raises(ValueError):
        ops.axpy_sched(y, dev(torch.ones(257)), scale=1.0, mask=dev(torch.ones(7, dtype=torch.int64)))
    torch.cuda.synchronize()
    assert not y.cpu().any()


def test_seg_glue_can_tell():
    HW = 63                                                            # a short plane: 63 / 62 in the variance is 0.8 % of y
    x = torch.randn(15, HW, generator=torch.Generator().manual_seed(63)).double() * 3 + 1
    _, y64, _ = _in_prelu(x, 0.17)
    d = x - x.mean(dim=1, keepdim=True)
    h = d / torch.sqrt(d.var(dim=1, keepdim=True, unbiased=True) + 1e-5)
    away = float((torch.where(h > 0, h, 0.17 * h) - y64).abs().max())
    print(f"InstanceNorm with the unbiased variance at HW {HW}: {away:.3e} = {away / 2e-6:.0f} bounds")
    assert away > 100 * 2e-6


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
def _torch_adam(x0, grads, lr, betas, dtype, state=None, start=1):
    """len(grads) torch.optim.Adam steps on the CPU with param.grad = -g -> [(x, m, v)] after every step"""
    p = torch.nn.Parameter(x0.to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=1e-8, foreach=False)
    if state is not None:
        opt.state[p] = dict(step=torch.tensor(float(start - 1)), exp_avg=state[0].to(dtype).clone(),
                            exp_avg_sq=state[1].to(dtype).clone())
    out = []
    for g in grads:
        p.grad = -g.to(dtype)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    assert int(opt.state[p]["step"]) == start - 1 + len(grads)
    return out


def _adam_run(ops, x0, grads, lr, betas, what, start=1, state=None, groups=None):
    """five adam_ascent calls against float64 torch.optim.Adam, x / m / v after every call, by the fp32-CPU idiom; groups: index
    sets judged on their own (components of very different size)"""
    n = x0.numel()
    m0, v0 = (torch.zeros(n), torch.zeros(n)) if state is None else state
    want = _torch_adam(x0, grads, lr, betas, torch.float64, None if state is None else (m0, v0), start)
    w32 = _torch_adam(x0, grads, lr, betas, torch.float32, None if state is None else (m0, v0), start)
    x, m, v = dev(x0.clone()), dev(m0.clone()), dev(v0.clone())
    worst = {}
    for k, g in enumerate(grads):
        assert ops.adam_ascent(x, dev(g), m, v, lr, start + k, betas=betas) is x
        for name, got, a, b in zip("xmv", (x, m, v), w32[k], want[k]):
            for gname, idx in (groups or {"": slice(None)}).items():
                e = _idiom(got.cpu()[idx], a[idx], b[idx], f"adam {what} step {start + k} {name}{gname}")
                worst[name] = max(worst.get(name, (0.0, 0.0)), e)
    print(f"adam {what} steps {start}..{start + len(grads) - 1} worst (err_gpu, err_cpu): {worst}")
    return want


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.5)])
@pytest.mark.parametrize("lr", [1e-2, 0.5])
def test_adam_ascent(ops, n, betas, lr):
    """steps 1..5 from m = v = 0, then steps 1000..1004 from the float64 run's m and v rounded to float32"""
    g = torch.Generator().manual_seed(n)
    x0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (1 + k) for k in range(5)]
    want = _adam_run(ops, x0, grads, lr, betas, f"n{n} betas {betas} lr {lr}")
    xs, ms, vs = want[-1]
    _adam_run(ops, xs.float(), grads[::-1], lr, betas, f"n{n} betas {betas} lr {lr}", start=1000, state=(ms.float(), vs.float()))


def test_adam_ascent_past_the_cap(ops):
    n = BIG[0] * BIG[1] * BIG[2]
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(5)]
    _adam_run(ops, x0, grads, 1e-2, (0.5, 0.5), f"n{n}")


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.5)])
def test_adam_ascent_zero_and_extreme_gradients(ops, betas):
    """components whose gradient is exactly 0 in every call keep the bits of x (m = v = 0: the step is 0 / eps); components of
    1e-20 (g^2 is a float32 denormal) and 1e15 stay finite and inside the bound of their own size"""
    n = 257
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(n, generator=g)
    x0[3] = -0.0
    zero, tiny, huge = torch.tensor([0, 3, 64, 255, 256]), torch.tensor([1, 65, 254]), torch.tensor([2, 66, 253])
    rest = torch.ones(n, dtype=torch.bool)
    rest[torch.cat([zero, tiny, huge])] = False
    grads = []
    for k in range(5):
        gr = torch.randn(n, generator=g)
        gr[zero], gr[tiny], gr[huge] = 0.0, 1e-20 * (1 + k), -1e15 * (1 + k)
        grads.append(gr)
    groups = {" (ordinary)": rest, " (zero)": zero, " (1e-20)": tiny, " (1e15)": huge}
    x, m, v = dev(x0.clone()), dev(torch.zeros(n)), dev(torch.zeros(n))
    for k, gr in enumerate(grads):
        ops.adam_ascent(x, dev(gr), m, v, 0.5, k + 1, betas=betas)
        assert torch.equal(x.cpu()[zero].view(torch.int32), x0[zero].view(torch.int32))
        assert not m.cpu()[zero].any() and not v.cpu()[zero].any()
    _adam_run(ops, x0, grads, 0.5, betas, f"zero / 1e-20 / 1e15 components betas {betas}", groups=groups)


def _adam_plain(x0, grads, lr, betas, bias_correction=True, eps=1e-8):
    """the kernel's header formula in float64 (bias_correction=False: the wrong kernel)"""
    x, m, v = x0.double().clone(), torch.zeros_like(x0).double(), torch.zeros_like(x0).double()
    for t, g in enumerate(grads, start=1):
        m = betas[0] * m + (1 - betas[0]) * (-g.double())
        v = betas[1] * v + (1 - betas[1]) * g.double() ** 2
        bc1, bc2 = (1 - betas[0] ** t, 1 - betas[1] ** t) if bias_correction else (1.0, 1.0)
        x = x - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return x


def test_adam_can_tell():
    """lr 0.5: with betas (0.5, 0.5) the correction is 1 / 32 of a step by the fifth call, 80 bounds at lr 1e-2"""
    g = torch.Generator().manual_seed(257)
    x0 = torch.randn(257, generator=g)
    grads = [torch.randn(257, generator=g) * (1 + k) for k in range(5)]
    for betas in [(0.9, 0.999), (0.5, 0.5)]:
        want = _torch_adam(x0, grads, 0.5, betas, torch.float64)[-1][0]
        assert float((_adam_plain(x0, grads, 0.5, betas) - want).abs().max()) < 1e-12       # the header formula is torch's
        away = float((_adam_plain(x0, grads, 0.5, betas, bias_correction=False) - want).abs().max())
        bound = 2e-5 * max(1.0, float(want.abs().max()))
        print(f"Adam without bias correction, betas {betas}, five steps of lr 0.5: {away:.3e} = {away / bound:.0f} bounds")
        assert away > 100 * bound


# ---- 3-D glue -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,W", [(1, 1, 1), (1, 1, 9), (2, 3, 7), (5, 5, 5), (8, 8, 12), (3, 40, 17), (8, 8, 128)])
def test_maxpool3d5_sizes(ops, D, H, W):
    """volumes below the window, below the block, ragged; 8 x 8 x 128 takes exactly the 64 KiB of LDS the launcher allows.  The
    second input is all negative: a zero border would show on every face"""
    g = torch.Generator().manual_seed(D * 100 + H * 10 + W)
    x = torch.randn(2, 3, D, H, W, generator=g)
    for t in (x, -1.0 - torch.rand(2, 3, D, H, W, generator=g)):
        assert torch.equal(ops.maxpool3d5(dev(t)).cpu(), F.max_pool3d(t, 5, 1, 2))


def test_maxpool3d5_many_planes_and_the_lds_limit(ops):
    from inverseproblemwithdiffusionmodel_amd._lib import IpdmUnsupported
    x = torch.randn(70000, 1, 2, 2, 3, generator=torch.Generator().manual_seed(7)) - 2.0
    assert torch.equal(ops.maxpool3d5(dev(x)).cpu(), F.max_pool3d(x, 5, 1, 2))
    with pytest.raises(IpdmUnsupported):
        ops.maxpool3d5(dev(torch.zeros(1, 1, 8, 8, 129)))


def _taps_ref(x, mode):
    """the index formula of volume.hip's comment on x [B, C, D, H, T] -> [B, 4C, D, H, T']:
    mode 0: out[k][t] = x[2t - 1 + k], T' = T / 2; mode 1: out[k][t] = xup[t + 1 - k], xup[u] = x[u / 2] for even u, T' = 2T"""
    B, C, D, H, T = x.shape
    To = T // 2 if mode == 0 else 2 * T
    out = np.zeros((B, C, 4, D, H, To), dtype=np.float32)
    for k in range(4):
        for t in range(To):
            if mode == 0:
                ti = 2 * t - 1 + k
                if 0 <= ti < T:
                    out[:, :, k, :, :, t] = x[..., ti]
            else:
                u = t + 1 - k
                if u >= 0 and u % 2 == 0 and u // 2 < T:
                    out[:, :, k, :, :, t] = x[..., u // 2]
    return torch.from_numpy(out.reshape(B, 4 * C, D, H, To))


@pytest.mark.parametrize("B,C,D,H,T,modes", [(2, 3, 1, 1, 2, (0, 1)), (2, 3, 1, 1, 1, (1,)), (2, 3, 4, 4, 5, (0, 1)),
                                             (2, 3, 8, 8, 12, (0, 1)), (2, 3, 3, 3, 31, (0, 1)), (3, 5, 11, 13, 155, (0,)),
                                             (3, 5, 11, 13, 77, (1,))])
def test_temporal_taps(ops, B, C, D, H, T, modes):
    """(S, T) = (1, 2), (1, 1), (16, 5), (64, 12), (9, 31); 15 planes of S = 143 write 660 660 (mode 0, T = 155) and 1 321 320
    (mode 1, T = 77) outputs: past the cap"""
    x = torch.randn(B, C, D, H, T, generator=torch.Generator().manual_seed(T)) + 3.0     # no zero in x: a zero is a padded tap
    for mode in modes:
        got = ops.temporal_taps(dev(x), mode).cpu()
        assert D * H != 143 or (got.numel() > CAP and got.numel() % 256)
        assert torch.equal(got, _taps_ref(x.numpy(), mode)), mode


def test_temporal_taps_are_the_convolutions_taps(ops):
    """(S, T) = (64, 12): the four taps contracted with a random weight in float64 are F.conv3d(stride (1,1,2), padding (0,0,1))
    in mode 0 and F.conv_transpose3d in mode 1, to 1e-12 -- tap order and direction, independent of the restated formula"""
    g = torch.Generator().manual_seed(12)
    B, Cin, Cout = 2, 3, 5
    x = torch.randn(B, Cin, 8, 8, 12, generator=g)
    w = torch.randn(Cout, Cin, 4, generator=g).double()
    for mode in (0, 1):
        taps = ops.temporal_taps(dev(x), mode).cpu().double()
        got = torch.einsum("ock,bckdht->bodht", w, taps.view(B, Cin, 4, 8, 8, taps.shape[-1]))
        if mode == 0:
            want = F.conv3d(x.double(), w[:, :, None, None, :], stride=(1, 1, 2), padding=(0, 0, 1))
        else:
            want = F.conv_transpose3d(x.double(), w.permute(1, 0, 2)[:, :, None, None, :], stride=(1, 1, 2), padding=(0, 0, 1))
        err = float((got - want).abs().max())
        print(f"temporal_taps mode {mode} contracted against torch: {err:.3e} (bound 1e-12)")
        assert got.shape == want.shape and err <= 1e-12


def test_volume_can_tell():
    x = -1.0 - torch.rand(2, 3, 2, 3, 7, generator=torch.Generator().manual_seed(1))
    zero_border = F.max_pool3d(F.pad(x, (2,) * 6, value=0.0), 5, 1, 0)
    away = float((zero_border - F.max_pool3d(x, 5, 1, 2)).abs().max())
    print(f"max-pool with a zero border on all-negative input: {away:.3e} (the bound is bit equality)")
    assert away >= 1.0
    # taps in the reverse order give another convolution
    g = torch.Generator().manual_seed(12)
    xx = torch.randn(2, 3, 8, 8, 12, generator=g)
    w = torch.randn(5, 3, 4, generator=g).double()
    taps = _taps_ref(xx.numpy(), 0).double().view(2, 3, 4, 8, 8, 6)
    want = F.conv3d(xx.double(), w[:, :, None, None, :], stride=(1, 1, 2), padding=(0, 0, 1))
    assert float((torch.einsum("ock,bckdht->bodht", w, taps) - want).abs().max()) <= 1e-12
    away = float((torch.einsum("ock,bckdht->bodht", w, taps.flip(2)) - want).abs().max())
    print(f"temporal taps in reverse order: {away:.3e} = {away / 1e-12:.0e} bounds")
    assert away > 100 * 1e-12
