"""Time-averaged calibration of 2D+time k-space on the GPU (csrc/kspace_tavg.hip, SENSE.from_cine_measurement, the cine
drivers) against the float64 restatement in tests/cine_helpers.py.

Bounds.  Composite: the kernel sums at most T <= 4096 floats in double (relative error at most T 2^-53) and divides in
double, so the stored float is one of the two floats next to the exact quotient: |gpu - float32(ref64)| <= 2^-23 |ref64|
per real and imaginary component; the count is exact and a pixel no frame sampled is exactly 0 + 0i.  Composition of the
pipeline: bit for bit against the same ops called by hand (the kernels underneath are held to float64 by their own tests;
single eigenvectors are ill-conditioned, test_coilcomp_gpu.py).  Maps against the float64 chain (helper composite, then
csm_helpers.estimate): max(3e-5, 4 err_cpu) max abs with at most 0.5 % of the pixels, those within 1e-3 of the support
threshold, left out -- the bound and the cap of test_csm_gpu.py; on the CPU the float64 chain left out 0 pixels of the
three cases and err_cpu was 1.6e-6, 5.5e-7, 6.4e-7."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cine_helpers as cineh
import coilcomp_helpers as cch
import csm_helpers as csmh

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 3e-5
THRESH = 0.02


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier
    return Namespace(lib=_lib, syn=synthetic, uf=undersampling_fourier)


def view(t):
    return torch.view_as_real(t)


# ---- the kernel against the float64 helper ------------------------------------------------------------------------------------
def counting_mask():
    """(5, 1, 16, 16): rows 0..2 sampled in all five frames, row 3 in frame 0 only, row 4 in frame 2 only, row 5 in frame 4
    only, rows 6..7 in none, the rest at random"""
    m = torch.from_numpy(np.random.default_rng(7).random((5, 1, 16, 16)) < 0.4)
    m[:, 0, 0:3] = True
    m[:, 0, 3:8] = False
    m[0, 0, 3], m[2, 0, 4], m[4, 0, 5] = True, True, True
    return m


def kernel_mask(name, H, W):
    rng = np.random.default_rng(11)
    if name == "line1":
        return torch.tensor([True, False, True, True])
    if name == "counting":
        return counting_mask()
    if name == "cine24":
        return cineh.frame_masks(H, W, 24, 8, seed=0, kind="line")
    if name == "vd1":
        from inverseproblemwithdiffusionmodel_amd.synthetic import vd_mask_2d
        return torch.as_tensor(vd_mask_2d(H, W, 3, seed=2))
    if name == "fold":
        return torch.tensor([[True, False], [True, True]]).reshape(2, 1, 1, 2)
    kind, tm = name.split(":")                                               # "2d:Tm" / "line:Tm": random planes
    shape = (int(tm), 1, H, W) if kind == "2d" else (int(tm), 1, 1, W)
    return torch.from_numpy(rng.random(shape) < 0.45)


KERNEL_CASES = [((1, 1, 1, 4, 4), "line1"),          # identity where sampled, zero elsewhere
                ((3, 2, 5, 16, 16), "counting"),     # the counting rule
                ((2, 1, 24, 16, 48), "cine24"),      # the cine default: generated line masks
                ((2, 2, 3, 5, 7), "2d:2"),           # (b*T + t) % Tm: the two images walk the planes differently; odd sizes
                ((4, 3, 3, 48, 80), "vd1"),          # one plane: the plain mean over the frames
                ((64, 1, 2, 8, 8), "2d:2"),          # many coils
                ((1, 2, 70, 3, 5), "line:70"),       # more than 32 and more than 64 frames: several words of the bit table
                ((2, 1, 1100, 2, 3), "2d:7")]        # above 1024 frames: the 64-thread launch


_KERNEL = {}


def kernel_case(shape, name, scale=1.0):
    """(y complex64 on the host, mask, mask_u8 on the GPU, ref ybar complex128, ref count int32): computed once, left unchanged"""
    key = (shape, name, scale)
    if key not in _KERNEL:
        from inverseproblemwithdiffusionmodel_amd import ops as _ops
        n, B, T, H, W = shape
        rng = np.random.default_rng(sum(shape))
        y = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)
        mask = kernel_mask(name, H, W)
        ybar, count = cineh.composite(y, mask)
        _KERNEL[key] = (torch.from_numpy(y), mask, _ops._mask_u8(mask, H, W, "cuda"), ybar, count)
    return _KERNEL[key]


def check_composite(got, count, ref, ref_count, what):
    got = got.cpu().numpy().astype(np.complex128)
    assert np.array_equal(count.cpu().numpy(), ref_count) and count.dtype == torch.int32
    r32 = ref.astype(np.complex64).astype(np.complex128)
    worst = 0.0
    for part in (np.real, np.imag):
        err, mag = np.abs(part(got) - part(r32)), np.abs(part(ref))
        worst = max(worst, float((err / np.where(mag > 0, mag, 1.0)).max()))
        assert (err <= 2.0 ** -23 * mag).all(), what
    empty = np.broadcast_to(ref_count[None] == 0, got.shape)
    assert not got[empty].any()                                              # exact zeros where no frame sampled
    print(f"{what}: worst relative component error {worst:.2e} (bound {2.0 ** -23:.2e}); count {ref_count.min()}..{ref_count.max()}")


@pytest.mark.parametrize("shape,name", KERNEL_CASES)
def test_composite_vs_float64(ops, shape, name):
    y, mask, mu8, ref, ref_count = kernel_case(shape, name)
    n, B, T, H, W = shape
    got, count = ops.kspace_time_average(y.cuda(), mu8, return_count=True)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (n, B, H, W) and tuple(count.shape) == (B, H, W)
    check_composite(got, count, ref, ref_count, f"{shape} {name}")
    if name == "line1":                                                      # one frame: the data where sampled
        keep = torch.tensor([True, False, True, True]).expand(4, 4)
        assert torch.equal(view(got.cpu()[0, 0]), view(torch.where(keep, y[0, 0, 0], torch.zeros(4, 4, dtype=torch.complex64))))
    if name == "counting":
        c = count.cpu()
        assert (c[:, 0:3] == 5).all() and (c[:, 3:6] == 1).all() and (c[:, 6:8] == 0).all() and 0 < c[:, 8:].float().mean() < 5
        assert torch.equal(view(got.cpu()[:, :, 3]), view(y[:, :, 0, 3])) and torch.equal(view(got.cpu()[:, :, 4]), view(y[:, :, 2, 4]))
        assert torch.equal(view(got.cpu()[:, :, 5]), view(y[:, :, 4, 5]))
    if B == 1:                                                               # (n, T, H, W) and (n, B, T, 1, H, W) are the same call
        assert torch.equal(view(ops.kspace_time_average(y[:, 0].cuda(), mu8)), view(got[:, 0]))
    assert torch.equal(view(ops.kspace_time_average(y[:, :, :, None].cuda().contiguous(), mu8)), view(got))
    assert torch.equal(view(ops.kspace_time_average(y.cuda(), mu8)), view(got))      # without the count


def test_composite_folds_a_batch_past_the_grid_limit(ops):
    """B = 65 537 images of 2 x 2: image b runs in workgroup row b % 65 535"""
    shape = (1, 65537, 2, 2, 2)
    y, mask, mu8, ref, ref_count = kernel_case(shape, "fold")
    got, count = ops.kspace_time_average(y.cuda(), mu8, return_count=True)
    check_composite(got, count, ref, ref_count, "B = 65537")
    assert torch.equal(view(got[:, 65535:].contiguous()), view(ops.kspace_time_average(y[:, 65535:].cuda().contiguous(), mu8)))


def test_unsampled_input_is_never_read(ops):
    shape = (3, 2, 5, 16, 16)
    y, mask, mu8, ref, ref_count = kernel_case(shape, "counting")
    sampled = torch.from_numpy(cineh.frame_planes(mask, 2, 5, 16, 16))[None].expand(3, -1, -1, -1, -1)
    zeros = torch.where(sampled, y, torch.zeros_like(y))
    nans = torch.where(sampled, y, torch.full_like(y, complex(float("nan"), float("nan"))))
    assert torch.isnan(view(nans)).any()
    a = ops.kspace_time_average(zeros.cuda(), mu8)
    b = ops.kspace_time_average(nans.cuda(), mu8)
    assert torch.equal(view(a), view(b)) and torch.isfinite(view(b)).all()
    assert torch.equal(view(a), view(ops.kspace_time_average(y.cuda(), mu8)))


def test_batch_and_alignment_invariance(ops):
    """an image gives the same bits alone and inside a batch; so do buffers 8 bytes past a 16-byte boundary"""
    shape = (3, 3, 5, 16, 16)
    y, mask, mu8, _, _ = kernel_case(shape, "counting")
    yd = y.cuda()
    batch, cnt = ops.kspace_time_average(yd, mu8, return_count=True)
    # image 1 alone starts at plane 0, inside the batch at plane (1*5) % 5 = 0 as well: the same planes, the same bits
    alone, cnt1 = ops.kspace_time_average(yd[:, 1:2].contiguous(), mu8, return_count=True)
    assert torch.equal(view(alone[:, 0]), view(batch[:, 1])) and torch.equal(cnt1[0], cnt[1])

    def offset(numel):
        base = torch.zeros(numel + 4, dtype=torch.complex64, device="cuda")
        off = 1 if base.data_ptr() % 16 == 0 else 0
        off += 1 if (base.data_ptr() + 8 * off) % 16 == 0 else 0
        t = base[off:off + numel]
        assert t.data_ptr() % 16 == 8
        return t
    ym = offset(yd.numel()).view(yd.shape)
    ym.copy_(yd)
    out = offset(batch.numel()).view(batch.shape)
    got = ops.kspace_time_average(ym, mu8, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(view(got), view(batch))


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_composite_at_other_scales(ops, scale):
    shape = (3, 2, 5, 16, 16)
    y, mask, mu8, ref, ref_count = kernel_case(shape, "counting", scale)
    got, count = ops.kspace_time_average(y.cuda(), mu8, return_count=True)
    check_composite(got, count, ref, ref_count, f"scale {scale}")
    assert 0.1 * scale < float(np.abs(ref).max()) < 10 * scale


def test_graph_capture_and_replay(ops):
    shape = (2, 1, 24, 16, 48)
    y, mask, mu8, ref, ref_count = kernel_case(shape, "cine24")
    static = torch.zeros(shape, dtype=torch.complex64, device="cuda")
    out = torch.empty((2, 1, 16, 48), dtype=torch.complex64, device="cuda")
    ops.kspace_time_average(static, mu8, out=out)                             # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.kspace_time_average(static, mu8, out=out)
    static.copy_(y.cuda())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(view(out), view(ops.kspace_time_average(y.cuda(), mu8)))


def test_refusals(ops, pkg):
    y = torch.zeros(2, 3, 8, 8, dtype=torch.complex64, device="cuda")
    m = torch.ones(1, 8, dtype=torch.uint8, device="cuda")
    ops.kspace_time_average(y, m)
    for bad in (y.to(torch.complex128), y.real.contiguous(),
                torch.zeros(2, 3, 8, 16, dtype=torch.complex64, device="cuda")[..., ::2], y.transpose(-1, -2)):
        with pytest.raises(TypeError):                                       # never converted: dtype, strides
            ops.kspace_time_average(bad, m)
    with pytest.raises(RuntimeError):
        ops.kspace_time_average(y.cpu(), m)
    with pytest.raises(RuntimeError):
        ops.kspace_time_average(y, m.cpu())
    for bad in (y[0], y[None, None, None]):                                  # 3-D, 7-D
        with pytest.raises(ValueError):
            ops.kspace_time_average(bad.contiguous(), m)
    with pytest.raises(ValueError):
        ops.kspace_time_average(torch.zeros(2, 1, 3, 2, 8, 8, dtype=torch.complex64, device="cuda"), m)   # a channel dim of 2
    with pytest.raises(TypeError):
        ops.kspace_time_average(y, m.bool())                                 # a non-uint8 mask
    with pytest.raises(ValueError):
        ops.kspace_time_average(y, torch.ones(1, 9, dtype=torch.uint8, device="cuda"))        # the wrong width
    with pytest.raises(ValueError):
        ops.kspace_time_average(y, torch.ones(1, 4, 8, dtype=torch.uint8, device="cuda"))     # the wrong height
    with pytest.raises(ValueError):
        ops.kspace_time_average(y, m, out=torch.empty(2, 1, 8, 8, dtype=torch.complex64, device="cuda"))
    with pytest.raises(pkg.lib.IpdmUnsupported):
        ops.kspace_time_average(torch.zeros(1, 4097, 1, 1, dtype=torch.complex64, device="cuda"),
                                torch.ones(1, 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(pkg.lib.IpdmError):                                   # the output inside the input
        ops.kspace_time_average(y, m, out=y.view(-1)[:2 * 64].view(2, 8, 8))
    torch.cuda.synchronize()


# ---- the pipeline -------------------------------------------------------------------------------------------------------------
PIPE_CASES = [(32, 32, 4, 6, 4, 0), (32, 32, 4, 6, 4, 1), (16, 16, 3, 5, 3, 0)]      # H, W, n, T, R, seed
_PIPE = {}


def pipe_case(case):
    """the cine data of a case (complex64 on the host), its masks, and the float64 chain on the very same numbers"""
    if case not in _PIPE:
        H, W, n, T, R, seed = case
        y, mask, maps, frames = cineh.cine_data(H, W, n, T, R, seed)
        y32 = y.to(torch.complex64)
        region = csmh.calibration_region(cineh.union_mask(mask, H, W), H, W)
        ybar, count = cineh.composite(y32[:, None], mask)
        ybar = torch.from_numpy(ybar)                                        # (n, 1, H, W) complex128
        want = csmh.estimate(ybar, *region, thresh=THRESH)
        w32 = csmh.estimate(ybar.to(torch.complex64), *region, thresh=THRESH, dtype=np.float32)
        _PIPE[case] = dict(y=y32, mask=mask, region=region, ybar=ybar, want=want, w32=w32)
    return _PIPE[case]


def test_time_average_front_end(ops, pkg):
    d = pipe_case(PIPE_CASES[0])
    H, W, n, T, R, seed = PIPE_CASES[0]
    want = ops.kspace_time_average(d["y"].cuda(), ops._mask_u8(d["mask"], H, W, "cuda"))
    for y in (d["y"], d["y"].numpy(), d["y"].cuda(), d["y"].to(torch.complex128), d["y"][:, None, :, None]):
        got = pkg.uf.SENSE.time_average(y, d["mask"])
        assert got.is_cuda and got.dtype == torch.complex64 and tuple(got.shape) == (n, H, W)
        assert torch.equal(view(got), view(want))
    assert torch.equal(view(pkg.uf.SENSE.time_average(d["y"], d["mask"][:, 0])), view(want))   # (T, H, W) masks
    check_composite(want[:, None], torch.from_numpy(cineh.composite(d["y"][:, None], d["mask"])[1]),
                    d["ybar"].numpy(), cineh.composite(d["y"][:, None], d["mask"])[1], "cine data")


@pytest.mark.parametrize("case", PIPE_CASES)
def test_from_cine_measurement_is_the_composition_of_its_ops(ops, pkg, case):
    H, W, n, T, R, seed = case
    d = pipe_case(case)
    yd = d["y"].cuda()
    ybar = ops.kspace_time_average(yd, ops._mask_u8(d["mask"], H, W, "cuda"))
    ah, aw = d["region"]
    cal = pkg.uf.SENSE.from_cine_measurement(d["y"], d["mask"], R=R, seed=seed, thresh=THRESH)
    assert cal.region == (ah, aw) == pkg.uf.calibration_region(d["mask"], H, W, composite=True)
    maps, _, rss_max = ops.estimate_sens_maps(ybar, ah, aw, thresh=THRESH, return_rss=True)
    assert cal.sens_maps.dtype == torch.complex128 and not cal.sens_maps.is_cuda and cal.coil_matrix is None
    assert torch.equal(view(cal.sens_maps.to(torch.complex64)), view(maps.cpu()))
    assert torch.equal(cal.op.sens_maps, cal.sens_maps) and cal.op.num_sens == n
    assert cal.rss_max == float(rss_max[0]) and cal.rss_max > 0
    assert torch.equal(view(cal.measurement), view(yd)) and torch.equal(view(cal.composite), view(ybar))
    assert torch.equal(torch.as_tensor(cal.op.random_under_fourier.mask), d["mask"])
    assert tuple(cal.op.mask_u8("cuda").shape) == (T, H, W)
    # whitened and compressed: one matrix from the composite, applied to every frame and to the composite
    psi = cch.noise_cov(n, 30.0, seed)
    cal = pkg.uf.SENSE.from_cine_measurement(d["y"], d["mask"], R=R, seed=seed, n_virtual=2, noise_cov=psi, thresh=THRESH)
    A = ops.coilcomp_matrix(ops.coil_gram(ybar, ah, aw), 2, psi)[0]
    assert tuple(cal.coil_matrix.shape) == (2, n) and cal.coil_matrix.dtype == torch.complex64 and not cal.coil_matrix.is_cuda
    assert torch.equal(view(cal.coil_matrix), view(A.cpu()))
    assert tuple(cal.measurement.shape) == (2, T, H, W) and torch.equal(view(cal.measurement), view(ops.coil_apply(yd, A)))
    ybar_v = ops.coil_apply(ybar, A)
    assert torch.equal(view(cal.composite), view(ybar_v))
    assert torch.equal(view(cal.sens_maps.to(torch.complex64)), view(ops.estimate_sens_maps(ybar_v, ah, aw, thresh=THRESH).cpu()))
    assert cal.op.num_sens == 2 and cal.region == (ah, aw)
    # compression commutes with the average, to the rounding of the two fp32 applications: each output is a sum of n complex
    # products (relative error about 2n 2^-24 of sum |A||y| <= n max|A| max|y|), on either side of the comparison
    again = ops.kspace_time_average(cal.measurement, ops._mask_u8(d["mask"], H, W, "cuda"))
    tol = 4 * n * n * 2.0 ** -24 * float(A.abs().max()) * float(yd.abs().max())
    assert float((again - ybar_v).abs().max()) <= tol


@pytest.mark.parametrize("case", PIPE_CASES)
def test_maps_vs_the_float64_chain(ops, pkg, case):
    H, W, n, T, R, seed = case
    d = pipe_case(case)
    want, w32 = d["want"], d["w32"]
    cal = pkg.uf.SENSE.from_cine_measurement(d["y"], d["mask"], R=R, seed=seed, thresh=THRESH)
    near = csmh.near_threshold(want["rss"], want["rss_max"], THRESH)
    assert float(near.float().mean()) <= 0.005
    keep = (~near).expand(n, -1, -1, -1)
    err_cpu = float((w32["maps"].to(torch.complex128) - want["maps"]).abs()[keep].max())
    bound = max(BOUND, 4 * err_cpu)
    err = float((cal.sens_maps[:, None] - want["maps"]).abs()[keep].max())
    print(f"cine maps {case}: err_gpu {err:.3e}, err_cpu {err_cpu:.3e}, bound {bound:.3e}, left out {int(near.sum())}, "
          f"support {float(want['support'].float().mean()):.3f}, region {cal.region}")
    assert err <= bound
    assert abs(cal.rss_max - float(want["rss_max"][0])) <= BOUND * float(want["rss_max"][0])


def test_estimated_cine_maps_serve_the_cg_proximal(ops, pkg):
    """frame 0 of the T = 24 cine default at 64 x 64 reconstructed with maps calibrated from the time average (NRMSE of |x|
    inside the support; the three values are printed and recorded in DESIGN.md 4.4g; measured: 0.5231 with the GPU
    pipeline's maps, 0.5231 with the float64 chain's, 0.5424 with uniform maps -- one frame holds a sixteenth of k-space)"""
    H = W = 64
    n, T = 4, 24
    y, mask, true_maps, frames = cineh.cine_data(H, W, n, T, 8, seed=0, kind="line")
    y32 = y.to(torch.complex64)
    cal = pkg.uf.SENSE.from_cine_measurement(y32, mask, R=8, seed=0)
    assert cal.region == (12, 5)
    ybar = torch.from_numpy(cineh.composite(y32[:, None], mask)[0])
    helper = csmh.estimate(ybar, *cal.region)
    sup = helper["support"][0]
    uniform = torch.full((n, H, W), 1 / np.sqrt(n), dtype=torch.complex64)
    y0 = y32[:, 0].reshape(n, 1, 1, H, W).cuda().contiguous()
    mask0 = ops._mask_u8(mask[0], H, W, "cuda")
    z = torch.zeros(1, 1, H, W, device="cuda")
    mag = frames[0].abs().double()

    def nrmse(maps):
        re_, im_, _ = ops.sense_cgprox(z, z.clone(), y0, maps.to(torch.complex64).cuda().contiguous(), mask0, 1e3, max_iter=300, tol=1e-6)
        x = torch.complex(re_, im_)[0, 0].cpu().abs().double()
        return float(torch.sqrt(((x - mag)[sup] ** 2).sum() / (mag[sup] ** 2).sum()))

    e_gpu, e_helper, e_uniform = nrmse(cal.sens_maps), nrmse(helper["maps"][:, 0]), nrmse(uniform)
    print(f"cine frame 0, NRMSE inside the support: GPU maps {e_gpu:.4f}, float64 chain's maps {e_helper:.4f}, uniform maps {e_uniform:.4f}")
    assert abs(e_gpu - e_helper) <= 1e-3
    assert e_gpu < e_uniform and e_helper < e_uniform


# ---- drivers ------------------------------------------------------------------------------------------------------------------
_CINE = ["--image_size", "64", "--start_level", "996", "--n_levels", "2", "--num_samples", "1", "--seed", "0"]
_MAP = ["--ds_name", "CINE127", "--R", "6", "--num_iters", "2", "--lr", "0.001", "--mode_T", "diffusion1d"]


def run_driver(script, args, save_dir):
    """one fresh child process with a time limit"""
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", script)] + args + ["--save_dir", save_dir],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout, lambda name: torch.load(os.path.join(save_dir, name), weights_only=False)


@pytest.fixture(scope="module")
def simulated_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("cine_simulated")
    stdout, load = run_driver("cine_SENSE_real_img_2d_time.py", _CINE + ["--estimate_maps"], str(d))
    return d, stdout, load


def test_cine_driver_estimates_maps(pkg, simulated_run):
    d, stdout, load = simulated_run
    rec, maps, meas, mask = load("reconstructions.pt"), load("sens_maps.pt"), load("measurement.pt"), load("mask.pt")
    assert "reconstruction time" in stdout and "k-space scale" not in stdout
    assert rec.shape == (1, 24, 1, 64, 64) and rec.dtype == torch.complex64 and torch.isfinite(view(rec)).all()
    assert tuple(maps.shape) == (4, 64, 64) and maps.dtype == torch.complex128 and tuple(meas.shape) == (4, 24, 64, 64)
    assert tuple(mask.shape) == (24, 1, 1, 64) and os.path.exists(d / "original.pt") and not os.path.exists(d / "coil_matrix.pt")
    again = pkg.uf.SENSE.from_cine_measurement(meas, mask)
    assert again.region == (12, 5) and float((again.sens_maps - maps).abs().max()) <= BOUND
    true_maps = pkg.uf.SENSE("exp", 4, 8, 0.05, (1, 64, 64), 0).sens_maps
    assert float((maps - true_maps).abs().max()) > 100 * BOUND               # estimated, not the maps the data were made with


def test_cine_driver_compresses_coils(tmp_path):
    _, load = run_driver("cine_SENSE_real_img_2d_time.py", _CINE + ["--estimate_maps", "--coil_compress", "2", "--num_sens", "8"],
                         str(tmp_path))
    A, maps, meas, rec = load("coil_matrix.pt"), load("sens_maps.pt"), load("measurement.pt"), load("reconstructions.pt")
    assert tuple(A.shape) == (2, 8) and A.dtype == torch.complex64
    assert tuple(maps.shape) == (2, 64, 64) and tuple(meas.shape) == (2, 24, 64, 64)
    assert rec.shape == (1, 24, 1, 64, 64) and torch.isfinite(view(rec)).all()


def test_cine_driver_takes_kspace_from_a_file(simulated_run, tmp_path):
    """the simulated measurement of the first run as a measured acquisition: the same data, the same maps, the same Philox
    noise -- the rerun is held to what test_scripts_gpu.py holds a rerun to, equal bits"""
    d, _, load = simulated_run
    torch.save(load("measurement.pt"), tmp_path / "kspace.pt")
    torch.save(load("mask.pt"), tmp_path / "mask.pt")
    out = tmp_path / "measured"
    stdout, load2 = run_driver("cine_SENSE_real_img_2d_time.py",
                               _CINE + ["--kspace", str(tmp_path / "kspace.pt"), "--mask", str(tmp_path / "mask.pt"), "--estimate_maps",
                                        "--kspace_scale", "1.0"], str(out))
    assert float(re.search(r"k-space scale = ([-+0-9.eE]+)", stdout).group(1)) == 1.0
    assert not os.path.exists(out / "original.pt")
    assert torch.equal(view(load2("sens_maps.pt")), view(load("sens_maps.pt")))
    assert torch.equal(view(load2("reconstructions.pt")), view(load("reconstructions.pt")))


def test_cine_MAP_driver_estimates_maps(tmp_path):
    stdout, load = run_driver("cine_SENSE_real_img_2d_time_MAP.py", _MAP + ["--estimate_maps"], str(tmp_path))
    rec, maps = load("reconstructions.pt"), load("sens_maps.pt")
    assert "reconstruction error" in stdout and rec.dim() == 5 and torch.isfinite(view(rec)).all()
    assert maps.dtype == torch.complex128 and maps.shape[0] == 4 and torch.isfinite(view(maps)).all()
