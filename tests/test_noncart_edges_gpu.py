"""Non-Cartesian kernels past one sample stage, one column tile and one grid round.

tests/test_noncart_gpu.py, test_noncart_frames_gpu.py and test_nc_calib_gpu.py compare with float64 at M = 237 samples and
W <= 128: one LDS stage of ndft_adjoint_kernel, one column tile, one grid round of nc_phasor_kernel, H <= W.  The shapes here
(tests/noncart_helpers.py, EDGE_CASES / EDGE_FRAME_CASES; tests/test_noncart_edges_host.py states what each is the first to
run) take every one of those loops past its first round:

1. the seven stage quantities (and the no-maps normal) against float64 at 16x320, 320x16, 8x1024, 2x64 and 64x2, with no
   weights, ramp weights and ramp weights that are exactly zero on whole stages; the two oracle-free identities at 16x320 / 320x16;
2. frame sets of M = 897 = 3 * 256 + 129 samples: rows t::T bit-equal to the one-trajectory call, and against float64;
3. the fixed summation order at 16x320: a call repeated, and row b of a B = 3 call against the B = 1 call, bit for bit;
4. the workspace formulas: every raw entry point with a workspace of exactly the stated bytes, followed in the same tensor
   by a guard of at least that size whose bits must not change;
5. nc_sense_cgprox against the float64 solver at 16x320 and 320x16.

Inputs are the float32 values the GPU gets, references float64, the metric max|err| / max|ref| (nh.relerr).  The bounds are
the TOL tables of test_noncart_gpu.py and test_noncart_frames_gpu.py, unchanged; every observed error is printed."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import noncart_helpers as nh
import test_noncart_gpu as base
import test_noncart_frames_gpu as frames

pytestmark = pytest.mark.gpu

TOL, FTOL = base.TOL, frames.TOL
dev, host, cplx = base.dev, base.host, base.cplx
TILED = ["wide", "tall"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import noncartesian
    return Namespace(nc=noncartesian)


_DEV = {}


def case(name):
    """nh.edge_inputs(name) with its operands on the GPU, made once"""
    if name not in _DEV:
        c = nh.edge_inputs(name)
        _DEV[name] = Namespace(**vars(c), kd=dev(c.k), Sd=dev(c.S), xd=dev(c.x), yd=dev(c.y), imgsd=dev(c.imgs))
    return _DEV[name]


def wdev(r):
    return None if r.w is None else dev(r.w)


# ---- 1. kernel stages against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", nh.EDGE_WEIGHTS)
@pytest.mark.parametrize("name", list(nh.EDGE_CASES))
def test_stages_vs_float64(ops, name, kind):
    c, r = case(name), nh.edge_refs(name, kind)
    H, W, wd = c.H, c.W, wdev(r)
    assert ops.nc_supported(H, W)
    e = {}
    e["forward"] = nh.relerr(host(ops.ndft_forward(c.xd, c.kd, c.Sd)), c.Ax)
    e["forward_coils"] = nh.relerr(host(ops.ndft_forward(c.imgsd, c.kd)), c.Aimgs)
    e["adjoint"] = nh.relerr(host(ops.ndft_adjoint(c.yd, c.kd, H, W, c.Sd, wd)), r.AHy)
    e["adjoint_coils"] = nh.relerr(host(ops.ndft_adjoint(c.yd, c.kd, H, W, None, wd)), r.coil_imgs)
    psf = ops.toeplitz_psf(c.kd, H, W, wd)
    e["psf"] = nh.relerr(host(psf), r.P)
    e["normal"] = nh.relerr(host(ops.toeplitz_normal(c.xd, dev(r.P.astype(np.float32)), c.Sd)), r.Tx)
    e["normal_gpu_psf"] = nh.relerr(host(ops.toeplitz_normal(c.xd, psf, c.Sd)), r.Tx)
    e["normal_nomaps"] = nh.relerr(host(ops.toeplitz_normal(c.xd, psf)), r.Tx_nomaps)       # sens None: S = 1
    print(f"edge stages {name} {H}x{W} B={c.B} n={c.n} M={c.M} weights={kind}: " + "  ".join(f"{k} {v:.3g}" for k, v in e.items()))
    assert psf.dtype == torch.float32 and tuple(psf.shape) == (2 * H, 2 * W)
    for q, v in e.items():
        assert v <= TOL[q.split("_")[0]], (q, v)


@pytest.mark.parametrize("kind", nh.EDGE_WEIGHTS)
@pytest.mark.parametrize("name", TILED)
def test_consistency(ops, name, kind):
    """without an oracle: T x against A^H W A x by the direct kernels, and the dot test <y, A x> = <A^H y, x> (no weights)"""
    c, r = case(name), nh.edge_refs(name, kind)
    H, W, wd = c.H, c.W, wdev(r)
    psf = ops.toeplitz_psf(c.kd, H, W, wd)
    Ax = ops.ndft_forward(c.xd, c.kd, c.Sd)
    direct = host(ops.ndft_adjoint(Ax, c.kd, H, W, c.Sd, wd))
    e_n = nh.relerr(host(ops.toeplitz_normal(c.xd, psf, c.Sd)), direct)
    AHy = host(ops.ndft_adjoint(c.yd, c.kd, H, W, c.Sd))
    lhs = np.vdot(c.y.astype(np.complex128), host(Ax).astype(np.complex128))
    rhs = np.vdot(AHy.astype(np.complex128), c.x.astype(np.complex128))
    e_d = abs(lhs - rhs) / abs(lhs)
    print(f"edge consistency {name} {H}x{W} weights={kind}: normal vs adjoint(forward) {e_n:.3g}  dot {e_d:.3g}")
    assert e_n <= TOL["normal_vs_direct"] and e_d <= TOL["dot"]


# ---- 2. frame sets across stages and grid rounds -------------------------------------------------------------------------
def frame_case(name, weighted):
    """inputs (the float32 values the GPU gets) and the float64 spectra of one framed shape, made once"""
    key = ("frames", name, weighted)
    if key not in _DEV:
        H, W, T, B, n = nh.EDGE_FRAME_CASES[name]
        rng = np.random.default_rng(H * 131 + W + 7 * n + T)
        k = frames.frame_trajectory(T, H, W, spokes=27, readout=33)
        assert np.array_equal(k, nh.frame_trajectory(T, H, W, 27, 33))           # the host file's restatement
        M = k.shape[1]
        w = np.stack([nh.ramp_weights(k[t], H, W) for t in range(T)]).astype(np.float32) if weighted else None
        S = nh.smooth_maps(n, H, W, seed=n) if n > 1 else None                      # n == 1: sens=None in every call
        x = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
        y = (rng.standard_normal((n, B, M)) + 1j * rng.standard_normal((n, B, M))).astype(np.complex64)
        P = np.stack([nh.toeplitz_psf(k[t], H, W, None if w is None else w[t]) for t in range(T)])
        _DEV[key] = Namespace(H=H, W=W, T=T, B=B, n=n, M=M, k=k, w=w, S=S, x=x, y=y, P=P, kd=dev(k),
                              wd=None if w is None else dev(w), Sd=None if S is None else dev(S), xd=dev(x), yd=dev(y))
    return _DEV[key]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", list(nh.EDGE_FRAME_CASES))
def test_framed_rows_equal_the_single_trajectory_call(ops, name, weighted):
    c = frame_case(name, weighted)
    H, W, T, n, xd, yd = c.H, c.W, c.T, c.n, c.xd, c.yd
    assert c.M == 897 and c.B == 2 * T
    coil_imgs = dev(np.stack([c.x] * n) if c.S is None else (c.S[:, None] * c.x[None]).astype(np.complex64))
    z_re, z_im = dev(c.x.real), dev(c.x.imag)
    a, kw = 1.5, dict(max_iter=12, tol=1e-5)
    f_fwd = ops.ndft_forward(xd, c.kd, c.Sd) if c.Sd is not None else ops.ndft_forward(xd[None], c.kd)
    f_fwd_coils = ops.ndft_forward(coil_imgs, c.kd)
    f_adj = ops.ndft_adjoint(yd, c.kd, H, W, c.Sd, c.wd)
    f_adj_coils = ops.ndft_adjoint(yd, c.kd, H, W, None, c.wd)
    f_psf = ops.toeplitz_psf(c.kd, H, W, c.wd)
    assert tuple(f_psf.shape) == (T, 2 * H, 2 * W) and f_psf.dtype == torch.float32
    ahy = f_adj if c.Sd is not None else f_adj_coils[0].contiguous()
    f_nrm = ops.toeplitz_normal(xd, f_psf, c.Sd)
    f_cg = ops.nc_sense_cgprox(z_re, z_im, ahy, c.Sd, f_psf, a, **kw)
    assert (0 < host(f_cg[2])).all()

    def adj_rows(t_, rows):                                                       # combined: [B, H, W]; sens None: [1, B, H, W]
        return t_[rows] if c.Sd is not None else t_[:, rows]
    for t in range(T):
        kt, wt, rows = c.kd[t].contiguous(), frames.wt(c, t), slice(t, None, T)
        r_fwd = ops.ndft_forward(xd, kt, c.Sd) if c.Sd is not None else ops.ndft_forward(xd[None], kt)
        assert torch.equal(f_fwd[:, rows], r_fwd[:, rows]), ("forward", t)
        assert torch.equal(f_fwd_coils[:, rows], ops.ndft_forward(coil_imgs, kt)[:, rows]), ("forward, coil images", t)
        assert torch.equal(adj_rows(f_adj, rows), adj_rows(ops.ndft_adjoint(yd, kt, H, W, c.Sd, wt), rows)), ("adjoint", t)
        assert torch.equal(f_adj_coils[:, rows], ops.ndft_adjoint(yd, kt, H, W, None, wt)[:, rows]), ("adjoint, coil images", t)
        pt = ops.toeplitz_psf(kt, H, W, wt)
        assert torch.equal(f_psf[t], pt), ("psf", t)
        assert torch.equal(f_nrm[rows], ops.toeplitz_normal(xd, pt, c.Sd)[rows]), ("normal", t)
        r_cg = ops.nc_sense_cgprox(z_re, z_im, ahy, c.Sd, pt, a, **kw)
        assert all(torch.equal(f[rows], r[rows]) for f, r in zip(f_cg, r_cg)), ("cgprox", t)
    # the frames are told apart: rows of frame 0 computed with frame 1's trajectory are other bits
    assert not torch.equal(f_fwd[:, 0], (ops.ndft_forward(xd, c.kd[1].contiguous(), c.Sd) if c.Sd is not None
                                         else ops.ndft_forward(xd[None], c.kd[1].contiguous()))[:, 0])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", list(nh.EDGE_FRAME_CASES))
def test_framed_calls_vs_float64(ops, pkg, name, weighted):
    c = frame_case(name, weighted)
    H, W, T, xd, yd = c.H, c.W, c.T, c.xd, c.yd
    w = (lambda t: None) if c.w is None else (lambda t: c.w[t])
    e = {}
    fwd = ops.ndft_forward(xd, c.kd, c.Sd) if c.Sd is not None else ops.ndft_forward(xd[None], c.kd)
    e["forward"] = frames._frame_err(host(fwd), lambda t: nh.sense_forward(c.x, c.S, c.k[t]), T, 1)
    if c.Sd is not None:
        e["adjoint"] = frames._frame_err(host(ops.ndft_adjoint(yd, c.kd, H, W, c.Sd, c.wd)),
                                         lambda t: nh.sense_adjoint(c.y, c.S, c.k[t], H, W, w(t)), T, 0)
    e["adjoint_coils"] = frames._frame_err(host(ops.ndft_adjoint(yd, c.kd, H, W, None, c.wd)),
                                           lambda t: nh.ndft_adjoint(c.y, c.k[t], H, W, w(t)), T, 1)
    psf = ops.toeplitz_psf(c.kd, H, W, c.wd)
    e["psf"] = max(nh.relerr(host(psf[t]), c.P[t]) for t in range(T))
    e["normal"] = frames._frame_err(host(ops.toeplitz_normal(xd, psf, c.Sd)), lambda t: nh.toeplitz_normal(c.x, c.S, c.P[t]), T, 0)
    # the dot test over the framed batch, through the operator: <y, A x> = <A^H y, x>, no weights
    op = pkg.nc.NonCartesianSENSE(c.k, (1, H, W), sens_maps=c.S, normalize=False)
    Ax = host(op(xd[:, None])).astype(np.complex128)[:, :, 0]
    AHy = host(op.conj_op(yd[:, :, None])).astype(np.complex128)[:, 0]
    lhs, rhs = np.vdot(c.y.astype(np.complex128), Ax), np.vdot(AHy, c.x.astype(np.complex128))
    e["dot"] = abs(lhs - rhs) / abs(lhs)
    print(f"edge framed stages {name} {H}x{W} T={T} B={c.B} n={c.n} M={c.M} weighted={weighted}: "
          + "  ".join(f"{k} {v:.3g}" for k, v in e.items()))
    for q, v in e.items():
        assert v <= FTOL[q.split("_")[0]], (q, v)


# ---- 3. fixed order ------------------------------------------------------------------------------------------------------
def test_repeated_calls_give_equal_bits(ops):
    c, r = case("wide"), nh.edge_refs("wide", "ramp")
    wd = wdev(r)
    for what, f in (("forward", lambda: ops.ndft_forward(c.xd, c.kd, c.Sd)),
                    ("adjoint", lambda: ops.ndft_adjoint(c.yd, c.kd, c.H, c.W, c.Sd, wd)),
                    ("psf", lambda: ops.toeplitz_psf(c.kd, c.H, c.W, wd))):
        first, second = f(), f()
        assert torch.equal(first, second), what


def test_batch_row_equals_the_single_image_call(ops):
    """row b of a B = 3 call == the B = 1 call on that image: no sum depends on the batch the image sits in"""
    c, r = case("wide"), nh.edge_refs("wide", "ramp")
    H, W, n, M, wd = c.H, c.W, c.n, c.M, wdev(r)
    rng = np.random.default_rng(3)
    x = dev((rng.standard_normal((3, H, W)) + 1j * rng.standard_normal((3, H, W))).astype(np.complex64))
    y = dev((rng.standard_normal((n, 3, M)) + 1j * rng.standard_normal((n, 3, M))).astype(np.complex64))
    psf = ops.toeplitz_psf(c.kd, H, W, wd)
    fwd, adj, adj_coils = ops.ndft_forward(x, c.kd, c.Sd), ops.ndft_adjoint(y, c.kd, H, W, c.Sd, wd), ops.ndft_adjoint(y, c.kd, H, W, None, wd)
    nrm = ops.toeplitz_normal(x, psf, c.Sd)
    for b in range(3):
        xb, yb = x[b:b + 1].contiguous(), y[:, b:b + 1].contiguous()
        assert torch.equal(fwd[:, b], ops.ndft_forward(xb, c.kd, c.Sd)[:, 0]), ("forward", b)
        assert torch.equal(adj[b], ops.ndft_adjoint(yb, c.kd, H, W, c.Sd, wd)[0]), ("adjoint", b)
        assert torch.equal(adj_coils[:, b], ops.ndft_adjoint(yb, c.kd, H, W, None, wd)[:, 0]), ("adjoint, coil images", b)
        assert torch.equal(nrm[b], ops.toeplitz_normal(xb, psf, c.Sd)[0]), ("normal", b)
    assert not torch.equal(fwd[:, 0], fwd[:, 1])


# ---- 4. workspace footprints ---------------------------------------------------------------------------------------------
GUARD = 0x5A5A5A5A                               # the guard's bit pattern, as int32


def guarded(nbytes):
    """-> (head, tail) of ONE int32 tensor prefilled with GUARD: head is exactly `nbytes` (the workspace handed to the
    kernel), tail at least as large.  An overrun of the formula lands in the tail -- inside the allocation -- and is seen"""
    assert nbytes > 0 and nbytes % 8 == 0
    words = nbytes // 4
    buf = torch.full((2 * words + 64,), GUARD, dtype=torch.int32, device="cuda")
    return buf[:words], buf[words:]


def tail_untouched(tail):
    return bool((tail == GUARD).all())


def _footprint_case(which):
    """-> (H, W, T, B, n, M, kd [T, M, 2], wd [T, M], Sd, xd, yd): the wide case as one set, or the framed 16 x 320 case"""
    if which == "wide":
        c, r = case("wide"), nh.edge_refs("wide", "ramp")
        return c.H, c.W, 1, c.B, c.n, c.M, c.kd[None].contiguous(), wdev(r)[None].contiguous(), c.Sd, c.xd, c.yd
    c = frame_case("wide", True)
    return c.H, c.W, c.T, c.B, c.n, c.M, c.kd, c.wd, c.Sd, c.xd, c.yd


def _wrapper_operands(T, kd, wd):
    """the wrapper's form of the same trajectory: [M, 2] for one set"""
    return (kd[0].contiguous(), wd[0].contiguous()) if T == 1 else (kd, wd)


@pytest.mark.parametrize("which", ["wide", "framed"])
@pytest.mark.parametrize("entry", ["forward", "adjoint", "psf", "normal", "cgprox"])
def test_workspace_footprint(ops, entry, which):
    from inverseproblemwithdiffusionmodel_amd import _lib
    L, ptr, st = _lib.lib, ops._ptr, ops._stream
    H, W, T, B, n, M, kd, wd, Sd, xd, yd = _footprint_case(which)
    k_w, w_w = _wrapper_operands(T, kd, wd)
    if entry == "forward":
        need = L.ipdm_ndft_workspace_bytes(T * M, H, W)
        assert need == (H + 2 * W) * T * M * 8
        head, tail = guarded(need)
        got = torch.empty((n, B, M), dtype=torch.complex64, device="cuda")
        ops.call("ipdm_ndft_forward_sets_c64", ptr(xd), ptr(Sd), ptr(kd), T, ptr(got), ptr(head), B, n, M, H, W, st())
        want = ops.ndft_forward(xd, k_w, Sd)
    elif entry == "adjoint":
        need = L.ipdm_ndft_workspace_bytes(T * M, H, W)
        head, tail = guarded(need)
        got = torch.empty((B, H, W), dtype=torch.complex64, device="cuda")
        ops.call("ipdm_ndft_adjoint_sets_c64", ptr(yd), ptr(Sd), ptr(kd), T, ptr(wd), ptr(got), ptr(head), B, n, M, H, W, st())
        want = ops.ndft_adjoint(yd, k_w, H, W, Sd, w_w)
        got2 = torch.empty((n, B, H, W), dtype=torch.complex64, device="cuda")             # the coil-image instantiation
        ops.call("ipdm_ndft_adjoint_sets_c64", ptr(yd), ptr(None), ptr(kd), T, ptr(wd), ptr(got2), ptr(head), B, n, M, H, W, st())
        assert torch.equal(got2, ops.ndft_adjoint(yd, k_w, H, W, None, w_w))
    elif entry == "psf":
        need = L.ipdm_toeplitz_psf_workspace_bytes(M, H, W)
        assert need == (2 * H + 4 * W) * M * 16 + 4 * H * W * 8                            # one set's: the sets share it
        head, tail = guarded(need)
        got = torch.empty((T, 2 * H, 2 * W), dtype=torch.float32, device="cuda")
        ops.call("ipdm_toeplitz_psf_sets_f32", ptr(kd), T, ptr(wd), ptr(got), ptr(head), M, H, W, st())
        want = ops.toeplitz_psf(k_w, H, W, w_w).reshape(T, 2 * H, 2 * W)
    elif entry == "normal":
        need = L.ipdm_toeplitz_workspace_bytes(B, n, H, W)
        assert need == n * B * H * 2 * W * 8
        psf = ops.toeplitz_psf(k_w, H, W, w_w)
        head, tail = guarded(need)
        got = torch.empty((B, H, W), dtype=torch.complex64, device="cuda")
        ops.call("ipdm_toeplitz_normal_sets_c64", ptr(xd), ptr(Sd), ptr(psf), T, ptr(got), ptr(head), B, n, H, W, st())
        want = ops.toeplitz_normal(xd, psf, Sd)
    else:
        need = L.ipdm_nc_sense_cg_workspace_bytes(B, n, H, W)
        assert need == (2 * n + 3) * B * H * W * 8 + B * 16
        psf = ops.toeplitz_psf(k_w, H, W, w_w)
        ahy = ops.ndft_adjoint(yd, k_w, H, W, Sd, w_w)
        z_re, z_im = xd.real.contiguous(), xd.imag.contiguous()
        head, tail = guarded(need)
        work = head.view(torch.float32)
        assert work.is_contiguous() and work.numel() * 4 == need
        got = torch.stack(ops.nc_sense_cgprox(z_re, z_im, ahy, Sd, psf, 1.5, max_iter=12, tol=1e-5, work=work)[:2])
        o_re, o_im, iters = ops.nc_sense_cgprox(z_re, z_im, ahy, Sd, psf, 1.5, max_iter=12, tol=1e-5)
        want = torch.stack((o_re, o_im))
        assert (0 < host(iters)).all()
    torch.cuda.synchronize()
    assert tail.numel() * 4 >= need and tail_untouched(tail), f"{entry}: the kernels wrote past the stated {need} workspace bytes"
    assert not tail_untouched(head)                                                        # the workspace was the one used
    assert torch.equal(got, want), entry


# ---- 5. the proximal at a tiled shape --------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [1.0, 4.0])
@pytest.mark.parametrize("H,W", [(16, 320), (320, 16)])
def test_cgprox_vs_float64(ops, H, W, a):
    p, ahy64, ref, it64 = nh.prox_reference(H, W, 27, 64, 2, 3, a, 40, 1e-5)
    kd, Sd = dev(p.k), dev(p.S)
    ahy = ops.ndft_adjoint(dev(p.y), kd, H, W, Sd)
    psf = ops.toeplitz_psf(kd, H, W)
    o_re, o_im, iters = ops.nc_sense_cgprox(dev(p.z.real), dev(p.z.imag), ahy, Sd, psf, a, max_iter=40, tol=1e-5)
    x = cplx(o_re, o_im)
    res = nh.prox_residual(x, p.z.astype(np.complex128), ahy64, p.S, p.k, a)
    err = nh.relerr(x, ref)
    it = host(iters)
    print(f"edge cgprox {H}x{W} a={a}: iters {it} float64 iters {it64}  |x - x64| {err:.3g}  residual {res}")
    assert (0 < it64).all() and (it64 < 40).all(), "the float64 reference itself must converge below the cap"
    assert (0 < it).all() and (it < 40).all()
    assert err <= TOL["cg_solution"] and res.max() <= TOL["cg_residual"]
