"""Geometric coil compression along the readout on the GPU (csrc/gcc.hip) against tests/gcc_helpers.py.

Individual matrices A_x estimated from data are NOT compared with float64: towards the edge of the field of view the
retained subspace is ill-conditioned (eigenvalue ratios up to 0.98), so they are held to the properties that define them
-- orthonormal rows in the psi inner product, the retained energy, a Hermitian positive semidefinite product with the
neighbour -- and to the float64 alignment only on a designed input whose polar factors are well-conditioned.

Bounds, the protocol of test_coilcomp_gpu.py: a quantity's bound is 4 err_cpu, err_cpu being the same quantity from the
helper's single-precision run on the same input; err_cpu <= 1e-3 is asserted.  err_gpu and err_cpu are printed per case
(DESIGN.md 4.4j tables them)."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import coilcomp_helpers as cch
import gcc_helpers as gh

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def pkg():
    from inverseproblemwithdiffusionmodel_amd import _lib, engine, synthetic
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, proximal_op
    return Namespace(lib=_lib, syn=synthetic, uf=undersampling_fourier, engine=engine, ncsnv2=ncsnv2, prox=proximal_op)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.complex64).cuda().contiguous()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def check(what, err_gpu, err_cpu):
    print(f"{what}: err_gpu {err_gpu:.3e}, err_cpu {err_cpu:.3e}, bound {4 * err_cpu:.3e}")
    assert err_cpu <= 1e-3
    assert err_gpu <= 4 * err_cpu


def rounded(a):
    """complex128 values that complex64 holds exactly"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def c64(a):
    return np.asarray(a).astype(np.complex64)


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


SCALES = (1.0, 1e-3, 1e3)


def designed_psi(n, cond=300.0):
    return rounded(cch.noise_cov(n, cond, n))


# ---- 1. the readout transform ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 8), (16, 24), (48, 8), (80, 24), (256, 24)])
def test_readout_fft_vs_float64(ops, H, W):
    rng = np.random.default_rng(H)
    x = rounded(rng.standard_normal((3, H, W)) + 1j * rng.standard_normal((3, H, W)))
    x[:, :, 2] = 0                                                           # a column that is exactly zero
    xd = dev(x)
    for inverse in (False, True):
        want, cpu = gh.readout(x, inverse), gh.readout(c64(x), inverse, np.float32)
        got = ops.readout_fft(xd, inverse=inverse)
        assert got.dtype == torch.complex64 and got.shape == xd.shape
        top = np.abs(want).max()
        check(f"readout {'inverse' if inverse else 'forward'} H {H} W {W}", np.abs(host(got) - want).max() / top,
              np.abs(cpu - want).max() / top)
        assert not bits(got[:, :, 2]).any()                                  # ... stays exactly zero
        for b in range(3):                                                   # alone and inside the batch: the same bits
            assert torch.equal(bits(ops.readout_fft(xd[b].contiguous(), inverse=inverse)), bits(got[b]))
    back = ops.readout_fft(ops.readout_fft(xd, inverse=True))
    cpu = gh.readout(gh.readout(c64(x), True, np.float32), False, np.float32)
    check(f"readout forward(inverse) H {H} W {W}", np.abs(host(back) - x).max() / np.abs(x).max(), np.abs(cpu - x).max() / np.abs(x).max())
    inplace = xd.clone()
    assert ops.readout_fft(inplace, inverse=True, out=inplace) is inplace    # a strip is read whole before it is stored
    assert torch.equal(bits(inplace), bits(ops.readout_fft(xd, inverse=True)))


def test_readout_fft_operand_checks(ops, pkg):
    x = torch.zeros(2, 16, 8, dtype=torch.complex64, device="cuda")
    with pytest.raises(TypeError):
        ops.readout_fft(x.to(torch.complex128))
    with pytest.raises(TypeError):
        ops.readout_fft(x.real.contiguous())
    with pytest.raises(TypeError):
        ops.readout_fft(x.transpose(-1, -2))                                 # strided
    with pytest.raises(ValueError):
        ops.readout_fft(x, out=torch.zeros(2, 16, 4, dtype=torch.complex64, device="cuda"))
    with pytest.raises(pkg.lib.IpdmUnsupported):
        ops.readout_fft(torch.zeros(2, 24, 8, dtype=torch.complex64, device="cuda"))
    big = torch.zeros(3, 16, 8, dtype=torch.complex64, device="cuda")
    with pytest.raises(pkg.lib.IpdmError):                                   # a partial overlap of out and x
        ops.readout_fft(big[:2], out=big[1:])


# ---- 2. windowed Gram matrices ----------------------------------------------------------------------------------------------------
GRAM_CASES = [(1, 16, 16, 2, 0), (3, 16, 16, 2, 3), (9, 32, 16, 3, 1), (33, 16, 32, 5, 2), (64, 16, 32, 12, 2)]


def hybrid_data(n, H, W):
    return cached(("h", n, H, W), lambda: rounded(gh.readout(cch.coil_data(H, W, n, B=3, seed=n, scales=SCALES), True)))


@pytest.mark.parametrize("n,H,W,aw,win", GRAM_CASES)
def test_gram_vs_float64(ops, n, H, W, aw, win):
    h = hybrid_data(n, H, W)
    want, cpu = gh.gram(h, aw, win), gh.gram(c64(h), aw, win, np.float32)
    hd = dev(h)
    G = ops.gcc_gram(hd, aw, win)
    assert G.dtype == torch.complex64 and tuple(G.shape) == (3, H, n, n)
    got = host(G)
    for b in range(3):                                                       # each image against its own scale
        for rows, xs in (("first", [0]), ("last", [H - 1]), ("all", range(H))):      # the clipped windows on their own
            xs = list(xs)
            top = np.abs(want[b, xs]).max()
            check(f"gcc gram {n} coils {H}x{W} aw {aw} win {win} scale {SCALES[b]:g} {rows} rows",
                  np.abs(got[b, xs] - want[b, xs]).max() / top, np.abs(cpu[b, xs].astype(np.complex128) - want[b, xs]).max() / top)
    assert np.array_equal(got, got.conj().transpose(0, 1, 3, 2))             # exactly Hermitian
    assert not np.diagonal(got, axis1=2, axis2=3).imag.any()
    assert torch.equal(bits(ops.gcc_gram(hd[:, 1].contiguous(), aw, win)), bits(G[1:2]))          # (n, H, W) is the same call
    # win = 0 at the centre row is coil_gram of that row's box
    G0 = host(ops.gcc_gram(hd, aw, 0))[:, H // 2]
    box = host(ops.coil_gram(hd, 0, aw))
    w0, c0 = gh.gram(h, aw, 0)[:, H // 2], gh.gram(c64(h), aw, 0, np.float32)[:, H // 2]
    for b in range(3):
        top = np.abs(w0[b]).max()
        check(f"gcc gram win 0 row {H // 2} against coil_gram, scale {SCALES[b]:g}", np.abs(G0[b] - box[b]).max() / top,
              np.abs(c0[b].astype(np.complex128) - w0[b]).max() / top)


# ---- 3. alignment on the designed input ---------------------------------------------------------------------------------------------
ALIGN_CASES = [(1, 2, 16), (3, 8, 16), (4, 9, 48), (32, 64, 16)]


def ortho_err(A, psi):
    M = np.eye(A.shape[-1]) if psi is None else psi
    A = A.astype(np.complex128)
    return max(np.abs(a @ M @ a.conj().T - np.eye(a.shape[0])).max() for a in A)


@pytest.mark.parametrize("psi_cond", [None, 300.0])
@pytest.mark.parametrize("nv,n,H", ALIGN_CASES)
def test_align_designed_input_vs_float64_svd(ops, nv, n, H, psi_cond):
    psi = None if psi_cond is None else designed_psi(n, psi_cond)
    Ahat = rounded(gh.designed_matrices(nv, n, H, seed=n, noise_cov=psi))
    ref = gh.align(Ahat, psi)
    cpu = gh.align(c64(Ahat), None if psi is None else c64(psi), np.float32)
    assert ref["smin"] >= 0.2 and ref["status"].tolist() == [0] and cpu["status"].tolist() == [0]
    A, status = ops.gcc_align(dev(Ahat), noise_cov=psi, return_status=True)
    assert tuple(A.shape) == (H, nv, n) and status.tolist() == [0]
    got = host(A)
    what = f"align {nv}x{n} H {H} psi {psi_cond}"
    check(what + " A against the float64 SVD", np.abs(got - ref["A"]).max(), np.abs(cpu["A"] - ref["A"]).max())
    check(what + " |A psi A^H - I|", ortho_err(got, psi), ortho_err(cpu["A"], psi))
    assert np.array_equal(got[H // 2], c64(Ahat[H // 2]))                    # the centre row: the input's bits
    batch = ops.gcc_align(dev(np.stack([Ahat, Ahat[::-1]])), noise_cov=psi)  # (B, H, nv, n); image 0 as alone
    assert torch.equal(bits(batch[0]), bits(A))


def test_align_degenerate_position(ops):
    nv, n, H = 3, 8, 16
    Ahat = rounded(gh.designed_matrices(nv, n, H, seed=n))
    clean = ops.gcc_align(dev(Ahat))
    Ahat[3] = 0
    A, status = ops.gcc_align(dev(Ahat), return_status=True)
    ref = gh.align(Ahat)
    assert status.tolist() == [1] and ref["status"].tolist() == [1]
    assert not bits(A[3]).any()                                              # A_3 = Ahat_3
    assert torch.equal(bits(A[H // 2:]), bits(clean[H // 2:]))               # the other direction is not disturbed
    assert torch.equal(bits(A[4:H // 2]), bits(clean[4:H // 2]))
    cpu = gh.align(c64(Ahat), None, np.float32)
    check("align past a degenerate position", np.abs(host(A) - ref["A"]).max(), np.abs(cpu["A"] - ref["A"]).max())


# ---- 4. the whole chain: properties --------------------------------------------------------------------------------------------------
CHAIN_CASES = [(12, 3, 32, 16, 3, 1, False), (8, 1, 16, 16, 2, 0, False), (64, 32, 16, 32, 12, 2, True)]


def chain_data(n, H, W, seed=None):
    return cached(("y", n, H, W, seed), lambda: rounded(cch.coil_data(H, W, n, B=1, seed=n if seed is None else seed)))


def chain_quantities(A, G, psi):
    """(|A psi A^H - I|, retained-energy error against the top eigenvalues, neighbour product: departure from Hermitian
    positive semidefinite), each the largest over x; G the float64 Gram matrices (H, n, n), A (H, nv, n)"""
    A = A.astype(np.complex128)
    H, nv, n = A.shape
    M = np.eye(n) if psi is None else psi
    X = np.eye(n) if psi is None else np.linalg.inv(np.linalg.cholesky(psi))
    ortho = energy = neigh = 0.0
    for x in range(H):
        ortho = max(ortho, np.abs(A[x] @ M @ A[x].conj().T - np.eye(nv)).max())
        Gw = X @ G[x] @ X.conj().T
        lam = np.linalg.eigvalsh(cch.hermitian(Gw))[::-1]
        energy = max(energy, abs(np.trace(A[x] @ G[x] @ A[x].conj().T).real - lam[:nv].sum()) / lam.sum())
        if x != H // 2:
            C = A[x] @ M @ A[x + (1 if x < H // 2 else -1)].conj().T
            neigh = max(neigh, np.abs(C - C.conj().T).max(), -np.linalg.eigvalsh(0.5 * (C + C.conj().T)).min())
    return ortho, energy, neigh


@pytest.mark.parametrize("n,nv,H,W,aw,win,whiten", CHAIN_CASES)
def test_chain_properties(ops, n, nv, H, W, aw, win, whiten):
    y = chain_data(n, H, W)
    psi = designed_psi(n) if whiten else None
    ref = gh.compress(y, aw, nv, win, psi)
    cpu = gh.compress(c64(y), aw, nv, win, None if psi is None else c64(psi), np.float32)
    out, A, eig, status = ops.coil_compress_geometric(dev(y), aw, nv, win, noise_cov=psi, return_matrix=True)
    assert tuple(out.shape) == (nv, 1, H, W) and tuple(A.shape) == (1, H, nv, n) and tuple(eig.shape) == (1, H, n)
    assert status.tolist() == [0] and cpu["status"].tolist() == [0] and ref["status"].tolist() == [0]
    q_gpu, q_cpu = chain_quantities(host(A)[0], ref["gram"][0], psi), chain_quantities(cpu["A"][0], ref["gram"][0], psi)
    what = f"chain {n} -> {nv}, {H}x{W}, aw {aw}, win {win}{', psi' if whiten else ''}"
    for name, g, c in zip(("|A psi A^H - I|", "retained energy", "neighbour product"), q_gpu, q_cpu):
        check(f"{what}: {name}", g, c)
    lam = host(eig)[0].astype(np.float64)
    assert (np.diff(lam, axis=-1) <= 0).all()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv,H,W,aw,win,seed", gh.END_TO_END)
def test_end_to_end_loss(ops, n, nv, H, W, aw, win, seed):
    """Measured (MI355X; GCC loss float64 / fp32 helper / GPU, then SCC loss of ops.coil_compress on the GPU): see DESIGN.md
    4.4j."""
    y = chain_data(n, H, W, seed)
    ref, cpu = gh.compress(y, aw, nv, win), gh.compress(c64(y), aw, nv, win, dtype=np.float32)
    yd = dev(y)
    out = ops.coil_compress_geometric(yd, aw, nv, win)
    l_ref, l_cpu, l_gpu = gh.loss(y, ref["y"]), gh.loss(y, cpu["y"]), gh.loss(y, host(out))
    l_scc = gh.loss(y, host(ops.coil_compress(yd, aw, aw, nv)))
    print(f"{n} -> {nv}, {H}x{W}, aw {aw}, win {win}: GCC loss float64 {l_ref:.6e}, fp32 helper {l_cpu:.6e}, GPU {l_gpu:.6e}; "
          f"SCC loss GPU {l_scc:.6e}, float64 {gh.scc_loss(y, aw, nv):.6e}; GCC / SCC on the GPU {l_gpu / l_scc:.3f}")
    check(f"loss {n} -> {nv}, {H}x{W}", abs(l_gpu - l_ref), abs(l_cpu - l_ref))
    assert l_gpu <= 0.5 * l_scc
    mask = gh.line_mask(W, aw)
    assert not mask.all()
    masked = ops.coil_compress_geometric(dev(y * mask[None, None, None, :]), aw, nv, win)
    assert not bits(masked[..., torch.from_numpy(~mask).cuda()]).any()       # unsampled columns: exactly zero
    assert masked.abs().sum() > 0


# ---- 6. compressed maps --------------------------------------------------------------------------------------------------------------
def test_compressed_maps_are_consistent(ops, pkg):
    n, nv, H, W, aw, win = 12, 3, 32, 16, 3, 1
    maps = pkg.syn.complex_coil_maps(n, H, W, 0).to(torch.complex64).cuda().contiguous()
    x = pkg.syn.phantom_image(H, W, seed=1)[0].to(torch.complex64).cuda().contiguous()            # (1, H, W)
    ones = torch.ones(1, W, dtype=torch.uint8, device="cuda")
    y = ops.sense_forward(x, maps, ones)                                     # (n, 1, H, W): the physical measurement
    yc, A, _, status = ops.coil_compress_geometric(y, aw, nv, win, return_matrix=True)
    assert status.tolist() == [0]
    vmaps = ops.coil_apply_rows(maps[:, None].contiguous(), A[0].contiguous())                    # shared (H, nv, n) form
    assert tuple(vmaps.shape) == (nv, 1, H, W)
    assert torch.equal(bits(vmaps), bits(ops.coil_apply_rows(maps[:, None].contiguous(), A)))     # per-image form: the same bits
    via_maps = ops.sense_forward(x, vmaps[:, 0].contiguous(), ones)
    # the float64 value of R A R^-1 y with the GPU's matrices, and the helper's single-precision run of the same
    yh, Ah = host(y), host(A)
    want = gh.readout(gh.apply_rows(gh.readout(yh, True), Ah), False)
    cpu = gh.readout(gh.apply_rows(gh.readout(yh, True, np.float32), Ah, np.float32), False, np.float32)
    top = np.abs(want).max()
    err_cpu = np.abs(cpu - want).max() / top
    check("compressed measurement", np.abs(host(yc) - want).max() / top, err_cpu)
    check("forward model on the compressed maps", np.abs(host(via_maps) - want).max() / top, err_cpu)
    with pytest.raises(pkg.lib.IpdmError):                                   # out inside y
        ops.coil_apply_rows(y, A, out=y[:nv])
    with pytest.raises(ValueError):
        ops.coil_apply_rows(y, A[:, :-1].contiguous())
    with pytest.raises(TypeError):
        ops.coil_apply_rows(y, A.to(torch.complex128))


# ---- 7. invariance and capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whiten", [False, True])
def test_batch_invariance_and_determinism(ops, whiten):
    n, nv, H, W, aw, win = 9, 4, 32, 16, 3, 1
    psi = designed_psi(n) if whiten else None
    yd = dev(rounded(cch.coil_data(H, W, n, B=3, seed=n, scales=SCALES)))

    def run(t):
        return ops.coil_compress_geometric(t, aw, nv, win, noise_cov=psi, return_matrix=True)
    alone = [run(yd[:, b:b + 1].contiguous()) for b in range(3)]
    for shift in range(3):                                                   # image b at position (b + shift) % 3
        order = [(p - shift) % 3 for p in range(3)]
        out, A, eig, status = run(yd[:, order].contiguous())
        assert status.tolist() == [0, 0, 0]
        for p, b in enumerate(order):
            assert torch.equal(bits(out[:, p]), bits(alone[b][0][:, 0])) and torch.equal(bits(A[p]), bits(alone[b][1][0]))
            assert torch.equal(eig[p], alone[b][2][0])
    first, again = run(yd), run(yd)                                          # a second call: the same bits
    for a, b in zip(first, again):
        assert torch.equal(bits(a), bits(b))
    single = run(yd[:, 1].contiguous())                                      # (n, H, W) is B = 1
    assert tuple(single[0].shape) == (nv, H, W) and torch.equal(bits(single[0]), bits(first[0][:, 1]))
    assert torch.equal(bits(single[1][0]), bits(first[1][1]))
    # the one call is the five steps
    h = ops.readout_fft(yd, inverse=True)
    Ahat, eig, st = ops.coilcomp_matrix(ops.gcc_gram(h, aw, win).reshape(3 * H, n, n), nv, noise_cov=psi, return_eig=True)
    A = ops.gcc_align(Ahat.reshape(3, H, nv, n), noise_cov=psi)
    out = ops.readout_fft(ops.coil_apply_rows(h, A))
    assert torch.equal(bits(A), bits(first[1])) and torch.equal(bits(out), bits(first[0])) and torch.equal(eig.reshape(3, H, n), first[2])


def test_graph_capture_and_replay(ops):
    n, nv, H, W, aw, win = 9, 4, 32, 16, 3, 1
    y = rounded(cch.coil_data(H, W, n, B=3, seed=n, scales=SCALES))
    y1, y2 = dev(y), dev(y[:, [2, 0, 1]] * 0.5)
    static = y1.clone()
    work = ops.gcc_workspace(3, n, nv, H, W, "cuda")
    assert work.numel() * 4 == ops._lib.lib.ipdm_gcc_workspace_bytes(3, n, nv, H, W)
    ops.coil_compress_geometric(static, aw, nv, win, work=work)              # warm-up: allocator, LDS opt-in
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, A, eig, status = ops.coil_compress_geometric(static, aw, nv, win, return_matrix=True, work=work)
    for src in (y2, y1):
        static.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        e_out, e_A, e_eig, e_status = ops.coil_compress_geometric(src, aw, nv, win, return_matrix=True)
        assert torch.equal(bits(out), bits(e_out)) and torch.equal(bits(A), bits(e_A)) and torch.equal(eig, e_eig)
        assert torch.equal(status, e_status) and out.abs().sum() > 0
    with pytest.raises(ValueError):
        ops.coil_compress_geometric(static, aw, nv, win, work=work[:-2])


# ---- 8. upper layers -------------------------------------------------------------------------------------------------------------------
def _line_mask(W):
    m = torch.zeros(W, dtype=torch.bool)
    m[::3] = True
    m[W // 2 - 8:W // 2 + 9] = True
    return m


def tiny_config():
    """the tiny NCSNv2Deepest configuration of the sampler tests"""
    return Namespace(
        device=torch.device("cuda"),
        data=Namespace(channels=1, image_size=32, logit_transform=False, rescaled=False,
                       uniform_dequantization=False, gaussian_dequantization=False),
        model=Namespace(ngf=4, num_classes=10, sigma_begin=1.0, sigma_end=0.01, sigma_dist="geometric",
                        normalization="InstanceNorm++", nonlinearity="elu", spec_norm=False),
        recons=Namespace(sigma_dist="geometric", sigma_begin=1.0, sigma_end=0.01, num_classes=10),
        sampling=Namespace(n_steps_each=3, step_lr=9e-7, final_only=True, denoise=True))


def test_operator_front_end(ops, pkg):
    S, n, nv, H, W = 2, 8, 3, 32, 32
    mask = _line_mask(W)
    y = torch.from_numpy(np.stack([rounded(cch.coil_data(H, W, n, B=1, seed=20 + s))[:, 0] for s in range(S)])) * mask   # (S, n, H, W)
    ys, As = pkg.uf.SENSE.compress_measurement(y, mask, nv, geometric=True)
    assert tuple(ys.shape) == (S, nv, H, W) and tuple(As.shape) == (S, H, nv, n) and not As.is_cuda and ys.is_cuda
    for s in range(S):                                                       # the stack is the single-slice calls, bit for bit
        y1, A1 = pkg.uf.SENSE.compress_measurement(y[s], mask, nv, geometric=True)
        assert tuple(y1.shape) == (nv, H, W) and tuple(A1.shape) == (H, nv, n)
        assert torch.equal(bits(y1), bits(ys[s])) and torch.equal(bits(A1), bits(As[s]))
    assert not bits(ys[..., torch.from_numpy(~mask.numpy()).cuda()]).any()
    y0, A0 = pkg.uf.SENSE.compress_measurement(y[0], mask, nv, geometric=True, window=0)
    assert not torch.equal(bits(A0), bits(As[0]))
    yp, Ap = pkg.uf.SENSE.compress_measurement(y[0], mask, nv)               # without the switch: one matrix, as before
    assert tuple(Ap.shape) == (nv, n)
    op = pkg.uf.SENSE.from_measurement(y[0], mask, n_virtual=nv, geometric=True)
    assert tuple(op.sens_maps.shape) == (nv, H, W)
    prox = pkg.prox.get_proximal("L2PenaltyCG")(op, max_iter=5, tol=1e-6)
    meas = ys[0].reshape(nv, 1, 1, H, W).contiguous()
    z = torch.zeros(1, 1, H, W, dtype=torch.complex64, device="cuda")
    x = prox(z, meas, 1.0, 1.0)
    torch.cuda.synchronize()
    assert tuple(x.shape[-2:]) == (H, W) and torch.isfinite(bits(x)).all() and x.abs().sum() > 0
    # rows below 10 seen by coil 0 alone, the others by coil 1 alone: one virtual coil cannot be carried across the seam,
    # and the ten rows beyond it find no neighbour to align with
    rng = np.random.default_rng(5)
    h = np.zeros((4, H, W), dtype=np.complex128)
    h[0, :10] = rng.standard_normal((10, W)) + 1j * rng.standard_normal((10, W))
    h[1, 10:] = rng.standard_normal((H - 10, W)) + 1j * rng.standard_normal((H - 10, W))
    seam = torch.from_numpy(rounded(gh.readout(h))) * mask
    with pytest.raises(RuntimeError, match=r"image 0: 10 readout position"):
        pkg.uf.SENSE.compress_measurement(seam, mask, 1, geometric=True, window=0)


def test_build_problem_compresses_geometrically(ops, pkg):
    H = W = 32
    n, nv = 12, 4
    mask = _line_mask(W)
    y = torch.from_numpy(rounded(cch.coil_data(H, W, n, B=1, seed=6))[:, 0]) * mask[None, None, :]
    torch.manual_seed(0)
    cfg = tiny_config()
    net = pkg.ncsnv2.NCSNv2Deepest(cfg).cuda().eval()
    kw = dict(H=H, W=W, scorenet=net, cfg=cfg, mask=mask, coil_compress=nv, coil_compress_mode="geometric")
    prob = pkg.engine.build_problem(torch.device("cuda"), 2, measurement=y, estimate_maps=True, **kw)
    A = prob.coil_matrix
    assert tuple(A.shape) == (H, nv, n) and A.dtype == torch.complex64 and not A.is_cuda
    assert tuple(prob.op.sens_maps.shape) == (nv, H, W) and tuple(prob.measurement.shape) == (nv, 2, 1, H, W)
    assert prob.estimated_maps and prob.kspace_scale > 0
    y1, A1 = pkg.uf.SENSE.compress_measurement(y, mask, nv, geometric=True)
    assert torch.equal(bits(A1), bits(A))
    want = host(y1) * prob.kspace_scale                                      # the sampler sees the compressed data, scaled
    assert np.abs(host(prob.measurement[:, 0, 0]) - want).max() <= 1e-6 * np.abs(want).max()
    runner = pkg.engine.IterationRunner(prob, use_graph=False)
    runner.run(0)
    runner.run(1)
    x = runner.current()
    torch.cuda.synchronize()
    assert tuple(x.shape) == (2, 1, H, W) and torch.isfinite(bits(x)).all() and x.abs().sum() > 0
    # given maps are compressed row by row with the same matrices
    maps = pkg.syn.complex_coil_maps(n, H, W, 0)
    given = pkg.engine.build_problem(torch.device("cuda"), 1, measurement=y, sens_maps=maps, **kw)
    norm = pkg.uf.SENSE.rss_normalize(maps).to(torch.complex128).numpy()
    want = gh.apply_rows(norm[:, None], given.coil_matrix.numpy().astype(np.complex128))[:, 0]
    assert np.abs(given.op.sens_maps.numpy() - want).max() <= 1e-5 * np.abs(want).max()
    sim = pkg.engine.build_problem(torch.device("cuda"), 1, num_sens=n, **kw)            # simulated, synthetic maps
    assert tuple(sim.coil_matrix.shape) == (H, nv, n) and tuple(sim.op.sens_maps.shape) == (nv, H, W)
    stack = pkg.engine.build_problem(torch.device("cuda"), 1, num_sens=n, n_slices=2, sens_maps=maps, **kw)
    assert tuple(stack.coil_matrix.shape) == (2, H, nv, n) and stack.op.n_map_sets == 2
    assert tuple(stack.op.sens_maps.shape) == (2, nv, H, W)
    pca = pkg.engine.build_problem(torch.device("cuda"), 1, measurement=y, estimate_maps=True, **dict(kw, coil_compress_mode="pca"))
    assert tuple(pca.coil_matrix.shape) == (nv, n)                           # the default is unchanged


def test_driver_compresses_geometrically(tmp_path):
    torch.save(_line_mask(32), tmp_path / "mask.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--image_size", "32", "--n_levels", "2",
                        "--num_samples", "1", "--seed", "0", "--seg_start_time", "1.0", "--num_sens", "12", "--coil_compress", "4",
                        "--coil_compress_mode", "geometric", "--coil_compress_window", "1", "--mask", str(tmp_path / "mask.pt"),
                        "--save_dir", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    A = torch.load(out / "coil_matrix.pt", weights_only=False)
    maps = torch.load(out / "sens_maps.pt", weights_only=False)
    rec = torch.load(out / "reconstructions.pt", weights_only=False)
    assert tuple(A.shape) == (32, 4, 12) and A.is_complex()
    assert tuple(maps.shape) == (4, 32, 32)
    assert torch.isfinite(torch.view_as_real(rec) if rec.is_complex() else rec).all()
