"""Coil compression and noise prewhitening on the GPU (csrc/coilcomp.hip) against tests/coilcomp_helpers.py.

Individual eigenvectors of a calibration Gram matrix are ill-conditioned in single precision (spectra decay by orders of
magnitude, neighbouring gaps of 1e-9 relative at 64 coils), so the matrix is held to the properties that define it, which
are well-conditioned and gauge-free, and to eigenvectors only where the gaps are designed.

Bounds.  Unless stated otherwise the bound of a quantity is 4 err_cpu, err_cpu being the same quantity from the helper's
single-precision run on the same input (the same algorithm in fp32 elsewhere: 4x for another summation and rotation
order); err_cpu <= 1e-3 is asserted, so a broken helper cannot loosen a bound.  err_gpu and err_cpu are printed per case
(DESIGN.md 4.4f tables them)."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import coilcomp_helpers as cch
import csm_helpers as csmh

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
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2
    return Namespace(lib=_lib, syn=synthetic, uf=undersampling_fourier, engine=engine, ncsnv2=ncsnv2)


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


def _misaligned_c64(shape):
    """complex64 tensor 8 bytes past a 16-byte boundary"""
    n = int(np.prod(shape)) * 2
    base = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    off = ((16 - base.data_ptr() % 16) % 16) // 4 + 2
    t = torch.view_as_complex(base[off:off + n].reshape(*shape, 2))
    assert t.data_ptr() % 16 == 8
    return t


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rounded(a):
    """complex128 values that complex64 holds exactly"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


# ---- 1. Gram matrix -------------------------------------------------------------------------------------------------------------
GRAM_CASES = [(1, 8, 8, 2, 2), (2, 16, 16, 2, 2), (3, 16, 16, 2, 2), (9, 32, 32, 4, 4), (33, 16, 64, 5, 12), (64, 32, 32, 12, 12)]
SCALES = (1.0, 1e-3, 1e3)


def gram_data(n, H, W):
    return cached(("y", n, H, W), lambda: rounded(cch.coil_data(H, W, n, B=3, seed=n, scales=SCALES)))


@pytest.mark.parametrize("n,H,W,ah,aw", GRAM_CASES)
def test_gram_vs_float64(ops, n, H, W, ah, aw):
    y = gram_data(n, H, W)
    want = cch.gram(y, ah, aw)
    cpu = cch.gram(y.astype(np.complex64), ah, aw, np.float32)
    G = ops.coil_gram(dev(y), ah, aw)
    assert G.dtype == torch.complex64 and tuple(G.shape) == (3, n, n)
    got = host(G)
    for b in range(3):                                                       # each image against its own scale
        top = np.abs(want[b]).max()
        check(f"gram {n} coils {H}x{W} box {2 * ah + 1}x{2 * aw + 1} scale {SCALES[b]:g}",
              np.abs(got[b] - want[b]).max() / top, np.abs(cpu[b].astype(np.complex128) - want[b]).max() / top)
    assert np.array_equal(got, got.conj().transpose(0, 2, 1))                # exactly Hermitian
    assert not np.diagonal(got, axis1=1, axis2=2).imag.any()
    assert torch.equal(bits(ops.coil_gram(dev(y[:, 1]), ah, aw)), bits(G[1:2]))          # (n, H, W) is the same call


def test_gram_box_at_the_image_edge(ops, pkg):
    y = rounded(cch.coil_data(8, 8, 2, B=1, seed=3))
    with pytest.raises(pkg.lib.IpdmError) as e:
        ops.coil_gram(dev(y), 3, 4)                                          # 8 // 2 + 4 = 8: outside
    assert not isinstance(e.value, pkg.lib.IpdmUnsupported)
    got = host(ops.coil_gram(dev(y), 3, 3))                                  # columns 1..7: touches the last one
    want = cch.gram(y, 3, 3)
    cpu = cch.gram(y.astype(np.complex64), 3, 3, np.float32)
    top = np.abs(want).max()
    check("gram 8x8 box 7x7", np.abs(got - want).max() / top, np.abs(cpu.astype(np.complex128) - want).max() / top)


# ---- 2. matrix properties -------------------------------------------------------------------------------------------------------
MATRIX_CASES = [(1, 1), (2, 1), (3, 3), (8, 4), (9, 4), (33, 12), (64, 16), (64, 32), (64, 8)]


def designed_gram(n, kind):
    """Gram matrix of Q diag(s) Z, rounded to complex64 and exactly Hermitian; 33 coils: 25 samples (a 5 x 5 box), rank 25"""
    def make():
        Y = cch.lowrank_samples(n, 25 if n == 33 else max(4 * n, 25), kind, n)
        return cch.hermitian(rounded(cch.hermitian(Y @ Y.conj().T)))
    return cached(("G", n, kind), make)


def helper_matrix(n, kind, nv, dtype, psi_cond=None):
    def make():
        G = designed_gram(n, kind)
        psi = None if psi_cond is None else designed_psi(n, psi_cond)
        return cch.matrix(G if dtype == np.float64 else G.astype(np.complex64), nv, noise_cov=psi, dtype=dtype)
    return cached(("M", n, kind, nv, dtype, psi_cond), make)


def designed_psi(n, cond):
    return cached(("psi", n, cond), lambda: cch.hermitian(rounded(cch.noise_cov(n, cond, n))))


def matrix_errors(A, eig, G, lam, psi=None):
    """in float64: (max |eig - lam| / lam_0, max |A G A^H - diag(lam[:nv])| / lam_0, max |A M A^H - I|), M = I or psi"""
    A = np.asarray(A).astype(np.complex128)
    nv = A.shape[0]
    M = np.eye(G.shape[0]) if psi is None else psi
    return (float(np.abs(np.asarray(eig).astype(np.float64) - lam).max() / lam[0]),
            float(np.abs(A @ G @ A.conj().T - np.diag(lam[:nv])).max() / lam[0]),
            float(np.abs(A @ M @ A.conj().T - np.eye(nv)).max()))


def _matrix_case(ops, n, nv, kind, psi_cond=None):
    G = designed_gram(n, kind)
    psi = None if psi_cond is None else designed_psi(n, psi_cond)
    ref, cpu = helper_matrix(n, kind, nv, np.float64, psi_cond), helper_matrix(n, kind, nv, np.float32, psi_cond)
    lam = ref["eig"][0]
    A, eig, status = ops.coilcomp_matrix(dev(G), nv, noise_cov=psi, return_eig=True)
    assert tuple(A.shape) == (1, nv, n) and tuple(eig.shape) == (1, n) and eig.dtype == torch.float32
    assert int(status[0]) == 0 and int(cpu["status"][0]) == 0
    A, eig = host(A)[0], host(eig)[0]
    e_gpu, e_cpu = matrix_errors(A, eig, G, lam, psi), matrix_errors(cpu["A"][0], cpu["eig"][0], G, lam, psi)
    tag = f"matrix {n}->{nv} {kind}" + ("" if psi is None else f" psi cond {psi_cond}")
    for name, g, c in zip(("eigenvalues", "A G A^H - diag", "A psi A^H - I" if psi is not None else "A A^H - I"), e_gpu, e_cpu):
        check(f"{tag} {name}", g, c)
    assert (np.diff(eig) <= 0).all()                                         # descending
    rows = np.linalg.norm(A, axis=1)
    assert (np.abs(A[:, 0].imag) <= 1e-6 * rows).all() and (A[:, 0].real >= 0).all()
    return A, eig


@pytest.mark.parametrize("kind", ["flat", "decay"])
@pytest.mark.parametrize("n,nv", MATRIX_CASES)
def test_matrix_properties(ops, n, nv, kind):
    A, eig = _matrix_case(ops, n, nv, kind)
    if n == 33:                                                              # rank 25: the tail is noise around zero
        assert np.abs(eig[25:]).max() <= 1e-5 * eig[0]


@pytest.mark.parametrize("n,nv", [(8, 4), (16, 6)])
def test_matrix_properties_with_noise_covariance(ops, n, nv):
    assert 250 < np.linalg.cond(designed_psi(n, 300.0)) < 350
    A, _ = _matrix_case(ops, n, nv, "decay", 300.0)
    plain, _ = _matrix_case(ops, n, nv, "decay")
    assert np.abs(A - plain).max() > 1e-2                                    # whitening changed the matrix


def test_matrix_of_a_batch(ops):
    Gs = np.stack([designed_gram(9, "flat"), designed_gram(9, "decay")])
    A, eig, status = ops.coilcomp_matrix(dev(Gs), 4, return_eig=True)
    for b, kind in enumerate(("flat", "decay")):
        one, e1, _ = ops.coilcomp_matrix(dev(Gs[b]), 4, return_eig=True)      # (n, n) is a batch of one
        assert torch.equal(bits(A[b:b + 1]), bits(one)) and torch.equal(eig[b:b + 1], e1)
    assert torch.equal(bits(ops.coilcomp_matrix(dev(Gs), 4)), bits(A)) and status.tolist() == [0, 0]


def test_indefinite_noise_covariance_sets_the_status(ops, pkg):
    n, nv = 8, 4
    G = dev(np.stack([designed_gram(n, "decay")] * 2))
    bad = designed_psi(n, 300.0).copy()
    bad[5, 5] = -bad[5, 5]                                                   # the sixth pivot is negative
    with pytest.raises(ValueError, match="positive definite"):
        ops.coilcomp_matrix(G, nv, noise_cov=bad)                            # the front end refuses it on the host
    A = torch.full((2, nv, n), float("nan"), dtype=torch.complex64, device="cuda")
    eig = torch.full((2, n), float("nan"), device="cuda")
    status = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    P = pkg.lib.P
    pkg.lib.call("ipdm_coilcomp_matrix_c64", P(G.data_ptr()), P(dev(bad).data_ptr()), nv, P(A.data_ptr()), P(eig.data_ptr()),
                 P(status.data_ptr()), 2, n, P(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status.tolist() == [1, 1] and not bits(A).any() and not eig.any()
    good = dev(designed_psi(n, 300.0))
    pkg.lib.call("ipdm_coilcomp_matrix_c64", P(G.data_ptr()), P(good.data_ptr()), nv, P(A.data_ptr()), P(eig.data_ptr()),
                 P(status.data_ptr()), 2, n, P(torch.cuda.current_stream().cuda_stream))
    assert status.tolist() == [0, 0] and torch.isfinite(bits(A)).all() and bits(A).any()


# ---- 3. eigenvectors where they are determined ----------------------------------------------------------------------------------
def test_eigenvectors_with_designed_gaps(ops):
    n = 8
    Q = cch.random_unitary(n, 5)
    G = cch.hermitian(rounded(cch.hermitian((Q * 0.49 ** np.arange(n)[None]) @ Q.conj().T)))
    A = host(ops.coilcomp_matrix(dev(G), 4))[0].astype(np.complex128)
    cpu = cch.matrix(G.astype(np.complex64), 4, dtype=np.float32)["A"][0].astype(np.complex128)

    def deficit(row, q):
        """1 - |<u, q>| / |u| for u = conj(row), from the residual of the projection (never negative)"""
        u = row.conj()
        d = np.linalg.norm(u - q * (q.conj() @ u)) ** 2 / np.linalg.norm(u) ** 2
        return d / (1 + np.sqrt(1 - d))

    for v in range(4):
        d_gpu, d_cpu = deficit(A[v], Q[:, v]), deficit(cpu[v], Q[:, v])
        print(f"eigenvector {v}: 1 - |<u_gpu, q>| = {d_gpu:.3e}, complex64 helper {d_cpu:.3e}")
        assert d_cpu <= 1e-3
        assert 1 - d_gpu >= 1 - 4 * d_cpu


# ---- 4. the streaming kernel ----------------------------------------------------------------------------------------------------
APPLY_CASES = [(2, 1, 1, 1), (3, 3, 2, 7), (9, 4, 3, 130), (33, 12, 2, 16 * 64), (64, 32, 1, 1024), (64, 8, 2, 1024), (4, 2, 1, 65537)]


def apply_inputs(ops, n, nv, B, P):
    def make():
        rng = np.random.default_rng(1000 * n + P)
        y = rounded(rng.standard_normal((n, B, P)) + 1j * rng.standard_normal((n, B, P)))
        Gs = np.stack([cch.hermitian(rounded(cch.hermitian(S @ S.conj().T)))
                       for S in (cch.lowrank_samples(n, max(4 * n, 25), "decay", 50 * n + b) for b in range(B))])
        A = host(ops.coilcomp_matrix(dev(Gs), nv))                           # the GPU's own matrix
        return y, A
    return cached(("apply", n, nv, B, P), make)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n,nv,B,P", APPLY_CASES)
def test_apply_vs_float64(ops, n, nv, B, P, shared):
    y, A = apply_inputs(ops, n, nv, B, P)
    A = A[0] if shared else A
    want = cch.apply(y, A.astype(np.complex128))
    cpu = cch.apply(y.astype(np.complex64), A, np.float32)
    yd, out = _misaligned_c64((n, B, P)), _misaligned_c64((nv, B, P))
    yd.copy_(dev(y))
    got = ops.coil_apply(yd, dev(A), out=out)
    assert got.data_ptr() == out.data_ptr() and yd.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
    top = np.abs(want).max()
    check(f"apply {n}->{nv} B={B} P={P} {'shared' if shared else 'per image'}", np.abs(host(got) - want).max() / top,
          np.abs(cpu.astype(np.complex128) - want).max() / top)
    aligned = ops.coil_apply(dev(y), dev(A))                                 # alignment never changes a bit
    assert aligned.data_ptr() % 16 == 0 and torch.equal(bits(aligned), bits(got))


def test_apply_compresses_maps_and_refuses_aliases(ops, pkg):
    n, nv, H, W = 9, 4, 16, 32
    y, A = apply_inputs(ops, n, nv, 3, 130)
    maps = dev(rounded(cch.coil_data(H, W, n, B=1, seed=4)))                 # (n, 1, H, W): an image as P = H W pixels
    got = ops.coil_apply(maps, dev(A[0]))
    assert tuple(got.shape) == (nv, 1, H, W)
    flat = ops.coil_apply(maps.reshape(n, 1, H * W), dev(A[0]))
    assert torch.equal(bits(got.reshape(nv, 1, H * W)), bits(flat))
    buf = torch.zeros(n * 3 * 130, dtype=torch.complex64, device="cuda")
    yd = buf.reshape(n, 3, 130)
    for out in (buf[:nv * 3 * 130].reshape(nv, 3, 130), buf[3 * 130:(nv + 1) * 3 * 130].reshape(nv, 3, 130)):
        with pytest.raises(pkg.lib.IpdmError) as e:
            ops.coil_apply(yd, dev(A), out=out)
        assert not isinstance(e.value, pkg.lib.IpdmUnsupported)
    for bad in (yd.to(torch.complex128), torch.zeros(n, 3, 130, device="cuda"), torch.zeros(n, 3, 130, dtype=torch.float64, device="cuda"),
                torch.zeros(n, 3, 260, dtype=torch.complex64, device="cuda")[..., ::2]):
        with pytest.raises(TypeError):
            ops.coil_apply(bad, dev(A))
    with pytest.raises(TypeError):
        ops.coil_apply(yd, dev(A).to(torch.complex128))
    with pytest.raises(ValueError):
        ops.coil_apply(yd, dev(A)[:2])                                       # two matrices for three images
    with pytest.raises(ValueError):
        ops.coil_apply(yd, dev(A)[..., :8].contiguous())                     # eight columns for nine coils
    with pytest.raises(pkg.lib.IpdmUnsupported):
        ops.coil_apply(torch.zeros(65, 1, 4, dtype=torch.complex64, device="cuda"), torch.zeros(8, 65, dtype=torch.complex64, device="cuda"))
    with pytest.raises(pkg.lib.IpdmUnsupported):
        ops.coil_apply(torch.zeros(64, 1, 4, dtype=torch.complex64, device="cuda"), torch.zeros(33, 64, dtype=torch.complex64, device="cuda"))
    for bad in (torch.zeros(4, 2, 16, 16, dtype=torch.complex128, device="cuda"), torch.zeros(4, 2, 16, 16, device="cuda"),
                torch.zeros(4, 2, 16, 32, dtype=torch.complex64, device="cuda")[..., ::2]):
        with pytest.raises(TypeError):
            ops.coil_gram(bad, 2, 2)
        with pytest.raises(TypeError):
            ops.coil_compress(bad, 2, 2, 2)
    with pytest.raises(TypeError):
        ops.coilcomp_matrix(torch.zeros(1, 4, 4, dtype=torch.complex128, device="cuda"), 2)
    y4 = torch.zeros(4, 2, 16, 16, dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):
        ops.coil_compress(y4, 2, 2, 5)
    with pytest.raises(ValueError, match="positive definite"):
        ops.coil_compress(y4, 2, 2, 2, noise_cov=-np.eye(4))
    with pytest.raises(ValueError, match="shape"):
        ops.coil_compress(y4, 2, 2, 2, noise_cov=np.eye(3))
    torch.cuda.synchronize()


# ---- 5. batch invariance and determinism ------------------------------------------------------------------------------------------
def _three_calls(ops, yd, ah, aw, nv, psi=None):
    G = ops.coil_gram(yd, ah, aw)
    A, eig, status = ops.coilcomp_matrix(G, nv, noise_cov=psi, return_eig=True)
    return G, A, eig, ops.coil_apply(yd, A)


@pytest.mark.parametrize("psi_cond", [None, 300.0])
def test_batch_invariance_determinism_and_the_one_call_entry(ops, psi_cond):
    n, nv, H, W, ah, aw = 9, 4, 32, 32, 4, 4
    psi = None if psi_cond is None else designed_psi(n, psi_cond)
    yd = dev(gram_data(n, H, W))
    alone = [_three_calls(ops, yd[:, b:b + 1].contiguous(), ah, aw, nv, psi) for b in range(3)]
    for shift in range(3):                                                   # image b at position (b + shift) % 3
        order = [(p - shift) % 3 for p in range(3)]
        G, A, eig, out = _three_calls(ops, yd[:, order].contiguous(), ah, aw, nv, psi)
        for p, b in enumerate(order):
            assert torch.equal(bits(G[p]), bits(alone[b][0][0])) and torch.equal(bits(A[p]), bits(alone[b][1][0]))
            assert torch.equal(eig[p], alone[b][2][0]) and torch.equal(bits(out[:, p]), bits(alone[b][3][:, 0]))
    G, A, eig, out = _three_calls(ops, yd, ah, aw, nv, psi)
    again = _three_calls(ops, yd, ah, aw, nv, psi)                           # a second call: the same bits
    for a, b in zip((G, A, eig, out), again):
        assert torch.equal(bits(a), bits(b))
    o1, A1, e1, s1 = ops.coil_compress(yd, ah, aw, nv, noise_cov=psi, return_matrix=True)          # one call = three calls
    assert torch.equal(bits(o1), bits(out)) and torch.equal(bits(A1), bits(A)) and torch.equal(e1, eig) and s1.tolist() == [0, 0, 0]
    assert torch.equal(bits(ops.coil_compress(yd, ah, aw, nv, noise_cov=psi)), bits(out))
    work = torch.zeros(ops.coilcomp_workspace(3, n, "cuda").numel(), device="cuda")
    assert work.numel() * 4 == 3 * n * n * 8
    assert torch.equal(bits(ops.coil_compress(yd, ah, aw, nv, noise_cov=psi, work=work)), bits(out))
    assert torch.equal(bits(torch.view_as_complex(work.reshape(3, n, n, 2))), bits(G))              # the workspace holds the Gram matrices
    with pytest.raises(ValueError):
        ops.coil_compress(yd, ah, aw, nv, work=work[:-2])


def test_graph_capture_and_replay(ops):
    n, nv, H, W, ah, aw = 9, 4, 32, 32, 4, 4
    y = gram_data(n, H, W)
    y1, y2 = dev(y), dev(y[:, [2, 0, 1]] * 0.5)
    static = y1.clone()
    ops.coil_compress(static, ah, aw, nv)                                    # warm-up: allocator
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, A, eig, status = ops.coil_compress(static, ah, aw, nv, return_matrix=True)
    for src in (y2, y1):
        static.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        e_out, e_A, e_eig, e_status = ops.coil_compress(src, ah, aw, nv, return_matrix=True)
        assert torch.equal(bits(out), bits(e_out)) and torch.equal(bits(A), bits(e_A)) and torch.equal(eig, e_eig)
        assert torch.equal(status, e_status) and out.abs().sum() > 0


# ---- 6. in use ------------------------------------------------------------------------------------------------------------------
def _line_mask(W):
    m = torch.zeros(W, dtype=torch.bool)
    m[::3] = True
    m[W // 2 - 8:W // 2 + 9] = True
    return m


def test_compressed_measurement_serves_the_cg_proximal(ops, pkg):
    """16 physical coils -> 6 virtual, maps estimated on the virtual coils, exact proximal by conjugate gradients.
    Measured (MI355X): NRMSE of |x| inside the support 0.0185 with the GPU's compression, 0.0185 with the float64
    helper's, 0.0182 with the 16 coils uncompressed; the six virtual coils retain 0.9951 of the calibration energy."""
    H = W = 64
    n, nv = 16, 6
    mask = _line_mask(W)
    img = pkg.syn.phantom_image(H, W, seed=0)
    op = pkg.uf.SENSE("custom", n, 3, 0.04, (1, H, W), seed=0, sens_maps=pkg.syn.complex_coil_maps(n, H, W, 0), mask_mode="custom",
                      mask=mask)
    y = op(img.cuda())                                                       # (n, 1, 1, H, W)
    ah, aw = pkg.uf.calibration_region(mask, H, W)
    assert (ah, aw) == (12, 8)
    mask_u8 = op.mask_u8("cuda")
    z = torch.zeros(1, 1, H, W, device="cuda")
    mag = img[0, 0].abs().double()
    sup = csmh.estimate(y[:, :, 0].cpu(), ah, aw)["support"][0]

    def nrmse(meas):
        maps = ops.estimate_sens_maps(meas, ah, aw)[:, 0, 0].contiguous()
        re, im, _ = ops.sense_cgprox(z, z.clone(), meas, maps, mask_u8, 1e3, max_iter=300, tol=1e-6)
        x = torch.complex(re, im)[0, 0].cpu().abs().double()
        return float(torch.sqrt(((x - mag)[sup] ** 2).sum() / (mag[sup] ** 2).sum()))

    y_gpu, A, eig, status = ops.coil_compress(y, ah, aw, nv, return_matrix=True)
    assert tuple(y_gpu.shape) == (nv, 1, 1, H, W) and int(status[0]) == 0
    ref = cch.compress(host(y)[:, :, 0], ah, aw, nv)                         # float64
    y_ref = dev(ref["y"])[:, :, None].contiguous()
    e_gpu, e_ref, e_full = nrmse(y_gpu), nrmse(y_ref), nrmse(y)
    lam = host(eig)[0].astype(np.float64)
    print(f"NRMSE inside the support: GPU compression {e_gpu:.4f}, float64 helper's compression {e_ref:.4f}, "
          f"uncompressed {n} coils {e_full:.4f}; retained calibration energy {lam[:nv].sum() / lam.sum():.6f}")
    assert abs(e_gpu - e_ref) <= 0.05 * e_ref
    y2, A2 = pkg.uf.SENSE.compress_measurement(y, mask, nv)                  # the operator's front end: the same bits
    assert tuple(y2.shape) == (nv, H, W) and tuple(A2.shape) == (nv, n) and not A2.is_cuda
    assert torch.equal(bits(y2), bits(y_gpu[:, 0, 0])) and torch.equal(bits(A2), bits(A[0].cpu()))
    op2 = pkg.uf.SENSE.from_measurement(y, mask, n_virtual=nv)
    assert tuple(op2.sens_maps.shape) == (nv, H, W)


# ---- 7. front end -----------------------------------------------------------------------------------------------------------------
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


def test_build_problem_compresses_33_coils(ops, pkg):
    H = W = 32
    mask = _line_mask(W)
    y = torch.from_numpy(rounded(cch.coil_data(H, W, 33, B=1, seed=6))[:, 0]) * mask[None, None, :]
    torch.manual_seed(0)
    cfg = tiny_config()
    net = pkg.ncsnv2.NCSNv2Deepest(cfg).cuda().eval()
    kw = dict(H=H, W=W, scorenet=net, cfg=cfg, mask=mask, measurement=y, estimate_maps=True)
    with pytest.raises(pkg.lib.IpdmUnsupported):                             # the estimator's 32-coil limit
        pkg.engine.build_problem(torch.device("cuda"), 2, **kw)
    prob = pkg.engine.build_problem(torch.device("cuda"), 2, coil_compress=8, **kw)
    assert tuple(prob.coil_matrix.shape) == (8, 33) and prob.coil_matrix.dtype == torch.complex64 and not prob.coil_matrix.is_cuda
    assert tuple(prob.op.sens_maps.shape) == (8, H, W) and tuple(prob.measurement.shape) == (8, 2, 1, H, W)
    assert prob.estimated_maps and prob.kspace_scale > 0
    A = prob.coil_matrix.numpy().astype(np.complex128)
    assert np.abs(A @ A.conj().T - np.eye(8)).max() <= 1e-4
    # the measurement the sampler sees is the compressed one, scaled
    want = cch.apply(y.numpy()[:, None], A)[:, 0] * prob.kspace_scale
    assert np.abs(host(prob.measurement[:, 0, 0]) - want).max() <= 1e-5 * np.abs(want).max()
    runner = pkg.engine.IterationRunner(prob, use_graph=False)
    runner.run(0)
    runner.run(1)
    x = runner.current()
    torch.cuda.synchronize()
    assert tuple(x.shape) == (2, 1, H, W) and torch.isfinite(bits(x)).all() and x.abs().sum() > 0
    base = pkg.engine.build_problem(torch.device("cuda"), 1, H=H, W=W, scorenet=net, cfg=cfg, mask=mask, num_sens=4)
    assert base.coil_matrix is None                                          # nothing new runs without the argument


def test_driver_compresses_a_simulated_problem(tmp_path):
    torch.save(_line_mask(64), tmp_path / "mask.pt")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--image_size", "64", "--n_levels", "2",
                        "--num_samples", "1", "--seed", "0", "--seg_start_time", "1.0", "--num_sens", "8", "--coil_compress", "4",
                        "--mask", str(tmp_path / "mask.pt"), "--save_dir", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    A = torch.load(out / "coil_matrix.pt", weights_only=False)
    maps = torch.load(out / "sens_maps.pt", weights_only=False)
    meas = torch.load(out / "measurement.pt", weights_only=False)
    rec = torch.load(out / "reconstructions.pt", weights_only=False)
    assert tuple(A.shape) in ((1, 4, 8), (4, 8)) and A.is_complex()
    assert tuple(maps.shape) == (4, 64, 64) and tuple(meas.shape) == (4, 1, 1, 64, 64)
    assert torch.isfinite(torch.view_as_real(rec)).all()
