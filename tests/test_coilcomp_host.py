"""Coil compression and noise prewhitening, host side: the float64 helper (tests/coilcomp_helpers.py) against
numpy.linalg.eigh on the properties that define the result, its single-precision run, the argument checks that need no
GPU (C entries and Python front ends), load_noise_cov, and that build_problem and the driver refuse bad arguments before
anything is built."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import coilcomp_helpers as cch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    from argparse import Namespace
    from inverseproblemwithdiffusionmodel_amd import _lib, engine, ops
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
    return Namespace(lib=_lib, ops=ops, load=load_data, uf=uf, engine=engine)


def line_mask(W):
    m = torch.zeros(W, dtype=torch.bool)
    m[::3] = True
    m[W // 2 - 8:W // 2 + 9] = True
    return m


def gram_of(n, kind, seed, K=None):
    Y = cch.lowrank_samples(n, K or max(4 * n, 25), kind, seed)
    return cch.hermitian(Y @ Y.conj().T)


def properties(A, eig, G, lam, psi=None):
    """(eigenvalue error, |A G A^H - diag(lam)|, |A M A^H - I|) in float64, the first two relative to lam[0]"""
    A = np.asarray(A).astype(np.complex128)
    nv = A.shape[0]
    M = np.eye(G.shape[0]) if psi is None else psi
    return (float(np.abs(np.asarray(eig, dtype=np.float64) - lam).max() / lam[0]),
            float(np.abs(A @ G @ A.conj().T - np.diag(lam[:nv])).max() / lam[0]),
            float(np.abs(A @ M @ A.conj().T - np.eye(nv)).max()))


# ---- the helper ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "decay"])
@pytest.mark.parametrize("n,nv,K", [(1, 1, None), (2, 1, None), (3, 3, None), (8, 4, None), (9, 4, None), (33, 12, 25), (64, 16, None)])
def test_helper_matrix_against_eigh(n, nv, K, kind):
    G = gram_of(n, kind, n, K)
    lam = np.linalg.eigvalsh(G)[::-1]
    r = cch.matrix(G, nv)
    A, eig = r["A"][0], r["eig"][0]
    assert A.shape == (nv, n) and A.dtype == np.complex128 and r["status"][0] == 0
    e = properties(A, eig, G, lam)
    print(f"{n}->{nv} {kind}: eig {e[0]:.1e}, AGA^H {e[1]:.1e}, AA^H {e[2]:.1e}; off-diagonal per sweep "
          + " ".join(f"{o:.0e}" for o in r["off"][0]))
    assert max(e) <= 1e-12
    assert (np.diff(eig) <= 0).all()
    assert np.abs(A[:, 0].imag).max() <= 1e-14 and A[:, 0].real.min() >= 0
    if K == 25:                                                             # rank 25 of 33: the tail is zero
        assert np.abs(eig[25:]).max() <= 1e-12 * eig[0]
    # the single-precision run of the same steps: what the GPU bounds come from
    G32 = cch.hermitian(G.astype(np.complex64))
    r32 = cch.matrix(G32, nv, dtype=np.float32)
    assert r32["A"].dtype == np.complex64 and r32["eig"].dtype == np.float32
    e32 = properties(r32["A"][0], r32["eig"][0], cch.hermitian(G32.astype(np.complex128)),
                     np.linalg.eigvalsh(G32.astype(np.complex128))[::-1])
    print(f"    float32: eig {e32[0]:.1e}, AGA^H {e32[1]:.1e}, AA^H {e32[2]:.1e}; converged to 6e-8 after sweep "
          f"{1 + next((i for i, o in enumerate(r32['off'][0]) if o <= 6e-8), -1)}")
    assert max(e32) <= 1e-3
    if n > 1:                                                               # two sweeps to spare
        assert r32["off"][0][cch.SWEEPS - 3] <= 6e-8


def test_helper_equal_eigenvalues_keep_their_order():
    G = np.diag([2.0, 5.0, 2.0, 5.0]).astype(np.complex128)
    r = cch.matrix(G, 4)
    assert np.array_equal(r["eig"][0], [5.0, 5.0, 2.0, 2.0])
    want = np.zeros((4, 4))
    want[[0, 1, 2, 3], [1, 3, 0, 2]] = 1                                     # the lower original index first
    assert np.array_equal(r["A"][0].real, want) and not r["A"][0].imag.any()
    z = cch.matrix(np.zeros((3, 3), dtype=np.complex128), 2)                 # a zero Gram matrix: identity rows, no NaN
    assert np.array_equal(z["A"][0], np.eye(3)[:2]) and not z["eig"].any()


@pytest.mark.parametrize("n,nv", [(8, 4), (16, 6)])
def test_helper_whitening_against_numpy(n, nv):
    psi = cch.noise_cov(n, 300.0, n)
    assert 250 < np.linalg.cond(psi) < 350
    G = gram_of(n, "decay", n)
    Li = np.linalg.inv(np.linalg.cholesky(psi))
    lam = np.linalg.eigvalsh(Li @ G @ Li.conj().T)[::-1]
    r = cch.matrix(G, nv, noise_cov=psi)
    e = properties(r["A"][0], r["eig"][0], G, lam, psi)
    print(f"{n}->{nv} with psi: {e}")
    assert max(e) <= 1e-11
    e32 = properties(cch.matrix(G.astype(np.complex64), nv, noise_cov=psi, dtype=np.float32)["A"][0], lam, G, lam, psi)
    assert e32[1] <= 1e-3 and e32[2] <= 1e-3
    bad = cch.matrix(G, nv, noise_cov=-psi)
    assert bad["status"][0] == 1 and not bad["A"].any() and not bad["eig"].any()


def test_helper_gram_and_apply():
    y = cch.coil_data(16, 16, 3, B=2, seed=2, scales=(1.0, 1e3))
    G = cch.gram(y, 2, 3)
    box = y[:, :, 6:11, 5:12].reshape(3, 2, -1)
    want = np.einsum("ibk,jbk->bij", box, box.conj())
    assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(G, G.conj().transpose(0, 2, 1)) and not np.diagonal(G, axis1=1, axis2=2).imag.any()
    with pytest.raises(ValueError):
        cch.gram(y, 8, 2)                                                    # 16 // 2 + 8 = 16 leaves the image
    rng = np.random.default_rng(0)
    A = rng.standard_normal((2, 2, 3)) + 1j * rng.standard_normal((2, 2, 3))
    want = np.einsum("bvc,cbhw->vbhw", A, y)
    got = cch.apply(y, A)
    assert got.shape == (2, 2, 16, 16) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    shared = cch.apply(y, A[0])
    assert np.abs(shared - np.einsum("vc,cbhw->vbhw", A[0], y)).max() <= 1e-12 * np.abs(want).max()
    got32 = cch.apply(y.astype(np.complex64), A.astype(np.complex64), np.float32)
    assert got32.dtype == np.complex64 and np.abs(got32 - want).max() <= 1e-5 * np.abs(want).max()
    c = cch.compress(y, 2, 3, 2)
    assert c["y"].shape == (2, 2, 16, 16) and c["A"].shape == (2, 2, 3)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_declarations(pkg):
    header = open(os.path.join(REPO, "include", "ipdm.h")).read()
    i, P, i64 = pkg.lib.c_int, pkg.lib.P, pkg.lib.c_int64
    want = {"ipdm_coilcomp_supported": ("int", [i, i]),
            "ipdm_coilcomp_workspace_bytes": ("size_t", [i, i]),
            "ipdm_coil_gram_c64": ("int", [P, i, i, P, i, i, i, i, P]),
            "ipdm_coilcomp_matrix_c64": ("int", [P, P, i, P, P, P, i, i, P]),
            "ipdm_coil_apply_c64": ("int", [P, P, i, P, i, i, i, i64, P]),
            "ipdm_coil_compress_c64": ("int", [P, i, i, i, P, P, P, P, P, P, i, i, i, i, P])}
    for name, (ret, args) in want.items():
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ipdm.h"
        assert m.group(1) == ret and len(m.group(2).split(",")) == len(args)
        assert pkg.lib.SIGNATURES[name] == args and hasattr(pkg.lib.lib, name)
    assert pkg.lib.lib.ipdm_coilcomp_workspace_bytes.restype is ctypes.c_size_t
    assert "#define IPDM_ABI_VERSION 4" in header and pkg.lib.lib.ipdm_abi_version() == 4


def test_abi_answers_without_a_gpu(pkg):
    lib = pkg.lib.lib
    for (n, nv), want in (((1, 1), 1), ((64, 32), 1), ((64, 33), 0), ((65, 8), 0), ((33, 12), 1), ((4, 5), 0), ((4, 0), 0),
                          ((0, 0), 0), ((32, 32), 1), ((40, 32), 1)):
        assert lib.ipdm_coilcomp_supported(n, nv) == want
        assert pkg.ops.coilcomp_supported(n, nv) == bool(want)
    assert lib.ipdm_coilcomp_workspace_bytes(3, 33) == 3 * 33 * 33 * 8
    for args in ((0, 4), (1, 65), (1, 0), (65536, 4)):
        assert lib.ipdm_coilcomp_workspace_bytes(*args) == 0
    # rejected before any launch: the box, the counts, NULL tensors (ah = 3, aw = 4 on 8 x 8: 8 // 2 + 4 = 8 is outside)
    EINVAL, EUNSUP = pkg.lib.IPDM_EINVAL, pkg.lib.IPDM_EUNSUPPORTED
    assert lib.ipdm_coil_gram_c64(None, 3, 4, None, 1, 2, 8, 8, None) == EINVAL
    assert lib.ipdm_coil_gram_c64(None, 3, 3, None, 1, 2, 8, 8, None) == EINVAL          # the box is fine, the tensors NULL
    assert lib.ipdm_coil_gram_c64(None, 3, 3, None, 0, 2, 8, 8, None) == 0               # an empty batch
    assert lib.ipdm_coil_gram_c64(None, -1, 3, None, 1, 2, 8, 8, None) == EINVAL
    assert lib.ipdm_coil_gram_c64(None, 3, 3, None, 1, 65, 8, 8, None) == EUNSUP
    assert lib.ipdm_coilcomp_matrix_c64(None, None, 8, None, None, None, 1, 65, None) == EUNSUP
    assert lib.ipdm_coilcomp_matrix_c64(None, None, 5, None, None, None, 1, 4, None) == EUNSUP
    assert lib.ipdm_coilcomp_matrix_c64(None, None, 0, None, None, None, 1, 4, None) == EINVAL
    assert lib.ipdm_coilcomp_matrix_c64(None, None, 2, None, None, None, 1, 4, None) == EINVAL
    assert lib.ipdm_coil_apply_c64(None, None, 1, None, 1, 64, 33, 16, None) == EUNSUP
    assert lib.ipdm_coil_apply_c64(None, None, 1, None, 1, 4, 2, 16, None) == EINVAL
    assert lib.ipdm_coil_apply_c64(None, None, 1, None, 1, 4, 2, 0, None) == 0
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf)
    assert lib.ipdm_coil_apply_c64(p, p + 2048, 0, p + 64, 1, 4, 2, 16, None) == EINVAL  # out inside y: 4 * 16 * 8 = 512 bytes
    assert lib.ipdm_coil_compress_c64(None, 3, 4, 2, None, None, None, None, None, None, 1, 4, 8, 8, None) == EINVAL
    assert lib.ipdm_coil_compress_c64(None, 3, 3, 33, None, None, None, None, None, None, 1, 64, 8, 8, None) == EUNSUP


# ---- Python front ends ----------------------------------------------------------------------------------------------------------
def test_check_noise_cov(pkg):
    psi = cch.noise_cov(4, 50.0, 0)
    got = pkg.ops.check_noise_cov(psi, 4)
    assert got.dtype == torch.complex128 and np.abs(got.numpy() - psi).max() <= 1e-15
    assert pkg.ops.check_noise_cov(torch.eye(3), 3).dtype == torch.complex128          # real is fine
    assert pkg.ops.check_noise_cov(np.eye(3, dtype=np.float32), 3).dtype == torch.complex128
    lop = psi.copy()
    lop[0, 1] += 0.1
    for bad in (-psi, psi[:3, :3], psi[:3], np.zeros((4, 4)), lop, np.full((4, 4), np.nan), psi[None]):
        with pytest.raises(ValueError):
            pkg.ops.check_noise_cov(bad, 4)
    for bad in (np.eye(4, dtype=np.int64), [[1.0]], None):
        with pytest.raises(TypeError):
            pkg.ops.check_noise_cov(bad, 4)


def test_ops_argument_checks_without_a_gpu(pkg):
    ops = pkg.ops
    y = torch.zeros(4, 1, 16, 16, dtype=torch.complex64)
    for call in (lambda: ops.coil_gram(y, 2, 2), lambda: ops.coil_compress(y, 2, 2, 2),
                 lambda: ops.coil_apply(y, torch.zeros(2, 4, dtype=torch.complex64)),
                 lambda: ops.coilcomp_matrix(torch.zeros(1, 4, 4, dtype=torch.complex64), 2)):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            call()
    with pytest.raises(ValueError):
        ops._coilcomp_counts(4, 5, "t")
    with pytest.raises(ValueError):
        ops._coilcomp_counts(4, 0, "t")
    with pytest.raises(ValueError):
        ops._coilcomp_counts(4, 2.5, "t")
    with pytest.raises(pkg.lib.IpdmUnsupported):
        ops._coilcomp_counts(65, 8, "t")
    with pytest.raises(pkg.lib.IpdmUnsupported):
        ops._coilcomp_counts(64, 33, "t")
    assert ops._coilcomp_counts(64, 32, "t") == 32
    assert ops.coilcomp_workspace(0, 4, "cpu") is None


def test_compress_measurement_checks_come_before_the_gpu(pkg):
    S = pkg.uf.SENSE
    mask = line_mask(32)
    y = torch.zeros(8, 32, 32, dtype=torch.complex64)
    with pytest.raises(TypeError):
        S.compress_measurement(y.real, mask, 4)
    with pytest.raises(TypeError):
        S.compress_measurement([1, 2], mask, 4)
    with pytest.raises(ValueError):
        S.compress_measurement(y[0], mask, 4)
    with pytest.raises(ValueError):
        S.compress_measurement(y, mask, 9)
    with pytest.raises(ValueError):
        S.compress_measurement(y, mask, 4, noise_cov=-np.eye(8))
    with pytest.raises(ValueError):
        S.compress_measurement(y, mask, 4, noise_cov=np.eye(7))
    with pytest.raises(pkg.lib.IpdmUnsupported):
        S.compress_measurement(torch.zeros(65, 32, 32, dtype=torch.complex64), mask, 8)
    with pytest.raises(ValueError, match="calibration region"):
        S.compress_measurement(y, torch.tensor([True, False] * 16), 4)       # every other line: no 5 x 5 centre
    with pytest.raises(ValueError, match="n_virtual"):
        S.from_measurement(y, mask, noise_cov=np.eye(8))


def test_load_noise_cov(pkg, tmp_path):
    psi = cch.noise_cov(5, 20.0, 1)
    torch.save(torch.from_numpy(psi), tmp_path / "psi.pt")
    np.save(tmp_path / "psi.npy", psi)
    np.save(tmp_path / "real.npy", psi.real.astype(np.float32))
    for name in ("psi.pt", "psi.npy"):
        got = pkg.load.load_noise_cov(str(tmp_path / name))
        assert got.dtype == torch.complex128 and tuple(got.shape) == (5, 5) and np.array_equal(got.numpy(), psi)
    got = pkg.load.load_noise_cov(str(tmp_path / "real.npy"))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), psi.real.astype(np.float32).astype(np.float64))
    np.save(tmp_path / "rect.npy", psi[:4])
    np.save(tmp_path / "rank3.npy", psi[None])
    torch.save({"psi": torch.from_numpy(psi)}, tmp_path / "dict.pt")
    np.save(tmp_path / "psi.dat.npy", psi)
    os.rename(tmp_path / "psi.dat.npy", tmp_path / "psi.dat")
    for name in ("rect.npy", "rank3.npy", "dict.pt", "psi.dat"):
        with pytest.raises(ValueError):
            pkg.load.load_noise_cov(str(tmp_path / name))
    np.save(tmp_path / "int.npy", np.eye(5, dtype=np.int32))
    with pytest.raises(TypeError):
        pkg.load.load_noise_cov(str(tmp_path / "int.npy"))


def test_build_problem_refuses_bad_arguments_before_any_gpu_work(pkg):
    """device "cpu": anything that reached a kernel, or the score network, would raise something else"""
    bp = pkg.engine.build_problem
    mask = line_mask(32)
    y = torch.zeros(8, 32, 32, dtype=torch.complex64)
    kw = dict(H=32, W=32, mask=mask, measurement=y, estimate_maps=True)
    with pytest.raises(ValueError, match="n_virtual"):
        bp("cpu", 1, coil_compress=9, **kw)
    with pytest.raises(ValueError, match="n_virtual"):
        bp("cpu", 1, coil_compress=0, **kw)
    with pytest.raises(pkg.lib.IpdmUnsupported):
        bp("cpu", 1, coil_compress=8, **dict(kw, measurement=torch.zeros(65, 32, 32, dtype=torch.complex64)))
    with pytest.raises(ValueError, match="positive definite"):
        bp("cpu", 1, coil_compress=4, noise_cov=-np.eye(8), **kw)
    with pytest.raises(ValueError, match="shape"):
        bp("cpu", 1, coil_compress=4, noise_cov=np.eye(4), **kw)
    with pytest.raises(ValueError, match="coil_compress"):
        bp("cpu", 1, noise_cov=np.eye(8), **kw)
    with pytest.raises(ValueError, match="n_virtual"):
        bp("cpu", 1, H=32, W=32, num_sens=4, coil_compress=5)               # simulated measurement


def test_driver_refuses_bad_compression_arguments_before_anything_is_written(tmp_path):
    np.save(tmp_path / "psi.npy", -np.eye(8))
    torch.save(line_mask(64), tmp_path / "mask.pt")
    base = [sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_real_img.py"), "--image_size", "64", "--n_levels", "1",
            "--num_sens", "8", "--mask", str(tmp_path / "mask.pt"), "--save_dir", str(tmp_path / "out")]
    for extra, word in ((["--coil_compress", "9"], "n_virtual"), (["--coil_compress", "0"], "n_virtual"),
                        (["--coil_compress", "4", "--noise_cov", str(tmp_path / "psi.npy")], "positive definite"),
                        (["--noise_cov", str(tmp_path / "psi.npy")], "--coil_compress")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode != 0 and word in r.stderr, r.stderr[-2000:]
        assert not (tmp_path / "out").exists()
