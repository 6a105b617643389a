"""Restatement of geometric coil compression along the readout for the gcc tests, steps 1-5 of its
contract: the centred readout transform, the windowed Gram matrix per readout position, the matrix stage of
coilcomp_helpers on every position, the alignment along x and the per-row application.  ``dtype=np.float64`` is the
reference (numpy's FFT, an SVD polar factor); ``dtype=np.float32`` performs the kernels' operations in the kernels' order
(csrc/gcc.hip, csrc/kspace_fft.h) on (real, imaginary) float32 array pairs -- the Stockham stages with the fp32 twiddle
table, the Newton-Schulz iteration sum by sum -- which is what the GPU tests take their bounds from.  Only the Gram matrix
differs, as in coilcomp_helpers: the kernel sums in double and rounds once, the float32 run is numpy's complex64 product."""
import numpy as np
import torch

import coilcomp_helpers as cc

NS_ITERS = 30                                   # the kernel's counts
NS_TOL = 1.0e-3
RADIX_CONST = dict(S3=0.86602540378443864676, C1=0.30901699437494742410, C2=-0.80901699437494742410,
                   S1=0.95105651629515357212, S2=0.58778525229247312917)


def _np(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def _cd(dtype):
    return np.complex128 if dtype == np.float64 else np.complex64


# ---- step 1: the readout transform --------------------------------------------------------------------------------------------
def _stages(N):
    """radices of the kernel's Stockham pass over a line of N = 2^a 3^b 5^c: 4s, a 2, 3s, 5s"""
    p2, out = N & -N, []
    Ns = 1
    while Ns * 4 <= p2:
        out.append(4)
        Ns *= 4
    if Ns < p2:
        out.append(2)
        Ns *= 2
    while (N // Ns) % 3 == 0:
        out.append(3)
        Ns *= 3
    while Ns < N:
        assert (N // Ns) % 5 == 0, f"{N} is not of the form 2^a 3^b 5^c"
        out.append(5)
        Ns *= 5
    return out


def _stockham32(xr, xi, inverse):
    """uncentred, unnormalised DFT along axis 0 of float32 (xr, xi) [N, lines], the operations of fft_stage in order"""
    f = np.float32
    N = xr.shape[0]
    q = np.arange(N)
    twr, twi = np.cos(-2.0 * np.pi * q / N).astype(f), np.sin(-2.0 * np.pi * q / N).astype(f)
    # sincospi is exact at the multiples of a quarter turn
    for m, (c, s) in ((0, (1, 0)), (N // 4, (0, -1)), (N // 2, (-1, 0)), (3 * N // 4, (0, 1))):
        if N % 4 == 0:
            twr[m], twi[m] = c, s
    if inverse:
        twi = -twi
    k_ = {k: f(v) for k, v in RADIX_CONST.items()}
    half = f(0.5)
    Ns = 1
    for R in _stages(N):
        nb = N // R
        j = np.arange(nb)
        k = j % Ns
        twstep = N // (Ns * R)
        vr, vi = [], []
        for t in range(R):
            ar, ai = xr[j + t * nb], xi[j + t * nb]
            if t > 0:
                wr, wi = twr[k * t * twstep][:, None], twi[k * t * twstep][:, None]
                ar, ai = ar * wr - ai * wi, ar * wi + ai * wr
            vr.append(ar)
            vi.append(ai)

        def jrot(nr, ni):                        # forward: -i n; inverse: +i n
            return (-ni, nr) if inverse else (ni, -nr)
        if R == 2:
            o = [(vr[0] + vr[1], vi[0] + vi[1]), (vr[0] - vr[1], vi[0] - vi[1])]
        elif R == 4:
            apc, amc = (vr[0] + vr[2], vi[0] + vi[2]), (vr[0] - vr[2], vi[0] - vi[2])
            bpd, bmd = (vr[1] + vr[3], vi[1] + vi[3]), (vr[1] - vr[3], vi[1] - vi[3])
            jb = jrot(*bmd)
            o = [(apc[0] + bpd[0], apc[1] + bpd[1]), (amc[0] + jb[0], amc[1] + jb[1]),
                 (apc[0] - bpd[0], apc[1] - bpd[1]), (amc[0] - jb[0], amc[1] - jb[1])]
        elif R == 3:
            t1 = (vr[1] + vr[2], vi[1] + vi[2])
            t2 = (vr[0] - half * t1[0], vi[0] - half * t1[1])
            t3 = (k_["S3"] * (vr[1] - vr[2]), k_["S3"] * (vi[1] - vi[2]))
            jt = jrot(*t3)
            o = [(vr[0] + t1[0], vi[0] + t1[1]), (t2[0] + jt[0], t2[1] + jt[1]), (t2[0] - jt[0], t2[1] - jt[1])]
        else:
            C1, C2, S1, S2 = k_["C1"], k_["C2"], k_["S1"], k_["S2"]
            t1, t3 = (vr[1] + vr[4], vi[1] + vi[4]), (vr[1] - vr[4], vi[1] - vi[4])
            t2, t4 = (vr[2] + vr[3], vi[2] + vi[3]), (vr[2] - vr[3], vi[2] - vi[3])
            m1 = (vr[0] + C1 * t1[0] + C2 * t2[0], vi[0] + C1 * t1[1] + C2 * t2[1])
            m2 = (vr[0] + C2 * t1[0] + C1 * t2[0], vi[0] + C2 * t1[1] + C1 * t2[1])
            n1 = (S1 * t3[0] + S2 * t4[0], S1 * t3[1] + S2 * t4[1])
            n2 = (S2 * t3[0] - S1 * t4[0], S2 * t3[1] - S1 * t4[1])
            j1, j2 = jrot(*n1), jrot(*n2)
            o = [(vr[0] + t1[0] + t2[0], vi[0] + t1[1] + t2[1]), (m1[0] + j1[0], m1[1] + j1[1]), (m2[0] + j2[0], m2[1] + j2[1]),
                 (m2[0] - j2[0], m2[1] - j2[1]), (m1[0] - j1[0], m1[1] - j1[1])]
        nr, ni = np.empty_like(xr), np.empty_like(xi)
        dst = (j - k) * R + k
        for t in range(R):
            nr[dst + t * Ns], ni[dst + t * Ns] = o[t]
        xr, xi = nr, ni
        Ns *= R
    return xr, xi


def readout(y, inverse=False, dtype=np.float64):
    """centred orthonormal (inverse) DFT along axis -2 of y (..., H, W), fft2c's centring"""
    y = _np(y)
    if dtype == np.float64:
        y = y.astype(np.complex128)
        f = np.fft.ifft if inverse else np.fft.fft
        return np.fft.fftshift(f(np.fft.ifftshift(y, axes=-2), axis=-2, norm="ortho"), axes=-2)
    H, W = y.shape[-2:]
    assert H % 4 == 0
    z = np.moveaxis(y.reshape(-1, H, W), 1, 0).reshape(H, -1)
    sign = np.where(np.arange(H) % 2 == 1, np.float32(-1), np.float32(1))[:, None]
    xr, xi = _stockham32(z.real.astype(np.float32) * sign, z.imag.astype(np.float32) * sign, bool(inverse))
    s = sign * (np.float32(1) / np.sqrt(np.float32(H)))
    out = (xr * s).astype(np.complex64) + np.complex64(1j) * (xi * s).astype(np.complex64)
    return np.moveaxis(out.reshape(H, -1, W), 0, 1).reshape(y.shape)


# ---- step 2: windowed Gram matrices -----------------------------------------------------------------------------------------
def window_rows(x, H, win):
    """[first, last] of the window of position x, clipped at the edges"""
    return max(0, x - win), min(H - 1, x + win)


def gram(h, aw, win, dtype=np.float64):
    """h (n, B, H, W) hybrid data -> G (B, H, n, n): rows [x-win, x+win] clipped, columns [W//2-aw, W//2+aw]"""
    h = _np(h).astype(_cd(dtype))
    n, B, H, W = h.shape
    if not (0 <= aw and W // 2 - aw >= 0 and W // 2 + aw <= W - 1):
        raise ValueError("the calibration columns leave the image")
    G = np.zeros((B, H, n, n), dtype=_cd(dtype))
    for x in range(H):
        r0, r1 = window_rows(x, H, win)
        s = h[:, :, r0:r1 + 1, W // 2 - aw:W // 2 + aw + 1].reshape(n, B, -1)
        for b in range(B):
            G[b, x] = cc.hermitian(s[:, b] @ s[:, b].conj().T)
    return G


# ---- step 3: the matrix stage on every position ------------------------------------------------------------------------------
def matrices(G, n_virtual, noise_cov=None, dtype=np.float64):
    """G (B, H, n, n) -> dict(A (B, H, nv, n) unaligned, eig (B, H, n), status (B, H))"""
    B, H, n, _ = G.shape
    m = cc.matrix(G.reshape(B * H, n, n), n_virtual, noise_cov, dtype)
    return dict(A=m["A"].reshape(B, H, n_virtual, n), eig=m["eig"].reshape(B, H, n), status=m["status"].reshape(B, H))


# ---- step 4: alignment ---------------------------------------------------------------------------------------------------------
def polar_svd(C):
    """the unitary P that makes P C Hermitian positive semidefinite: C = U S V^H -> P = V U^H"""
    U, s, Vh = np.linalg.svd(C)
    return Vh.conj().T @ U.conj().T, s


def _mm32(ar, ai, br, bi, conj_a=False, conj_b=False):
    """(ar + i ai)[i][k] (br + i bi)[k][j] summed over k ascending, float32, products and sums rounded one by one;
    conj_a: conj(a[k][i]) b[k][j] (a^H b); conj_b: a[i][k] conj(b[j][k]) (a b^H)"""
    if conj_a:
        ar, ai = ar.T, -ai.T
    if conj_b:
        br, bi = br.T, -bi.T
    outr = np.zeros((ar.shape[0], br.shape[1]), dtype=np.float32)
    outi = np.zeros_like(outr)
    for k in range(ar.shape[1]):
        pr, pi = ar[:, k:k + 1], ai[:, k:k + 1]
        qr, qi = br[k:k + 1, :], bi[k:k + 1, :]
        # the kernels' three product forms: a b, a conj(b) and conj(a) b, each two products and one sum per component
        outr = outr + (pr * qr - pi * qi)
        outi = outi + (pr * qi + pi * qr)
    return outr, outi


def newton_schulz32(Cr, Ci):
    """-> (Xr, Xi, degenerate): X <- 1.5 X - 0.5 X (X^H X) from X = C, NS_ITERS times, then the test on X^H X - I"""
    f = np.float32
    Xr, Xi = Cr.astype(f), Ci.astype(f)
    with np.errstate(all="ignore"):
        for _ in range(NS_ITERS):
            Yr, Yi = _mm32(Xr, Xi, Xr, Xi, conj_a=True)
            Zr, Zi = _mm32(Xr, Xi, Yr, Yi)
            Xr, Xi = f(1.5) * Xr - f(0.5) * Zr, f(1.5) * Xi - f(0.5) * Zi
        Yr, Yi = _mm32(Xr, Xi, Xr, Xi, conj_a=True)
        dr, di = np.abs(Yr - np.eye(Yr.shape[0], dtype=f)), np.abs(Yi)
    return Xr, Xi, bool((~(dr <= f(NS_TOL)) | ~(di <= f(NS_TOL))).any())


def align(Ahat, noise_cov=None, dtype=np.float64):
    """Ahat (B, H, nv, n) or (H, nv, n) -> dict(A of the same shape, status (B,), smin: the smallest singular value of any
    C = Ahat_x psi A_p^H met (float64 only)).  The centre row H // 2 is kept; outward in both directions A_x = P_x Ahat_x
    with p the nearest position on the centre side that was not degenerate; a degenerate position keeps Ahat_x."""
    Ahat = _np(Ahat)
    squeeze = Ahat.ndim == 3
    Ahat = (Ahat[None] if squeeze else Ahat).astype(_cd(dtype))
    B, H, nv, n = Ahat.shape
    psi = None if noise_cov is None else _np(noise_cov).astype(_cd(dtype))
    A = Ahat.copy()
    status = np.zeros(B, dtype=np.int32)
    smin = np.inf
    x0 = H // 2
    for b in range(B):
        for step in (-1, 1):
            prev = Ahat[b, x0]
            x = x0 + step
            while 0 <= x < H:
                cur = Ahat[b, x]
                if dtype == np.float64:
                    C = (cur if psi is None else cur @ psi) @ prev.conj().T
                    P, s = polar_svd(C)
                    smin = min(smin, float(s.min()))
                    bad = not s.min() > 1e-6
                    new = cur if bad else P @ cur
                else:
                    cr, ci = cur.real.astype(np.float32), cur.imag.astype(np.float32)
                    wr, wi = (cr, ci) if psi is None else _mm32(cr, ci, psi.real.astype(np.float32), psi.imag.astype(np.float32))
                    Cr, Ci = _mm32(wr, wi, prev.real.astype(np.float32), prev.imag.astype(np.float32), conj_b=True)
                    Xr, Xi, bad = newton_schulz32(Cr, Ci)
                    if bad:
                        new = cur
                    else:
                        nr, ni = _mm32(Xr, Xi, cr, ci, conj_a=True)
                        new = (nr + 1j * ni.astype(np.float64)).astype(np.complex64)
                A[b, x] = new
                if bad:
                    status[b] += 1
                else:
                    prev = new
                x += step
    return dict(A=A[0] if squeeze else A, status=status, smin=smin)


# ---- step 5: application ---------------------------------------------------------------------------------------------------------
def apply_rows(h, A, dtype=np.float64):
    """h (n, B, H, W), A (B, H, nv, n) or (H, nv, n) -> (nv, B, H, W): coil_apply's arithmetic with the matrix of each row"""
    h = _np(h)
    A = _np(A)
    n, B, H, W = h.shape
    A = np.broadcast_to(A, (B,) + A.shape[-3:]) if A.ndim == 3 else A
    return np.stack([cc.apply(h[:, :, x, :], A[:, x], dtype) for x in range(H)], axis=2)


def compress(y, aw, n_virtual, win=2, noise_cov=None, dtype=np.float64):
    """the whole chain -> dict(y (nv, B, H, W), A, Ahat, eig, status, gram, hybrid)"""
    y = _np(y)
    y = y[:, None] if y.ndim == 3 else y
    h = readout(y, True, dtype)
    G = gram(h, aw, win, dtype)
    m = matrices(G, n_virtual, noise_cov, dtype)
    al = align(m["A"], noise_cov, dtype)
    out = readout(apply_rows(h, al["A"], dtype), False, dtype)
    return dict(y=out, A=al["A"], Ahat=m["A"], eig=m["eig"], status=al["status"], gram=G, hybrid=h, smin=al["smin"])


def loss(y, yc):
    """1 - |y'|^2 / |y|^2 over all of k-space (an energy without whitening: the rows of the matrices are orthonormal)"""
    y, yc = _np(y).astype(np.complex128), _np(yc).astype(np.complex128)
    return 1.0 - float((np.abs(yc) ** 2).sum() / (np.abs(y) ** 2).sum())


def scc_loss(y, aw, n_virtual, dtype=np.float64):
    """the loss of the one-matrix-per-image compression from the calibration box (aw, aw)"""
    y = _np(y)
    y = y[:, None] if y.ndim == 3 else y
    return loss(y, cc.compress(y, aw, aw, n_virtual, None, dtype)["y"])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
# end-to-end cases: (n, nv, H, W, aw, win, seed); the float64 GCC / SCC loss ratio of each is at most 0.25 (test_gcc_host.py)
END_TO_END = ((12, 3, 32, 16, 3, 1, 3), (3, 1, 16, 16, 2, 0, 7), (16, 4, 48, 48, 6, 2, 0))


def line_mask(W, aw, extra=()):
    """bool (W,): the calibration columns [W//2-aw, W//2+aw] plus every fourth column and `extra`"""
    m = np.zeros(W, dtype=bool)
    m[W // 2 - aw:W // 2 + aw + 1] = True
    m[::4] = True
    m[list(extra)] = True
    return m


def designed_matrices(nv, n, H, seed, noise_cov=None, delta=1.6):
    """Ahat (H, nv, n) complex128 for the alignment test: Q_x times the first nv rows of U(x) = U0 exp(i delta x K), K a
    fixed Hermitian matrix of unit 2-norm (U smooth in x: the smallest singular value of any neighbour product C is 0.46 to
    0.77 on the tests' shapes), Q_x a seeded
    random nv x nv unitary; with a covariance psi = L L^H times L^-1, so that Ahat psi Ahat^H = I"""
    rng = np.random.default_rng(seed + 5)
    K = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    K = K + K.conj().T
    lam, V = np.linalg.eigh(K)
    lam = lam / np.abs(lam).max()
    U0 = cc.random_unitary(n, seed + 11)
    Linv = None if noise_cov is None else np.linalg.inv(np.linalg.cholesky(_np(noise_cov).astype(np.complex128)))
    out = np.zeros((H, nv, n), dtype=np.complex128)
    for x in range(H):
        U = U0 @ (V * np.exp(1j * delta * x * lam)[None]) @ V.conj().T
        a = cc.random_unitary(nv, seed + 1000 + x) @ U[:nv]
        out[x] = a if Linv is None else a @ Linv
    return out
