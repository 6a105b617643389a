"""float64 numpy model of the non-Cartesian self-calibration chain, written from the formulas alone: cell
occupancy of a trajectory, the largest covered box, the raised-cosine window on the samples, the weighted Gram matrix of
the samples, the regularised per-coil inverse by conjugate gradients (the solver's stopping rule, ``noncart_helpers.cg_prox``
on the Toeplitz operator) and its centred FFT, the Cartesian calibration k-space.  The estimators that follow are the
models the Cartesian tests already have (``csm_helpers.estimate``, ``espirit_helpers.estimate``, ``coilcomp_helpers.matrix``).
Inputs are whatever the GPU gets (complex64 samples, float32 window, float64 trajectory), promoted."""
import numpy as np

import noncart_helpers as nch


def pooled(k):
    """(M, 2), or (T, M, 2) pooled frame by frame -> (T M, 2)"""
    return np.asarray(k, dtype=np.float64).reshape(-1, 2)


def cell_occupancy(k, H, W):
    """bool (H, W): cell (p, q) is sampled when some sample rounds (half up) to (p - H//2, q - W//2)"""
    k = pooled(k)
    occ = np.zeros((H, W), dtype=bool)
    for ky, kx in k:
        p, q = int(np.floor(ky + 0.5)) + H // 2, int(np.floor(kx + 0.5)) + W // 2
        if 0 <= p < H and 0 <= q < W:
            occ[p, q] = True
    return occ


def largest_box(occ, calib_max=12):
    """-> (ah, aw) of the largest box about (H//2, W//2) covered everywhere; ties: smaller |ah - aw|, then larger aw; None
    when the centre cell is empty"""
    H, W = occ.shape
    best = None
    for ah in range(min(H // 2, H - 1 - H // 2, calib_max) + 1):
        for aw in range(min(W // 2, W - 1 - W // 2, calib_max) + 1):
            if occ[H // 2 - ah:H // 2 + ah + 1, W // 2 - aw:W // 2 + aw + 1].all():
                key = ((2 * ah + 1) * (2 * aw + 1), -abs(ah - aw), aw)
                if best is None or key > best[0]:
                    best = (key, ah, aw)
    return None if best is None else (best[1], best[2])


def window_weights(k, ah, aw, taper=2.0):
    """1 where d = max(|k_y| - ah, |k_x| - aw) <= 0.5, 0.5 (1 + cos(pi (d - 0.5) / taper)) over the next `taper` cycles, 0
    beyond"""
    k = pooled(k)
    d = np.maximum(np.abs(k[:, 0]) - ah, np.abs(k[:, 1]) - aw) - 0.5
    w = np.zeros(len(k))
    for m, dm in enumerate(d):
        if dm <= 0:
            w[m] = 1.0
        elif dm < taper:
            w[m] = 0.5 * (1.0 + np.cos(np.pi * dm / taper))
    return w


def window(k, H, W, calib_max=12, taper=2.0):
    """-> (ah, aw, w (M,)); ValueError when the box is below 5 x 5"""
    box = largest_box(cell_occupancy(k, H, W), calib_max)
    if box is None or min(box) < 2:
        raise ValueError(f"no usable calibration window: {box}")
    return box[0], box[1], window_weights(k, box[0], box[1], taper)


def gram(y, w=None):
    """y [n, B, M] -> G [B, n, n] = sum_m w_m y_i conj(y_j), Hermitian by construction (upper triangle mirrored, real
    diagonal); y is looked at only where w_m > 0"""
    y = np.asarray(y).astype(np.complex128)
    n, B, M = y.shape
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    use = w > 0
    ys, ws = y[:, :, use], w[use]
    G = np.einsum("m,ibm,jbm->bij", ws, ys, ys.conj(), optimize=True)
    iu = np.triu_indices(n, 1)
    for b in range(B):
        G[b][(iu[1], iu[0])] = G[b][iu].conj()
        G[b][np.diag_indices(n)] = G[b][np.diag_indices(n)].real
    return G


def calib_images(y, k, H, W, w, lam=1e-2, max_iter=40, tol=1e-4):
    """y [n, B, M] -> (x [n, B, H, W], iters [n, B]): (A^H W A + lam t0 I) x_c = A^H W y_c, t0 = sum(w) / (H W), as the
    solver poses it: (I + a N) x = a A^H W y from x0 = 0 with a = 1 / (lam t0), N the Toeplitz operator"""
    y = np.asarray(y).astype(np.complex128)
    n, B, M = y.shape
    w = np.asarray(w, dtype=np.float64)
    t0 = w.sum() / (H * W)
    a = 1.0 / (lam * t0)
    P = nch.toeplitz_psf(k, H, W, w)
    ahy = nch.ndft_adjoint(y, k, H, W, w).reshape(n * B, H, W)
    x, iters = nch.cg_prox(np.zeros_like(ahy), ahy, lambda v: nch.toeplitz_normal(v, None, P), a, max_iter, tol)
    return x.reshape(n, B, H, W), iters.reshape(n, B)


def calib_kspace(y, k, H, W, w, lam=1e-2, max_iter=40, tol=1e-4):
    x, iters = calib_images(y, k, H, W, w, lam, max_iter, tol)
    return nch.fft2c(x), iters


def ellipse_phantom(H, W):
    """a few overlapping ellipses with a smooth phase, zero outside the body: complex128 (H, W)"""
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    img = 0.7 * ((xx / 0.72) ** 2 + (yy / 0.82) ** 2 <= 1.0)
    img = img + 0.3 * (((xx + 0.2) / 0.3) ** 2 + ((yy - 0.1) / 0.4) ** 2 <= 1.0)
    img = img - 0.4 * (((xx - 0.3) / 0.18) ** 2 + ((yy + 0.25) / 0.25) ** 2 <= 1.0)
    return img * np.exp(1j * (0.3 + 0.4 * xx - 0.5 * yy * xx))


def acquisition(H, W, spokes, readout, n, seed=0, B=1):
    """a simulated radial acquisition of the ellipse phantom through ``smooth_maps`` -> dict(k (M, 2), S (n, H, W), obj
    (B, H, W): the phantom times 1, 1/2, ...; y [n, B, M] complex64 as the GPU gets it; full [n, B, H, W]: the fully sampled
    Cartesian k-space of the same coil images)"""
    k = nch.radial(spokes, readout, H, W)
    S = nch.smooth_maps(n, H, W, seed).astype(np.complex128)
    obj = np.stack([ellipse_phantom(H, W) / (b + 1) for b in range(B)])
    coil = S[:, None] * obj[None]
    return dict(k=k, S=S, obj=obj, y=nch.ndft_forward(coil, k).astype(np.complex64), full=nch.fft2c(coil))


def box_of(ks, ah, aw):
    H, W = ks.shape[-2:]
    return ks[..., H // 2 - ah:H // 2 + ah + 1, W // 2 - aw:W // 2 + aw + 1]


def energy_kept(A, samples):
    """fraction of sum |samples|^2 (samples [n, K]) that the rows of A (nv, n) keep after orthonormalisation"""
    Q, _ = np.linalg.qr(np.asarray(A).astype(np.complex128).conj().T)
    s = np.asarray(samples).astype(np.complex128)
    return float((np.abs(Q.conj().T @ s) ** 2).sum() / (np.abs(s) ** 2).sum())
