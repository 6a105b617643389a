"""float64 restatement of the ESPIRiT estimator (csrc/espirit.hip) for the espirit tests, step by step:
calibration Gram matrix, row space, kernel correlation K, per-pixel G(x) by the direct DFT of K's taps, power iteration
from normalise(G 1), Rayleigh quotient, conj, coil-0 gauge, crop.  ``dtype=np.float32`` runs stage 4 (everything after K,
which is rounded to complex64 as the kernel stores it) in single precision on the CPU: the GPU tests' rounding yardstick.
``exp_sign=+1`` and ``conj=False`` are deliberate mutations for the tests' own sensitivity checks."""
import itertools

import numpy as np
import torch

_CDTYPE = {np.float64: np.complex128, np.float32: np.complex64}


def calib_box(y, ah, aw):
    """y (n, H, W) -> the calibration box (n, 2ah+1, 2aw+1)"""
    H, W = y.shape[-2:]
    return y[..., H // 2 - ah:H // 2 + ah + 1, W // 2 - aw:W // 2 + aw + 1]


def gram(y, ah, aw, k):
    """y (n, H, W) complex -> (Gm (M, M) complex128, n_patches); columns in the order (coil, ty, tx)"""
    box = np.asarray(calib_box(np.asarray(y), ah, aw)).astype(np.complex128)
    bh, bw = box.shape[-2:]
    A = np.array([box[:, r:r + k, c:c + k].reshape(-1) for r in range(bh - k + 1) for c in range(bw - k + 1)])
    return A.conj().T @ A, A.shape[0]


def row_space(Gm, sv_thresh):
    """-> (lam descending, V, rank, margin): margin is the relative distance of the nearest singular value to the threshold"""
    lam, V = np.linalg.eigh(Gm)
    lam, V = lam[::-1], V[:, ::-1]
    s = np.sqrt(np.maximum(lam, 0))
    r = int((s > sv_thresh * s[0]).sum())
    t = sv_thresh * s[0]
    margin = float(np.abs(s - t).min() / t) if t > 0 else np.inf
    return lam, V, r, margin


def correlation(V, r, n, k):
    """K (n, n, 2k-1, 2k-1) complex128 from the first r columns of V"""
    P = (V[:, :r] @ V[:, :r].conj().T).reshape(n, k, k, n, k, k)
    K = np.zeros((n, n, 2 * k - 1, 2 * k - 1), np.complex128)
    for ty, tx, uy, ux in itertools.product(range(k), repeat=4):
        K[:, :, ty - uy + k - 1, tx - ux + k - 1] += P[:, ty, tx, :, uy, ux]
    return K


def pixel_stage(K, k, H, W, crop=0.8, power_iters=30, dtype=np.float64, exp_sign=-1, conj=True):
    """K (n, n, 2k-1, 2k-1) -> dict(maps (n, H, W), eigval (H, W), lam2 (H, W): the second eigenvalue of G(x), from a
    float64 eigvalsh), in `dtype` arithmetic"""
    cdt = _CDTYPE[dtype]
    n = K.shape[0]
    d = np.arange(-(k - 1), k)
    Ey = np.exp(exp_sign * 2j * np.pi * np.outer(np.arange(H) - H // 2, d) / H).astype(cdt)
    Ex = np.exp(exp_sign * 2j * np.pi * np.outer(np.arange(W) - W // 2, d) / W).astype(cdt)
    Kc = K.astype(cdt)
    T = np.einsum('abyx,wx->abyw', Kc, Ex)
    G = (np.einsum('abyw,hy->hwab', T, Ey) / dtype(k * k)).astype(cdt)

    def normalise(v):
        nrm = np.sqrt((v.real ** 2 + v.imag ** 2).sum(-1, keepdims=True)).astype(dtype)
        return (v / np.where(nrm == 0, dtype(1), nrm)).astype(cdt)

    u = normalise(G.sum(-1))
    for _ in range(power_iters):
        u = normalise(np.einsum('hwab,hwb->hwa', G, u))
    Gu = np.einsum('hwab,hwb->hwa', G, u)
    eigval = (u.conj() * Gu).sum(-1).real.astype(dtype)
    m = u.conj() if conj else u
    mag = np.abs(m[..., 0])
    ph = np.where(mag > 0, m[..., 0].conj() / np.where(mag > 0, mag, 1), 1).astype(cdt)
    m = m * ph[..., None]
    m[..., 0] = np.where(mag > 0, mag, m[..., 0])
    maps = np.where((eigval > dtype(crop))[..., None], m, 0).astype(cdt)
    ev = np.linalg.eigvalsh(G.astype(np.complex128))
    return dict(maps=np.moveaxis(maps, -1, 0), eigval=eigval, lam2=ev[..., -2] if n > 1 else np.zeros((H, W)),
                lam1=ev[..., -1])


def estimate(y, ah, aw, k=6, sv_thresh=0.02, crop=0.8, power_iters=30, dtype=np.float64, **mut):
    """y (n, H, W) complex -> dict(gram, n_patches, lam, rank, margin, K (complex64-rounded, as complex128), maps, eigval,
    lam1, lam2, leave_out (H, W) bool: pixels near the crop threshold or kept and near-degenerate)"""
    y = np.asarray(torch.as_tensor(y).numpy() if isinstance(y, torch.Tensor) else y)
    n, H, W = y.shape
    Gm, n_patches = gram(y, ah, aw, k)
    lam, V, r, margin = row_space(Gm, sv_thresh)
    K = correlation(V, r, n, k)
    K32 = K.astype(np.complex64).astype(np.complex128)            # the kernel's K is stored as complex64
    out = pixel_stage(K32, k, H, W, crop, power_iters, dtype, **mut)
    ev = out["eigval"].astype(np.float64)
    near_crop = np.abs(ev - crop) < 1e-3
    degenerate = (ev > crop) & (out["lam1"] - out["lam2"] < 0.05)
    out.update(gram=Gm, n_patches=n_patches, lam=lam, rank=r, margin=margin, K=K, leave_out=near_crop | degenerate)
    return out


def true_maps(maps):
    """unit-RSS, coil-0-gauged version of true maps (n, H, W)"""
    maps = np.asarray(maps).astype(np.complex128)
    rss = np.sqrt((np.abs(maps) ** 2).sum(0))
    m = maps / np.where(rss > 0, rss, 1)
    mag = np.abs(m[0])
    return m * np.where(mag > 0, m[0].conj() / np.where(mag > 0, mag, 1), 1)
