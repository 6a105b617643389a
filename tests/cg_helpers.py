"""float64 reference of the exact multi-coil proximal for the CG tests: the SENSE operators of oracle/kspace.py with the
same centring and orthonormal scale, kept in complex128 (the oracle's own round to complex64 inside every transform),
and a textbook conjugate-gradient solver of (I + a A^H A) x = z + a A^H y per sample."""
import numpy as np


def fft2c(x):
    k = np.fft.fftn(np.fft.ifftshift(x, axes=(-1, -2)), axes=(-1, -2), norm="ortho")
    return np.fft.fftshift(k, axes=(-1, -2))


def ifft2c(k):
    x = np.fft.ifftn(np.fft.ifftshift(k, axes=(-1, -2)), axes=(-1, -2), norm="ortho")
    return np.fft.fftshift(x, axes=(-1, -2))


def forward(x, maps, mask):
    """x (B,1,H,W), maps (n,H,W), mask broadcastable against (B,1,H,W) -> (n,B,1,H,W) complex128"""
    x = np.asarray(x, dtype=np.complex128)
    return np.stack([mask * fft2c(np.asarray(maps[i], dtype=np.complex128) * x) for i in range(maps.shape[0])], 0)


def adjoint(s, maps, mask):
    s = np.asarray(s, dtype=np.complex128)
    return sum(np.conj(np.asarray(maps[i], dtype=np.complex128)) * ifft2c(mask * s[i]) for i in range(maps.shape[0]))


def normal(x, a, maps, mask):
    """N x = x + a A^H A x"""
    return x + a * adjoint(forward(x, maps, mask), maps, mask)


def rhs(z, y, a, maps, mask):
    """b = z + a A^H y"""
    return np.asarray(z, dtype=np.complex128) + a * adjoint(y, maps, mask)


def sample_norm(v):
    """per-sample 2-norm of (B, ...) -> (B,)"""
    return np.sqrt((np.abs(v) ** 2).reshape(v.shape[0], -1).sum(1))


def cg_solve(z, y, a, maps, mask, rtol=1e-13, max_iter=500):
    """float64 CG from x0 = z, every sample to |b - N x| <= rtol |b| (recursive residual) -> x* (B,1,H,W) complex128"""
    b = rhs(z, y, a, maps, mask)
    x = np.asarray(z, dtype=np.complex128).copy()
    r = b - normal(x, a, maps, mask)
    p = r.copy()
    bn = sample_norm(b)
    dot = lambda u, v: (u.conj() * v).real.reshape(u.shape[0], -1).sum(1)
    rr = dot(r, r)
    sh = (-1,) + (1,) * (x.ndim - 1)
    for _ in range(max_iter):
        live = np.sqrt(rr) > rtol * bn
        if not live.any():
            break
        q = normal(p, a, maps, mask)
        alpha = np.where(live, rr / np.where(live, dot(p, q), 1.0), 0.0)
        x = x + alpha.reshape(sh) * p
        r = r - alpha.reshape(sh) * q
        rr_new = dot(r, r)
        beta = np.where(live, rr_new / np.where(live, rr, 1.0), 0.0)
        p = r + beta.reshape(sh) * p
        rr = np.where(live, rr_new, rr)
    return x


def check_solution(x, z, y, a, maps, mask):
    """the product classes' check_solution in float64: mean over the batch of |x + a A^H A x - (z + a A^H y)|^2"""
    d = normal(np.asarray(x, dtype=np.complex128), a, maps, mask) - rhs(z, y, a, maps, mask)
    return float((sample_norm(d) ** 2).mean())
