"""float64 numpy restatement of the non-Cartesian SENSE formulas, written from the formulas alone:
direct non-uniform DFT forward / adjoint, the Toeplitz kernel T, its spectrum P, the Toeplitz normal operator and the
conjugate-gradient proximal.  Inputs are whatever the GPU gets (float32 images / maps, float64 trajectory), promoted.

Conventions: trajectory k (M, 2) = (k_y, k_x) in cycles per field of view; images [..., H, W]; samples [..., M];
maps S [n, H, W]; coil axis first, as in the package ([n, B, ...]).
"""
from argparse import Namespace

import numpy as np


def radial(n_spokes, n_readout, H, W, golden=True):
    """spokes through the centre: t = (j - n_readout/2)/n_readout, angle i*pi*(sqrt(5)-1)/2 (golden) or i*pi/n_spokes"""
    t = (np.arange(n_readout, dtype=np.float64) - n_readout / 2) / n_readout
    i = np.arange(n_spokes, dtype=np.float64)
    ang = i * np.pi * (np.sqrt(5.0) - 1.0) / 2.0 if golden else i * np.pi / n_spokes
    ky = (t[None, :] * np.sin(ang)[:, None]) * H
    kx = (t[None, :] * np.cos(ang)[:, None]) * W
    return np.stack([ky.reshape(-1), kx.reshape(-1)], axis=1)


def edge_trajectory(n_spokes, n_readout, H, W):
    """the radial trajectory plus the points the bounds allow and the kernels must serve: -N/2, +N/2, 0 on both axes"""
    k = radial(n_spokes, n_readout, H, W)
    extra = np.array([[-H / 2, -W / 2], [H / 2, W / 2], [0.0, 0.0], [-H / 2, W / 2], [H / 2, 0.0], [0.25, -W / 2 + 0.5]])
    k = np.concatenate([k, extra])
    return k


def ramp_weights(k, H, W):
    """|k| in normalised units, sum w = H W"""
    r = np.sqrt((k[:, 0] / H) ** 2 + (k[:, 1] / W) ** 2)
    r = r + 0.5 / max(H, W)
    return r * (H * W / r.sum())


def smooth_maps(n, H, W, seed=0, rss=True):
    """smooth complex maps (low-order plane waves times Gaussians), RSS-normalised"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    maps = []
    for c in range(n):
        cy, cx = rng.uniform(-1, 1, 2)
        ph = rng.uniform(-1.5, 1.5, 3)
        mag = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 2.0) + 0.1
        maps.append(mag * np.exp(1j * (ph[0] + ph[1] * yy + ph[2] * xx)))
    S = np.stack(maps)
    if rss:
        S = S / np.sqrt((np.abs(S) ** 2).sum(0, keepdims=True))
    return S.astype(np.complex64)


def _phasors(k, H, W):
    """Ey [M, H] = exp(-2 pi i k_y (r - H/2)/H), Ex [M, W] likewise"""
    k = np.asarray(k, dtype=np.float64)
    Ey = np.exp(-2j * np.pi * k[:, 0:1] * (np.arange(H) - H // 2)[None, :] / H)
    Ex = np.exp(-2j * np.pi * k[:, 1:2] * (np.arange(W) - W // 2)[None, :] / W)
    return Ey, Ex


def ndft_forward(img, k):
    """img [..., H, W] -> [..., M]"""
    img = np.asarray(img, dtype=np.complex128)
    H, W = img.shape[-2:]
    Ey, Ex = _phasors(k, H, W)
    return np.einsum("mr,mc,...rc->...m", Ey, Ex, img, optimize=True) / np.sqrt(H * W)


def ndft_adjoint(y, k, H, W, w=None):
    """y [..., M] -> [..., H, W], weights w [M] applied to the samples first"""
    y = np.asarray(y, dtype=np.complex128)
    if w is not None:
        y = y * np.asarray(w, dtype=np.float64)
    Ey, Ex = _phasors(k, H, W)
    return np.einsum("mr,mc,...m->...rc", Ey.conj(), Ex.conj(), y, optimize=True) / np.sqrt(H * W)


def sense_forward(x, S, k):
    """x [B, H, W], S [n, H, W] or None -> y [n, B, M]"""
    x = np.asarray(x, dtype=np.complex128)
    S = np.ones((1,) + x.shape[-2:]) if S is None else np.asarray(S, dtype=np.complex128)
    return ndft_forward(S[:, None] * x[None], k)


def sense_adjoint(y, S, k, H, W, w=None):
    """y [n, B, M] -> x [B, H, W]"""
    img = ndft_adjoint(y, k, H, W, w)
    S = np.ones((1, H, W)) if S is None else np.asarray(S, dtype=np.complex128)
    return (S.conj()[:, None] * img).sum(0)


def toeplitz_T(k, H, W, w=None):
    """T [2H, 2W], lag 0 at (H, W); row 0 and column 0 (the unused lag -N) are zero"""
    k = np.asarray(k, dtype=np.float64)
    w = np.ones(len(k)) if w is None else np.asarray(w, dtype=np.float64)
    Ly = np.exp(2j * np.pi * k[:, 0:1] * (np.arange(2 * H) - H)[None, :] / H)
    Lx = np.exp(2j * np.pi * k[:, 1:2] * (np.arange(2 * W) - W)[None, :] / W)
    T = np.einsum("m,mr,mc->rc", w, Ly, Lx, optimize=True)
    T[0, :] = 0
    T[:, 0] = 0
    return T


def fft2c(a, inverse=False):
    """centred orthonormal 2-D FFT over the last two axes"""
    f = np.fft.ifft2 if inverse else np.fft.fft2
    return np.fft.fftshift(f(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def toeplitz_psf_complex(k, H, W, w=None):
    """P before its (vanishing) imaginary part is dropped: centred unnormalised DFT of T, over H W"""
    T = toeplitz_T(k, H, W, w)
    return fft2c(T) * np.sqrt(4.0 * H * W) / (H * W)


def toeplitz_psf(k, H, W, w=None):
    return toeplitz_psf_complex(k, H, W, w).real


def toeplitz_normal(x, S, P):
    """x [B, H, W] -> sum_c conj(S_c) crop(F^-1(P F(pad(S_c x))))"""
    x = np.asarray(x, dtype=np.complex128)
    B, H, W = x.shape
    S = np.ones((1, H, W)) if S is None else np.asarray(S, dtype=np.complex128)
    pad = np.zeros((S.shape[0], B, 2 * H, 2 * W), dtype=np.complex128)
    pad[:, :, H // 2:H // 2 + H, W // 2:W // 2 + W] = S[:, None] * x[None]
    out = fft2c(np.asarray(P, dtype=np.float64) * fft2c(pad), inverse=True)[:, :, H // 2:H // 2 + H, W // 2:W // 2 + W]
    return (S.conj()[:, None] * out).sum(0)


def normal_direct(x, S, k, w=None):
    """A^H W A x by the direct transforms"""
    H, W = x.shape[-2:]
    return sense_adjoint(sense_forward(x, S, k), S, k, H, W, w)


def cg_prox(z, ahy, normal, a, max_iter, tol):
    """(I + a N) x = z + a A^H y per sample by CG from x0 = z, the solver's stopping rule: |r| <= tol |b|, or <r,r> /
    <p,q> not positive.  z, ahy [B, H, W]; normal: [B, H, W] -> [B, H, W].  -> (x, iters [B])"""
    z = np.asarray(z, dtype=np.complex128)
    ahy = np.asarray(ahy, dtype=np.complex128)
    B = z.shape[0]
    x = z.copy()
    iters = np.zeros(B, dtype=np.int64)
    if a == 0:
        return x, iters
    b = z + a * ahy
    r = -a * (normal(z) - ahy)
    p = r.copy()
    rr = (np.abs(r) ** 2).sum((1, 2))
    bb = (np.abs(b) ** 2).sum((1, 2))
    frozen = ~(rr > 0) | (rr <= tol * tol * bb)
    for _ in range(max_iter):
        if frozen.all():
            break
        q = p + a * normal(p)
        pq = (p.conj() * q).real.sum((1, 2))
        for i in range(B):
            if frozen[i]:
                continue
            if not pq[i] > 0:
                frozen[i] = True
                continue
            alpha = rr[i] / pq[i]
            x[i] += alpha * p[i]
            r[i] -= alpha * q[i]
            new = (np.abs(r[i]) ** 2).sum()
            iters[i] += 1
            if not new > 0:
                frozen[i] = True
            else:
                p[i] = r[i] + (new / rr[i]) * p[i]
                frozen[i] = new <= tol * tol * bb[i]
            rr[i] = new
    return x, iters


def prox_residual(x, z, ahy, S, k, a, w=None):
    """|b - (I + a A^H W A) x| / |b| per sample, with the direct transforms"""
    b = z + a * ahy
    res = b - (x + a * normal_direct(x, S, k, w))
    return np.sqrt((np.abs(res) ** 2).sum((1, 2)) / (np.abs(b) ** 2).sum((1, 2)))


def relerr(got, ref):
    """max |err| / max |ref|"""
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


# ---- the edge cases of tests/test_noncart_edges_{gpu,host}.py: shapes past one sample stage, column tile and grid round -----
NC_STAGE = 256                                   # samples per LDS stage and columns per tile of ndft_adjoint_kernel (NC_THREADS)
NC_FORWARD_TILE = 64                             # samples per workgroup of ndft_forward_kernel (NC_TILE)
NC_GRID_ROUND = 2048 * 256                       # table entries per grid round of nc_phasor_kernel (ipdm_ew_grid's cap x 256)

# name -> (H, W, B, coils, spokes, readout) with nh.edge_trajectory(spokes, readout, H, W)
EDGE_CASES = {"wide": (16, 320, 2, 3, 27, 64), "tall": (320, 16, 2, 3, 27, 64), "widest": (8, 1024, 1, 2, 9, 64),
              "smallest_wide": (2, 64, 3, 4, 5, 64), "smallest_tall": (64, 2, 3, 4, 5, 64)}
EDGE_WEIGHTS = ("none", "ramp", "blocky")
# (H, W, T, B, coils); frame_trajectory(T, H, W, 27, 33): 897 = 3 * 256 + 129 samples per frame
EDGE_FRAME_CASES = {"wide": (16, 320, 2, 4, 2), "tall": (320, 16, 3, 6, 1)}


def blocky_weights(k, H, W):
    """ramp weights, exactly zero on the samples [256, 512) and on the whole last partial stage of 256"""
    w = ramp_weights(k, H, W).astype(np.float32)
    w[NC_STAGE:2 * NC_STAGE] = 0
    w[len(k) // NC_STAGE * NC_STAGE:] = 0
    return w


def edge_weights(kind, k, H, W):
    """float32 weights [M] as the GPU gets them; None for "none\""""
    return {"none": lambda: None, "ramp": lambda: ramp_weights(k, H, W).astype(np.float32),
            "blocky": lambda: blocky_weights(k, H, W)}[kind]()


def frame_trajectory(T, H, W, spokes, readout):
    """(T, M, 2): frame t = `spokes` consecutive golden-angle spokes of radial(spokes * T, ...) plus the six bound points of
    edge_trajectory (tests/test_noncart_frames_gpu.py's frame_trajectory, restated here for the host file)"""
    whole = radial(spokes * T, readout, H, W).reshape(T, spokes * readout, 2)
    extra = edge_trajectory(1, 1, H, W)[1:]
    return np.ascontiguousarray(np.stack([np.concatenate([whole[t], extra]) for t in range(T)]))


_EDGE_INPUTS, _EDGE_REFS = {}, {}


def edge_inputs(name):
    """the inputs of one edge case, made once: the float32 / complex64 values the GPU gets, the float64 trajectory, and the
    weight-free float64 references (forward with maps, forward of coil images)"""
    if name not in _EDGE_INPUTS:
        H, W, B, n, spokes, readout = EDGE_CASES[name]
        rng = np.random.default_rng(H * 131 + W + 7 * n)
        k = edge_trajectory(spokes, readout, H, W)
        S = smooth_maps(n, H, W, seed=n)
        x = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
        y = (rng.standard_normal((n, B, len(k))) + 1j * rng.standard_normal((n, B, len(k)))).astype(np.complex64)
        imgs = (S[:, None] * x[None]).astype(np.complex64)
        _EDGE_INPUTS[name] = Namespace(name=name, H=H, W=W, B=B, n=n, M=len(k), k=k, S=S, x=x, y=y, imgs=imgs,
                                       Ax=sense_forward(x, S, k), Aimgs=ndft_forward(imgs, k))
    return _EDGE_INPUTS[name]


def edge_refs(name, kind):
    """the float64 references of one edge case that depend on the weights (kind in EDGE_WEIGHTS), made once and never
    written to: A^H W y combined and per coil, the spectrum P, T x with and without maps"""
    if (name, kind) not in _EDGE_REFS:
        c = edge_inputs(name)
        w = edge_weights(kind, c.k, c.H, c.W)
        coil_imgs = ndft_adjoint(c.y, c.k, c.H, c.W, w)
        AHy = (np.asarray(c.S, dtype=np.complex128).conj()[:, None] * coil_imgs).sum(0)
        P = toeplitz_psf(c.k, c.H, c.W, w)
        r = Namespace(w=w, coil_imgs=coil_imgs, AHy=AHy, P=P, Tx=toeplitz_normal(c.x, c.S, P),
                      Tx_nomaps=toeplitz_normal(c.x, None, P))
        for a in (coil_imgs, AHy, P, r.Tx, r.Tx_nomaps):
            a.setflags(write=False)
        _EDGE_REFS[name, kind] = r
    return _EDGE_REFS[name, kind]


def prox_problem(H, W, spokes, readout, B=3, n=4):
    """the proximal problem of tests/test_noncart_gpu.py's _prox_problem, host arrays only: seed H + W, radial trajectory,
    measurements of a random-phase image through the float64 forward transform"""
    rng = np.random.default_rng(H + W)
    k = radial(spokes, readout, H, W)
    S = smooth_maps(n, H, W, seed=1)
    z = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
    img = (rng.random((B, H, W)) * np.exp(1j * rng.standard_normal((B, H, W)))).astype(np.complex64)
    y = sense_forward(img, S, k).astype(np.complex64)
    return Namespace(H=H, W=W, B=B, n=n, k=k, S=S, z=z, y=y)


_PROX_REFS = {}


def prox_reference(H, W, spokes, readout, B, n, a, max_iter, tol):
    """-> (problem, A^H y, float64 CG solution, its iteration counts), made once per argument list"""
    key = (H, W, spokes, readout, B, n, a, max_iter, tol)
    if key not in _PROX_REFS:
        p = prox_problem(H, W, spokes, readout, B, n)
        ahy = sense_adjoint(p.y, p.S, p.k, H, W)
        P = toeplitz_psf(p.k, H, W)
        ref, it = cg_prox(p.z, ahy, lambda v: toeplitz_normal(v, p.S, P), a, max_iter, tol)
        _PROX_REFS[key] = (p, ahy, ref, it)
    return _PROX_REFS[key]
