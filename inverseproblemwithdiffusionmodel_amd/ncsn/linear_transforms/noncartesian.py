"""Multi-coil SENSE for samples at arbitrary k-space positions (radial, spiral, ...): DESIGN.md 4.4l.

``NonCartesianSENSE`` is the measurement model  y[c, b, m] = (HW)^-1/2 sum_{r,col} S_c x[b] exp(-2 pi i (k_y,m (r - H/2)/H +
k_x,m (col - W/2)/W))  in the package's centred orthonormal convention: a trajectory on integer grid points reproduces
``i2k_complex`` at index (k_y + H/2, k_x + W/2).  The forward and adjoint transforms are exact direct sums in HIP kernels
(``ops.ndft_forward`` / ``ops.ndft_adjoint``) and run once per reconstruction; the sampler's data-consistency step,
``L2PenaltyCG``, applies A^H W A as a Toeplitz operator through the FFT passes (``ops.nc_sense_cgprox``).

Radial cine: a trajectory (T, M, 2) holds one trajectory per frame -- a *framed* operator.  Row b of
every image batch belongs to frame b % T, the rule of the Cartesian coil-map sets, so the (posterior sample, frame) batch
of ``ALD2DTime``, flattened frame-fastest, is served as it lies in memory.

Self-calibration: ``calibration_window`` finds the box of grid cells the samples cover about the centre
and a window on the samples; ``NonCartesianSENSE.estimate_sens_maps`` / ``compress_measurement`` / ``from_measurement``
take coil maps and a compression matrix from the samples themselves (a regularised per-coil inverse of the windowed
samples gives Cartesian calibration k-space for the Walsh and ESPIRiT estimators; cine frames are pooled).

The reference has no non-Cartesian code.  Out of scope: map sets and stacks, geometric compression, a second ESPIRiT map
set, view-shared composites, a noise covariance estimated from a noise scan, frames of unequal length other than by zero
weights, gridding approximations, off-resonance, trajectories beyond Nyquist.
"""
import numpy as np
import torch

from . import LinearTransform
from .undersampling_fourier import SENSE, _check_gpu, _largest_box
from ... import ops


def check_trajectory(trajectory, H, W, what="NonCartesianSENSE"):
    """-> host float64 (M, 2) tensor, or (T, M, 2): one trajectory per frame; ValueError unless of either shape, finite and
    inside [-H/2, H/2] x [-W/2, W/2] (a framed trajectory is checked frame by frame and the message names the frame)"""
    if not isinstance(trajectory, (torch.Tensor, np.ndarray)):
        raise TypeError(f"{what}: trajectory must be a torch tensor or numpy array, got {type(trajectory).__name__}")
    k = torch.as_tensor(trajectory).detach().cpu()
    if k.is_complex() or not (k.is_floating_point() or k.dtype in (torch.int32, torch.int64)):
        raise TypeError(f"{what}: trajectory must be real, got {k.dtype}")
    if k.dim() == 3 and k.shape[2] == 2 and k.shape[0] >= 1 and k.shape[1] >= 1:
        k = k.to(torch.float64).contiguous()
        for t in range(k.shape[0]):
            _check_positions(k[t], H, W, f"{what}: frame {t} of", "trajectory")
        return k
    if k.dim() != 2 or k.shape[1] != 2 or k.shape[0] < 1:
        raise ValueError(f"{what}: trajectory {tuple(k.shape)} is not (M, 2) = (k_y, k_x) per sample"
                         + (" nor (T, M, 2), one trajectory per frame" if k.dim() > 2 else ""))
    k = k.to(torch.float64).contiguous()
    _check_positions(k, H, W, f"{what}:", "trajectory")
    return k


def _check_positions(k, H, W, who, noun):
    if not bool(torch.isfinite(k).all()):
        raise ValueError(f"{who} the {noun} holds non-finite positions")
    if float(k[:, 0].abs().max()) > H / 2 or float(k[:, 1].abs().max()) > W / 2:
        raise ValueError(f"{who} the {noun} leaves [-N/2, N/2] (k_y within +-{H / 2}, k_x within +-{W / 2} cycles per "
                         "field of view; positions beyond Nyquist are out of scope)")


def check_weights(weights, M, what="NonCartesianSENSE", frames=None):
    """-> host float64 (M,) tensor; ValueError unless (M,), finite and >= 0.  frames = T: -> (T, M), from (T, M) or from (M,)
    repeated for every frame"""
    w = torch.as_tensor(weights).detach().cpu()
    if w.is_complex():
        raise TypeError(f"{what}: weights must be real, got {w.dtype}")
    w = w.to(torch.float64).reshape(-1) if w.dim() <= 1 else w.to(torch.float64)
    if frames is not None:
        if tuple(w.shape) == (M,):
            w = w[None].expand(frames, M)
        elif tuple(w.shape) != (frames, M):
            raise ValueError(f"{what}: weights {tuple(w.shape)} match neither the {M} samples nor ({frames}, {M}), the frames")
    elif tuple(w.shape) != (M,):
        raise ValueError(f"{what}: weights {tuple(w.shape)} do not match the {M} samples")
    if not bool(torch.isfinite(w).all()) or float(w.min()) < 0:
        raise ValueError(f"{what}: weights must be finite and not negative")
    return w.contiguous()


def _in_shape_hw(in_shape, what):
    if len(in_shape) not in (2, 3) or (len(in_shape) == 3 and in_shape[0] != 1):
        raise ValueError(f"{what}: in_shape {tuple(in_shape)} is not (1, H, W)")
    return int(in_shape[-2]), int(in_shape[-1])


def calibration_window(trajectory, H, W, calib_max=12, taper=2.0):
    """-> (ah, aw, weights (M,) float64): the calibration box of a non-Cartesian acquisition and the window on its samples
    (DESIGN.md 4.4n).  Grid cell (p, q) counts as sampled when some sample rounds to it (k_y + H//2, k_x + W//2); that
    occupancy goes through the largest-box rule of ``calibration_region`` (symmetric about DC, half-widths at most
    calib_max, the same tie-breaks).  weights: 1 where max(|k_y| - ah, |k_x| - aw) <= 0.5, a raised cosine down to 0 over
    the next `taper` cycles, 0 beyond.  A framed trajectory (T, M, 2) is pooled over its frames -- the non-Cartesian
    time average -- and the weights are (T * M,), frame by frame.  ValueError, naming the box found, when ah < 2 or
    aw < 2.  Host only."""
    if isinstance(calib_max, bool) or int(calib_max) != calib_max or calib_max < 0:
        raise ValueError(f"calibration_window: calib_max must be an integer >= 0, got {calib_max}")
    taper = float(taper)
    if not (taper >= 0.0 and taper < float("inf")):
        raise ValueError(f"calibration_window: taper must be finite and not negative, got {taper}")
    k = check_trajectory(trajectory, H, W, "calibration_window").reshape(-1, 2).numpy()
    p = np.floor(k[:, 0] + 0.5).astype(np.int64) + H // 2
    q = np.floor(k[:, 1] + 0.5).astype(np.int64) + W // 2
    inside = (p >= 0) & (p < H) & (q >= 0) & (q < W)                        # k = +N/2 rounds to the cell past the grid
    occupied = np.zeros((H, W), dtype=bool)
    occupied[p[inside], q[inside]] = True
    best = _largest_box(occupied, H, W, calib_max)
    if best is None:
        raise ValueError(f"calibration window: no sample of the trajectory rounds to the k-space centre of the {H}x{W} grid; "
                         "coil maps cannot be estimated from this acquisition: pass measured maps (sens_maps=)")
    ah, aw = best
    if ah < 2 or aw < 2:
        raise ValueError(f"calibration window: the samples cover every grid cell of a {2 * ah + 1} x {2 * aw + 1} box about the "
                         f"centre of the {H}x{W} grid and no larger one (half-widths ah = {ah}, aw = {aw}); the coil-map "
                         "estimator needs at least 5 x 5 (ah >= 2 and aw >= 2): acquire more spokes, or pass measured maps "
                         "(sens_maps=)")
    d = np.maximum(np.abs(k[:, 0]) - ah, np.abs(k[:, 1]) - aw) - 0.5
    w = np.zeros(len(k), dtype=np.float64)
    w[d <= 0] = 1.0
    if taper > 0:
        ramp = (d > 0) & (d < taper)
        w[ramp] = 0.5 * (1.0 + np.cos(np.pi * d[ramp] / taper))
    return ah, aw, torch.from_numpy(w)


CALIB_DEFAULTS = dict(lam=1e-2, max_iter=40, tol=1e-4)                      # DESIGN.md 4.4n, the lam / iteration table


class NonCartesianSENSE(LinearTransform):
    def __init__(self, trajectory, in_shape, sens_maps=None, weights=None, normalize=True):
        """trajectory (M, 2) = (k_y, k_x) in cycles per field of view, or (T, M, 2): one per frame (`framed`, `n_frames` = T;
        row b of a batch, B % T == 0, belongs to frame b % T; weights (M,) for every frame or (T, M));
        in_shape (1, H, W); sens_maps (n, H, W) real or
        complex (None: one coil, S = 1), RSS-normalised when `normalize`; weights (M,) >= 0: the likelihood's W in
        |W^1/2 (A x - y)|^2 (None: 1, right for i.i.d. noise -- density compensation belongs to zero_filled alone).
        Every refusal happens here, on the host."""
        if len(in_shape) != 3 or in_shape[0] != 1:
            raise ValueError(f"NonCartesianSENSE: in_shape {tuple(in_shape)} is not (1, H, W)")
        H, W = int(in_shape[-2]), int(in_shape[-1])
        self.in_shape = (1, H, W)
        self.trajectory = check_trajectory(trajectory, H, W)
        self.framed = self.trajectory.dim() == 3
        self.n_frames = self.trajectory.shape[0] if self.framed else 1
        self.n_samples = self.trajectory.shape[-2]                            # per frame
        self.weights = None if weights is None else check_weights(weights, self.n_samples,
                                                                  frames=self.n_frames if self.framed else None)
        if sens_maps is None:
            maps = torch.ones(1, H, W, dtype=torch.float64)
        else:
            maps = SENSE._as_host_maps(sens_maps)
            if maps.dim() == 4:
                raise ValueError(f"NonCartesianSENSE: sens_maps {tuple(maps.shape)}: stacks of map sets (S, n, H, W) are out of "
                                 "scope for the non-Cartesian operator; one set (n, H, W)")
            if maps.dim() != 3 or tuple(maps.shape[-2:]) != (H, W) or maps.shape[0] < 1:
                raise ValueError(f"NonCartesianSENSE: sens_maps {tuple(maps.shape)} do not match (n_coils, {H}, {W})")
            if normalize:
                maps = SENSE.rss_normalize(maps)
        self.sens_maps = maps.contiguous()
        self.num_sens = maps.shape[0]
        if not ops.nc_supported(H, W):
            raise ops._lib.IpdmUnsupported(f"NonCartesianSENSE: no non-Cartesian kernel for {H}x{W}: {ops.NC_SIZE_RULE}")
        self._dev = {}

    # ---- cached device operands ----
    def _cached(self, name, device, make):
        key = (name, str(device))
        if key not in self._dev:
            self._dev[key] = make()
        return self._dev[key]

    def traj_dev(self, device):
        return self._cached("traj", device, lambda: self.trajectory.to(device).contiguous())

    def weights_dev(self, device):
        if self.weights is None:
            return None
        return self._cached("w", device, lambda: self.weights.to(torch.float32).to(device).contiguous())

    def sens_dev(self, device):
        """complex64 (n, H, W) on the device: the kernels' layout (real maps are converted here, on the host)"""
        return self._cached("sens", device, lambda: self.sens_maps.to(torch.complex64).to(device).contiguous())

    def psf_dev(self, device):
        """float32 (2H, 2W), framed (T, 2H, 2W): the real spectrum of the trajectory's Toeplitz kernel (with the likelihood's
        weights)"""
        H, W = self.in_shape[-2:]
        return self._cached("psf", device, lambda: ops.toeplitz_psf(self.traj_dev(device), H, W, self.weights_dev(device)))

    # ---- the operator ----
    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        """X (B, 1, H, W) complex -> y (n, B, 1, M) complex64 (framed: B % T == 0, row b at the samples of frame b % T)"""
        _check_gpu(X, "NonCartesianSENSE")
        self._check_image(X, "NonCartesianSENSE")
        X = X.to(torch.complex64).contiguous()
        y = ops.ndft_forward(X, self.traj_dev(X.device), self.sens_dev(X.device))
        return y.reshape(self.num_sens, X.shape[0], 1, self.n_samples)

    def _check_image(self, X, what):
        if X.dim() != 4 or tuple(X.shape[1:]) != self.in_shape:
            raise ValueError(f"{what}: images {tuple(X.shape)} are not (B,) + {self.in_shape}")
        self._check_rows(X.shape[0], what)

    def _check_rows(self, B, what):
        if self.framed and B % self.n_frames != 0:
            raise ValueError(f"{what}: B = {B} rows are not a multiple of the T = {self.n_frames} frames (row b belongs to "
                             "frame b % T)")

    def _samples(self, S, what):
        _check_gpu(S, what)
        if S.dim() != 4 or S.shape[0] != self.num_sens or S.shape[2] != 1 or S.shape[3] != self.n_samples:
            raise ValueError(f"{what}: samples {tuple(S.shape)} are not ({self.num_sens}, B, 1, {self.n_samples})")
        self._check_rows(S.shape[1], what)
        return S.to(torch.complex64).contiguous().reshape(self.num_sens, S.shape[1], self.n_samples)

    def _adjoint(self, S, weights, what):
        y = self._samples(S, what)
        H, W = self.in_shape[-2:]
        x = ops.ndft_adjoint(y, self.traj_dev(y.device), H, W, self.sens_dev(y.device), weights)
        return x.reshape(y.shape[1], 1, H, W)

    def conj_op(self, S: torch.Tensor) -> torch.Tensor:
        """A^H y: y (n, B, 1, M) -> (B, 1, H, W); the exact adjoint of __call__ (no weights)"""
        return self._adjoint(S, None, "NonCartesianSENSE.conj_op")

    def adjoint_weighted(self, S: torch.Tensor) -> torch.Tensor:
        """A^H W y with the likelihood's weights: the right-hand side of the proximal's normal equations"""
        return self._adjoint(S, None if self.weights is None else self.weights_dev(S.device), "NonCartesianSENSE.adjoint_weighted")

    def zero_filled(self, S: torch.Tensor, density=None) -> torch.Tensor:
        """A^H (w_dc y), the density-compensated adjoint: the image a gridding reconstruction shows.  density (M,) >= 0;
        None: the ramp of ``synthetic.radial_density`` (framed: (M,) or (T, M); the ramp is normalised per frame)"""
        from ...synthetic import radial_density
        H, W = self.in_shape[-2:]
        w = radial_density(self.trajectory, H, W) if density is None else check_weights(
            density, self.n_samples, "zero_filled", frames=self.n_frames if self.framed else None)
        return self._adjoint(S, w.to(torch.float32).to(S.device).contiguous(), "NonCartesianSENSE.zero_filled")

    def projection(self, X: torch.Tensor, S: torch.Tensor, lamda: float) -> torch.Tensor:
        raise NotImplementedError("NonCartesianSENSE: the k-space projection has no meaning off the grid; use L2PenaltyCG")

    # ---- self-calibration: maps and compression from the samples themselves ----
    @staticmethod
    def _calib_operands(y, trajectory, in_shape, what):
        """host-side normalisation -> (y complex tensor (n, M) or (n, T, M), trajectory float64 (M, 2) or (T, M, 2), H, W):
        singleton batch / channel dims of a saved (n, 1, 1, M) measurement are dropped.  TypeError / ValueError."""
        H, W = _in_shape_hw(in_shape, what)
        k = check_trajectory(trajectory, H, W, what)
        if not isinstance(y, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{what}: y must be a torch tensor or numpy array, got {type(y).__name__}")
        y = torch.as_tensor(y).detach()
        if not y.is_complex():
            raise TypeError(f"{what}: y must be complex samples, got {y.dtype}")
        if y.dim() > k.dim() and all(s == 1 for s in y.shape[1:y.dim() - (k.dim() - 1)]):
            y = y.reshape((y.shape[0],) + tuple(y.shape[y.dim() - (k.dim() - 1):]))
        want = tuple(k.shape[:-1])
        if y.dim() != k.dim() or tuple(y.shape[1:]) != want or y.shape[0] < 1:
            raise ValueError(f"{what}: y {tuple(y.shape)}; (n_coils,) + {want} expected for a trajectory {tuple(k.shape)}")
        return y, k, H, W

    @staticmethod
    def _check_calib(n, n_virtual, noise_cov, H, W, ah, aw, method, kw, what):
        """every host-side refusal of the calibration chain, before any GPU work -> (n_virtual, noise_cov, return_eig)"""
        if n_virtual is not None:
            n_virtual = ops._coilcomp_counts(n, n_virtual, what)
            if noise_cov is not None:
                noise_cov = ops.check_noise_cov(noise_cov, n, f"{what}: noise_cov")
        elif noise_cov is not None:
            raise ValueError(f"{what}: noise_cov= goes with n_virtual= (whitening is part of the compression)")
        if ops.kspace_size_class(H, W) == ops.KSPACE_NONE or not ops.nc_supported(H, W):
            raise ops._lib.IpdmUnsupported(f"{what}: no calibration kernels for {H}x{W}: {ops.KSPACE_SIZE_RULE}, and "
                                           f"{ops.NC_SIZE_RULE}")
        n_est = n if n_virtual is None else n_virtual
        return_eig = SENSE._check_maps_method(method, n_est, H, W, ah, aw, kw, what)
        if method == "walsh" and not ops.csm_supported(n_est, kw.get("radius", 2), H, W):
            raise ops._lib.IpdmUnsupported(f"{what}: the map estimator serves 1..32 coils and radius 1..4, got {n_est} coils, "
                                           f"radius {kw.get('radius', 2)}: compress the measurement first (n_virtual=)")
        return n_virtual, noise_cov, return_eig

    @staticmethod
    def _calib_dev(y, k, w):
        """-> (samples (n, 1, Mt) complex64, pooled trajectory (Mt, 2) float64, window (Mt,) float32) on the GPU"""
        dev = y.device if y.is_cuda else "cuda"
        yd = y.to(torch.complex64).to(dev).reshape(y.shape[0], 1, -1).contiguous()
        return yd, k.reshape(-1, 2).to(dev).contiguous(), w.to(torch.float32).to(dev).contiguous()

    @staticmethod
    def _maps_dev(yd, kd, wd, H, W, ah, aw, method, kw, solver, what):
        """calibration k-space and maps of the pooled samples yd (n, 1, Mt) -> (maps (n, H, W) on the GPU, eigval (H, W) or
        None, rss_max, calibration k-space (n, H, W), CG iterations (n,))"""
        ks, iters = ops.nc_calib_kspace(yd, kd, H, W, wd, return_iters=True, **solver)
        if method == "espirit":                                             # rss_max: the peak of the Walsh calibration image
            _, _, rss_max = ops.estimate_sens_maps(ks, ah, aw, return_rss=True)
            maps, eigval = SENSE._espirit_maps(ks, ah, aw, what, **kw)
            eigval = eigval[0]
        else:
            maps, _, rss_max = ops.estimate_sens_maps(ks, ah, aw, return_rss=True, **kw)
            eigval = None
        return maps[:, 0], eigval, float(rss_max[0]), ks[:, 0], iters[:, 0]

    @staticmethod
    def _solver_kw(lam, max_iter, tol):
        d = dict(CALIB_DEFAULTS)
        d.update({k: v for k, v in (("lam", lam), ("max_iter", max_iter), ("tol", tol)) if v is not None})
        return d

    @staticmethod
    def estimate_sens_maps(y, trajectory, in_shape, calib_max=12, method="walsh", lam=None, max_iter=None, tol=None, **kw):
        """coil maps from non-Cartesian samples themselves: y (n, M) at trajectory (M, 2), or (n, T, M) at (T, M, 2) -- the
        frames are pooled.  The samples inside ``calibration_window(trajectory, H, W, calib_max)`` are gridded by a
        regularised per-coil inverse (``ops.nc_calib_kspace``: lam, max_iter, tol; defaults CALIB_DEFAULTS) and the
        Cartesian estimators run on that k-space with the window's box: ``ops.estimate_sens_maps`` (method="walsh"; kw:
        radius, power_iters, thresh) or ``ops.espirit_maps`` (method="espirit"; kw: ksize, sv_thresh, crop, power_iters;
        return_eig=True: -> (maps, eigval (H, W) float32 on the host)).  -> host complex128 (n, H, W), unit RSS inside
        the support and zero outside: ready for ``sens_maps=``.  Every argument is checked on the host first."""
        what = "NonCartesianSENSE.estimate_sens_maps"
        y, k, H, W = NonCartesianSENSE._calib_operands(y, trajectory, in_shape, what)
        ah, aw, w = calibration_window(k, H, W, calib_max)
        _, _, return_eig = NonCartesianSENSE._check_calib(y.shape[0], None, None, H, W, ah, aw, method, kw, what)
        yd, kd, wd = NonCartesianSENSE._calib_dev(y, k, w)
        maps, eigval, _, _, _ = NonCartesianSENSE._maps_dev(yd, kd, wd, H, W, ah, aw, method, kw,
                                                            NonCartesianSENSE._solver_kw(lam, max_iter, tol), what)
        maps = maps.cpu().to(torch.complex128)
        return (maps, eigval.cpu()) if return_eig else maps

    @staticmethod
    def compress_measurement(y, trajectory, in_shape, n_virtual, noise_cov=None, calib_max=12):
        """whitening and coil compression of non-Cartesian samples: y (n, M) or (n, T, M) as for estimate_sens_maps (up to 64
        coils) to n_virtual 1..min(n, 32) virtual coils.  The Gram matrix is ``ops.nc_coil_gram`` of the pooled samples
        under the calibration window's weights, the matrix ``ops.coilcomp_matrix`` (noise_cov: the (n, n) coil noise
        covariance, optional), applied to the samples of every frame by ``ops.coil_apply``.  -> (y' of y's shape with
        n_virtual coils, complex64 on the GPU; A (n_virtual, n) complex64 on the host)."""
        what = "NonCartesianSENSE.compress_measurement"
        y, k, H, W = NonCartesianSENSE._calib_operands(y, trajectory, in_shape, what)
        n_virtual = ops._coilcomp_counts(y.shape[0], n_virtual, what)
        if noise_cov is not None:
            noise_cov = ops.check_noise_cov(noise_cov, y.shape[0], f"{what}: noise_cov")
        _, _, w = calibration_window(k, H, W, calib_max)
        yd, _, wd = NonCartesianSENSE._calib_dev(y, k, w)
        out, A = NonCartesianSENSE._compress_dev(yd, wd, n_virtual, noise_cov, what)
        return out.reshape((n_virtual,) + tuple(y.shape[1:])), A.cpu()

    @staticmethod
    def _compress_dev(yd, wd, n_virtual, noise_cov, what):
        A, _, status = ops.coilcomp_matrix(ops.nc_coil_gram(yd, wd), n_virtual, noise_cov, return_eig=True)
        if int(status[0]) != 0:
            raise RuntimeError(f"{what}: the noise covariance has a non-positive Cholesky pivot in fp32")
        return ops.coil_apply(yd, A[0].contiguous()), A[0]

    @classmethod
    def from_measurement(cls, y, trajectory, in_shape, weights=None, n_virtual=None, noise_cov=None, method="walsh",
                         calib_max=12, lam=None, max_iter=None, tol=None, **kw):
        """the operator of a non-Cartesian acquisition, calibrated from its own samples: y (n, M) at trajectory (M, 2), or cine
        data (n, T, M) at (T, M, 2) -- the operator is then framed and the maps come from the pool of the frames.  With
        n_virtual the samples are whitened (noise_cov) and compressed first (compress_measurement; up to 64 physical
        coils) and the maps are those of the virtual coils; weights: the likelihood's, handed to the operator.  method, kw,
        lam, max_iter, tol: estimate_sens_maps'.  -> Namespace(op, measurement (n', M) / (n', T, M) complex64 on the GPU,
        sens_maps (n', H, W) complex128 on the host, coil_matrix (n', n) complex64 on the host or None, region (ah, aw),
        rss_max (the peak of the calibration image), calib_kspace (n', H, W) complex64 on the GPU, cg_iters (n',) int32 on
        the host, eigval (the ESPIRiT eigenvalue map on the host, None for Walsh)).  Every argument is checked on the host
        before any GPU work."""
        from argparse import Namespace
        what = "NonCartesianSENSE.from_measurement"
        y, k, H, W = cls._calib_operands(y, trajectory, in_shape, what)
        if weights is not None:
            check_weights(weights, k.shape[-2], what, frames=k.shape[0] if k.dim() == 3 else None)
        ah, aw, w = calibration_window(k, H, W, calib_max)
        n_virtual, noise_cov, _ = cls._check_calib(y.shape[0], n_virtual, noise_cov, H, W, ah, aw, method, kw, what)
        yd, kd, wd = cls._calib_dev(y, k, w)
        A = None
        if n_virtual is not None:
            yd, A = cls._compress_dev(yd, wd, n_virtual, noise_cov, what)
        maps, eigval, rss_max, ks, iters = cls._maps_dev(yd, kd, wd, H, W, ah, aw, method, kw,
                                                         cls._solver_kw(lam, max_iter, tol), what)
        maps = maps.cpu().to(torch.complex128)
        op = cls(k, (1, H, W), sens_maps=maps, weights=weights, normalize=False)
        return Namespace(op=op, measurement=yd.reshape((yd.shape[0],) + tuple(y.shape[1:])), sens_maps=op.sens_maps,
                         coil_matrix=None if A is None else A.cpu(), region=(ah, aw), rss_max=rss_max, calib_kspace=ks,
                         cg_iters=iters.cpu(), eigval=None if eigval is None else eigval.cpu())


def refuse_noncartesian(lin_tfm, who, framed_ok=False):
    """the optimisers built on the Cartesian kernel chains (mask tables, per-frame proximals) name the operator they refuse;
    framed_ok: a framed operator (one trajectory per frame) passes -- the 2D+time sampler"""
    if isinstance(lin_tfm, NonCartesianSENSE) and not (framed_ok and lin_tfm.framed):
        raise NotImplementedError(f"{who}: NonCartesianSENSE is not served here; the non-Cartesian operator runs in "
                                  "ALDInvSegProximalRealImag with L2PenaltyCG")
