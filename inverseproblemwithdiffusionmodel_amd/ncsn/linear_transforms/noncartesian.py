"""Multi-coil SENSE for samples at arbitrary k-space positions (radial, spiral, ...): DESIGN.md 4.4l.

``NonCartesianSENSE`` is the measurement model  y[c, b, m] = (HW)^-1/2 sum_{r,col} S_c x[b] exp(-2 pi i (k_y,m (r - H/2)/H +
k_x,m (col - W/2)/W))  in the package's centred orthonormal convention: a trajectory on integer grid points reproduces
``i2k_complex`` at index (k_y + H/2, k_x + W/2).  The forward and adjoint transforms are exact direct sums in HIP kernels
(``ops.ndft_forward`` / ``ops.ndft_adjoint``) and run once per reconstruction; the sampler's data-consistency step,
``L2PenaltyCG``, applies A^H W A as a Toeplitz operator through the FFT passes (``ops.nc_sense_cgprox``).

Radial cine: a trajectory (T, M, 2) holds one trajectory per frame -- a *framed* operator.  Row b of
every image batch belongs to frame b % T, the rule of the Cartesian coil-map sets, so the (posterior sample, frame) batch
of ``ALD2DTime``, flattened frame-fastest, is served as it lies in memory.

The reference has no non-Cartesian code.  Out of scope: coil-map estimation or compression from non-Cartesian data, map
sets, view sharing, frames of unequal length other than by zero weights, gridding approximations, off-resonance,
trajectories beyond Nyquist.
"""
import numpy as np
import torch

from . import LinearTransform
from .undersampling_fourier import SENSE, _check_gpu
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


def refuse_noncartesian(lin_tfm, who, framed_ok=False):
    """the optimisers built on the Cartesian kernel chains (mask tables, per-frame proximals) name the operator they refuse;
    framed_ok: a framed operator (one trajectory per frame) passes -- the 2D+time sampler"""
    if isinstance(lin_tfm, NonCartesianSENSE) and not (framed_ok and lin_tfm.framed):
        raise NotImplementedError(f"{who}: NonCartesianSENSE is not served here; the non-Cartesian operator runs in "
                                  "ALDInvSegProximalRealImag with L2PenaltyCG")
