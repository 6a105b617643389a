"""Undersampled-Fourier and multi-coil SENSE operators (mirror of the reference's
``ncsn/linear_transforms/undersampling_fourier.py``: UndersamplingFourier :10-36, RandomUndersamplingFourier :39-97,
SENSE :100-176).

Differences the reference forces on a drop-in, all explicit:
* the checked-in ``_generate_mask`` ignores ``R`` and is hard-wired to T=24 / "R=16" parameters
  (:63-75).  Here ``mask_T`` selects the variant: ``mask_T=24`` reproduces the live code bit for bit,
  ``mask_T=1`` (default) is the single-frame variant the reference keeps commented out (:72-73) with the
  (sw, sm, sa) set looked up from ``R`` (``MASK_PARAMS``); ``mask_params=`` overrides the set.
* ``mask_mode="uniform"`` is the LEGACY mask the reference keeps commented out (:50-61): ``rand(1, 1, W) <= 1 / R`` from torch's
  generator plus a fully sampled centre window of ``int(W * center_lines_frac)`` lines -- the only mode in which ``R`` and
  ``center_lines_frac`` act as the constructor's signature promises, for any R (bit-exact against tests/golden/g30).
* coil maps are kept float64 (real) or complex128 (measured, complex maps) on the host (``.sens_maps``, as the reference)
  and float32 / complex64 on the device (``sens_dev``); the kernels multiply by S_c forward and conj(S_c) in the adjoint
  and the proximal tail, as the reference's ``conj_op`` (:157).  ``sens_maps`` is a property: the reference's idiom
  ``op.sens_maps = maps`` validates the shape and drops the cached device copies, before or after first use.
* ``sens_type="custom"`` takes ``sens_maps=`` (tensor or ndarray, real or complex, (num_sens, H, W)); ``normalize=True``
  divides by the root-sum-of-squares where it is non-zero (measured maps are masked to the body: zero-support pixels stay
  zero), ``normalize=False`` takes the maps as given.  ``"exp"`` is the reference's synthetic real map, unchanged.
* ``mask_mode="custom"`` takes ``mask=``: the sampling pattern of an actual acquisition, a line mask ((W,), (1, 1, W),
  (T, 1, 1, W)) or a 2-D mask ((H, W), (1, 1, H, W), (T, 1, H, W)) -- whatever the reference's ``mask * i2k_complex(X)``
  broadcasts against a (B, 1, H, W) stack.  ``mask`` is a property like ``SENSE.sens_maps``: the reference's idiom
  ``op.random_under_fourier.mask = m`` validates the shape and drops the cached device copy, before or after first use.
"""
import warnings

import numpy as np
import torch

from . import LinearTransform, generate_mask, i2k_complex, k2i_complex, MASK_PARAMS
from .masking import SkipLines
from ... import ops


def _check_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: expected a GPU tensor (no CPU fallback in this build)")


def _largest_box(full, H, W, calib_max):
    """-> (ah, aw) of the largest box symmetric about (H//2, W//2) inside which the host bool array `full` (H, W) is True
    everywhere, each half-width at most min(N//2, N-1-N//2, calib_max); ties go to the smaller |ah - aw|, then to the
    larger aw.  None when the centre itself is False."""
    # prefix sums: box (ah, aw) is fully sampled iff its count equals its area
    cs = np.zeros((H + 1, W + 1), dtype=np.int64)
    cs[1:, 1:] = np.cumsum(np.cumsum(full, axis=0), axis=1)
    ch, cw = H // 2, W // 2
    best = None
    for ah in range(min(ch, H - 1 - ch, int(calib_max)) + 1):
        for aw in range(min(cw, W - 1 - cw, int(calib_max)) + 1):
            r0, r1, c0, c1 = ch - ah, ch + ah + 1, cw - aw, cw + aw + 1
            area = (r1 - r0) * (c1 - c0)
            if cs[r1, c1] - cs[r0, c1] - cs[r1, c0] + cs[r0, c0] != area:
                continue
            key = (area, -abs(ah - aw), aw)
            if best is None or key > best[0]:
                best = (key, ah, aw)
    return None if best is None else best[1:]


def _sampled_planes(mask, H, W, union):
    """host bool (H, W): where every plane (union: at least one plane) of the mask sampled; a line mask covers every row"""
    m = ops._mask_u8(mask, H, W, "cpu").bool()
    full = m.any(dim=0) if union else m.all(dim=0)
    if full.dim() == 1:                                         # a line mask [W]: every row is sampled
        full = full.reshape(1, W).expand(H, W)
    return full.numpy(), m.shape[0]


def calibration_region(mask, H, W, calib_max=12, composite=False):
    """-> (ah, aw), the half-widths of the calibration box [H//2-ah, H//2+ah] x [W//2-aw, W//2+aw] the coil-map estimator
    works from: symmetric about DC, fully sampled in every frame of `mask` (any shape ``ops._mask_u8`` takes; a line mask
    is fully sampled along H), each half-width at most min(N//2, N-1-N//2, calib_max).  Of the fully sampled candidates
    the largest area wins; ties go to the smaller |ah - aw|, then to the larger aw.  ValueError, naming the sampled centre
    it found, when ah < 2 or aw < 2 (the generated R = 40 line mask keeps the two adjacent centre lines W//2 - 1 and
    W//2, so the box symmetric about W//2 has aw = 0 and the mask is refused this way).  composite=True: the box of the
    time-averaged composite of a cine acquisition (``ops.kspace_time_average``), sampled at every position in AT LEAST ONE
    frame -- interleaved per-frame patterns share little more than the centre line, their union is what such acquisitions
    calibrate from.  Host only."""
    if isinstance(calib_max, bool) or int(calib_max) != calib_max or calib_max < 0:
        raise ValueError(f"calibration_region: calib_max must be an integer >= 0, got {calib_max}")
    full, planes = _sampled_planes(mask, H, W, union=bool(composite))
    best = _largest_box(full, H, W, calib_max)
    hint = ""
    if not composite and planes > 1 and (best is None or min(best) < 2):
        both = _largest_box(_sampled_planes(mask, H, W, union=True)[0], H, W, calib_max)
        if both is not None and min(both) >= 2:
            hint = (f"; the union of its {planes} frames is fully sampled on {2 * both[0] + 1} x {2 * both[1] + 1}: for a cine "
                    "acquisition calibrate from the time-averaged composite (composite=True)")
    if best is None:
        raise ValueError(f"calibration region: the k-space centre ({H // 2}, {W // 2}) of the {H}x{W} mask is not sampled in "
                         f"{'any' if composite else 'every'} frame; coil maps cannot be estimated from this acquisition{hint}")
    ah, aw = best
    if ah < 2 or aw < 2:
        raise ValueError(f"calibration region: the fully sampled centre of the {H}x{W} mask is {2 * ah + 1} x {2 * aw + 1} "
                         f"samples (half-widths ah = {ah}, aw = {aw}); the coil-map estimator needs at least 5 x 5 "
                         f"(ah >= 2 and aw >= 2): acquire more centre lines, or pass measured maps (sens_maps=){hint}")
    return ah, aw


def readout_fully_sampled(mask, H, W):
    """whether every sampled column of `mask` (any shape ``ops._mask_u8`` takes) is sampled at all H rows in every frame: a
    line mask always is, a 2-D mask only when each of its columns is full or empty.  Host only."""
    m = ops._mask_u8(mask, H, W, "cpu").bool()
    if m.dim() == 2:                                            # line mask [T][W]
        return True
    return bool((m.all(dim=-2) == m.any(dim=-2)).all())


def geometric_compression_check(mask, n, n_virtual, H, W, calib_max=12, window=2, what="compress_measurement"):
    """host checks of a geometric coil compression along the readout axis H -> (n_virtual, aw, window), aw the column
    half-width of ``calibration_region(mask, H, W, calib_max)``.  ValueError: a mask whose readout is not fully sampled, a
    window outside 0..8 or with fewer samples than virtual coils; IpdmUnsupported: an H x W without a k-space kernel, coil
    counts outside ``ops.coilcomp_supported``.  No GPU work."""
    n_virtual = ops._coilcomp_counts(n, n_virtual, what)
    window = ops.gcc_window(window, what)
    if not readout_fully_sampled(mask, H, W):
        raise ValueError(f"{what}: geometric coil compression needs a fully sampled readout: some sampled column of the "
                         f"{H}x{W} mask is not sampled at all {H} rows (a 2-D (ky, kz) pattern); use the PCA compression")
    if ops.kspace_size_class(H, W) == ops.KSPACE_NONE:
        raise ops._lib.IpdmUnsupported(f"{what}: no k-space kernel for {H}x{W}; {ops.KSPACE_SIZE_RULE}")
    _, aw = calibration_region(mask, H, W, calib_max)
    n_virtual, window = ops.gcc_check(n, n_virtual, H, W, aw, window, what)
    return n_virtual, aw, window


def composite_mask(mask, H, W):
    """-> host bool tensor, (W,) for a line mask and (H, W) for a 2-D mask: the union over the frames of `mask` (any shape
    ``ops._mask_u8`` takes), where the time-averaged composite of a cine acquisition holds data"""
    return ops._mask_u8(mask, H, W, "cpu").bool().any(dim=0)


class UndersamplingFourier(LinearTransform):
    """every ``num_skip_lines``-th k-space ROW of the centred FFT (reference :10-36): S = P M F x, adjoint F^-1 M^T P^T"""

    def __init__(self, num_skip_lines, in_shape):
        self.skip_lines = SkipLines(num_skip_lines, in_shape)

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        _check_gpu(X, "UndersamplingFourier")
        return self.skip_lines(i2k_complex(X.to(torch.complex64))).contiguous()

    def conj_op(self, S: torch.Tensor) -> torch.Tensor:
        _check_gpu(S, "UndersamplingFourier.conj_op")
        return k2i_complex(self.skip_lines.conj_op(S.to(torch.complex64)))

    def projection(self, X: torch.Tensor, S: torch.Tensor, lamda: float) -> torch.Tensor:
        warnings.warn("Not used!")
        return X


class RandomUndersamplingFourier(LinearTransform):
    def __init__(self, R, center_lines_frac, in_shape, seed=None, mask_T=1, mask_params=None, mask_mode="variable",
                 mask=None):
        """in_shape: (C, H, W); mask_mode "variable" (generate_mask, the live reference), "uniform" (the legacy formula) or
        "custom" (mask=: a line or 2-D sampling mask, see the module docstring)"""
        if mask_mode not in ("variable", "uniform", "custom"):
            raise ValueError(f"mask_mode {mask_mode!r}: 'variable', 'uniform' or 'custom'")
        if mask_mode == "custom" and mask is None:
            raise ValueError("mask_mode='custom' needs mask= (a line mask (..., W) or a 2-D mask (..., H, W))")
        if mask_mode != "custom" and mask is not None:
            raise ValueError("mask= goes with mask_mode='custom'")
        self.R = R
        self.center_lines_frac = center_lines_frac
        self.in_shape = in_shape
        self.seed = seed
        self.mask_T = mask_T
        self.mask_params = mask_params
        self.mask_mode = mask_mode
        self.mask = mask if mask_mode == "custom" else self._generate_mask()

    @property
    def mask(self):
        return self._mask

    @mask.setter
    def mask(self, mask):
        """tensor / ndarray of bool, integer or real floating dtype (non-zero = sampled), kept as given on the host"""
        if not isinstance(mask, (torch.Tensor, np.ndarray)):
            raise TypeError(f"mask: a torch tensor or numpy array, got {type(mask).__name__}")
        t = torch.as_tensor(mask).detach().cpu()
        ops._mask_u8(t, self.in_shape[-2], self.in_shape[-1], "cpu")          # shape and dtype checks only
        self._mask = t
        self._dev = {}                                                        # the device copy belongs to the old mask

    def _generate_uniform_mask(self):
        """reference :50-61 (commented out there): float (1, 1, W), torch's default generator seeded with `seed`"""
        torch.random.manual_seed(self.seed if self.seed is not None else torch.seed())
        W = self.in_shape[-1]
        mask = (torch.rand(1, 1, W) <= 1 / self.R).float()
        win_size = int(W * self.center_lines_frac)
        half_win_size = W // 2
        start_idx = half_win_size - win_size // 2
        end_idx = start_idx + win_size
        mask[..., start_idx:end_idx] = 1.
        return mask

    def _generate_mask(self):
        if self.mask_mode == "uniform":
            return self._generate_uniform_mask()
        torch.random.manual_seed(self.seed if self.seed is not None else torch.seed())
        W = self.in_shape[-1]
        if self.mask_params is not None:
            params = self.mask_params
        elif self.mask_T == 24:
            params = MASK_PARAMS[16]                      # the live reference ignores R
        elif self.R in MASK_PARAMS:
            params = MASK_PARAMS[self.R]
        else:
            raise ValueError(f"no variable-density mask parameters for R={self.R}; pass mask_params=dict(sw, sm, sa) or "
                             "mask_mode='uniform' (the legacy rand <= 1/R mask, any R)")
        mask = generate_mask(self.mask_T, W, seed=self.seed, **params)
        return mask.unsqueeze(1)                          # (1, 1, W) or (T, 1, 1, W)

    def mask_u8(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = ops._mask_u8(self._mask, self.in_shape[-2], self.in_shape[-1], device)
        return self._dev[key]

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        """S = mask * i2k_complex(X): one kernel (FFT in LDS, mask applied on the way out)"""
        _check_gpu(X, "RandomUndersamplingFourier")
        X = X.to(torch.complex64)
        return ops.sense_forward(X, None, self.mask_u8(X.device))[0]

    def conj_op(self, S: torch.Tensor) -> torch.Tensor:
        return k2i_complex(S)

    def projection(self, X: torch.Tensor, S: torch.Tensor, lamda: float) -> torch.Tensor:
        """k-space mix F^-1[lamda S + (1 - lamda) M F X + (1 - M) F X] (:89-97).  The reference's `(1 - mask)` raises for
        its own bool masks; the documented formula is applied, as one kernel."""
        _check_gpu(X, "RandomUndersamplingFourier.projection")
        zr = torch.view_as_real(X.to(torch.complex64))
        o_re, o_im = ops.singlecoil_prox(zr[..., 0].contiguous(), zr[..., 1].contiguous(),
                                         S.to(torch.complex64).contiguous(), self.mask_u8(X.device), float(lamda),
                                         ops.SC_PROJECTION)
        return torch.complex(o_re, o_im)


class SENSE(LinearTransform):
    def __init__(self, sens_type, num_sens, R, center_lines_frac, in_shape, seed, mask_T=1, mask_params=None,
                 mask_mode="variable", sens_maps=None, normalize=True, mask=None):
        assert sens_type in ["exp", "custom"]
        self.random_under_fourier = RandomUndersamplingFourier(R, center_lines_frac, in_shape, seed, mask_T,
                                                               mask_params, mask_mode, mask)
        self.num_sens = num_sens
        self._dev = {}
        if sens_type == "custom":
            if sens_maps is None:
                raise ValueError("SENSE('custom', ...) needs sens_maps= (num_sens, H, W) or, one set per slice, "
                                 "(S, num_sens, H, W), real or complex")
            maps = self._as_host_maps(sens_maps)
            self.sens_maps = self.rss_normalize(maps) if normalize else maps
            return
        if sens_maps is not None:
            raise ValueError("sens_maps= goes with sens_type='custom'")
        maps = []
        for i in range(num_sens):
            s = self.random_under_fourier.seed
            maps.append(self._generate_sens_map(sens_type, None if s is None else s + i))
        maps = torch.stack(maps, dim=0)                                     # (num_sens, H, W) float64
        self.sens_maps = maps / torch.sqrt((torch.abs(maps) ** 2).sum(dim=0))
        energy = (torch.abs(self.sens_maps) ** 2).sum(dim=0)
        assert torch.allclose(energy, torch.ones_like(energy))

    @staticmethod
    def rss_normalize(maps):
        """maps / root-sum-of-squares over the coils where it is non-zero; zero-support pixels stay zero.  (S, n, H, W):
        each set over its own coil axis"""
        maps = SENSE._as_host_maps(maps)
        rss = torch.sqrt((torch.abs(maps) ** 2).sum(dim=-3, keepdim=True)) if maps.dim() > 3 else \
            torch.sqrt((torch.abs(maps) ** 2).sum(dim=0))
        return maps / torch.where(rss > 0, rss, torch.ones_like(rss))

    @staticmethod
    def estimate_sens_maps(y, mask, calib_max=12, method="walsh", **kw):
        """coil maps from the measurement itself: y (n, H, W) multi-coil k-space (tensor or ndarray; singleton batch /
        channel dims as in a saved (n, 1, 1, H, W) measurement are dropped), centred with orthonormal scale as this
        operator produces it, mask its sampling mask.  The calibration box is ``calibration_region(mask, H, W, calib_max)``,
        the estimator ``ops.estimate_sens_maps`` on the current GPU (method="walsh"; kw: radius, power_iters, thresh) or
        ``ops.espirit_maps`` (method="espirit"; kw: ksize, sv_thresh, crop, power_iters; up to 16 coils and
        n ksize^2 <= 432 -- compress more coils first; return_eig=True: -> (maps, eigval (H, W) float32 on the host)).
        -> host complex128 (n, H, W), unit RSS inside the support and zero outside: ready for ``sens_maps=``.
        y (S, n, H, W), a stack of slices: one batched estimator call, each slice from its own calibration data
        -> (S, n, H, W)."""
        y, stack = SENSE._measurement_operand(y, "estimate_sens_maps")
        n, H, W = y.shape[-3:]
        ah, aw = calibration_region(mask, H, W, calib_max)                  # host only: fails before any GPU work
        return_eig = SENSE._check_maps_method(method, n, H, W, ah, aw, kw, "estimate_sens_maps")
        yd = y.to(torch.complex64).to(y.device if y.is_cuda else "cuda")
        yd = yd.transpose(0, 1).contiguous() if stack else yd.contiguous()  # (n, S, H, W), one per image
        if method == "espirit":
            maps, eigval = SENSE._espirit_maps(yd, ah, aw, "estimate_sens_maps", **kw)
        else:
            maps = ops.estimate_sens_maps(yd, ah, aw, **kw)
        maps = maps.transpose(0, 1).cpu().to(torch.complex128).contiguous() if stack else maps.cpu().to(torch.complex128)
        if return_eig:
            return maps, (eigval if stack else eigval[0]).cpu()
        return maps

    ESPIRIT_KW = ("ksize", "sv_thresh", "crop", "power_iters")

    @staticmethod
    def _check_maps_method(method, n, H, W, ah, aw, kw, what):
        """host-side check of the estimator choice, before any GPU work; pops and returns kw's return_eig (espirit only)"""
        if method == "walsh":
            return False
        if method != "espirit":
            raise ValueError(f"{what}: method {method!r}; 'walsh' or 'espirit'")
        return_eig = bool(kw.pop("return_eig", False))
        unknown = sorted(set(kw) - set(SENSE.ESPIRIT_KW))
        if unknown:
            raise TypeError(f"{what}: method='espirit' takes {', '.join(SENSE.ESPIRIT_KW)}; got {', '.join(unknown)}")
        ops.espirit_check(n, kw.get("ksize", 6), ah, aw, H, W, what)
        return return_eig

    @staticmethod
    def _espirit_maps(yd, ah, aw, what, **kw):
        """ops.espirit_maps of yd (n, H, W) / (n, B, H, W) on the GPU -> (maps, eigval (B, H, W)); RuntimeError naming the
        images whose decomposition failed"""
        maps, eigval, _, status = ops.espirit_maps(yd, ah, aw, return_eig=True, **kw)
        bad = torch.nonzero(status.cpu()).flatten().tolist()
        if bad:
            raise RuntimeError(f"{what}: the ESPIRiT eigendecomposition did not converge, or met a non-finite value, for "
                               f"image(s) {bad} of the batch")
        return maps, eigval

    @staticmethod
    def _measurement_operand(y, what):
        """-> (y, stack): y a complex tensor (n, H, W), stack False (singleton batch / channel dims of a saved
        (n, 1, 1, H, W) measurement dropped), or (S, n, H, W), stack True.  TypeError / ValueError."""
        if not isinstance(y, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{what}: y must be a torch tensor or numpy array, got {type(y).__name__}")
        y = torch.as_tensor(y).detach()
        if not y.is_complex():
            raise TypeError(f"{what}: y must be complex k-space, got {y.dtype}")
        if y.dim() > 3 and all(s == 1 for s in y.shape[1:-2]):
            y = y.reshape(y.shape[0], y.shape[-2], y.shape[-1])
        if y.dim() not in (3, 4) or min(y.shape) < 1:
            raise ValueError(f"{what}: y {tuple(y.shape)}; (n_coils, H, W) or, a stack of slices, (S, n_coils, H, W) expected")
        return y, y.dim() == 4

    @staticmethod
    def compress_measurement(y, mask, n_virtual, noise_cov=None, calib_max=12, geometric=False, window=2):
        """whitening and coil compression of a measurement: y (n, H, W) multi-coil k-space as for estimate_sens_maps (up to
        64 coils), n_virtual 1..min(n, 32) virtual coils by PCA of the calibration box ``calibration_region(mask, H, W,
        calib_max)``, noise_cov the (n, n) Hermitian positive definite coil noise covariance of the prescan (None: white
        noise assumed).  ``ops.coil_compress`` on the current GPU.  -> (y' (n_virtual, H, W) complex64 on the GPU,
        A (n_virtual, n) complex64 on the host).  y (S, n, H, W), a stack of slices: one batched call, one matrix per slice
        -> (y' (S, n_virtual, H, W), A (S, n_virtual, n)).  Every argument is checked on the host before any GPU work.
        geometric=True: geometric coil compression along the readout axis H, which the mask must sample fully
        (``ops.coil_compress_geometric``): one matrix per readout position from the calibration columns (aw of the
        calibration box) and `window` rows on either side (0..8) -> A (H, n_virtual, n), or (S, H, n_virtual, n)."""
        y, stack = SENSE._measurement_operand(y, "compress_measurement")
        n, H, W = y.shape[-3:]
        if geometric:
            n_virtual, aw, window = geometric_compression_check(mask, n, n_virtual, H, W, calib_max, window)
            if noise_cov is not None:
                noise_cov = ops.check_noise_cov(noise_cov, n, "compress_measurement: noise_cov")
            yd = y.to(torch.complex64).to(y.device if y.is_cuda else "cuda")
            yd = yd.transpose(0, 1).contiguous() if stack else yd.contiguous()
            out, A, _, status = ops.coil_compress_geometric(yd, aw, n_virtual, window, noise_cov, return_matrix=True)
            for b, st in enumerate(status.cpu().tolist()):
                if st != 0:
                    raise RuntimeError(f"compress_measurement: image {b}: " + (
                        "the noise covariance has a non-positive Cholesky pivot in fp32" if st < 0 else
                        f"{st} readout position(s) could not be aligned with their neighbour (no signal in the calibration "
                        "columns there?)"))
            return (out.transpose(0, 1).contiguous(), A.cpu()) if stack else (out, A[0].cpu())
        n_virtual = ops._coilcomp_counts(n, n_virtual, "compress_measurement")
        if noise_cov is not None:
            noise_cov = ops.check_noise_cov(noise_cov, n, "compress_measurement: noise_cov")
        ah, aw = calibration_region(mask, H, W, calib_max)
        yd = y.to(torch.complex64).to(y.device if y.is_cuda else "cuda")
        if stack:
            out, A, _, _ = ops.coil_compress(yd.transpose(0, 1).contiguous(), ah, aw, n_virtual, noise_cov, return_matrix=True)
            return out.transpose(0, 1).contiguous(), A.cpu()
        out, A, _, _ = ops.coil_compress(yd.contiguous(), ah, aw, n_virtual, noise_cov, return_matrix=True)
        return out, A[0].cpu()

    @classmethod
    def from_measurement(cls, y, mask, R=1, seed=None, calib_max=12, n_virtual=None, noise_cov=None, method="walsh",
                         geometric=False, window=2, **kw):
        """the ``"custom"`` operator of an acquisition: maps estimated from its own measurement y (n, H, W) and sampling
        mask (estimate_sens_maps; method and kw go to the estimator).  R is informational, as for every custom mask.  n_virtual:
        the measurement is whitened (noise_cov) and compressed first (compress_measurement) and the maps are those of the
        virtual coils -- the operator then has n_virtual coils and serves the compressed measurement.  y (S, n, H, W), a
        stack of slices: the multi-set operator, maps (and compression) per slice (n_map_sets == S).  geometric, window:
        compress_measurement's (they go with n_virtual=)."""
        if geometric and n_virtual is None:
            raise ValueError("from_measurement: geometric= goes with n_virtual=")
        if method != "walsh":                                               # host only: fails before the compression runs
            y0, _ = cls._measurement_operand(y, "from_measurement")
            n0, H0, W0 = y0.shape[-3:]
            cls._check_maps_method(method, n0 if n_virtual is None else int(n_virtual), H0, W0,
                                   *calibration_region(mask, H0, W0, calib_max), dict(kw), "from_measurement")
        if n_virtual is not None:
            y, _ = cls.compress_measurement(y, mask, n_virtual, noise_cov=noise_cov, calib_max=calib_max, geometric=geometric,
                                            window=window)
        elif noise_cov is not None:
            raise ValueError("from_measurement: noise_cov= goes with n_virtual= (whitening is part of the compression)")
        kw.pop("return_eig", None)
        maps = cls.estimate_sens_maps(y, mask, calib_max=calib_max, method=method, **kw)
        n, H, W = maps.shape[-3:]
        return cls("custom", n, R, 0.04, (1, H, W), seed, mask_mode="custom", mask=mask, sens_maps=maps, normalize=False)

    @staticmethod
    def _cine_operands(y, mask, what):
        """host-side normalisation of a cine measurement and its mask -> (y (n, T, H, W) complex tensor, mask as the
        operator takes it, planes): singleton batch / channel dims of a saved (n, 1, T, 1, H, W) measurement are dropped, a
        (T, H, W) mask stack becomes (T, 1, H, W), the mask has one plane or one per frame.  TypeError / ValueError."""
        if not isinstance(y, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{what}: y must be a torch tensor or numpy array, got {type(y).__name__}")
        y = torch.as_tensor(y).detach()
        if not y.is_complex():
            raise TypeError(f"{what}: y must be complex k-space, got {y.dtype}")
        if y.dim() == 6 and y.shape[1] == 1 and y.shape[3] == 1:
            y = y.reshape(y.shape[0], y.shape[2], y.shape[4], y.shape[5])
        elif y.dim() == 5 and (y.shape[1] == 1 or y.shape[2] == 1):
            y = y.reshape(y.shape[0], y.shape[2] if y.shape[1] == 1 else y.shape[1], y.shape[3], y.shape[4])
        if y.dim() != 4 or min(y.shape) < 1:
            raise ValueError(f"{what}: y {tuple(y.shape)}; (n_coils, T, H, W) expected")
        n, T, H, W = y.shape
        if not isinstance(mask, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{what}: mask must be a torch tensor or numpy array, got {type(mask).__name__}")
        mask = torch.as_tensor(mask).detach().cpu()
        if mask.dim() == 3 and tuple(mask.shape[-2:]) == (H, W) and mask.shape[0] != 1:
            mask = mask[:, None]                                            # per-frame 2-D masks, as driver_mask
        planes = ops._mask_u8(mask, H, W, "cpu").shape[0]
        if planes not in (1, T):
            raise ValueError(f"{what}: the mask has {planes} planes for {T} frames; one plane, or one per frame")
        return y, mask, planes

    @staticmethod
    def time_average(y, mask):
        """the time-averaged composite of a cine measurement: y (n, T, H, W) complex k-space (tensor or ndarray, host or
        GPU; singleton batch / channel dims dropped), mask its sampling mask with one plane or T (anything ``ops._mask_u8``
        takes, or (T, H, W)).  ``ops.kspace_time_average`` on the current GPU -> ybar (n, H, W) complex64 on the GPU: the
        mean over the frames that sampled each position, zero where none did."""
        y, mask, _ = SENSE._cine_operands(y, mask, "time_average")
        yd = y.to(torch.complex64).to(y.device if y.is_cuda else "cuda").contiguous()
        return ops.kspace_time_average(yd, ops._mask_u8(mask, y.shape[-2], y.shape[-1], yd.device))

    @classmethod
    def from_cine_measurement(cls, y, mask, R=1, seed=None, calib_max=12, n_virtual=None, noise_cov=None, method="walsh",
                              **kw):
        """the ``"custom"`` operator of a 2D+time acquisition, calibrated from its time-averaged composite: y (n, T, H, W)
        multi-coil k-space and its per-frame sampling mask, as for ``time_average``.  The calibration box is
        ``calibration_region(mask, H, W, calib_max, composite=True)``; with n_virtual ONE compression matrix
        (``ops.coilcomp_matrix`` of the composite's Gram matrix, whitened with noise_cov) is applied to every frame and to
        the composite; the maps are those of the (virtual) coils of the composite (``ops.estimate_sens_maps``, or
        ``ops.espirit_maps`` with method="espirit"; kw goes to the estimator; eigval: the ESPIRiT eigenvalue map (H, W) on
        the host, None for Walsh) and serve every frame.  -> Namespace(op, measurement (n', T, H, W) complex64 on the GPU, sens_maps
        (n', H, W) complex128 on the host, coil_matrix (n', n) complex64 on the host or None, region (ah, aw), rss_max (the
        peak of the composite's calibration image), composite (n', H, W) complex64 on the GPU).  Every argument is
        checked on the host before any GPU work."""
        from argparse import Namespace
        y, mask, planes = cls._cine_operands(y, mask, "from_cine_measurement")
        n, T, H, W = y.shape
        if n_virtual is not None:
            n_virtual = ops._coilcomp_counts(n, n_virtual, "from_cine_measurement")
            if noise_cov is not None:
                noise_cov = ops.check_noise_cov(noise_cov, n, "from_cine_measurement: noise_cov")
        elif noise_cov is not None:
            raise ValueError("from_cine_measurement: noise_cov= goes with n_virtual= (whitening is part of the compression)")
        ah, aw = calibration_region(mask, H, W, calib_max, composite=True)
        cls._check_maps_method(method, n if n_virtual is None else n_virtual, H, W, ah, aw, kw, "from_cine_measurement")
        yd = y.to(torch.complex64).to(y.device if y.is_cuda else "cuda").contiguous()
        ybar = ops.kspace_time_average(yd, ops._mask_u8(mask, H, W, yd.device))
        A = None
        if n_virtual is not None:
            A = ops.coilcomp_matrix(ops.coil_gram(ybar, ah, aw), n_virtual, noise_cov)[0]
            yd, ybar = ops.coil_apply(yd, A), ops.coil_apply(ybar, A)
        eigval = None
        if method == "espirit":                                             # rss_max: the peak of the Walsh calibration image
            _, _, rss_max = ops.estimate_sens_maps(ybar, ah, aw, return_rss=True)
            maps, eigval = cls._espirit_maps(ybar, ah, aw, "from_cine_measurement", **kw)
            eigval = eigval[0].cpu()
        else:
            maps, _, rss_max = ops.estimate_sens_maps(ybar, ah, aw, return_rss=True, **kw)
        maps = maps.cpu().to(torch.complex128)
        op = cls("custom", maps.shape[0], R, 0.04, (1, H, W), seed, mask_T=planes, mask_mode="custom", mask=mask, sens_maps=maps,
                 normalize=False)
        return Namespace(op=op, measurement=yd, sens_maps=op.sens_maps, coil_matrix=None if A is None else A.cpu(),
                         region=(ah, aw), rss_max=float(rss_max[0]), composite=ybar, eigval=eigval)

    @staticmethod
    def _as_host_maps(maps):
        """tensor / ndarray -> host tensor, float64 (real input) or complex128 (complex input)"""
        if not isinstance(maps, (torch.Tensor, np.ndarray)):
            raise TypeError(f"sens_maps: a torch tensor or numpy array, got {type(maps).__name__}")
        t = torch.as_tensor(maps).detach().cpu()
        if t.is_complex():
            return t.to(torch.complex128)
        if t.is_floating_point():
            return t.to(torch.float64)
        raise TypeError(f"sens_maps: a real or complex floating dtype, got {t.dtype}")

    @property
    def sens_maps(self):
        return self._sens_maps

    @sens_maps.setter
    def sens_maps(self, maps):
        t = self._as_host_maps(maps)
        want = (self.num_sens,) + tuple(self.random_under_fourier.in_shape[-2:])
        if tuple(t.shape[-3:]) != want or t.dim() not in (3, 4) or t.shape[0] < 1:
            raise ValueError(f"sens_maps: shape {tuple(t.shape)}, expected (num_sens, H, W) = {want} or, one set per slice, "
                             f"(S,) + {want}")
        self._sens_maps = t.contiguous()
        self._dev = {}                                                      # the device copies belong to the old maps

    @property
    def n_map_sets(self):
        """S of (S, num_sens, H, W) maps, one set per slice: batch row b is sample b // S of slice b % S; 1 for
        (num_sens, H, W) maps"""
        return self._sens_maps.shape[0] if self._sens_maps.dim() == 4 else 1

    def _generate_sens_map(self, sens_type, seed=0, **kwargs):
        """exp(-dist / (2 l)) around a random anchor, l = max(dist) / 2.  The reference builds the pixel list
        from np.mgrid[0:W, 0:H] and reshapes the distances to (H, W) (:131-134); kept literally."""
        H, W = self.random_under_fourier.in_shape[-2:]
        anchor = kwargs.get("anchor", None)
        if anchor is None:
            np.random.seed(seed)
            anchor = np.array([np.random.choice(H), np.random.choice(W)])
        ww, hh = np.mgrid[0:W, 0:H]
        dist = np.sqrt((ww.ravel() - anchor[0]).astype(np.float64) ** 2 +
                       (hh.ravel() - anchor[1]).astype(np.float64) ** 2)
        length = kwargs.get("l", dist.max() / 2)
        return torch.exp(-torch.tensor(dist.reshape(H, W)) / (2 * length))

    # device-side cached copies (the reference re-uploads on every call, :143,154)
    def sens_dev(self, device):
        """the only producer of device maps: float32 for real maps, complex64 for complex ones (ops dispatches on it)"""
        key = str(device)
        if key not in self._dev:
            dt = torch.complex64 if self._sens_maps.is_complex() else torch.float32
            self._dev[key] = self._sens_maps.to(dt).to(device).contiguous()
        return self._dev[key]

    def sens_f32(self, device):
        if self._sens_maps.is_complex():
            raise TypeError("SENSE.sens_f32: the coil maps are complex; use sens_dev(device) (complex64)")
        return self.sens_dev(device)

    def mask_u8(self, device):
        return self.random_under_fourier.mask_u8(device)

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        """X (B, C, H, W) complex -> (num_sens, B, C, H, W) complex64; with S map sets B is a multiple of S and row b is
        measured through set b % S"""
        _check_gpu(X, "SENSE")
        X = X.to(torch.complex64)
        return ops.sense_forward(X, self.sens_dev(X.device), self.mask_u8(X.device))

    def conj_op(self, S: torch.Tensor) -> torch.Tensor:
        _check_gpu(S, "SENSE.conj_op")
        S = S.to(torch.complex64)
        return ops.sense_adjoint(S, self.sens_dev(S.device))

    def SSOS(self, S: torch.Tensor) -> torch.Tensor:
        _check_gpu(S, "SENSE.SSOS")
        return ops.sense_ssos(S.to(torch.complex64))

    def projection(self, X: torch.Tensor, S: torch.Tensor, lamda: float) -> torch.Tensor:
        warnings.warn("Not implemented!")
        return X
