"""Assembly of the headline workload: ACDC-style multi-coil ALD reconstruction on synthetic k-space
(128x128 complex phantom, 4 'exp' coils, variable-density mask, NCSNv2Deepest ngf=128 with
seeded random-init weights, sigma 348 -> 0.01 in 2311 levels x 3 steps, L2Penalty proximal, denoise).

Used by bench.py, __graft_entry__.smoke(), scripts/ and the tests, so that they all run the same thing.
"""
from argparse import Namespace

import numpy as np
import torch

from . import ops as ops_mod

from .helpers.load_data import load_config
from .ncsn.linear_transforms.undersampling_fourier import (RandomUndersamplingFourier, SENSE, calibration_region,
                                                           geometric_compression_check)
from .ncsn.models import get_sigmas
from .ncsn.models.ALD_optimizers import ALDInvSegProximalRealImag, SCHED_DTYPE, step_schedule
from .ncsn.models.ncsnv2 import NCSNv2Deepest
from .ncsn.models.proximal_op import get_proximal
from .synthetic import phantom_image, synth_state_dict


def conv_census(net, x, labels):
    """run one eager forward with per-launch HIP events around every convolution.
    -> list of dict(B, Cin, Cout, H, W, k, dil, flops, ms): the exact 2*MAC count and the measured duration of
    each conv launch (events are recorded on the stream the kernels run on)."""
    from . import ops
    ops.CONV_TRACE = []
    try:
        with torch.no_grad():
            net(x, labels)
        torch.cuda.synchronize()
        rec = ops.CONV_TRACE
    finally:
        ops.CONV_TRACE = None
    out = []
    for r in rec:
        ms = r.pop("e0").elapsed_time(r.pop("e1"))
        r["flops"] = 2 * r["B"] * r["Cin"] * r["Cout"] * r["k"] ** 2 * r["H"] * r["W"]
        r["ms"] = ms
        out.append(r)
    return out


def acdc_config(device, image_size=128):
    cfg = load_config("ACDC", mode="real-valued", device=device)
    cfg.data.image_size = image_size
    return cfg


def build_scorenet(cfg, seed=0):
    net = NCSNv2Deepest(cfg)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed)
    net.load_state_dict(sd, strict=False)
    return net.to(cfg.device).eval()


def build_problem(device, n_samples, R=40, H=128, W=128, num_sens=4, seed=0, scorenet=None, cfg=None, lr_scaled=1.0,
                  sens_maps=None, proximal="L2Penalty", proximal_kwargs=None, mask=None, estimate_maps=False, measurement=None,
                  calib_max=12, kspace_scale=None, coil_compress=None, noise_cov=None, n_slices=None, maps_method="walsh",
                  maps_kwargs=None, coil_compress_mode="pca", coil_compress_window=2, trajectory=None, traj_weights=None,
                  self_calibrate=False, virtual_coils=None):
    """-> Namespace(sampler, scorenet, sigmas, op, image, measurement, call_kwargs); sens_maps: measured coil maps
    (num_sens, H, W), real or complex, instead of the synthetic "exp" maps (RSS-normalised where non-zero); proximal: a
    get_proximal name ("L2PenaltyCG": the exact proximal, proximal_kwargs = dict(max_iter=, tol=)); mask: the sampling mask
    of an acquisition, a line or 2-D mask (SENSE mask_mode="custom"), instead of the generated line mask at R.
    estimate_maps: the sampler runs on coil maps estimated from the measurement's calibration region
    (SENSE.estimate_sens_maps, calib_max); without `measurement` the measurement is still simulated with the true maps.
    maps_method: "walsh" (default) or "espirit", maps_kwargs the estimator's keywords (espirit: ksize, sv_thresh, crop,
    power_iters); ESPIRiT serves up to 16 coils with n ksize^2 <= 432 (more coils: coil_compress=), and the Namespace then
    carries the eigenvalue map as espirit_eigval ((H, W), or (S, H, W) for a stack, float32 on the host; None for Walsh).
    measurement: measured k-space (n, H, W) instead of the simulated one: no phantom (image is None), maps from
    sens_maps or estimated, the data multiplied by kspace_scale -- None: 1 / rss_max of its calibration image, since the
    score prior expects magnitudes in [0, 1].  The Namespace then carries kspace_scale; estimated_maps is True when the
    operator's maps were estimated.
    coil_compress: the measurement (measured or simulated; up to 64 coils) is whitened with noise_cov (the (n, n) coil
    noise covariance, optional) and compressed to this many virtual coils by PCA of its calibration region
    (ops.coil_compress) before anything else sees it: the maps are estimated on the virtual coils (estimate_maps=True) or
    the given / synthetic maps are compressed with the same matrix (ops.coil_apply), the automatic kspace_scale comes from
    the compressed data, and the operator, the measurement and the sampler have coil_compress coils.  The Namespace
    carries the matrix as coil_matrix ((coil_compress, n) complex64 on the host; None without compression).
    coil_compress_mode="geometric": geometric coil compression along the readout axis H, which the mask must sample fully
    (ops.coil_compress_geometric; coil_compress_window rows on either side of a readout position, 0..8): one matrix per
    readout position, given / synthetic maps compressed row by row (ops.coil_apply_rows); coil_matrix is then
    (H, coil_compress, n), or (S, H, coil_compress, n) for a stack.  "pca" (default) is the one matrix per image above.
    A stack of S slices in one batch: measurement (S, n, H, W), or n_slices=S without a measurement (not both).  Each
    slice has its own coil maps -- sens_maps (S, n, H, W), or (n, H, W) shared by the slices, or estimated / compressed per
    slice (coil_matrix (S, coil_compress, n)) -- and the operator holds them as S map sets (op.n_map_sets).  The sampler's
    batch is n_samples * S rows, row b = sample b // S of slice b % S, the measurement (n, n_samples * S, 1, H, W) in the
    same order.  The automatic kspace_scale is ONE number, 1 / the largest rss_max over the slices: the slices of a volume
    share a grey scale.  A simulated stack draws slice s from phantom seed `seed + s` and, with sens_maps=None, from "exp"
    maps of seed `seed + s * num_sens` (every coil anchor of the stack its own seed); the mask is the one of `seed`.  The
    Namespace carries n_slices (1 without a stack); image is then (S, 1, H, W).
    trajectory: (M, 2) k-space positions (k_y, k_x) in cycles per field of view -- non-Cartesian SENSE (NonCartesianSENSE;
    traj_weights its optional likelihood weights).  Simulated: the phantom through the exact forward transform with the
    synthetic complex maps (or sens_maps=).  Measured: measurement (n_coils, M) with sens_maps= required, scaled by
    kspace_scale -- None: 1 / the peak magnitude of the density-compensated adjoint zero_filled(y).  The proximal is
    L2PenaltyCG (the default name "L2Penalty" is replaced by it; any other is refused); mask, R, estimate_maps,
    coil_compress and n_slices do not go with a trajectory and are refused before anything is allocated.  The Namespace
    carries zero_filled, the density-compensated adjoint of the (scaled) measurement, (1, 1, H, W) on the device.
    self_calibrate=True (with trajectory=): the coil maps come from the non-Cartesian samples themselves
    (NonCartesianSENSE.from_measurement: calib_max, maps_method, maps_kwargs as above; virtual_coils=N whitens with noise_cov
    and compresses up to 64 coils to N first).  Measured: measurement (n_coils, M) and no sens_maps=; the automatic
    kspace_scale is taken after the calibration.  Simulated: measured through the true synthetic maps, reconstructed with
    the estimated ones.  sens_maps= with self_calibrate is a ValueError.  The Namespace carries sens_maps (host), coil_matrix
    ((N, n) on the host, None without compression), calib_region (ah, aw) and calib_kspace ((n', H, W) on the device)."""
    if trajectory is not None:
        return _build_noncartesian(device, n_samples, H, W, num_sens, seed, scorenet, cfg, lr_scaled, sens_maps, proximal,
                                   proximal_kwargs, measurement, kspace_scale, trajectory, traj_weights,
                                   dict(mask=mask is not None, estimate_maps=bool(estimate_maps), coil_compress=coil_compress is not None,
                                        noise_cov=noise_cov is not None and not self_calibrate, n_slices=n_slices is not None),
                                   dict(virtual_coils=virtual_coils, noise_cov=noise_cov, calib_max=calib_max, method=maps_method,
                                        kw=dict(maps_kwargs or {})) if self_calibrate else None, virtual_coils)
    if traj_weights is not None:
        raise ValueError("build_problem: traj_weights= goes with trajectory=")
    if self_calibrate or virtual_coils is not None:
        raise ValueError("build_problem: self_calibrate= and virtual_coils= go with trajectory= (Cartesian data: estimate_maps=, "
                         "coil_compress=)")
    prox_cls = get_proximal(proximal)                        # an unknown name fails here, before any GPU work
    kspace_scale = None if kspace_scale is None else float(kspace_scale)
    region = None
    maps_kwargs = dict(maps_kwargs or {})
    if maps_method != "walsh" and not estimate_maps:
        raise ValueError(f"build_problem: maps_method={maps_method!r} goes with estimate_maps=True")
    if noise_cov is not None and coil_compress is None:
        raise ValueError("build_problem: noise_cov= goes with coil_compress= (whitening is part of the compression)")
    if coil_compress_mode not in ("pca", "geometric"):
        raise ValueError(f"build_problem: coil_compress_mode={coil_compress_mode!r}; \"pca\" or \"geometric\"")
    geo = None                                               # the window of a geometric compression
    if coil_compress_mode == "geometric":
        if coil_compress is None:
            raise ValueError("build_problem: coil_compress_mode=\"geometric\" goes with coil_compress=")
        geo = ops_mod.gcc_window(coil_compress_window, "build_problem(coil_compress_window=...)")
    if n_slices is not None:
        if measurement is not None:
            raise ValueError("build_problem: n_slices= simulates a stack; a measured stack is measurement (S, n_coils, H, W)")
        if isinstance(n_slices, bool) or int(n_slices) != n_slices or n_slices < 1:
            raise ValueError(f"build_problem: n_slices must be an integer >= 1, got {n_slices!r}")
    if n_slices is not None or (measurement is not None and torch.as_tensor(measurement).dim() == 4):
        return _build_stack(device, n_samples, R, H, W, num_sens, seed, scorenet, cfg, lr_scaled, sens_maps, prox_cls,
                            proximal_kwargs, mask, estimate_maps, measurement, calib_max, kspace_scale, coil_compress, noise_cov,
                            None if n_slices is None else int(n_slices), maps_method, maps_kwargs, geo)
    if measurement is not None:                              # host-side checks: all fail before any GPU work
        if mask is None:
            raise ValueError("build_problem(measurement=...): pass mask=, the sampling mask of the acquisition")
        if (sens_maps is None) != bool(estimate_maps):
            raise ValueError("build_problem(measurement=...): the coil maps come from sens_maps= or from estimate_maps=True")
        measurement = torch.as_tensor(measurement)
        if measurement.dim() != 3 or not measurement.is_complex() or tuple(measurement.shape[-2:]) != (H, W):
            raise ValueError(f"build_problem: measurement {tuple(measurement.shape)} {measurement.dtype}; complex "
                             f"(n_coils, {H}, {W}) or, a stack of slices, (S, n_coils, {H}, {W}) expected")
        num_sens = measurement.shape[0]
        if estimate_maps or kspace_scale is None or coil_compress is not None:
            region = calibration_region(mask, H, W, calib_max)
    if coil_compress is not None:                            # host-side as well
        coil_compress = ops_mod._coilcomp_counts(num_sens, coil_compress, "build_problem(coil_compress=...)")
        if noise_cov is not None:
            noise_cov = ops_mod.check_noise_cov(noise_cov, num_sens, "build_problem: noise_cov")
        if geo is not None:                                  # without mask=: the line mask the operator will generate
            geometric_compression_check(mask if mask is not None else RandomUndersamplingFourier(R, 0.04, (1, H, W), seed).mask,
                                        num_sens, coil_compress, H, W, calib_max, geo, "build_problem")
    n_est = num_sens if coil_compress is None else coil_compress
    _check_maps(maps_method, maps_kwargs, n_est, H, W, region)
    coil_matrix = eigval = None
    cfg = acdc_config(device, H) if cfg is None else cfg
    scorenet = build_scorenet(cfg, seed) if scorenet is None else scorenet
    sigmas = get_sigmas(cfg, "recons")
    mk = {} if mask is None else dict(mask_mode="custom", mask=mask)
    if measurement is not None:
        img = None
        y = measurement.to(torch.complex64).to(device).contiguous()
        if coil_compress is not None:
            y, A = _compress(y, region, coil_compress, noise_cov, geo)
            coil_matrix = A[0]
            if sens_maps is not None:
                sens_maps = _compress_maps(SENSE.rss_normalize(sens_maps), coil_matrix, num_sens, H, W, device)
            num_sens = coil_compress
        if region is not None:
            # one call serves both uses: the maps (kept only with estimate_maps) and rss_max for the automatic scale; with
            # sens_maps= given and no kspace_scale the maps are computed and dropped (a fraction of a millisecond, once)
            maps, _, rss_max = ops_mod.estimate_sens_maps(y, *region, return_rss=True)
            if kspace_scale is None:
                peak = float(rss_max[0])
                if not peak > 0.0:
                    raise ValueError("build_problem: the measurement's calibration region holds no signal")
                kspace_scale = 1.0 / peak
        if estimate_maps and maps_method == "espirit":
            maps, eigval = SENSE._espirit_maps(y, *region, "build_problem", **maps_kwargs)
            eigval = eigval[0]
        if estimate_maps:
            op = SENSE("custom", num_sens, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=maps.cpu(), normalize=False, **mk)
        else:
            op = SENSE("custom", num_sens, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=sens_maps,
                       normalize=coil_compress is None, **mk)
        meas1 = (y * kspace_scale).reshape(num_sens, 1, 1, H, W)
    else:
        if sens_maps is None:
            op = SENSE("exp", num_sens, R, 0.04, (1, H, W), seed=seed, mask_T=1, **mk)
        else:
            op = SENSE("custom", num_sens, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=sens_maps, **mk)
        if estimate_maps or coil_compress is not None:       # host only: an unusable centre fails before the forward model runs
            region = calibration_region(op.random_under_fourier.mask, H, W, calib_max)
            _check_maps(maps_method, maps_kwargs, n_est, H, W, region)
        img = phantom_image(H, W, seed=seed).to(device)
        meas1 = op(img)
        if coil_compress is not None:                        # simulated with the physical coils, compressed like a measured scan
            meas1, A = _compress(meas1, region, coil_compress, noise_cov, geo)
            coil_matrix = A[0]
            if not estimate_maps:
                op = SENSE("custom", coil_compress, R, 0.04, (1, H, W), seed=seed, mask_T=1, normalize=False, mask_mode="custom",
                           mask=op.random_under_fourier.mask,
                           sens_maps=_compress_maps(op.sens_maps, coil_matrix, num_sens, H, W, device))
        if estimate_maps:                                    # simulated with the true maps, reconstructed with the estimated ones
            op, eigval = _maps_from_simulated(meas1, op.random_under_fourier.mask, R, seed, calib_max, maps_method, maps_kwargs)
    return _assemble(device, n_samples, 1, H, W, scorenet, cfg, sigmas, op, img, meas1, prox_cls, proximal_kwargs, lr_scaled,
                     estimate_maps, kspace_scale, coil_matrix, eigval)


def _build_noncartesian(device, n_samples, H, W, num_sens, seed, scorenet, cfg, lr_scaled, sens_maps, proximal, proximal_kwargs,
                        measurement, kspace_scale, trajectory, traj_weights, refused, calib=None, virtual_coils=None):
    """build_problem(trajectory=...), its docstring.  Every check runs on the host before the network is built.  calib: the
    self-calibration request (virtual_coils, noise_cov, calib_max, method, kw), None without self_calibrate"""
    from .ncsn.linear_transforms.noncartesian import NonCartesianSENSE, calibration_window
    from .synthetic import complex_coil_maps
    for name, given in refused.items():
        if given:
            raise ValueError(f"build_problem: {name}= does not go with trajectory= (non-Cartesian SENSE takes given coil maps, "
                             "one slice, and no sampling mask)")
    if proximal not in ("L2Penalty", "L2PenaltyCG"):
        get_proximal(proximal)
        raise ValueError(f"build_problem: proximal={proximal!r} does not serve a trajectory; non-Cartesian SENSE takes L2PenaltyCG")
    prox_cls = get_proximal("L2PenaltyCG")
    if torch.as_tensor(trajectory).dim() > 2:
        raise ValueError(f"build_problem: trajectory {tuple(torch.as_tensor(trajectory).shape)}: a 2-D problem takes (M, 2); one "
                         "trajectory per frame (T, M, 2) is the 2D+time sampler's (ALD2DTime, scripts/cine_SENSE_real_img_2d_time.py)")
    if calib is None and virtual_coils is not None:
        raise ValueError("build_problem: virtual_coils= goes with self_calibrate=True")
    if calib is not None and sens_maps is not None:
        raise ValueError("build_problem: self_calibrate=True estimates the coil maps; it does not go with sens_maps=")
    if measurement is not None:
        if sens_maps is None and calib is None:
            raise ValueError("build_problem(measurement=..., trajectory=...): pass sens_maps=, the coil maps, or "
                             "self_calibrate=True to estimate them from the samples")
        measurement = torch.as_tensor(measurement)
        M = torch.as_tensor(trajectory).shape[0] if torch.as_tensor(trajectory).dim() == 2 else -1
        if measurement.dim() != 2 or not measurement.is_complex() or measurement.shape[1] != M:
            raise ValueError(f"build_problem: measurement {tuple(measurement.shape)} {measurement.dtype}; complex (n_coils, M = {M}) "
                             "expected with a trajectory")
        num_sens = measurement.shape[0]
    measured_calib = calib is not None and measurement is not None    # no maps yet: the operator comes from the calibration
    if sens_maps is None and not measured_calib:
        sens_maps = complex_coil_maps(num_sens, H, W, seed)
    # the remaining host checks (measured self-calibration: trajectory, weights and size alone, on the one-coil operator)
    op = NonCartesianSENSE(trajectory, (1, H, W), sens_maps=sens_maps, weights=traj_weights)
    if not measured_calib and op.num_sens != num_sens:
        raise ValueError(f"build_problem: {num_sens} coil signals, {op.num_sens} coil maps")
    if calib is not None:                                    # the window and the estimator's limits, on the host as well
        ah, aw, _ = calibration_window(op.trajectory, H, W, calib["calib_max"])
        NonCartesianSENSE._check_calib(num_sens, calib["virtual_coils"], calib["noise_cov"], H, W, ah, aw, calib["method"],
                                       dict(calib["kw"]), "build_problem(self_calibrate=True)")
    cfg = acdc_config(device, H) if cfg is None else cfg
    scorenet = build_scorenet(cfg, seed) if scorenet is None else scorenet
    sigmas = get_sigmas(cfg, "recons")
    cal = None
    if calib is not None:                                    # simulated with the true maps, reconstructed with the estimated ones
        img = None if measurement is not None else phantom_image(H, W, seed=seed).to(device)
        y = measurement.to(torch.complex64).to(device) if measurement is not None else op(img).reshape(num_sens, -1)
        kw = dict(calib["kw"])
        kw.pop("return_eig", None)
        cal = NonCartesianSENSE.from_measurement(y, op.trajectory, (1, H, W), weights=traj_weights, n_virtual=calib["virtual_coils"],
                                                 noise_cov=calib["noise_cov"], method=calib["method"], calib_max=calib["calib_max"],
                                                 **kw)
        op, num_sens = cal.op, cal.op.num_sens
        measurement = cal.measurement if measurement is not None else None
        meas1 = cal.measurement.reshape(num_sens, 1, 1, -1).contiguous()
    if measurement is not None:
        img = None
        meas1 = measurement.to(torch.complex64).to(device).reshape(num_sens, 1, 1, -1).contiguous()
        if kspace_scale is None:                             # the score prior expects magnitudes in [0, 1]
            peak = float(op.zero_filled(meas1).abs().max())
            if not peak > 0.0:
                raise ValueError("build_problem: the measurement holds no signal")
            kspace_scale = 1.0 / peak
        meas1 = meas1 * float(kspace_scale)
    elif cal is None:
        img = phantom_image(H, W, seed=seed).to(device)
        meas1 = op(img)
    meas = meas1.repeat(1, n_samples, 1, 1).contiguous()
    params = dict(n_steps_each=cfg.sampling.n_steps_each, step_lr=cfg.sampling.step_lr, denoise=True, final_only=True)
    sampler = ALDInvSegProximalRealImag(prox_cls(op, **(proximal_kwargs or {})), 1.0, "linear", (n_samples, 1, H, W), scorenet,
                                        sigmas, params, cfg, meas, op, seg=None, device=device)
    return Namespace(sampler=sampler, scorenet=scorenet, sigmas=sigmas, op=op, image=img, measurement=meas, cfg=cfg, params=params,
                     call_kwargs=dict(label=None, lamda=0.1, save_dir=None, lr_scaled=lr_scaled, seg_mode="full"),
                     estimated_maps=cal is not None, kspace_scale=kspace_scale,
                     coil_matrix=None if cal is None else cal.coil_matrix, n_slices=1,
                     espirit_eigval=None if cal is None else cal.eigval, zero_filled=op.zero_filled(meas1), sens_maps=op.sens_maps,
                     calib_region=None if cal is None else cal.region, calib_kspace=None if cal is None else cal.calib_kspace)


def build_pc_sampler(prob, sde, **kw):
    """predictor-corrector reconstruction with a VE-SDE score network (NCSN++) on a build_problem Namespace: its operator
    and measurement -- measured k-space, estimated maps, compression and stacks included (row b = sample b // n_slices of
    slice b % n_slices) -- with sde.inverse.get_pc_inverse_sampler's keywords -> sampler(model, ...) -> (x, nfe).
    build_problem(scorenet=...) takes the NCSN++ (it is only stored), which spares building the NCSNv2 network."""
    from .sde.inverse import get_pc_inverse_sampler
    kw.setdefault("device", prob.measurement.device)
    return get_pc_inverse_sampler(sde, prob.op, prob.measurement, **kw)


def _check_maps(maps_method, maps_kwargs, n_coils, H, W, region):
    """host-side check of the estimator choice; while the region is unknown (a mask still to be simulated) the box test
    waits for it: 9 x 9 passes every ksize"""
    if maps_method != "walsh":
        ah, aw = region if region is not None else (4, 4)
        SENSE._check_maps_method(maps_method, n_coils, H, W, ah, aw, dict(maps_kwargs), "build_problem")


def _maps_from_simulated(meas, mask, R, seed, calib_max, maps_method, maps_kwargs):
    """the operator with maps estimated from a simulated measurement ((n, 1, 1, H, W), or a stack (S, n, H, W)) -> (op,
    ESPIRiT eigenvalue map on the host or None)"""
    if maps_method == "walsh":
        return SENSE.from_measurement(meas, mask, R=R, seed=seed, calib_max=calib_max), None
    maps, eigval = SENSE.estimate_sens_maps(meas, mask, calib_max=calib_max, method=maps_method, return_eig=True, **maps_kwargs)
    n, H, W = maps.shape[-3:]
    return SENSE("custom", n, R, 0.04, (1, H, W), seed, mask_mode="custom", mask=mask, sens_maps=maps, normalize=False), eigval


def _assemble(device, n_samples, S, H, W, scorenet, cfg, sigmas, op, img, meas1, prox_cls, proximal_kwargs, lr_scaled,
              estimate_maps, kspace_scale, coil_matrix, eigval=None):
    """the sampler on n_samples copies of meas1 (n, S, 1, H, W): repeat along the batch axis gives row sample * S + slice"""
    meas = meas1.repeat(1, n_samples, 1, 1, 1).contiguous()
    params = dict(n_steps_each=cfg.sampling.n_steps_each, step_lr=cfg.sampling.step_lr, denoise=True,
                  final_only=True)
    sampler = ALDInvSegProximalRealImag(prox_cls(op, **(proximal_kwargs or {})), 1.0, "linear", (n_samples * S, 1, H, W),
                                        scorenet, sigmas, params, cfg, meas, op, seg=None, device=device)
    return Namespace(sampler=sampler, scorenet=scorenet, sigmas=sigmas, op=op, image=img, measurement=meas, cfg=cfg,
                     params=params, call_kwargs=dict(label=None, lamda=0.1, save_dir=None, lr_scaled=lr_scaled,
                                                     seg_mode="full"),
                     estimated_maps=bool(estimate_maps), kspace_scale=kspace_scale,
                     coil_matrix=None if coil_matrix is None else coil_matrix.cpu(), n_slices=S,
                     espirit_eigval=None if eigval is None else eigval.cpu())


def _build_stack(device, n_samples, R, H, W, num_sens, seed, scorenet, cfg, lr_scaled, sens_maps, prox_cls, proximal_kwargs,
                 mask, estimate_maps, measurement, calib_max, kspace_scale, coil_compress, noise_cov, n_slices,
                 maps_method="walsh", maps_kwargs=None, geo=None):
    """build_problem for a stack of slices (its docstring): measurement (S, n, H, W), or n_slices simulated ones.  Every
    shape, mask and calibration-region check runs on the host before the score network is built or the GPU is touched."""
    region = None
    if measurement is not None:
        if mask is None:
            raise ValueError("build_problem(measurement=...): pass mask=, the sampling mask of the acquisition")
        if (sens_maps is None) != bool(estimate_maps):
            raise ValueError("build_problem(measurement=...): the coil maps come from sens_maps= or from estimate_maps=True")
        measurement = torch.as_tensor(measurement)
        if (measurement.dim() != 4 or not measurement.is_complex() or tuple(measurement.shape[-2:]) != (H, W)
                or min(measurement.shape) < 1):
            raise ValueError(f"build_problem: measurement {tuple(measurement.shape)} {measurement.dtype}; complex "
                             f"(S, n_coils, {H}, {W}) expected")
        S, num_sens = measurement.shape[0], measurement.shape[1]
        if estimate_maps or kspace_scale is None or coil_compress is not None:
            region = calibration_region(mask, H, W, calib_max)
    else:
        S = n_slices
    if sens_maps is not None:
        sens_maps = torch.as_tensor(sens_maps)
        if tuple(sens_maps.shape) not in ((num_sens, H, W), (S, num_sens, H, W)):
            raise ValueError(f"build_problem: sens_maps {tuple(sens_maps.shape)}, expected {(num_sens, H, W)} (shared by the "
                             f"slices) or {(S, num_sens, H, W)}")
        if sens_maps.dim() == 3:
            sens_maps = sens_maps[None].expand(S, num_sens, H, W)
    if coil_compress is not None:
        coil_compress = ops_mod._coilcomp_counts(num_sens, coil_compress, "build_problem(coil_compress=...)")
        if noise_cov is not None:
            noise_cov = ops_mod.check_noise_cov(noise_cov, num_sens, "build_problem: noise_cov")
    mk = {} if mask is None else dict(mask_mode="custom", mask=mask)
    op = None
    if measurement is None:
        # the simulating operator, host only so far: its mask is the one a calibration region has to be found in
        if sens_maps is None:
            sens_maps = torch.stack([SENSE("exp", num_sens, R, 0.04, (1, H, W), seed=seed + s * num_sens).sens_maps
                                     for s in range(S)])
            op = SENSE("custom", num_sens, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=sens_maps, normalize=False, **mk)
        else:
            op = SENSE("custom", num_sens, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=sens_maps, **mk)
        if estimate_maps or coil_compress is not None:
            region = calibration_region(op.random_under_fourier.mask, H, W, calib_max)
    if geo is not None:
        geometric_compression_check(mask if measurement is not None else op.random_under_fourier.mask, num_sens, coil_compress,
                                    H, W, calib_max, geo, "build_problem")
    maps_kwargs = dict(maps_kwargs or {})
    _check_maps(maps_method, maps_kwargs, num_sens if coil_compress is None else coil_compress, H, W, region)
    coil_matrix = eigval = None
    cfg = acdc_config(device, H) if cfg is None else cfg
    scorenet = build_scorenet(cfg, seed) if scorenet is None else scorenet
    sigmas = get_sigmas(cfg, "recons")
    n_out = num_sens if coil_compress is None else coil_compress
    if measurement is not None:
        img = None
        y = measurement.to(torch.complex64).to(device).transpose(0, 1).contiguous()          # (n, S, H, W): one image per slice
        if coil_compress is not None:
            y, coil_matrix = _compress(y, region, coil_compress, noise_cov, geo)
            if sens_maps is not None:
                sens_maps = _compress_map_sets(SENSE.rss_normalize(sens_maps), coil_matrix, device)
        if region is not None:
            maps, _, rss_max = ops_mod.estimate_sens_maps(y, *region, return_rss=True)
            if kspace_scale is None:
                peak = float(rss_max.max())
                if not peak > 0.0:
                    raise ValueError("build_problem: the measurement's calibration region holds no signal")
                kspace_scale = 1.0 / peak
        if estimate_maps and maps_method == "espirit":
            maps, eigval = SENSE._espirit_maps(y, *region, "build_problem", **maps_kwargs)
        if estimate_maps:
            op = SENSE("custom", n_out, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=maps.transpose(0, 1).cpu(),
                       normalize=False, **mk)
        else:
            op = SENSE("custom", n_out, R, 0.04, (1, H, W), seed=seed, mask_T=1, sens_maps=sens_maps,
                       normalize=coil_compress is None, **mk)
        meas1 = (y * kspace_scale).reshape(n_out, S, 1, H, W)
    else:
        img = torch.cat([phantom_image(H, W, seed=seed + s) for s in range(S)], dim=0).to(device)
        meas1 = op(img)                                                                       # (n, S, 1, H, W)
        sim_mask = op.random_under_fourier.mask
        if coil_compress is not None:
            meas1, coil_matrix = _compress(meas1, region, coil_compress, noise_cov, geo)
            if not estimate_maps:
                op = SENSE("custom", n_out, R, 0.04, (1, H, W), seed=seed, mask_T=1, normalize=False, mask_mode="custom",
                           mask=sim_mask, sens_maps=_compress_map_sets(op.sens_maps, coil_matrix, device))
        if estimate_maps:
            op, eigval = _maps_from_simulated(meas1[:, :, 0].transpose(0, 1), sim_mask, R, seed, calib_max, maps_method,
                                              maps_kwargs)
    return _assemble(device, n_samples, S, H, W, scorenet, cfg, sigmas, op, img, meas1, prox_cls, proximal_kwargs, lr_scaled,
                     estimate_maps, kspace_scale, coil_matrix, eigval)


def _compress(y, region, n_virtual, noise_cov, geo):
    """the measurement y (n, B, ..., H, W) compressed to n_virtual coils -> (y', A): by PCA of the calibration box, A
    (B, nv, n), or -- geo: the window -- geometrically along the readout, A (B, H, nv, n); a position that could not be
    aligned is an error"""
    if geo is None:
        out, A, _, _ = ops_mod.coil_compress(y, *region, n_virtual, noise_cov, return_matrix=True)
        return out, A
    out, A, _, status = ops_mod.coil_compress_geometric(y, region[1], n_virtual, geo, noise_cov, return_matrix=True)
    for b, st in enumerate(status.cpu().tolist()):
        if st != 0:
            raise RuntimeError(f"build_problem: geometric coil compression of image {b}: " + (
                "the noise covariance has a non-positive Cholesky pivot in fp32" if st < 0 else
                f"{st} readout position(s) could not be aligned with their neighbour"))
    return out, A


def _compress_map_sets(maps, A, device):
    """coil maps (S, n, H, W) of the physical coils -> (S, nv, H, W) of the virtual coils, host complex128: slice s by its own
    matrix A[s] of A (S, nv, n), one call of the streaming kernel with a matrix per image (A (S, H, nv, n): per row)"""
    m = torch.as_tensor(maps).to(torch.complex64).to(device).transpose(0, 1).contiguous()    # (n, S, H, W)
    fn = ops_mod.coil_apply_rows if A.dim() == 4 else ops_mod.coil_apply
    return fn(m, A.contiguous()).transpose(0, 1).cpu().to(torch.complex128).contiguous()


def _compress_maps(maps, A, n, H, W, device):
    """coil maps (n, H, W) of the physical coils -> the (nv, H, W) maps of the virtual coils, host complex128: the same
    matrix A (nv, n) that compressed the measurement, applied by the streaming kernel"""
    maps = torch.as_tensor(maps)
    if tuple(maps.shape) != (n, H, W):
        raise ValueError(f"build_problem: sens_maps {tuple(maps.shape)}, expected {(n, H, W)}")
    m = maps.to(torch.complex64).to(device).reshape(n, 1, H, W).contiguous()
    fn = ops_mod.coil_apply_rows if A.dim() == 3 else ops_mod.coil_apply           # A (H, nv, n): one matrix per row
    return fn(m, A.contiguous())[:, 0].cpu().to(torch.complex128)


class IterationRunner:
    """One Langevin iteration of the SENSE sampler as a replayable hipGraph, with the level chosen per call.
    This is the unit bench.py times ("step"); ALDInvSegProximalRealImag.__call__ runs the same launches."""

    def __init__(self, prob, seed=0, sample_offset=0, use_graph=True):
        s = prob.sampler
        dev = s.device
        meas = s.measurement.to(dev).to(torch.complex64).contiguous()
        x0 = s.linear_tfm.conj_op(meas)
        B, H, W = x0.shape[0], x0.shape[-2], x0.shape[-1]
        self.B, self.H, self.W = B, H, W
        self.sampler = s
        self.x = torch.cat([x0.real, x0.imag], dim=0).contiguous().float()
        steps, noise_scales = step_schedule(s.sigmas, s.params["step_lr"])
        L, n_each = len(s.sigmas), s.params["n_steps_each"]
        coef = s.proximal.coef(s.params["step_lr"] * prob.call_kwargs["lr_scaled"], 1., x0.shape)
        table = np.zeros(L * n_each, dtype=SCHED_DTYPE)
        lv = np.repeat(np.arange(L), n_each)
        table["step"], table["noise_scale"] = steps.numpy()[lv], noise_scales.numpy()[lv]
        table["coef"], table["sigma"] = coef, s.sigmas.detach().cpu().numpy()[lv]
        table["step_id"] = np.arange(L * n_each)
        self.levels = lv
        self.table_dev = torch.from_numpy(table.view(np.uint8).reshape(L * n_each, -1).copy()).to(dev)
        self.label_table = torch.arange(L, device=dev)[:, None].repeat(1, 2 * B)
        cg, work = s._cg_state(B, s.linear_tfm.sens_maps.shape[-3], H, W, dev, x0)
        self.st = dict(x=self.x, B=B, y=meas, sc_mode=None, sens=s.linear_tfm.sens_dev(dev), mask=s.linear_tfm.mask_u8(dev),
                       work=work, cg=cg,
                       labels=torch.zeros(2 * B, dtype=torch.long, device=dev), noise_re=None, noise_im=None,
                       seed=seed, sample_offset=sample_offset,
                       sched_dev=torch.zeros(SCHED_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        self.n_iterations = L * n_each
        self.graph = None
        self.use_graph = use_graph

    def set_iteration(self, k):
        self.st["sched_dev"].copy_(self.table_dev[k], non_blocking=True)
        self.st["labels"].copy_(self.label_table[int(self.levels[k])], non_blocking=True)

    @torch.no_grad()
    def run(self, k):
        self.set_iteration(k)
        if not self.use_graph:
            self.sampler._iteration(self.st)
        elif self.graph is None:
            self.sampler._iteration(self.st)           # warm-up: weight packing, allocator, LDS attributes
            self.graph = self.sampler._capture(self.st)
        else:
            self.graph.replay()

    def current(self):
        return torch.complex(self.x[:self.B], self.x[self.B:])
