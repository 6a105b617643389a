#!/usr/bin/env python3
"""2D+time ALD reconstruction on synthetic k-space (counterpart of the reference's
``scripts/cine_SENSE_real_img_2d_time.py``, BASELINE config 4): spatial NCSNv2Deepest prior + temporal
NCSN3DShallow prior on 8x8xT patches (`--temporal_type Diffusion1D`: NCSN1D on the same patches as (kx*ky, T) sequences), SENSE with the T=24 mask.  Same flags; prints `reconstruction time` as the
reference does.  --kspace PATH reconstructs measured 2D+time k-space (n, T, H, W) with its --mask PATH (no ground truth: original.pt
is skipped); --estimate_maps calibrates from the time-averaged composite of the per-frame patterns (sens_maps.pt), --coil_compress N
whitens (--noise_cov PATH) and compresses all frames with one matrix first (coil_matrix.pt); both also run on the simulated
measurement.  Radial cine: --trajectory radial --spokes N [--readout M] simulates a golden-angle acquisition of the pulsating
phantom with N spokes per frame (the spoke index runs on across the --T frames, so every frame has its own trajectory),
--trajectory PATH one on the (T, M, 2) positions of a file, --kspace PATH --trajectory PATH --sens_maps PATH reconstructs
measured samples (n_coils, T, M).  The proximal is then L2PenaltyCG (--proximal_type L2PenaltyCG); trajectory.pt, ZF.pt and
measurement.pt are written and no mask.pt.  --self_calibrate ([--virtual_coils N] [--noise_cov PATH] [--calib_max N]
[--maps_method walsh|espirit]) takes the coil maps from the samples themselves, pooled over the frames, so that --kspace PATH
--trajectory PATH --self_calibrate needs no --sens_maps (sens_maps.pt, calib_kspace.pt, coil_matrix.pt).  Under torchrun the `--num_samples` posterior samples are block-partitioned over the ranks (Philox noise
keyed by the global sample id, the per-step random shift drawn from identically seeded host generators), rank 0 writes the
artefacts and the posterior mean / std: the result does not depend on the number of ranks."""
import argparse
import os
import pickle
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROXIMAL_NAMES = ["L2Penalty", "Constrained", "SingleCoil", "L2PenaltyCG"]     # get_proximal's names

if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument("--R", type=int, default=8)
    parser.add_argument("--center_lines_frac", type=float, default=1 / 20)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--step_lr", type=float, default=0.0001)
    parser.add_argument("--num_steps_each", type=int, default=3)
    parser.add_argument("--lr_scaled", type=float, default=1.)
    parser.add_argument("--proximal_type", default="L2Penalty", choices=PROXIMAL_NAMES,
                        help="data-consistency operator; L2PenaltyCG: the exact multi-coil proximal by conjugate gradients")
    parser.add_argument("--cg_iters", type=int, default=10, help="L2PenaltyCG: CG iterations at most")
    parser.add_argument("--cg_tol", type=float, default=1e-5, help="L2PenaltyCG: stop at |r| <= cg_tol |b|")
    parser.add_argument("--num_samples", type=int, default=1)
    parser.add_argument("--sens_type", default="exp")
    parser.add_argument("--temporal_type", default="Diffusion3D", choices=["Diffusion3D", "Diffusion1D"],
                        help="temporal prior: NCSN3DShallow on 8x8xT patches, or NCSN1D on (kx*ky, T) sequences")
    parser.add_argument("--num_sens", type=int, default=4)
    parser.add_argument("--mode_T", default="diffusion1d", choices=["tv", "diffusion1d", "none", "diffusion1d-only", "tv-only"])
    parser.add_argument("--lamda_T", type=float, default=10.)
    parser.add_argument("--if_random_shift", action="store_true")
    parser.add_argument("--save_dir", default="../outputs")
    parser.add_argument("--image_size", type=int, default=128, help="image height (and width, without --image_width)")
    parser.add_argument("--image_width", type=int, default=None,
                        help="image width (default: --image_size); sides: powers of two, or multiples of 16 of the form "
                             "2^a 3^b 5^c up to 2048, e.g. 96, 144, 160, 192, 240, 288, 320, 384")
    parser.add_argument("--T", type=int, default=24)
    parser.add_argument("--n_levels", type=int, default=None)
    parser.add_argument("--start_level", type=int, default=0, help="first noise level (with --n_levels: a slice of the schedule)")
    parser.add_argument("--sens_maps", default=None,
                        help=".npy / .pt file with measured coil maps (num_sens, H, W), real or complex")
    parser.add_argument("--sens_phase", action="store_true",
                        help="synthetic COMPLEX coil maps: the exp magnitudes times a smooth seeded phase")
    parser.add_argument("--mask", default=None,
                        help=".npy / .pt file with the sampling mask: a line mask (..., W) or a 2-D mask (..., H, W), "
                             "per frame as (T, 1, 1, W), (T, 1, H, W) or (T, H, W)")
    parser.add_argument("--mask_2d", action="store_true",
                        help="synthetic variable-density 2-D (ky, kz) sampling mask at --R instead of the line mask")
    parser.add_argument("--trajectory", default=None, metavar="radial|PATH",
                        help="radial cine: 'radial' (golden-angle spokes, --spokes per frame, --readout) or a .npy / .pt file "
                             "with the positions (T, M, 2) = (k_y, k_x) in cycles per field of view; needs --proximal_type "
                             "L2PenaltyCG")
    parser.add_argument("--spokes", type=int, default=None, metavar="N", help="--trajectory radial: spokes per frame")
    parser.add_argument("--readout", type=int, default=None, metavar="M",
                        help="--trajectory radial: samples per spoke (default: 2 x the larger image side)")
    from inverseproblemwithdiffusionmodel_amd.helpers import load_data
    load_data.add_cine_measurement_args(parser)
    load_data.add_self_calibrate_args(parser)
    a = parser.parse_args()
    H, W = a.image_size, a.image_size if a.image_width is None else a.image_width
    from inverseproblemwithdiffusionmodel_amd import ops
    trajectory, nc_kspace, self_cal = None, None, None
    if not a.trajectory:
        load_data.driver_self_calibrate(a, None, H, W, a.num_sens)          # the flags alone: they go with --trajectory
    if a.trajectory:                                  # every refusal before a network is built
        if a.proximal_type != "L2PenaltyCG":
            sys.exit(f"--trajectory: non-Cartesian SENSE takes --proximal_type L2PenaltyCG, not {a.proximal_type}")
        for flag, given in (("mask", a.mask), ("mask_2d", a.mask_2d), ("estimate_maps", a.estimate_maps),
                            ("coil_compress", a.coil_compress is not None), ("noise_cov", a.noise_cov and not a.self_calibrate),
                            ("maps_method", a.maps_method != "walsh" and not a.self_calibrate)):
            if given:
                sys.exit(f"--trajectory does not go with --{flag}: non-Cartesian SENSE takes given coil maps and no sampling mask")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("--trajectory: one process (sharded non-Cartesian runs are not built)")
        if not ops.nc_supported(H, W):
            sys.exit(f"--image_size {H} --image_width {W}: no non-Cartesian kernel for {H}x{W}; {ops.NC_SIZE_RULE}")
        from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.noncartesian import check_trajectory
        from inverseproblemwithdiffusionmodel_amd.synthetic import radial_cine_trajectory
        try:
            if a.trajectory == "radial":
                if a.spokes is None or a.spokes < 1:
                    sys.exit("--trajectory radial needs --spokes N (>= 1), the spokes per frame")
                if a.kspace:
                    sys.exit("--kspace PATH needs --trajectory PATH, the positions of its samples")
                trajectory = radial_cine_trajectory(a.T, a.spokes, a.readout if a.readout is not None else 2 * max(H, W), H, W)
            else:
                if a.spokes is not None or a.readout is not None:
                    sys.exit("--spokes / --readout go with --trajectory radial")
                trajectory = load_data.load_trajectory(a.trajectory, cine=True)
            trajectory = check_trajectory(trajectory, H, W, "--trajectory")
            a.T = int(trajectory.shape[0])
            if a.kspace:
                if not a.self_calibrate and (not a.sens_maps or a.sens_phase):
                    sys.exit("--kspace PATH --trajectory PATH needs --sens_maps PATH, or --self_calibrate to estimate the maps "
                             "from the samples")
                nc_kspace = load_data.load_kspace(a.kspace, noncartesian=True, cine=True)
                if tuple(nc_kspace.shape[1:]) != tuple(trajectory.shape[:2]):
                    sys.exit(f"--kspace holds {tuple(nc_kspace.shape)}; (n_coils, {trajectory.shape[0]}, {trajectory.shape[1]}) "
                             "expected for this trajectory")
                a.num_sens = int(nc_kspace.shape[0])
                maps_shape = tuple(load_data.load_sens_maps(a.sens_maps).shape) if a.sens_maps else None
                if a.sens_maps and maps_shape != (a.num_sens, H, W):
                    sys.exit(f"--sens_maps holds {maps_shape}; ({a.num_sens}, {H}, {W}) expected for this measurement")
        except (ValueError, TypeError) as e:
            sys.exit(str(e))
        self_cal = load_data.driver_self_calibrate(a, trajectory, H, W, a.num_sens)     # the pooled window, before any network
    elif a.spokes is not None or a.readout is not None:
        sys.exit("--spokes / --readout go with --trajectory radial")
    checked = None
    if trajectory is None and load_data.cine_measurement_requested(a):       # the file, the flags and the calibration region, before any model is built
        try:
            cal_mask = load_data.driver_mask(a.mask, a.mask_2d, H, W, a.R, a.seed) if not a.kspace else (
                load_data.load_mask(a.mask) if a.mask else None)
        except (ValueError, TypeError) as e:
            sys.exit(str(e))
        checked = load_data.driver_cine_checks(a, H, W, a.T, a.num_sens, cal_mask)
        H, W, a.T, a.num_sens = checked.H, checked.W, checked.T, checked.num_sens
    if trajectory is None and ops.kspace_size_class(H, W) == ops.KSPACE_NONE:                    # before any allocation
        sys.exit(f"--image_size {H} --image_width {W}: no k-space kernel for {H}x{W}; {ops.KSPACE_SIZE_RULE}")
    from inverseproblemwithdiffusionmodel_amd.helpers.load_model import reload_model
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import get_sigmas
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ALD_optimizers import ALD2DTime
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.proximal_op import get_proximal
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
    from inverseproblemwithdiffusionmodel_amd.helpers.load_data import driver_mask, driver_sens_maps
    from inverseproblemwithdiffusionmodel_amd.synthetic import phantom_image
    from inverseproblemwithdiffusionmodel_amd import sharding
    world, rank, device = sharding.init_distributed()
    lo, hi = sharding.shard_range(a.num_samples, world, rank)
    n_local = max(hi - lo, 1)                 # a rank without samples still runs one (discarded): collectives stay aligned
    np.random.seed(a.seed)                    # if_random_shift: one shift per step for the whole batch, on every rank
    scorenet = reload_model("Diffusion", "CINE127", device=device)
    scorenet_T = reload_model(a.temporal_type, "CINE127", device=device)
    sigmas = get_sigmas(scorenet.config, "recons")
    sigmas_T = get_sigmas(scorenet_T.config, "recons")
    sens_maps = None
    if checked is None or checked.kspace is None:
        sens_maps, a.num_sens = driver_sens_maps(a.sens_maps, a.sens_phase, a.num_sens, H, W, a.seed)
    if trajectory is not None:
        # radial cine: a framed operator, the samples (n, B, T, 1, M), L2PenaltyCG
        from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.noncartesian import NonCartesianSENSE
        from inverseproblemwithdiffusionmodel_amd.synthetic import complex_coil_maps
        if sens_maps is None:
            sens_maps = complex_coil_maps(a.num_sens, H, W, a.seed)
        op = NonCartesianSENSE(trajectory, (1, H, W), sens_maps=sens_maps)
        M = op.n_samples
        frames, kspace_scale, cal = None, None, None
        if nc_kspace is None:
            base = phantom_image(H, W, seed=a.seed).to(device)
            beat = torch.cos(torch.arange(a.T, device=device) * (2 * torch.pi / a.T)).view(a.T, 1, 1, 1)
            frames = base * (1.0 + 0.1 * beat)                             # (T, 1, H, W): a slowly pulsating phantom
            y = op(frames.to(torch.complex64))                             # (n, T, 1, M): frame t on trajectory t
        else:
            y = nc_kspace.to(device).reshape(a.num_sens, a.T, 1, M)
        if self_cal is not None:               # simulated with the true maps (or measured), reconstructed with the estimated ones
            cal = NonCartesianSENSE.from_measurement(y.reshape(a.num_sens, a.T, M), trajectory, (1, H, W),
                                                     n_virtual=self_cal.virtual_coils, noise_cov=self_cal.noise_cov,
                                                     method=self_cal.maps_method, calib_max=self_cal.calib_max,
                                                     **self_cal.maps_kwargs)
            op, a.num_sens = cal.op, cal.op.num_sens
            y = cal.measurement.reshape(a.num_sens, a.T, 1, M)
        if nc_kspace is not None:
            kspace_scale = float(a.kspace_scale) if a.kspace_scale != "auto" else None
            if kspace_scale is None:                                       # 1 / peak |zero_filled(y)| over all frames
                peak = float(op.zero_filled(y).abs().max())
                if not peak > 0:
                    sys.exit("--kspace: the measurement holds no signal")
                kspace_scale = 1.0 / peak
            y = y * kspace_scale
        zf = op.zero_filled(y)                                             # (T, 1, H, W)
        meas = y.reshape(a.num_sens, 1, a.T, 1, M).repeat(1, n_local, 1, 1, 1)
        params = dict(n_steps_each=a.num_steps_each, step_lr=a.step_lr, denoise=False, final_only=True)
        sampler = ALD2DTime(get_proximal("L2PenaltyCG")(op, max_iter=a.cg_iters, tol=a.cg_tol), scorenet_T, sigmas_T,
                            (n_local, a.T, 1, H, W), scorenet, sigmas, params, scorenet.config, meas, op, device=device)
        t0 = time.time()
        out = sampler(save_dir=a.save_dir, lr_scaled=a.lr_scaled, mode_T=a.mode_T, lamda_T=a.lamda_T,
                      if_random_shift=a.if_random_shift, seed=a.seed, sample_offset=lo, n_levels=a.n_levels,
                      start_level=a.start_level, verbose=True)[0][: hi - lo]
        torch.cuda.synchronize()
        print(f"reconstruction time: {time.time() - t0}")
        if kspace_scale is not None:
            print(f"k-space scale = {kspace_scale!r}")
        os.makedirs(a.save_dir, exist_ok=True)
        torch.save(out.cpu(), os.path.join(a.save_dir, "reconstructions.pt"))
        if frames is not None:                                             # measured data: no ground truth
            torch.save(frames.cpu(), os.path.join(a.save_dir, "original.pt"))
        torch.save(op.trajectory, os.path.join(a.save_dir, "trajectory.pt"))
        torch.save(zf.cpu(), os.path.join(a.save_dir, "ZF.pt"))
        torch.save(y.cpu(), os.path.join(a.save_dir, "measurement.pt"))
        torch.save(op.sens_maps, os.path.join(a.save_dir, "sens_maps.pt"))
        if cal is not None:
            torch.save(cal.calib_kspace.cpu(), os.path.join(a.save_dir, "calib_kspace.pt"))
            if cal.coil_matrix is not None:
                torch.save(cal.coil_matrix, os.path.join(a.save_dir, "coil_matrix.pt"))
            if cal.eigval is not None:
                torch.save(cal.eigval, os.path.join(a.save_dir, "espirit_eigval.pt"))
        if a.num_samples > 1:
            flat = out.to(device).reshape(out.shape[0], -1, H, W)
            torch.save({k: v.cpu() for k, v in sharding.all_reduce_posterior(flat, a.num_samples).items()},
                       os.path.join(a.save_dir, "posterior.pt"))
        with open(os.path.join(a.save_dir, "args_dict.pkl"), "wb") as wf:
            pickle.dump(vars(a), wf)
        sys.exit(0)
    op = SENSE(a.sens_type, a.num_sens, a.R, a.center_lines_frac, (1, H, W), a.seed, mask_T=24 if a.T == 24 else 1)
    if sens_maps is not None:
        op.sens_maps = sens_maps
    mask = driver_mask(a.mask, a.mask_2d, H, W, a.R, a.seed)
    if mask is not None:
        op.random_under_fourier.mask = mask
    frames, cal = None, None
    if checked is None or checked.kspace is None:
        base = phantom_image(H, W, seed=a.seed).to(device)
        beat = torch.cos(torch.arange(a.T, device=device) * (2 * torch.pi / a.T)).view(a.T, 1, 1, 1)
        frames = base * (1.0 + 0.1 * beat)                                 # (T, 1, H, W): a slowly pulsating phantom
    if checked is None:
        meas = op(frames).reshape(a.num_sens, 1, a.T, 1, H, W).repeat(1, n_local, 1, 1, 1, 1)
    else:                                     # simulated with the true maps (or measured), reconstructed with the estimated ones
        cal, op = load_data.driver_cine_measurement(a, checked, op, frames, device)
        a.num_sens = op.num_sens
        meas = cal.measurement.reshape(a.num_sens, 1, a.T, 1, H, W).repeat(1, n_local, 1, 1, 1, 1)
    params = dict(n_steps_each=a.num_steps_each, step_lr=a.step_lr, denoise=False, final_only=True)
    prox_kw = dict(max_iter=a.cg_iters, tol=a.cg_tol) if a.proximal_type == "L2PenaltyCG" else {}
    sampler = ALD2DTime(get_proximal(a.proximal_type)(op, **prox_kw), scorenet_T, sigmas_T, (n_local, a.T, 1, H, W), scorenet,
                        sigmas, params, scorenet.config, meas, op, device=device)
    t0 = time.time()
    out = sampler(save_dir=a.save_dir, lr_scaled=a.lr_scaled, mode_T=a.mode_T, lamda_T=a.lamda_T,
                  if_random_shift=a.if_random_shift, seed=a.seed, sample_offset=lo, n_levels=a.n_levels, start_level=a.start_level,
                  verbose=(rank == 0))[0][: hi - lo]
    torch.cuda.synchronize()
    if rank == 0:
        print(f"reconstruction time: {time.time() - t0}")
        if cal is not None and cal.kspace_scale is not None:
            print(f"k-space scale = {cal.kspace_scale!r}")
    B, T = out.shape[:2]
    flat = out.to(device).reshape(out.shape[0], -1, H, W)                  # (n_local, T, H, W): frames as "channels"
    post = sharding.all_reduce_posterior(flat, a.num_samples) if a.num_samples > 1 else None
    out = sharding.gather_samples(out.to(device), a.num_samples, world, rank).cpu()
    if rank == 0:
        os.makedirs(a.save_dir, exist_ok=True)
        torch.save(out, os.path.join(a.save_dir, "reconstructions.pt"))
        if frames is not None:                                             # measured data: no ground truth
            torch.save(frames.cpu(), os.path.join(a.save_dir, "original.pt"))
        torch.save(op.random_under_fourier.mask, os.path.join(a.save_dir, "mask.pt"))
        if sens_maps is not None or cal is not None:
            torch.save(op.sens_maps, os.path.join(a.save_dir, "sens_maps.pt"))
        if cal is not None:
            torch.save(cal.measurement.cpu(), os.path.join(a.save_dir, "measurement.pt"))
            if cal.coil_matrix is not None:
                torch.save(cal.coil_matrix, os.path.join(a.save_dir, "coil_matrix.pt"))
            if cal.eigval is not None:
                torch.save(cal.eigval, os.path.join(a.save_dir, "espirit_eigval.pt"))
        if post is not None:
            torch.save({k: v.cpu() for k, v in post.items()}, os.path.join(a.save_dir, "posterior.pt"))
        with open(os.path.join(a.save_dir, "args_dict.pkl"), "wb") as wf:
            pickle.dump(vars(a), wf)
    if world > 1:
        sharding.barrier(last=True)
        torch.distributed.destroy_process_group()
