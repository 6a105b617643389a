#!/usr/bin/env python3
"""Multi-coil ALD reconstruction on synthetic k-space -- the MI355X counterpart of the reference's
``scripts/acdc_SENSE_real_img.py`` with the same flags and output artefacts (original.pt, measurement.pt,
reconstructions.pt, ZF.pt, mask.pt, args_dict.pkl).  Data and weights are synthetic (phantom + seeded weights)
unless --ckpt points at a Lightning checkpoint of the reference and --kspace at measured multi-coil k-space (with its
--mask; no ground truth then: original.pt and the RMSE line are skipped); --estimate_maps takes the coil maps from the
measurement's own calibration region (sens_maps.pt); --coil_compress N whitens (--noise_cov PATH) and compresses the
measurement to N virtual coils first (coil_matrix.pt; --coil_compress_mode geometric: one matrix per readout position).
Samples are sharded over the launched ranks (torchrun) and rank 0 writes the posterior mean / std next to the reconstructions.
A stack of slices in ONE batch: --n_slices S simulates S slices (phantom seeds seed .. seed + S - 1, coil maps per slice),
--kspace PATH --slices reads a measured stack (S, n_coils, H, W).  --num_samples then counts samples PER SLICE: the batch
axis of reconstructions.pt has num_samples * S rows in the order sample * S + slice, sens_maps.pt is (S, n, H, W), and
posterior_slices.pt holds the per-slice mean / std over the rows b % S == s.  One process only (no sharded volumes).
Non-Cartesian sampling: --trajectory radial --spokes N [--readout M] simulates a golden-angle radial acquisition of the
phantom, --trajectory PATH one on the (M, 2) positions of a file, --kspace PATH --trajectory PATH --sens_maps PATH
reconstructs measured samples (n_coils, M).  The proximal is then L2PenaltyCG; trajectory.pt is written instead of
mask.pt and ZF.pt is the density-compensated adjoint.  --self_calibrate takes the coil maps from the non-Cartesian samples
themselves ([--virtual_coils N] [--noise_cov PATH] [--calib_max N] [--maps_method walsh|espirit]), so that
--kspace PATH --trajectory PATH --self_calibrate needs no --sens_maps; sens_maps.pt, calib_kspace.pt and (with
--virtual_coils) coil_matrix.pt are written."""
import argparse
import os
import pickle
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROXIMAL_NAMES = ["L2Penalty", "Constrained", "SingleCoil", "L2PenaltyCG"]     # get_proximal's names

if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument("--R", type=int, default=40)
    parser.add_argument("--center_lines_frac", type=float, default=1 / 4)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--seg_start_time", type=float, default=0.)      # the reference's default: guidance ramps in from level 0
    parser.add_argument("--seg_step_type", default="linear")
    parser.add_argument("--lamda", type=float, default=0.1)
    parser.add_argument("--step_lr", type=float, default=0.0000009)
    parser.add_argument("--num_steps_each", type=int, default=3)
    parser.add_argument("--lr_scaled", type=float, default=1.)
    parser.add_argument("--proximal_type", default=None, choices=PROXIMAL_NAMES,
                        help="data-consistency operator (default L2Penalty; with --trajectory: L2PenaltyCG, the only one); "
                             "L2PenaltyCG: the exact multi-coil proximal by conjugate gradients")
    parser.add_argument("--cg_iters", type=int, default=10, help="L2PenaltyCG: CG iterations at most")
    parser.add_argument("--cg_tol", type=float, default=1e-5, help="L2PenaltyCG: stop at |r| <= cg_tol |b|")
    parser.add_argument("--num_samples", type=int, default=1)
    parser.add_argument("--sens_type", default="exp")
    parser.add_argument("--num_sens", type=int, default=4)
    parser.add_argument("--seg_mode", choices=["full", "FG"], default="full")
    parser.add_argument("--seg_fraction", type=float, default=1.)
    parser.add_argument("--ds_idx", type=int, default=0)
    parser.add_argument("--save_dir", default="../outputs")
    # extras
    parser.add_argument("--image_size", type=int, default=128, help="image height (and width, without --image_width)")
    parser.add_argument("--image_width", type=int, default=None,
                        help="image width (default: --image_size); sides: powers of two, or multiples of 16 of the form "
                             "2^a 3^b 5^c up to 2048, e.g. 96, 144, 160, 192, 240, 288, 320, 384")
    parser.add_argument("--ckpt", default=None, help="Lightning .ckpt of the reference (EMA weights); default: synthetic")
    parser.add_argument("--n_levels", type=int, default=None, help="run only the first n noise levels")
    parser.add_argument("--seg_ckpt", default=None, help="Lightning TrainSeg .ckpt (MONAI UNet weights) for the guidance")
    parser.add_argument("--sens_maps", default=None,
                        help=".npy / .pt file with measured coil maps (num_sens, H, W), real or complex")
    parser.add_argument("--sens_phase", action="store_true",
                        help="synthetic COMPLEX coil maps: the exp magnitudes times a smooth seeded phase")
    parser.add_argument("--mask", default=None,
                        help=".npy / .pt file with the sampling mask: a line mask (..., W) or a 2-D mask (..., H, W)")
    parser.add_argument("--mask_2d", action="store_true",
                        help="synthetic variable-density 2-D (ky, kz) sampling mask at --R instead of the line mask")
    parser.add_argument("--kspace", default=None,
                        help=".npy / .pt file with measured multi-coil k-space (n_coils, H, W), complex, centred with "
                             "orthonormal scale; needs --mask PATH and either --sens_maps PATH or --estimate_maps")
    parser.add_argument("--slices", action="store_true",
                        help="--kspace holds a stack of slices (S, n_coils, H, W), reconstructed in one batch with coil maps "
                             "per slice; --num_samples counts samples per slice")
    parser.add_argument("--n_slices", type=int, default=None, metavar="S",
                        help="simulate a stack of S slices (phantom seed + s, coil maps per slice) in one batch")
    parser.add_argument("--estimate_maps", action="store_true",
                        help="estimate the coil maps from the fully sampled calibration region of the measurement")
    parser.add_argument("--calib_max", type=int, default=12, help="--estimate_maps: largest calibration half-width")
    parser.add_argument("--coil_compress", type=int, default=None, metavar="N",
                        help="whiten and compress the measurement (up to 64 coils) to N <= 32 virtual coils by PCA of its "
                             "calibration region; the maps are estimated on, or compressed to, the virtual coils")
    parser.add_argument("--coil_compress_mode", choices=["pca", "geometric"], default="pca",
                        help="--coil_compress: pca: one matrix per image; geometric: one per readout position (the readout "
                             "axis H must be fully sampled, as with every line mask), aligned along the readout")
    parser.add_argument("--coil_compress_window", type=int, default=2, metavar="K",
                        help="--coil_compress_mode geometric: readout positions on either side of a position (0..8)")
    parser.add_argument("--noise_cov", default=None,
                        help="--coil_compress: .npy / .pt file with the (n_coils, n_coils) coil noise covariance of the prescan")
    parser.add_argument("--kspace_scale", default="auto",
                        help="--kspace: factor on the measurement; auto: 1 / the peak of its calibration image")
    from inverseproblemwithdiffusionmodel_amd.helpers.load_data import (add_maps_method_args, add_self_calibrate_args,
                                                                         driver_maps_method, driver_self_calibrate)
    add_maps_method_args(parser)
    add_self_calibrate_args(parser)
    parser.add_argument("--trajectory", default=None, metavar="radial|PATH",
                        help="non-Cartesian sampling: 'radial' (golden-angle spokes, --spokes / --readout) or a .npy / .pt file "
                             "with (M, 2) positions (k_y, k_x) in cycles per field of view; implies --proximal_type L2PenaltyCG")
    parser.add_argument("--spokes", type=int, default=None, metavar="N", help="--trajectory radial: number of spokes")
    parser.add_argument("--readout", type=int, default=None, metavar="M",
                        help="--trajectory radial: samples per spoke (default: 2 x the larger image side)")
    parser.add_argument("--seg_synthetic", action="store_true",
                        help="run the guidance with seeded random UNet weights (exercises the path; not meaningful imaging)")
    args_dict = vars(parser.parse_args())
    if args_dict["seg_start_time"] < 1. and not (args_dict["seg_ckpt"] or args_dict["seg_synthetic"]):
        print("no --seg_ckpt: segmentation-likelihood guidance needs trained UNet weights -> running with seg_start_time = 1 "
              "(guidance off); pass --seg_synthetic to exercise the path with random weights")
        args_dict["seg_start_time"] = 1.

    stack = args_dict["slices"] or args_dict["n_slices"] is not None
    if args_dict["slices"] and not args_dict["kspace"]:
        sys.exit("--slices goes with --kspace PATH, a measured stack (S, n_coils, H, W); --n_slices S simulates one")
    if args_dict["n_slices"] is not None and (args_dict["kspace"] or args_dict["n_slices"] < 1):
        sys.exit("--n_slices S (>= 1) simulates a stack; a measured one is --kspace PATH --slices")
    if stack and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("--slices / --n_slices: a stack of slices runs in one process; sharding a volume over ranks is not built")
    if stack and args_dict["seg_start_time"] < 1.:
        sys.exit("--slices / --n_slices: segmentation-likelihood guidance is per image; run with --seg_start_time 1")
    if stack and args_dict["sens_phase"]:
        sys.exit("--slices / --n_slices: --sens_phase builds one map set; pass --sens_maps PATH or leave the per-slice maps")
    H = args_dict["image_size"]
    W = args_dict["image_width"] if args_dict["image_width"] is not None else H
    kspace = None
    trajectory = None
    self_cal = None
    if not args_dict["trajectory"]:
        driver_self_calibrate(args_dict, None, H, W, args_dict["num_sens"])       # the flags alone: they go with --trajectory
    if args_dict["trajectory"]:                                           # every refusal before the network is built
        if args_dict["proximal_type"] not in (None, "L2PenaltyCG"):
            sys.exit(f"--trajectory: non-Cartesian SENSE takes --proximal_type L2PenaltyCG, not {args_dict['proximal_type']}")
        args_dict["proximal_type"] = "L2PenaltyCG"
        for flag in ("mask", "mask_2d", "estimate_maps", "coil_compress", "noise_cov", "slices", "n_slices"):
            if args_dict[flag] not in (None, False) and not (flag == "noise_cov" and args_dict["self_calibrate"]):
                sys.exit(f"--trajectory does not go with --{flag}: non-Cartesian SENSE takes given coil maps, one slice and no "
                         "sampling mask")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("--trajectory: one process (sharded non-Cartesian runs are not built)")
        from inverseproblemwithdiffusionmodel_amd import ops
        from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_kspace, load_trajectory
        from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.noncartesian import check_trajectory
        from inverseproblemwithdiffusionmodel_amd.synthetic import radial_trajectory
        if not ops.nc_supported(H, W):
            sys.exit(f"--image_size {H} --image_width {W}: no non-Cartesian kernel for {H}x{W}; {ops.NC_SIZE_RULE}")
        try:
            if args_dict["trajectory"] == "radial":
                if args_dict["spokes"] is None or args_dict["spokes"] < 1:
                    sys.exit("--trajectory radial needs --spokes N (>= 1)")
                if args_dict["kspace"]:
                    sys.exit("--kspace PATH needs --trajectory PATH, the positions of its samples")
                readout = args_dict["readout"] if args_dict["readout"] is not None else 2 * max(H, W)
                trajectory = radial_trajectory(args_dict["spokes"], readout, H, W)
            else:
                if args_dict["spokes"] is not None or args_dict["readout"] is not None:
                    sys.exit("--spokes / --readout go with --trajectory radial")
                trajectory = load_trajectory(args_dict["trajectory"])
            trajectory = check_trajectory(trajectory, H, W, "--trajectory")
            if args_dict["kspace"]:
                if not args_dict["self_calibrate"] and (not args_dict["sens_maps"] or args_dict["sens_phase"]):
                    sys.exit("--kspace PATH --trajectory PATH needs --sens_maps PATH, or --self_calibrate to estimate the maps "
                             "from the samples")
                kspace = load_kspace(args_dict["kspace"], noncartesian=True)
                if kspace.shape[1] != trajectory.shape[0]:
                    sys.exit(f"--kspace holds {tuple(kspace.shape)}; (n_coils, {trajectory.shape[0]}) expected for this trajectory")
                args_dict["num_sens"] = int(kspace.shape[0])
        except (ValueError, TypeError) as e:
            sys.exit(str(e))
        self_cal = driver_self_calibrate(args_dict, trajectory, H, W, args_dict["num_sens"])     # the window, before the network
    elif args_dict["spokes"] is not None or args_dict["readout"] is not None:
        sys.exit("--spokes / --readout go with --trajectory radial")
    if args_dict["proximal_type"] is None:
        args_dict["proximal_type"] = "L2Penalty"
    if args_dict["kspace"] and trajectory is None:
        if not args_dict["mask"]:
            sys.exit("--kspace PATH needs --mask PATH, the sampling mask of the acquisition")
        if bool(args_dict["sens_maps"]) == args_dict["estimate_maps"] or args_dict["sens_phase"]:
            sys.exit("--kspace PATH takes its coil maps from --sens_maps PATH or from --estimate_maps (one of them)")
        from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_kspace
        try:
            kspace = load_kspace(args_dict["kspace"], slices=args_dict["slices"])
        except ValueError as e:
            sys.exit(str(e))
        args_dict["num_sens"], H, W = (int(s) for s in kspace.shape[-3:])
        if args_dict["slices"]:
            args_dict["n_slices"] = int(kspace.shape[0])
    if stack and args_dict["sens_maps"]:                                  # a stack's shapes are settled before anything is built
        from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_sens_maps
        try:
            shape = tuple(load_sens_maps(args_dict["sens_maps"]).shape)
        except (ValueError, TypeError) as e:
            sys.exit(str(e))
        if shape[1:] != (H, W) or (kspace is not None and shape[0] != args_dict["num_sens"]):
            sys.exit(f"--sens_maps holds {shape}; the stack needs ({args_dict['num_sens'] if kspace is not None else 'n_coils'}, "
                     f"{H}, {W}), shared by its slices")
    kspace_scale = None if args_dict["kspace_scale"] == "auto" else float(args_dict["kspace_scale"])
    from inverseproblemwithdiffusionmodel_amd import ops
    if trajectory is None and ops.kspace_size_class(H, W) == ops.KSPACE_NONE:     # before any allocation
        sys.exit(f"--image_size {H} --image_width {W}: no k-space kernel for {H}x{W}; {ops.KSPACE_SIZE_RULE}")
    # the mask, and the calibration region the run depends on, before the score network is built or a GPU is touched
    from inverseproblemwithdiffusionmodel_amd.helpers.load_data import driver_mask
    mask = None if trajectory is not None else driver_mask(args_dict["mask"], args_dict["mask_2d"], H, W, args_dict["R"],
                                                           args_dict["seed"])
    noise_cov = region = None
    if args_dict["noise_cov"] and args_dict["coil_compress"] is None and self_cal is None:
        sys.exit("--noise_cov PATH goes with --coil_compress N (whitening is part of the compression)")
    if args_dict["coil_compress"] is not None:                            # a bad N or a bad covariance fails here
        from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_noise_cov
        try:
            ops._coilcomp_counts(args_dict["num_sens"], args_dict["coil_compress"], "--coil_compress")
            if args_dict["noise_cov"]:
                noise_cov = ops.check_noise_cov(load_noise_cov(args_dict["noise_cov"]), args_dict["num_sens"], "--noise_cov")
        except (ValueError, TypeError, NotImplementedError) as e:
            sys.exit(str(e))
    if trajectory is None and (args_dict["estimate_maps"] or args_dict["coil_compress"] is not None
                               or (kspace is not None and kspace_scale is None)):
        from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
        try:
            region = uf.calibration_region(mask if mask is not None else
                                  uf.RandomUndersamplingFourier(args_dict["R"], 0.04, (1, H, W), args_dict["seed"]).mask,
                                  H, W, args_dict["calib_max"])
        except ValueError as e:
            sys.exit(f"--estimate_maps / --coil_compress / --kspace: {e}")
    geometric = args_dict["coil_compress_mode"] == "geometric"
    if geometric and args_dict["coil_compress"] is None:
        sys.exit("--coil_compress_mode geometric goes with --coil_compress N")
    if geometric:                                                         # refused here, before the score network is built
        try:
            uf.geometric_compression_check(mask if mask is not None else
                                           uf.RandomUndersamplingFourier(args_dict["R"], 0.04, (1, H, W), args_dict["seed"]).mask,
                                           args_dict["num_sens"], args_dict["coil_compress"], H, W, args_dict["calib_max"],
                                           args_dict["coil_compress_window"], "--coil_compress_mode geometric")
        except (ValueError, NotImplementedError) as e:
            sys.exit(str(e))
    if self_cal is not None:
        maps_method, maps_kwargs, noise_cov = self_cal.maps_method, self_cal.maps_kwargs, self_cal.noise_cov
    else:
        maps_method, maps_kwargs = driver_maps_method(
            args_dict, args_dict["estimate_maps"],
            args_dict["num_sens"] if args_dict["coil_compress"] is None else args_dict["coil_compress"], H, W, region)
    from inverseproblemwithdiffusionmodel_amd import engine, sharding
    world, rank, device = sharding.init_distributed()
    from inverseproblemwithdiffusionmodel_amd.helpers.load_model import load_scorenet_weights

    total = args_dict["num_samples"]
    lo, hi = sharding.shard_range(total, world, rank)
    n_local = max(hi - lo, 1)                 # a rank without samples still runs one (discarded) to keep collectives aligned
    cfg = engine.acdc_config(device, H)
    cfg.sampling.step_lr, cfg.sampling.n_steps_each = args_dict["step_lr"], args_dict["num_steps_each"]
    scorenet = engine.build_scorenet(cfg, args_dict["seed"])
    if args_dict["ckpt"]:
        load_scorenet_weights(scorenet, args_dict["ckpt"])
    sens_maps = None
    if args_dict["sens_maps"]:
        from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_sens_maps
        sens_maps = load_sens_maps(args_dict["sens_maps"])
        args_dict["num_sens"] = sens_maps.shape[0]
    elif args_dict["sens_phase"]:
        from inverseproblemwithdiffusionmodel_amd.synthetic import complex_coil_maps
        sens_maps = complex_coil_maps(args_dict["num_sens"], H, W, args_dict["seed"])
    prob = engine.build_problem(device, n_local, R=args_dict["R"], H=H, W=W, num_sens=args_dict["num_sens"],
                                seed=args_dict["seed"], scorenet=scorenet, cfg=cfg, lr_scaled=args_dict["lr_scaled"],
                                sens_maps=sens_maps, mask=mask, estimate_maps=args_dict["estimate_maps"], measurement=kspace,
                                calib_max=args_dict["calib_max"], kspace_scale=kspace_scale,
                                coil_compress=args_dict["coil_compress"], noise_cov=noise_cov,
                                coil_compress_mode=args_dict["coil_compress_mode"],
                                coil_compress_window=args_dict["coil_compress_window"],
                                n_slices=None if kspace is not None else args_dict["n_slices"],
                                maps_method=maps_method, maps_kwargs=maps_kwargs,
                                proximal=args_dict["proximal_type"],
                                proximal_kwargs=(dict(max_iter=args_dict["cg_iters"], tol=args_dict["cg_tol"])
                                                 if args_dict["proximal_type"] == "L2PenaltyCG" else None),
                                trajectory=trajectory, self_calibrate=self_cal is not None,
                                virtual_coils=args_dict["virtual_coils"])
    label = None
    if args_dict["seg_start_time"] < 1.:
        from inverseproblemwithdiffusionmodel_amd.helpers.load_model import reload_model
        from inverseproblemwithdiffusionmodel_amd.helpers.utils import undersample_seg_mask
        from inverseproblemwithdiffusionmodel_amd.ncsn.models.ALD_optimizers import ALDInvSegProximalRealImag
        seg = reload_model("Seg", "ACDC", ckpt_path=args_dict["seg_ckpt"], device=device)
        if prob.image is None:
            sys.exit("--kspace: the synthetic segmentation label needs the phantom; run with --seg_start_time 1")
        label = (prob.image.abs() > 0.5).long()                       # synthetic stand-in for the myocardium label
        label = undersample_seg_mask(label, args_dict["seg_fraction"], seed=args_dict["seed"])
        s0 = prob.sampler
        prob.sampler = ALDInvSegProximalRealImag(s0.proximal, args_dict["seg_start_time"], args_dict["seg_step_type"],
                                                 s0.x_mod_shape, s0.scorenet, s0.sigmas, s0.params, s0.config, s0.measurement,
                                                 s0.linear_tfm, seg=seg, device=device)
    save_dir = args_dict["save_dir"]
    if rank == 0:
        os.makedirs(save_dir, exist_ok=True)
    S = prob.n_slices if stack else 1                                 # rows of one sample: its slices, in order
    # non-Cartesian: the density-compensated adjoint (the plain adjoint of radial data is a blur)
    direct_recons = prob.zero_filled if trajectory is not None else prob.op.conj_op(prob.measurement[:, :S])

    t0 = time.time()
    kw = dict(prob.call_kwargs, label=label, lamda=args_dict["lamda"], save_dir=save_dir, seg_mode=args_dict["seg_mode"],
              seed=args_dict["seed"], sample_offset=lo, n_levels=args_dict["n_levels"], verbose=(rank == 0))
    img_out = prob.sampler(**kw)[0][: (hi - lo) * S]
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    post = post_slices = None
    if stack:                                                         # one process: rows sample * S + slice, all here
        per = [sharding.posterior_from_moments(sharding.moment_planes(img_out[s::S].to(device)), total) for s in range(S)]
        post_slices = {k: torch.stack([p[k] for p in per]).cpu() for k in per[0]}        # each (S, 1, H, W)
        for s in range(S):
            print(f"slice {s}: posterior mean |x| = {post_slices['mag_mean'][s].mean():.4e}, "
                  f"std |x| = {post_slices['mag_std'][s].mean():.4e} over {total} sample(s)")
    else:
        post = sharding.all_reduce_posterior(img_out.to(device), total) if total > 1 else None
        img_out = sharding.gather_samples(img_out.to(device), total, world, rank).cpu()
    if rank == 0:
        resid = prob.op(img_out[:S].to(device)) - prob.measurement[:, :S]
        l2 = torch.sum(torch.abs(resid) ** 2).item()
        print(f"reconstruction time: {elapsed:.1f} s for {total} sample(s) on {world} GPU(s)")
        if prob.kspace_scale is not None:
            print(f"k-space scale = {prob.kspace_scale!r}")
        if prob.image is None:                                        # measured data: no ground truth
            print(f"data error ||A x - y||^2 = {l2:.4e}")
        else:
            err = torch.sqrt(torch.mean(torch.abs(img_out[:S].to(device) - prob.image) ** 2)).item()
            print(f"data error ||A x - y||^2 = {l2:.4e}; reconstruction error (RMSE vs phantom) = {err:.4e}")
            torch.save(prob.image.cpu(), os.path.join(save_dir, "original.pt"))
        torch.save(prob.measurement[:, :S].cpu(), os.path.join(save_dir, "measurement.pt"))
        torch.save(img_out.cpu(), os.path.join(save_dir, "reconstructions.pt"))
        torch.save(direct_recons.cpu(), os.path.join(save_dir, "ZF.pt"))
        if trajectory is not None:
            torch.save(prob.op.trajectory, os.path.join(save_dir, "trajectory.pt"))
        else:
            torch.save(prob.op.random_under_fourier.mask, os.path.join(save_dir, "mask.pt"))
        if sens_maps is not None or prob.estimated_maps or prob.coil_matrix is not None or stack:
            torch.save(prob.op.sens_maps, os.path.join(save_dir, "sens_maps.pt"))
        if prob.coil_matrix is not None:
            torch.save(prob.coil_matrix, os.path.join(save_dir, "coil_matrix.pt"))
        if self_cal is not None:
            torch.save(prob.calib_kspace.cpu(), os.path.join(save_dir, "calib_kspace.pt"))
        if prob.espirit_eigval is not None:
            torch.save(prob.espirit_eigval, os.path.join(save_dir, "espirit_eigval.pt"))
        if post is not None:
            torch.save({k: v.cpu() for k, v in post.items()}, os.path.join(save_dir, "posterior.pt"))
        if post_slices is not None:
            torch.save(post_slices, os.path.join(save_dir, "posterior_slices.pt"))
        with open(os.path.join(save_dir, "args_dict.pkl"), "wb") as wf:
            pickle.dump(args_dict, wf)
    if world > 1:
        dist.destroy_process_group()
