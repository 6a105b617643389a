#!/usr/bin/env python3
"""Multi-coil reconstruction by predictor-corrector sampling with the NCSN++ VE-SDE score network and a data-consistency
step after every predictor and corrector update (sde/inverse.py; Song et al. ICLR 2022, Chung & Ye MedIA 2022).  The
problem flags are those of acdc_SENSE_real_img.py that engine.build_problem serves (synthetic phantom and coil maps, or
--kspace PATH --mask PATH --estimate_maps for measured k-space; --coil_compress N; --n_slices S for a stack in one
batch), the sampling flags those of ncsnpp_pc_sampling.py, plus --dc / --dc_weight / --cg_iters / --cg_tol.  NCSN++ runs
with one channel on the [real | imag] rows; weights: --ckpt (a state dict) or seeded synthetic.  Under torchrun the
--num_samples samples are block-partitioned over the ranks; the Langevin step is per sample and the noise keyed by the
global sample id, so the result does not depend on the number of ranks (no all-reduce).
Writes reconstructions.pt, measurement.pt, sens_maps.pt (and original.pt with the RMSE line when a ground truth exists)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=8, help="acceleration of the generated mask: 8, 16, 20 or 40")
    ap.add_argument("--image_size", type=int, default=128, help="image height (and width, without --image_width)")
    ap.add_argument("--image_width", type=int, default=None)
    ap.add_argument("--num_sens", type=int, default=4)
    ap.add_argument("--mask", default=None, help=".npy / .pt sampling mask: a line mask (..., W) or a 2-D mask (..., H, W)")
    ap.add_argument("--mask_2d", action="store_true", help="synthetic variable-density 2-D mask at --R")
    ap.add_argument("--kspace", default=None, help=".npy / .pt measured k-space (n_coils, H, W); needs --mask and --estimate_maps")
    ap.add_argument("--estimate_maps", action="store_true", help="coil maps from the measurement's calibration region")
    ap.add_argument("--coil_compress", type=int, default=None, metavar="N", help="compress to N virtual coils (PCA)")
    ap.add_argument("--n_slices", type=int, default=None, metavar="S", help="simulate a stack of S slices in one batch")
    ap.add_argument("--num_samples", type=int, default=1, help="samples (per slice, with --n_slices)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save_dir", default="../outputs")
    ap.add_argument("--snr", type=float, default=None, help="default: config.sampling.snr")
    ap.add_argument("--n_steps_each", type=int, default=None, help="corrector steps per level (default: config)")
    ap.add_argument("--predictor", default=None)
    ap.add_argument("--corrector", default=None)
    ap.add_argument("--n_iters", type=int, default=None, help="run only the first n of the config's num_scales levels")
    ap.add_argument("--tiny", action="store_true", help="a 20-level, nf-16 network (tests)")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--dc", default=None, choices=["gradient", "cg"], help="data consistency (default: gradient)")
    ap.add_argument("--dc_weight", type=float, default=1.0)
    ap.add_argument("--cg_iters", type=int, default=10)
    ap.add_argument("--cg_tol", type=float, default=1e-5)
    a = ap.parse_args()

    H = a.image_size
    W = a.image_width if a.image_width is not None else H
    stack = a.n_slices is not None
    if stack and (a.kspace or a.n_slices < 1):
        sys.exit("--n_slices S (>= 1) simulates a stack; it does not go with --kspace")
    if stack and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("--n_slices: a stack of slices runs in one process")
    kspace = None
    if a.kspace:
        if not a.mask or not a.estimate_maps:
            sys.exit("--kspace PATH needs --mask PATH and --estimate_maps")
        from inverseproblemwithdiffusionmodel_amd.helpers.load_data import load_kspace
        try:
            kspace = load_kspace(a.kspace, slices=False)
        except ValueError as e:
            sys.exit(str(e))
        a.num_sens, H, W = (int(s) for s in kspace.shape[-3:])
    # the k-space size, the mask and the calibration region, before the network is built or a GPU is touched
    from inverseproblemwithdiffusionmodel_amd import ops
    if ops.kspace_size_class(H, W) == ops.KSPACE_NONE:
        sys.exit(f"--image_size {H} --image_width {W}: no k-space kernel for {H}x{W}; {ops.KSPACE_SIZE_RULE}")
    from inverseproblemwithdiffusionmodel_amd.helpers.load_data import driver_mask
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms import undersampling_fourier as uf
    mask = driver_mask(a.mask, a.mask_2d, H, W, a.R, a.seed)
    try:
        if a.coil_compress is not None:
            ops._coilcomp_counts(a.num_sens, a.coil_compress, "--coil_compress")
        if a.estimate_maps or a.coil_compress is not None or kspace is not None:
            uf.calibration_region(mask if mask is not None else uf.RandomUndersamplingFourier(a.R, 0.04, (1, H, W), a.seed).mask,
                                  H, W, 12)
    except (ValueError, TypeError, NotImplementedError) as e:
        sys.exit(f"--estimate_maps / --coil_compress / --kspace: {e}")

    from inverseproblemwithdiffusionmodel_amd import engine, sharding
    from inverseproblemwithdiffusionmodel_amd.configs import ve_ncsnpp
    from inverseproblemwithdiffusionmodel_amd.models import ncsnpp
    from inverseproblemwithdiffusionmodel_amd.sde import sde_lib
    from inverseproblemwithdiffusionmodel_amd.synthetic import synth_state_dict
    world, rank, device = sharding.init_distributed()
    cfg = ve_ncsnpp.get_config()
    cfg.device = device
    if a.tiny:
        cfg.model.nf, cfg.model.ch_mult, cfg.model.num_res_blocks, cfg.model.attn_resolutions = 16, (1, 2, 2), 1, (8,)
        cfg.model.num_scales = 20
    cfg.data.image_size, cfg.data.num_channels = H, 1
    for k in ("snr", "n_steps_each", "predictor", "corrector"):
        if getattr(a, k) is not None:
            setattr(cfg.sampling, k, getattr(a, k))
    net = ncsnpp.NCSNpp(cfg)
    if a.ckpt:
        net.load_state_dict(torch.load(a.ckpt, map_location="cpu"))
    else:
        net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=a.seed), strict=False)
    net = net.to(device).eval()
    sde = sde_lib.VESDE(cfg.model.sigma_min, cfg.model.sigma_max, cfg.model.num_scales)

    total = a.num_samples
    lo, hi = sharding.shard_range(total, world, rank)
    n_local = max(hi - lo, 1)                 # a rank without samples still runs one (discarded)
    prob = engine.build_problem(device, n_local, R=a.R, H=H, W=W, num_sens=a.num_sens, seed=a.seed, scorenet=net,
                                cfg=engine.acdc_config(device, H), mask=mask, estimate_maps=a.estimate_maps, measurement=kspace,
                                coil_compress=a.coil_compress, n_slices=a.n_slices)
    S = prob.n_slices if stack else 1
    sampler = engine.build_pc_sampler(prob, sde, predictor=cfg.sampling.predictor, corrector=cfg.sampling.corrector,
                                      snr=cfg.sampling.snr, n_steps=cfg.sampling.n_steps_each, dc=a.dc, dc_weight=a.dc_weight,
                                      cg_iters=a.cg_iters, cg_tol=a.cg_tol, continuous=cfg.training.continuous,
                                      denoise=cfg.sampling.noise_removal, device=device)
    t0 = time.time()
    x, nfe = sampler(net, n_iters=a.n_iters, seed=a.seed, sample_offset=lo * S)
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    x = x[: (hi - lo) * S].contiguous()
    if not stack:
        x = sharding.gather_samples(x, total, world, rank)
    x = x.cpu()
    if rank == 0:
        n_it = cfg.model.num_scales if a.n_iters is None else a.n_iters
        print(f"reconstruction time: {elapsed:.1f} s for {total} sample(s) on {world} GPU(s), {n_it} predictor-corrector "
              f"levels, {nfe} score evaluations, dc = {sampler.dc}")
        os.makedirs(a.save_dir, exist_ok=True)
        resid = prob.op(x[:S].to(device)) - prob.measurement[:, :S]
        l2 = torch.sum(torch.abs(resid) ** 2).item()
        if prob.image is None:
            print(f"data error ||A x - y||^2 = {l2:.4e}")
        else:
            err = torch.sqrt(torch.mean(torch.abs(x[:S].to(device) - prob.image) ** 2)).item()
            print(f"data error ||A x - y||^2 = {l2:.4e}; reconstruction error (RMSE vs phantom) = {err:.4e}")
            torch.save(prob.image.cpu(), os.path.join(a.save_dir, "original.pt"))
        torch.save(x, os.path.join(a.save_dir, "reconstructions.pt"))
        torch.save(prob.measurement[:, :S].cpu(), os.path.join(a.save_dir, "measurement.pt"))
        torch.save(prob.op.sens_maps, os.path.join(a.save_dir, "sens_maps.pt"))
    if world > 1:
        sharding.barrier(last=True)
        torch.distributed.destroy_process_group()
