#!/usr/bin/env python3
"""Non-Cartesian SENSE reconstruction, timed: milliseconds per fused Langevin + conjugate-gradient tail
(ops.ald_nc_sense_cg_step, tol = 0 so that every sample runs all cg_iters iterations; device events, after a warm-up) and
per whole ALD iteration (score network + tail, replayed as a hipGraph), at 128x128, 4 coils, B = 14, golden-angle radial
32 spokes x 256, cg_iters = 10.  Two yardsticks with the same settings: the Cartesian tail ops.ald_sense_cg_step at
256x256 (the FFT grid the Toeplitz chain runs on) and at 128x128.  One JSON line.
--frames T: the tail alone with T psf sets, one golden-angle trajectory per frame (--batch a multiple of
T), against the one-set tail on the same operands: each arm captured as a hipGraph, the arms replayed alternately for
--rounds rounds, median and range per arm.  --frames 1 is the one-set spectrum in the sets form, [1, 2H, 2W].

    python scripts/bench_nc_sense.py [--size 128] [--batch 14] [--spokes 32] [--readout 256] [--cg_iters 10] [--tiny]
    python scripts/bench_nc_sense.py --frames 24 --batch 24
--calibrate: the stages of the self-calibration, each timed once -- a report, not a gate.

    python scripts/bench_nc_sense.py --calibrate [--coils 8]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn, n, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def cartesian_tail_ms(ops, size, B, coils, cg_iters, dev):
    """the Cartesian CG tail on a line mask at R = 8, complex maps, tol = 0"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
    from inverseproblemwithdiffusionmodel_amd.synthetic import complex_coil_maps
    op = SENSE("custom", coils, 8, 0.04, (1, size, size), seed=0, sens_maps=complex_coil_maps(coils, size, size, 0))
    x = torch.randn(2 * B, 1, size, size, device=dev)
    g = torch.randn(2 * B, 1, size, size, device=dev)
    y = op(torch.complex(x[:B], x[B:]))
    sens, mask = op.sens_dev(dev), op.mask_u8(dev)
    ahy = ops.sense_adjoint(y, sens, mask, apply_mask=True)
    work = ops.sense_cg_workspace(B, coils, size, size, dev)

    def tail():
        ops.ald_sense_cg_step(x[:B], x[B:], g[:B], g[B:], y, sens, mask, work, step=0.0, noise_scale=0.0, coef=1.0, ahy=ahy,
                              max_iter=cg_iters, tol=0.0)
    return event_ms(tail, 20)


def bench(size, B, coils, spokes, readout, cg_iters, levels, tiny):
    from inverseproblemwithdiffusionmodel_amd import engine, ops
    from inverseproblemwithdiffusionmodel_amd.synthetic import radial_trajectory
    dev = torch.device("cuda")
    cfg = engine.acdc_config(dev, size)
    if tiny:
        cfg.model.ngf = 16
    k = radial_trajectory(spokes, readout, size, size)
    prob = engine.build_problem(dev, B, H=size, W=size, num_sens=coils, seed=0, cfg=cfg, trajectory=k,
                                proximal_kwargs=dict(max_iter=cg_iters, tol=0.0), lr_scaled=1.0 / cfg.sampling.step_lr)
    op = prob.op
    with torch.no_grad():
        t_once = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ahy = op.adjoint_weighted(prob.measurement).contiguous()
        torch.cuda.synchronize()
        t_once["ms_adjoint_once"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        psf = ops.toeplitz_psf(op.traj_dev(dev), size, size)
        torch.cuda.synchronize()
        t_once["ms_psf_once"] = (time.perf_counter() - t0) * 1e3
        x = torch.randn(2 * B, 1, size, size, device=dev)
        g = torch.randn(2 * B, 1, size, size, device=dev)
        sens = op.sens_dev(dev)
        work = ops.nc_sense_cg_workspace(B, coils, size, size, dev)

        def tail():
            ops.ald_nc_sense_cg_step(x[:B], x[B:], g[:B], g[B:], ahy, sens, psf, work, step=0.0, noise_scale=0.0, coef=1.0,
                                     max_iter=cg_iters, tol=0.0)
        ms_tail = event_ms(tail, 20)
        vc = torch.complex(x[:B], x[B:]).contiguous()
        ms_normal = event_ms(lambda: ops.toeplitz_normal(vc, psf, sens), 20)
        ms_cart_grid = cartesian_tail_ms(ops, 2 * size, B, coils, cg_iters, dev)
        ms_cart_same = cartesian_tail_ms(ops, size, B, coils, cg_iters, dev)
        # whole iterations: the difference of two replayed runs cancels the start state, the warm-up and the capture
        kw = dict(prob.call_kwargs, seed=0)
        prob.sampler(**dict(kw, n_levels=1))
        k1, k2 = 1, 1 + levels
        t1 = wall_ms(lambda: prob.sampler(**dict(kw, n_levels=k1)))
        t2 = wall_ms(lambda: prob.sampler(**dict(kw, n_levels=k2)))
        ms_iter = (t2 - t1) / ((k2 - k1) * prob.params["n_steps_each"])
    return dict(bench="nc_sense", size=size, batch=B, coils=coils, spokes=spokes, readout=readout, cg_iters=cg_iters,
                tiny=bool(tiny), ms_tail=round(ms_tail, 4), ms_ald_iteration_graph=round(ms_iter, 3),
                ms_toeplitz_normal=round(ms_normal, 4), ms_cartesian_tail_padded_grid=round(ms_cart_grid, 4),
                ms_cartesian_tail_same_size=round(ms_cart_same, 4), tail_vs_padded_grid=round(ms_tail / ms_cart_grid, 3),
                tail_vs_same_size=round(ms_tail / ms_cart_same, 3), **{k_: round(v, 2) for k_, v in t_once.items()})


def bench_frames(size, B, coils, spokes, readout, cg_iters, T, rounds):
    from inverseproblemwithdiffusionmodel_amd import ops
    from inverseproblemwithdiffusionmodel_amd.synthetic import complex_coil_maps, radial_cine_trajectory
    if B % T:
        sys.exit(f"--frames {T}: --batch {B} is not a multiple of it")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        psf_sets = ops.toeplitz_psf(radial_cine_trajectory(T, spokes, readout, size, size).to(dev), size, size)
        arms = {"one_set": psf_sets[0].contiguous(), "frames": psf_sets}
        sens = complex_coil_maps(coils, size, size, 0).to(torch.complex64).to(dev).contiguous()
        x = torch.empty(2 * B, 1, size, size, device=dev)
        g = torch.randn(2 * B, 1, size, size, device=dev, generator=gen)
        ahy = torch.complex(torch.randn(B, 1, size, size, device=dev, generator=gen),
                            torch.randn(B, 1, size, size, device=dev, generator=gen)).contiguous()
        work = ops.nc_sense_cg_workspace(B, coils, size, size, dev)
        graphs = {}
        for name, psf in arms.items():
            def tail(psf=psf):
                ops.ald_nc_sense_cg_step(x[:B], x[B:], g[:B], g[B:], ahy, sens, psf, work, step=0.0, noise_scale=0.0, coef=1.0,
                                         max_iter=cg_iters, tol=0.0)
            x.normal_(generator=gen)
            tail()                                                   # LDS attributes, allocator
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                tail()
        times = {name: [] for name in arms}
        for _ in range(rounds):                                      # alternating arms: drift of a shared card hits both
            for name in arms:
                x.normal_(generator=gen)
                times[name].append(event_ms(graphs[name].replay, 20))
    out = dict(bench="nc_sense_frames", size=size, batch=B, coils=coils, frames=T, spokes_per_frame=spokes, readout=readout,
               cg_iters=cg_iters, rounds=rounds)
    for name, t in times.items():
        t = sorted(t)
        out[f"ms_tail_{name}"] = round(t[len(t) // 2], 4)
        out[f"ms_tail_{name}_range"] = [round(t[0], 4), round(t[-1], 4)]
    out["frames_vs_one_set"] = round(out["ms_tail_frames"] / out["ms_tail_one_set"], 4)
    return out


def bench_calibrate(size, coils, spokes, readout):
    """self-calibration, each stage timed once after one untimed warm-up pass (wall clock around a device
    synchronisation): the window on the host, the sample Gram matrix, the Toeplitz spectrum, the adjoint, the conjugate
    gradients of the calibration images (the default lam, cap and tolerance), the FFT and the Walsh estimator.  A report."""
    from inverseproblemwithdiffusionmodel_amd import ops
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.noncartesian import (CALIB_DEFAULTS, NonCartesianSENSE,
                                                                                          calibration_window)
    from inverseproblemwithdiffusionmodel_amd.synthetic import complex_coil_maps, phantom_image, radial_trajectory
    dev = torch.device("cuda")
    k = radial_trajectory(spokes, readout, size, size)
    t0 = time.perf_counter()
    ah, aw, w = calibration_window(k, size, size)
    ms_window = (time.perf_counter() - t0) * 1e3
    with torch.no_grad():
        op = NonCartesianSENSE(k, (1, size, size), sens_maps=complex_coil_maps(coils, size, size, 0))
        y = op(phantom_image(size, size, seed=0).to(dev)).reshape(coils, 1, -1).contiguous()
        kd, wd = k.to(dev).contiguous(), w.to(torch.float32).to(dev).contiguous()
        t0v = float(wd.sum(dtype=torch.float64)) / (size * size)
        z = torch.zeros(coils, size, size, device=dev)
        t, iters = {}, None
        for _ in range(2):                                           # the first pass warms up; the second one's times are kept
            t["ms_gram"] = wall_ms(lambda: ops.nc_coil_gram(y, wd))
            psf, ahy = [None], [None]
            t["ms_psf"] = wall_ms(lambda: psf.__setitem__(0, ops.toeplitz_psf(kd, size, size, wd)))
            t["ms_adjoint"] = wall_ms(lambda: ahy.__setitem__(0, ops.ndft_adjoint(y, kd, size, size, None, wd).reshape(coils, size, size)))
            x = [None]
            t["ms_cg"] = wall_ms(lambda: x.__setitem__(0, ops.nc_sense_cgprox(
                z, z, ahy[0], None, psf[0], 1.0 / (CALIB_DEFAULTS["lam"] * t0v), max_iter=CALIB_DEFAULTS["max_iter"],
                tol=CALIB_DEFAULTS["tol"])))
            ks = ops.fft2c(torch.complex(x[0][0], x[0][1]).reshape(coils, 1, size, size))
            t["ms_estimator_walsh"] = wall_ms(lambda: ops.estimate_sens_maps(ks, ah, aw))
            iters = x[0][2].cpu().tolist()
    return dict(bench="nc_sense_calibrate", size=size, coils=coils, spokes=spokes, readout=readout, box=[ah, aw],
                window_samples=int((w > 0).sum()), cg_iters=iters, ms_window_host=round(ms_window, 2),
                **{k_: round(v, 3) for k_, v in t.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calibrate", action="store_true",
                    help="time the self-calibration stages once (window, Gram, psf, adjoint, CG, estimator): a report")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=14)
    ap.add_argument("--coils", type=int, default=4)
    ap.add_argument("--spokes", type=int, default=32)
    ap.add_argument("--readout", type=int, default=256)
    ap.add_argument("--cg_iters", type=int, default=10)
    ap.add_argument("--levels", type=int, default=4, help="replayed noise levels timed (3 iterations each)")
    ap.add_argument("--tiny", action="store_true", help="an ngf-16 network (a quick check of the script)")
    ap.add_argument("--frames", type=int, default=None, metavar="T",
                    help="time the tail with T psf sets (radial cine) against the one-set tail; --batch a multiple of T")
    ap.add_argument("--rounds", type=int, default=7, help="--frames: alternating rounds of 20 replays per arm")
    a = ap.parse_args()
    if a.calibrate:
        print(json.dumps(bench_calibrate(a.size, a.coils, a.spokes, a.readout)), flush=True)
        sys.exit(0)
    if a.frames is not None:
        if a.frames < 1:
            sys.exit("--frames T: T >= 1")
        print(json.dumps(bench_frames(a.size, a.batch, a.coils, a.spokes, a.readout, a.cg_iters, a.frames, a.rounds)), flush=True)
        sys.exit(0)
    print(json.dumps(bench(a.size, a.batch, a.coils, a.spokes, a.readout, a.cg_iters, a.levels, a.tiny)), flush=True)
