#!/usr/bin/env python3
"""Predictor-corrector SENSE reconstruction with NCSN++ (sde/inverse.py), timed: milliseconds per level (one Langevin
corrector step + the reverse-diffusion predictor, each with data consistency) replayed as a hipGraph and run eagerly, and
the per-level time of the coefficient launch plus the two fused tails against the two score evaluations (device events,
after a warm-up).  NCSN++ (celebahq_256_ncsnpp_continuous, one channel, seeded synthetic weights), 4 coils, B = 4, at
128x128 and 256x256.  One JSON line per size.

    python scripts/bench_pc_sense.py [--sizes 128 256] [--levels 6] [--batch 4] [--tiny]"""
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


def bench(size, B, levels, tiny):
    from inverseproblemwithdiffusionmodel_amd import engine, ops
    from inverseproblemwithdiffusionmodel_amd.configs import ve_ncsnpp
    from inverseproblemwithdiffusionmodel_amd.models import ncsnpp
    from inverseproblemwithdiffusionmodel_amd.models.utils import get_score_fn
    from inverseproblemwithdiffusionmodel_amd.sde import sde_lib
    from inverseproblemwithdiffusionmodel_amd.synthetic import synth_state_dict
    dev = torch.device("cuda")
    cfg = ve_ncsnpp.get_config()
    cfg.device = dev
    if tiny:
        cfg.model.nf, cfg.model.ch_mult, cfg.model.num_res_blocks, cfg.model.attn_resolutions = 16, (1, 2, 2), 1, (8,)
    cfg.data.image_size, cfg.data.num_channels = size, 1
    net = ncsnpp.NCSNpp(cfg)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=0), strict=False)
    net = net.to(dev).eval()
    sde = sde_lib.VESDE(cfg.model.sigma_min, cfg.model.sigma_max, cfg.model.num_scales)
    prob = engine.build_problem(dev, B, R=8, H=size, W=size, num_sens=4, seed=0, scorenet=net, cfg=engine.acdc_config(dev, size))
    sampler = engine.build_pc_sampler(prob, sde, snr=cfg.sampling.snr, n_steps=1)
    with torch.no_grad():
        sampler(net, n_iters=2, seed=0)                                       # warm-up: weight packing, LDS attributes
        # per replayed / eager level: the difference of two runs cancels the start state, the warm-up level and the capture
        k1, k2 = 2, 2 + levels
        per = {}
        for name, graph in (("graph", True), ("eager", False)):
            t1 = wall_ms(lambda: sampler(net, n_iters=k1, seed=0, use_graph=graph))
            t2 = wall_ms(lambda: sampler(net, n_iters=k2, seed=0, use_graph=graph))
            per[name] = (t2 - t1) / (k2 - k1)
        # the parts of one level on their own: two score evaluations; the coefficient launch and the two tails.  The tails'
        # record has coef = 1 (step = noise_scale = 0): with a zero coefficient the whole-image kernels return before their
        # transforms and the figure would be that of the Langevin update alone.  The state drifts towards consistency; no matter.
        x = torch.randn(2 * B, 1, size, size, device=dev)
        t = torch.full((2 * B,), 0.5, device=dev)
        y, sens, mask = prob.measurement.contiguous(), prob.op.sens_dev(dev), prob.op.mask_u8(dev)
        work, coef_work = ops.sense_workspace(B, 4, size, size, dev), ops.pc_langevin_coef_workspace(B, dev)
        sample_sched = torch.zeros(B, ops.SCHED_BYTES, dtype=torch.uint8, device=dev)
        score_fn = get_score_fn(sde, net, train=False, continuous=True)
        score = score_fn(x, t).contiguous()
        ms_score = 2 * event_ms(lambda: score_fn(x, t), 5)
        rec = torch.zeros(ops.SCHED_BYTES, dtype=torch.uint8, device=dev)
        rec[8:12] = torch.tensor([1.0], dtype=torch.float32).view(torch.uint8).to(dev)       # ipdm_sched_t.coef
        kw = dict(seed=0, sample_offset=0)

        def coef():
            ops.pc_langevin_coef(score[:B], score[B:], sample_sched, 0.0, 1.0, dev_sched=rec, work=coef_work, **kw)

        def tails():
            coef()
            ops.pc_sense_step(x[:B], x[B:], score[:B], score[B:], y, sens, mask, work, sample_sched=sample_sched, **kw)
            ops.pc_sense_step(x[:B], x[B:], score[:B], score[B:], y, sens, mask, work, dev_sched=rec, **kw)
        ms_tails = event_ms(tails, 20)
        ms_coef = event_ms(coef, 20)
    return dict(bench="pc_sense", size=size, batch=B, coils=4, tiny=bool(tiny), ms_per_level_graph=round(per["graph"], 3),
                ms_per_level_eager=round(per["eager"], 3), ms_score_evaluations_per_level=round(ms_score, 3),
                ms_coef_and_tails_per_level=round(ms_tails, 4), ms_coef_launch=round(ms_coef, 4),
                tails_share_of_level=round(ms_tails / (ms_tails + ms_score), 4))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--levels", type=int, default=6, help="replayed levels timed")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--tiny", action="store_true", help="an nf-16 network (a quick check of the script)")
    a = ap.parse_args()
    for s in a.sizes:
        print(json.dumps(bench(s, a.batch, a.levels, a.tiny)), flush=True)
