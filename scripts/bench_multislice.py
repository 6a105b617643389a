#!/usr/bin/env python3
"""Time one full sampler iteration (score network + fused Langevin / SENSE tail) at the headline shape -- 128x128, 4 coils,
a batch of 14 rows -- filled two ways: 14 samples of ONE slice (one coil-map set, the bench.py workload) against 2 samples
of each of 7 slices (seven map sets, row b reads set b % 7).  The single-slice arm is built twice, so that the spread
between two identical arms is measured beside the difference the map sets make.  Every arm is engine.IterationRunner's
hipGraph of one iteration; the arms alternate in one process, each timed with device events around `--steps` replays
after a warm-up.  The data-consistency tail alone (ops.ald_sense_step, also as a hipGraph) is timed the same way, which
names the kernel if the full iteration moves.  Prints one JSON line.

    python scripts/bench_multislice.py [--steps 40] [--rounds 5] [--slices 7] [--samples 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, n, warmup):
    for k in range(warmup):
        fn(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        fn(warmup + k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slices", type=int, default=7)
    ap.add_argument("--samples", type=int, default=2, help="samples per slice; the single-slice arms run slices * samples")
    ap.add_argument("--image_size", type=int, default=128)
    a = ap.parse_args()
    from inverseproblemwithdiffusionmodel_amd import engine, ops

    dev = torch.device("cuda:0")
    S, B, H, n = a.slices, a.slices * a.samples, a.image_size, 4
    cfg = engine.acdc_config(dev, H)
    net = engine.build_scorenet(cfg, 0)
    probs = {"single_a": engine.build_problem(dev, B, H=H, W=H, num_sens=n, scorenet=net, cfg=cfg),
             "single_b": engine.build_problem(dev, B, H=H, W=H, num_sens=n, scorenet=net, cfg=cfg),
             f"stack_{S}x{a.samples}": engine.build_problem(dev, a.samples, H=H, W=H, num_sens=n, scorenet=net, cfg=cfg, n_slices=S)}
    runners = {k: engine.IterationRunner(p) for k, p in probs.items()}
    for r in runners.values():
        assert r.B == B
        r.run(0)                                             # warm-up and capture
        r.run(1)
    torch.cuda.synchronize()

    # the tail alone, on each arm's own operands
    tails = {}
    for name, r in runners.items():
        st = r.st
        g = torch.randn_like(st["x"])

        def tail(st=st, g=g):
            ops.ald_sense_step(st["x"][:B], st["x"][B:], g[:B], g[B:], st["y"], st["sens"], st["mask"], st["work"], seed=1,
                               dev_sched=st["sched_dev"])
        tail()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            tail()
        tails[name] = gr

    full = {k: [] for k in runners}
    tail_ms = {k: [] for k in runners}
    n_it = min(r.n_iterations for r in runners.values())
    for _ in range(a.rounds):
        for name, r in runners.items():
            full[name].append(timed(lambda k, r=r: r.run(k % n_it), a.steps, a.warmup))
        for name, gr in tails.items():
            tail_ms[name].append(timed(lambda k, gr=gr: gr.replay(), 200, 10))
    med = lambda d: {k: float(np.median(v)) for k, v in d.items()}
    fm, tm = med(full), med(tail_ms)
    stack = f"stack_{S}x{a.samples}"
    print(json.dumps(dict(shape=[B, n, H, H], slices=S, samples_per_slice=a.samples, steps=a.steps, rounds=a.rounds,
                          map_bytes={k: int(r.st["sens"].numel() * r.st["sens"].element_size()) for k, r in runners.items()},
                          full_iteration_ms_median=fm, full_iteration_ms_all={k: [round(t, 4) for t in v] for k, v in full.items()},
                          tail_ms_median=tm, tail_ms_all={k: [round(t, 5) for t in v] for k, v in tail_ms.items()},
                          single_vs_single=fm["single_b"] / fm["single_a"],
                          stack_vs_single=fm[stack] / (0.5 * (fm["single_a"] + fm["single_b"])),
                          tail_stack_vs_single=tm[stack] / (0.5 * (tm["single_a"] + tm["single_b"])))))
