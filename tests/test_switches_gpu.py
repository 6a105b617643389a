"""The documented `IPDM_*` A/B / fallback / tuning switches (README.md), each in a fresh process: the native ones are read with
getenv once per process, the Python ones at import.  Run as a script (`python tests/test_switches_gpu.py OUTDIR`) this file is the
child: it computes a census of layers through `ops`, a set of module-level probes and the tiny-network forwards with
`ops.CONV_TRACE` recording, and writes results + observables to OUTDIR.  The parent starts one child per arm, strictly one after
another, and asserts per arm:
  * every census layer within the float64 bound the existing default-path test sets for it (reference: torch.nn.functional in
    float64 on the CPU, never another arm): 4e-6 * max|ref| per image for the Winograd and split-operand direct kernels
    (test_kernels_gpu.test_conv2d_winograd_bx3 / test_conv_bx3 / test_wino16_gpu), 2e-5 where a fused norm / activation leads
    (test_conv_bx3), 4e-6 for the 3-D direct kernels (test_conv3d_two_slices_per_workgroup), 1e-5 for the streaming FIR shapes
    (test_upfirdn2d_stream_kernel) and 2e-6 for the g09 goldens (test_upfirdn2d_golden);
  * every network within the bound its golden test asserts (1e-4 NCSNv2 / NCSNv1, 2e-4 NCSN++ / NCSN3D);
  * inside the arm, a sample's bits do not depend on its batch and the per-image maxima are exact (flags the child computes);
  * THE SWITCH TOOK EFFECT: an observable named in ARMS differs from the baseline child's.  `IPDM_W1D_COMPACT`, `IPDM_FIR_GPS`
    have no host-visible observable (the former picks a column mapping inside the launcher, the latter a strip length): for
    them the parent asserts that the name occurs as an ipdm_env_int("...") literal in csrc/ (the one reader of the native
    switches, env_int.h), so a renamed switch cannot turn the arm
    into a second baseline;
  * bit-identity with the baseline where the source claims it (`IPDM_BX3_KSPLIT`: conv_bx3.hip, "the answer is either 1 or the
    number of groups, and both give bit-identical results"); everywhere else the parent only prints whether the bits were equal.
Left out: `IPDM_BX3_CFG`, `IPDM_CONV_CFG` (they FORCE a tile configuration: an id outside its image-width class is ignored, and
inside it the launcher no longer asks whether the layer's channel counts suit the tile -- the unforced rule does, e.g. Cout % 128
for the 128-channel tile -- so an arm is valid per layer shape, not for a census: tuning aids, not fallbacks), `IPDM_W1D_STAGGER` (a cycle count with optional group
fields: open-ended), `IPDM_WBX3_SMALL_MIN` (an integer threshold: open-ended); the distributed switches and
`IPDM_ALLOW_MULTI_STREAM` are out of scope.
A child that dies by signal, exits 134 / 139 / 124 / 137 or times out ends the module: every later arm fails at once without
starting a process.  Children run one at a time.  Measured on one MI355X: a child takes 3.5 to 4 s (most of it start-up; the
baseline child, the first process to load the library on that box, took 3.5 s as well), the whole module 75 s; every child gets
30 s.  The census calls pass `in_amax=True` themselves, so under `IPDM_HX2_DYNAMIC=0` only the module probes and the networks leave
the default path."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
CHILD_TIMEOUT = 30

# arm name -> (environment, observables that must differ from the baseline child (any of), getenv literals to find in csrc/,
#              census entries that must be bit-identical to the baseline (regex) or None)
ARMS = {
    "WBX3_PERSIST=0": (dict(IPDM_WBX3_PERSIST="0"), ["form_256_256_16_16_1", "wino_splitk_256_256_16", "stats_partials_64", "pooled_unsupported"], [], None),
    "WBX3_DMA4=0": (dict(IPDM_WBX3_DMA4="0"), ["stats_has_partials"], ["IPDM_WBX3_DMA4"], None),
    "WBX3_POLY=0": (dict(IPDM_WBX3_POLY="0"), ["form_256_256_16_16_2"], [], None),
    "WBX3_CO32=0": (dict(IPDM_WBX3_CO32="0"), ["probe_conv2d_16"], [], None),              # the layer runs as two K halves
    "WBX3_CO32=0+WBX3_KSPLIT=0": (dict(IPDM_WBX3_CO32="0", IPDM_WBX3_KSPLIT="0"), ["wino_splitk_256_256_16"], [], None),
    "W1D_COMPACT=0": (dict(IPDM_W1D_COMPACT="0"), [], ["IPDM_W1D_COMPACT"], None),        # no host-visible observable
    "BX3_KSPLIT=0": (dict(IPDM_BX3_KSPLIT="0"), ["bx3_splitk_small_batch"], [], r"^(direct|conv3d)_"),
    "BX3_KSPLIT=1": (dict(IPDM_BX3_KSPLIT="1"), ["bx3_splitk_large_batch"], [], r"^(direct|conv3d)_"),
    "FIR_GPS=3": (dict(IPDM_FIR_GPS="3"), [], ["IPDM_FIR_GPS"], None),                    # no host-visible observable
    "FIR_GPS=32": (dict(IPDM_FIR_GPS="32"), [], ["IPDM_FIR_GPS"], None),
    "WINOGRAD=0": (dict(IPDM_WINOGRAD="0"), ["probe_conv2d"], [], None),
    "WINO1D=0": (dict(IPDM_WINO1D="0"), ["probe_conv2d"], [], None),
    "WINO1D_STATS=0": (dict(IPDM_WINO1D_STATS="0"), ["probe_conv2d_stats"], [], None),
    "WINO1D_VOL=0": (dict(IPDM_WINO1D_VOL="0"), ["probe_conv3d"], [], None),
    "THIN_CONV=0": (dict(IPDM_THIN_CONV="0"), ["net_thin_layers"], [], None),
    "STATS_EPILOGUE=0": (dict(IPDM_STATS_EPILOGUE="0"), ["stats_has_partials"], [], None),
    "FUSE_POOL=0": (dict(IPDM_FUSE_POOL="0"), ["probe_fused_pool"], [], None),
    "GN_PARTIALS=0": (dict(IPDM_GN_PARTIALS="0"), ["probe_pp_conv_stats"], [], None),
    "HX2_DYNAMIC=0": (dict(IPDM_HX2_DYNAMIC="0"), ["probe_conv2d_amax"], [], None),         # no maxima measured / produced
    "CONV_IMPL=bx3": (dict(IPDM_CONV_IMPL="bx3"), ["probe_conv2d"], [], None),               # fmt of the launch
    "CONV_IMPL=f32": (dict(IPDM_CONV_IMPL="f32"), ["probe_conv2d"], [], None),
}

# ---- the census (built on the CPU from seeds, every image its own range 1e-3 .. 1e3, as test_wino16_gpu._inputs) ---------------
WINO16 = [("c256_256_d1", 256, 256, 1), ("c512_512_d4", 512, 512, 4), ("c512_512_d2", 512, 512, 2), ("c256_512_d2", 256, 512, 2),
          ("c512_256_d1", 512, 256, 1), ("c256_256_d2", 256, 256, 2)]
# name, B, Cin, Cout, H, W, dilation, pooled, statistics
WINO_BIG = [("w128_64", 2, 128, 128, 64, 64, 1, False, False), ("w256_32", 2, 256, 256, 32, 32, 1, False, False),
            ("w32_40x36", 3, 32, 64, 40, 36, 1, False, False), ("w32_34x44_pool", 1, 32, 64, 34, 44, 1, True, False),
            ("w64_64x32_pool_stats", 2, 64, 128, 64, 32, 1, True, True), ("w128_32_d2", 2, 128, 128, 32, 32, 2, False, False)]
DIRECT = [  # test_kernels_gpu.CONV_CASES
    (2, 16, 32, 32, 32, 3, 1, False, "none", False), (2, 128, 128, 64, 64, 3, 1, True, "elu", True),
    (1, 128, 256, 32, 32, 3, 1, False, "elu", False), (3, 256, 256, 16, 16, 3, 1, True, "elu", True),
    (2, 256, 512, 16, 16, 3, 2, True, "elu", False), (2, 512, 512, 16, 16, 3, 4, False, "elu", True),
    (2, 1, 128, 32, 32, 3, 1, False, "none", False), (2, 128, 1, 32, 32, 3, 1, True, "elu", False),
    (2, 128, 256, 32, 32, 1, 1, False, "none", False), (1, 6, 5, 12, 10, 3, 1, True, "elu", True),
    (1, 7, 9, 19, 45, 3, 1, False, "relu", False), (2, 24, 40, 8, 8, 3, 2, False, "none", False)]
CONV3D = [(2, 128, 128, 8, 8, 12), (1, 64, 128, 5, 8, 12), (1, 128, 256, 3, 6, 16)]          # test_conv3d_two_slices_per_workgroup
VOL1D = [(2, 128, 128, 4, 8, 24)]                  # 12-pair planes (W = 24): the 1-D kernel's compact column mapping
FIR = [((2, 8, 100, 64), "down"), ((2, 8, 100, 64), "up"), ((1, 4, 72, 128), "down"), ((1, 4, 72, 128), "up")]   # 50 / 100 / 36 / 72 row groups
FIR_GOLDEN = ["down2", "up2", "down2_nonsq", "up2_nonsq", "up3_down2_k5", "negpad_k3", "up1_down3_k2x4", "up2_down1_k6"]
FMTS = ["hx2", "bx3"]


def _ranged(gen, B, *shape):
    return F.elu(torch.randn(B, *shape, generator=gen)) * (10.0 ** torch.linspace(-3, 3, B)).view(B, *([1] * len(shape)))


def _layer_inputs(name, B, Cin, Cout, H, W, oh=None, ow=None):
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = _ranged(gen, B, Cin, H, W)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=gen)
    r = torch.randn(B, Cout, oh or H, ow or W, generator=gen)
    return x, w, b, r


def _probe_inputs(name, B, Cin, Cout, H, W):
    """module-level probes: O(1) activations, the precondition of the static-range arm (IPDM_HX2_DYNAMIC=0) they also run under"""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    return (torch.randn(B, Cin, H, W, generator=gen), torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5,
            torch.randn(Cout, generator=gen), torch.randn(B, Cout, H, W, generator=gen))


def _direct_inputs(i):
    B, Cin, Cout, H, W, k, dil, norm, actname, res = DIRECT[i]
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=gen)
    resid = torch.randn(B, Cout, H, W, generator=gen) if res else None
    p = {"alpha": 1 + 0.1 * torch.randn(Cin, generator=gen), "gamma": 1 + 0.1 * torch.randn(Cin, generator=gen),
         "beta": 0.1 * torch.randn(Cin, generator=gen)}
    return x, w, bias, resid, p


def _conv3d_inputs(B, Cin, Cout, D, H, W):
    gen = torch.Generator().manual_seed(20 + D)
    x = torch.randn(B, Cin, D, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=gen) / (Cin * 27) ** 0.5
    return x, w, torch.randn(Cout, generator=gen), torch.randn(B, Cout, D, H, W, generator=gen)


def _fir_inputs(shape, mode):
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape).astype(np.float32)
    k = rng.standard_normal((4, 4)).astype(np.float32)
    return x, k, ((1, 1, 2, 2, 1, 1, 1, 1) if mode == "down" else (2, 2, 1, 1, 2, 1, 2, 1))


# ---- child ---------------------------------------------------------------------------------------------------------------------
def _child(outdir):
    sys.path.insert(0, REPO)
    sys.path.insert(0, TESTS)
    from inverseproblemwithdiffusionmodel_amd import _lib, ops
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers
    from inverseproblemwithdiffusionmodel_amd.models import layers as pp_layers
    lib = _lib.lib
    res, obs, flags = {}, {}, {}

    def keep(name, t):
        res[name] = t.detach().cpu().numpy()

    def amax_exact(name, t):
        am = ops.amax_of(t)
        if am is not None:
            flags[f"amax:{name}"] = bool(torch.equal(ops.amax_value(am), t.abs().amax(dim=tuple(range(1, t.dim())))))

    # host-visible observables
    forms = {ops.WINO_FORM_OTHER: "OTHER", ops.WINO_FORM_CO32: "CO32", ops.WINO_FORM_HALF: "HALF", ops.WINO_FORM_POLY: "POLY", None: None}
    obs["form_256_256_16_16_1"] = forms[ops.wino_hx2_form(256, 256, 16, 16, 1)]
    obs["form_256_256_16_16_2"] = forms[ops.wino_hx2_form(256, 256, 16, 16, 2)]
    obs["wino_splitk_256_256_16"] = ops.wino_bx3_splitk(256, 256, 16, 16)
    obs["stats_partials_64"] = int(lib.ipdm_conv2d_wino_bx3_stats_partials(128, 128, 64, 64, 1, 0))
    obs["bx3_splitk_small_batch"] = int(lib.ipdm_conv_bx3_splitk(3, 1, 256, 256, 16, 16, 3, 1))
    obs["bx3_splitk_large_batch"] = int(lib.ipdm_conv_bx3_splitk(64, 1, 256, 256, 16, 16, 3, 1))
    obs["py_WBX3_CO32"], obs["py_CONV_IMPL"], obs["py_dynamic_range"] = ops.WBX3_CO32, ops.CONV_IMPL, bool(ops.dynamic_range())

    # 1. layer census through ops
    for fmt in FMTS:
        for name, Cin, Cout, dil in WINO16:
            x, w, b, r = (t.cuda() for t in _layer_inputs(name, 3, Cin, Cout, 16, 16))
            U = ops.conv_wino_bx3_weight(w, fmt=fmt)
            kw = dict(dilation=dil, in_amax=True, want_amax=True)
            with ops.amax_scope():
                plain = ops.conv2d_wino_bx3(x, U, b, **kw)
                resd = ops.conv2d_wino_bx3(x, U, b, r, **kw)
                two, act = ops.conv2d_wino_bx3(x, U, b, r, act_out=ops.ACT_ELU, **kw)
                for nm, t in (("plain", plain), ("residual", resd), ("two_out", two), ("two_act", act)):
                    keep(f"wino16_{fmt}_{name}_{nm}", t)
                    amax_exact(f"wino16_{fmt}_{name}_{nm}", t)
                one = ops.conv2d_wino_bx3(x[2:].contiguous(), U, b, r[2:].contiguous(), **kw)
                flags[f"batch:wino16_{fmt}_{name}"] = bool(torch.equal(one, resd[2:]))
        for name, B, Cin, Cout, H, W, dil, pool, stats in WINO_BIG:
            oh, ow = (H // 2, W // 2) if pool else (H, W)
            x, w, b, r = (t.cuda() for t in _layer_inputs(name, B, Cin, Cout, H, W, oh, ow))
            U = ops.conv_wino_bx3_weight(w, fmt=fmt)
            kw = dict(dilation=dil, in_amax=True, pool2=pool, want_stats=stats)
            try:
                y = ops.conv2d_wino_bx3(x, U, b, r, **kw)
                if pool:
                    obs["pooled_unsupported"] = False
                if stats:
                    obs["stats_has_partials"] = hasattr(y, "_ipdm_partials")
                keep(f"wino_{fmt}_{name}", y)
                one = ops.conv2d_wino_bx3(x[B - 1:].contiguous(), U, b, r[B - 1:].contiguous(), **kw)
                flags[f"batch:wino_{fmt}_{name}"] = bool(torch.equal(one, y[B - 1:]))
            except _lib.IpdmUnsupported:
                assert pool, name                                  # only the pooled epilogue may be missing (conv + meanpool2 instead)
                obs["pooled_unsupported"] = True
                obs.setdefault("stats_has_partials", False)
                y = ops.add(ops.meanpool2(ops.conv2d_wino_bx3(x, U, b, dilation=dil, in_amax=True)), r)
                keep(f"wino_{fmt}_{name}", y)
        for i, (B, Cin, Cout, H, W, k, dil, norm, actname, has_res) in enumerate(DIRECT):
            x, w, bias, resid, p = _direct_inputs(i)
            xd = x.cuda()
            coef = ops.instnorm_plus_coef(xd, p["alpha"].cuda(), p["gamma"].cuda(), p["beta"].cuda()) if norm else None
            wq = ops.conv_bx3_weight(w.cuda(), fmt=fmt)
            rd = None if resid is None else resid.cuda()
            y = ops.conv_bx3(xd, wq, bias.cuda(), coef, ops.ACT_CODES[actname], rd, dil)
            keep(f"direct_{fmt}_{i}", y)
            if not norm:                                          # (the fused norm's coefficients are per image already)
                one = ops.conv_bx3(xd[B - 1:].contiguous(), wq, bias.cuda(), None, ops.ACT_CODES[actname],
                                   None if rd is None else rd[B - 1:].contiguous(), dil)
                flags[f"batch:direct_{fmt}_{i}"] = bool(torch.equal(one, y[B - 1:]))
        for shp in CONV3D + VOL1D:
            x, w, b, r = (t.cuda() for t in _conv3d_inputs(*shp))
            keep("conv3d_%s_%s" % (fmt, "_".join(map(str, shp))), ops.conv3d(x, ops.conv_bx3_weight(w, fmt=fmt), b, residual=r))
    for shp in VOL1D:
        B, Cin, Cout, D, H, W = shp
        x, w, b, r = (t.cuda() for t in _conv3d_inputs(*shp))
        if lib.ipdm_conv3d_wino1d_supported(Cin, Cout, D, H, W):
            keep("vol1d_" + "_".join(map(str, shp)), ops.conv3d_wino1d(x, ops.conv_wino1d_weight3d(w), b, r))
    for shape, mode in FIR:
        x, k, args = _fir_inputs(shape, mode)
        N, C, H, W = shape
        y = ops.upfirdn2d_raw(torch.from_numpy(x).cuda().reshape(N * C, H, W, 1), torch.from_numpy(k).cuda(), *args)
        keep("fir_%s_%s" % (mode, "x".join(map(str, shape))), y.reshape(N, C, y.shape[1], y.shape[2]))
    g = np.load(os.path.join(TESTS, "golden", "g09_upfirdn.npz"))
    for name in FIR_GOLDEN:
        x, k = g[f"{name}_x"], g[f"{name}_k"]
        up, down, p0, p1 = (int(v) for v in g[f"{name}_udp"])
        N, C, H, W = x.shape
        y = ops.upfirdn2d_raw(torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(N * C, H, W, 1), torch.from_numpy(k).cuda(),
                              up, up, down, down, p0, p1, p0, p1)
        keep(f"firgold_{name}", y.reshape(N, C, y.shape[1], y.shape[2]))

    # 2. module-level probes: which kernels the dispatch picks (CONV_TRACE flags), results against float64 in the parent
    def traced(fn):
        ops.CONV_TRACE = []
        try:
            with torch.no_grad():
                y = fn()
            return y, [{k: v for k, v in t.items() if k not in ("e0", "e1")} for t in ops.CONV_TRACE]
        finally:
            ops.CONV_TRACE = None

    def flagset(trace):
        return [[k for k in ("wino", "wino1d", "thin", "stats", "pool2", "bx3") if t.get(k)] + [f"fmt={t.get('fmt')}", f"ksplit={t.get('ksplit', 1)}"]
                for t in trace]
    x, w, b, r = (t.cuda() for t in _probe_inputs("probe", 2, 64, 128, 32, 64))
    conv = layers.Conv2d(64, 128, 3).cuda()
    conv.weight.data.copy_(w)
    conv.bias.data.copy_(b)
    measured = ops.AMAX_MEASURED
    y, t = traced(lambda: conv(x, residual=r))
    keep("probe_conv2d", y)
    obs["probe_conv2d"] = flagset(t)
    # dynamic range at the launch: the untagged input was measured for it, and the epilogue was asked for the result's maxima
    obs["probe_conv2d_amax"] = [ops.AMAX_MEASURED - measured, ops.amax_of(y) is not None]
    y, t = traced(lambda: conv(x, residual=r, want_stats=True))
    keep("probe_conv2d_stats", y)
    obs["probe_conv2d_stats"] = flagset(t)
    cmp_ = layers.ConvMeanPool(64, 128, 3).cuda()
    cmp_.conv.weight.data.copy_(w)
    cmp_.conv.bias.data.copy_(b)
    y, t = traced(lambda: cmp_.fused(x))
    obs["probe_fused_pool"] = None if y is None else flagset(t)
    if y is None:
        y, t = traced(lambda: cmp_(x))
    keep("probe_pool", y[0] if isinstance(y, tuple) else y)
    x16, w16, b16, r16 = (t.cuda() for t in _probe_inputs("probe16", 3, 256, 256, 16, 16))
    conv16 = layers.Conv2d(256, 256, 3).cuda()
    conv16.weight.data.copy_(w16)
    conv16.bias.data.copy_(b16)
    y, t = traced(lambda: conv16(x16, residual=r16))
    keep("probe_conv2d_16", y)
    obs["probe_conv2d_16"] = flagset(t)
    ppc = pp_layers.Conv(64, 128, 3).cuda()
    ppc.weight.data.copy_(w)
    ppc.bias.data.copy_(b)
    y, t = traced(lambda: ppc(x, residual=r, want_stats=True))
    keep("probe_pp_conv", y)
    obs["probe_pp_conv_stats"] = flagset(t) + [ops.stats_partials_of(y) is not None]
    xv, wv, bv, rv = (t.cuda() for t in _conv3d_inputs(*VOL1D[0]))
    conv3 = layers.Conv2d(VOL1D[0][1], VOL1D[0][2], 3, ndim=3).cuda()
    conv3.weight.data.copy_(wv)
    conv3.bias.data.copy_(bv)
    y, t = traced(lambda: conv3(xv, residual=rv))
    keep("probe_conv3d", y)
    obs["probe_conv3d"] = flagset(t)

    # 3. tiny-network forwards through the modules
    from conftest import state_dict_from_golden
    import test_2dtime_gpu as t3
    from test_ncsn1_gpu import NETS, tiny_config as cfg_v1
    from test_score_sde_gpu import tiny_cfg as cfg_pp
    from test_scorenet_gpu import tiny_config as cfg_v2
    from inverseproblemwithdiffusionmodel_amd.models import ncsnpp
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsn, ncsnv2
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ncsn3d import NCSN3DShallow

    def gold(n):
        return np.load(os.path.join(TESTS, "golden", n + ".npz"))
    thin = 0
    g = gold("g07_layers")
    net = ncsnv2.NCSNv2Deepest(cfg_v2())
    net.load_state_dict(state_dict_from_golden(g, "net"), strict=True)
    net = net.cuda().eval()
    y, t = traced(lambda: net(torch.from_numpy(g["net_x"]).cuda(), torch.from_numpy(g["net_labels"]).cuda()))
    keep("net_ncsnv2", y)
    thin += sum(1 for r_ in t if r_.get("thin"))
    g = gold("g14_ncsnpp")
    net = ncsnpp.NCSNpp(cfg_pp())
    net.load_state_dict(state_dict_from_golden(g, "pp"), strict=True)
    net = net.cuda().eval()
    y, t = traced(lambda: net(torch.from_numpy(g["pp_x"]).cuda(), torch.from_numpy(g["pp_sigma"]).cuda()))
    keep("net_ncsnpp", y)
    thin += sum(1 for r_ in t if r_.get("thin"))
    g = gold("g16_ncsn3d")
    net = NCSN3DShallow(t3.cfg3d())
    net.load_state_dict(state_dict_from_golden(g, "net3d"), strict=True)
    net = net.cuda().eval()
    y, t = traced(lambda: net(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["labels"]).cuda()))
    keep("net_ncsn3d", y)
    g = gold("g31_ncsn1")
    cls, kw = NETS["n32"]
    net = getattr(ncsn, cls)(cfg_v1(**kw))
    net.load_state_dict(state_dict_from_golden(g, "n32"), strict=True)
    net = net.cuda().eval()
    y, t = traced(lambda: net(torch.from_numpy(g["n32_x"]).cuda(), torch.from_numpy(g["n32_labels"]).cuda()))
    keep("net_ncsn1", y)
    thin += sum(1 for r_ in t if r_.get("thin"))
    obs["net_thin_layers"] = thin

    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, "results.npz"), **res)
    with open(os.path.join(outdir, "obs.json"), "w") as f:
        json.dump(dict(obs=obs, flags=flags), f)


# ---- parent --------------------------------------------------------------------------------------------------------------------
_DEAD = []                                          # a child that faulted / hung ends the module


def _run_child(tmp_path_factory, arm, env):
    if _DEAD:
        pytest.fail(f"not started: an earlier child ended abnormally ({_DEAD[0]})")
    outdir = str(tmp_path_factory.mktemp("switch_" + re.sub(r"\W", "_", arm)))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), outdir], env=dict(os.environ, **env), cwd=REPO,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"{arm}: timeout after {CHILD_TIMEOUT} s")
        pytest.fail(_DEAD[0])
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        _DEAD.append(f"{arm}: exit status {p.returncode}")
        pytest.fail(_DEAD[0] + "\n" + p.stderr[-3000:])
    assert p.returncode == 0, p.stderr[-3000:]
    with open(os.path.join(outdir, "obs.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(outdir, "results.npz"))), meta["obs"], meta["flags"]


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    for name in os.environ:
        assert not (name.startswith("IPDM_") and any(name in env for env, *_ in ARMS.values())), f"{name} is set: this module tests from the defaults"
    return _run_child(tmp_path_factory, "baseline", {})


@pytest.fixture(scope="module")
def refs():
    """float64 references on the CPU, and the bound of each census entry: name -> (reference, relative bound, per image?)"""
    sys.path.insert(0, REPO)
    from oracle import resample, scorenet
    out = {}
    for name, Cin, Cout, dil in WINO16:
        x, w, b, r = _layer_inputs(name, 3, Cin, Cout, 16, 16)
        conv = F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil)
        for fmt in FMTS:
            out[f"wino16_{fmt}_{name}_plain"] = (conv, conv, 4e-6)
            out[f"wino16_{fmt}_{name}_residual"] = out[f"wino16_{fmt}_{name}_two_out"] = (conv + r.double(), conv + r.double(), 4e-6)
            out[f"wino16_{fmt}_{name}_two_act"] = (F.elu(conv + r.double()), conv + r.double(), 4e-6)
    for name, B, Cin, Cout, H, W, dil, pool, stats in WINO_BIG:
        oh, ow = (H // 2, W // 2) if pool else (H, W)
        x, w, b, r = _layer_inputs(name, B, Cin, Cout, H, W, oh, ow)
        conv = F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil)
        if pool:
            conv = (conv[..., ::2, ::2] + conv[..., 1::2, ::2] + conv[..., ::2, 1::2] + conv[..., 1::2, 1::2]) / 4
        for fmt in FMTS:
            out[f"wino_{fmt}_{name}"] = (conv + r.double(), conv + r.double(), 4e-6)
    for i, (B, Cin, Cout, H, W, k, dil, norm, actname, has_res) in enumerate(DIRECT):
        x, w, bias, resid, p = _direct_inputs(i)
        fn = {"none": lambda t: t, "elu": F.elu, "relu": F.relu}[actname]
        h = scorenet.instance_norm_plus(x.double(), {a: v.double() for a, v in p.items()}) if norm else x.double()
        want = F.conv2d(fn(h), w.double(), bias.double(), padding=(k // 2) * dil, dilation=dil)
        want = want + resid.double() if has_res else want
        for fmt in FMTS:
            out[f"direct_{fmt}_{i}"] = (want, None, 2e-5 if norm or actname != "none" else 4e-6)       # test_conv_bx3: * max(1, max|ref|)
    for shp in CONV3D + VOL1D:
        x, w, b, r = _conv3d_inputs(*shp)
        want = F.conv3d(x.double(), w.double(), b.double(), padding=1) + r.double()
        for fmt in FMTS:
            out["conv3d_%s_%s" % (fmt, "_".join(map(str, shp)))] = (want, None, 4e-6)
        if shp in VOL1D:
            out["vol1d_" + "_".join(map(str, shp))] = (want, None, 4e-6)
    for shape, mode in FIR:
        x, k, args = _fir_inputs(shape, mode)
        out["fir_%s_%s" % (mode, "x".join(map(str, shape)))] = (torch.from_numpy(resample.upfirdn2d(x.astype(np.float64), k.astype(np.float64), *args)), "abs", 1e-5)
    g = np.load(os.path.join(TESTS, "golden", "g09_upfirdn.npz"))
    for name in FIR_GOLDEN:
        out[f"firgold_{name}"] = (torch.from_numpy(g[f"{name}_y"]).double(), "abs", 2e-6)
    x, w, b, r = _probe_inputs("probe", 2, 64, 128, 32, 64)
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    out["probe_conv2d"] = out["probe_conv2d_stats"] = out["probe_pp_conv"] = (conv + r.double(), conv + r.double(), 4e-6)
    out["probe_pool"] = ((conv[..., ::2, ::2] + conv[..., 1::2, ::2] + conv[..., ::2, 1::2] + conv[..., 1::2, 1::2]) / 4,) * 2 + (4e-6,)
    x, w, b, r = _probe_inputs("probe16", 3, 256, 256, 16, 16)
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=1) + r.double()
    out["probe_conv2d_16"] = (conv, conv, 4e-6)
    x, w, b, r = _conv3d_inputs(*VOL1D[0])
    out["probe_conv3d"] = (F.conv3d(x.double(), w.double(), b.double(), padding=1) + r.double(), None, 4e-6)
    gold = {"net_ncsnv2": ("g07_layers", "net_y", 1e-4), "net_ncsnpp": ("g14_ncsnpp", "pp_y", 2e-4), "net_ncsn3d": ("g16_ncsn3d", "y", 2e-4),
            "net_ncsn1": ("g31_ncsn1", "n32_y", 1e-4)}
    for name, (f, key, rel) in gold.items():
        out[name] = (torch.from_numpy(np.load(os.path.join(TESTS, "golden", f + ".npz"))[key]).double(), "net", rel)
    return out


def _check_values(arm, env, results, refs):
    worst = {}
    for name, got in sorted(results.items()):
        ref, scale, rel = refs[name]
        if env.get("IPDM_CONV_IMPL") == "f32" and name.startswith("probe_"):
            # the f32 family's bounds, * max(1, max|ref|): 2e-5 direct (test_conv2d; NCSN++ and 3-D layers), 4e-5 fp32 Winograd
            # (test_conv2d_winograd; the ncsn 2-D layers)
            rel, scale = (2e-5 if name in ("probe_conv3d", "probe_pp_conv") else 4e-5), None
        got = torch.from_numpy(got).double()
        assert got.shape == ref.shape, (arm, name, got.shape, ref.shape)
        if isinstance(scale, str) and scale == "abs":
            err, lim = float((got - ref).abs().max()), rel
        elif isinstance(scale, str):                               # networks: rel * max|golden|
            err, lim = float((got - ref).abs().max() / ref.abs().max()), rel
        elif scale is None:                                        # rel * max(1, max|ref|)
            err, lim = float((got - ref).abs().max() / max(1.0, float(ref.abs().max()))), rel
        else:                                                      # per image: rel * max|ref of that image|
            dims = tuple(range(1, ref.dim()))
            err, lim = float(((got - ref).abs().amax(dim=dims) / scale.abs().amax(dim=dims)).max()), rel
        worst[name] = err / lim
        assert err <= lim, (arm, name, err, lim)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print(f"[{arm}] {len(results)} results within their bounds; closest: " + ", ".join(f"{n} {v:.2f} x bound" for n, v in top))


def test_baseline(baseline, refs):
    results, obs, flags = baseline
    assert set(results) == set(refs), sorted(set(refs) ^ set(results))
    _check_values("baseline", {}, results, refs)
    assert flags and all(flags.values()), [k for k, v in flags.items() if not v]
    assert obs["form_256_256_16_16_1"] == "HALF" and obs["form_256_256_16_16_2"] == "POLY" and obs["net_thin_layers"] >= 3
    assert obs["stats_has_partials"] is True and obs["pooled_unsupported"] is False and obs["probe_fused_pool"] is not None


@pytest.mark.parametrize("arm", list(ARMS))
def test_switch(arm, baseline, refs, tmp_path_factory):
    env, differs, literals, identical = ARMS[arm]
    base_results, base_obs, _ = baseline
    results, obs, flags = _run_child(tmp_path_factory, arm, env)
    _check_values(arm, env, results, refs)
    assert set(results) == set(base_results)
    assert all(flags.values()), (arm, [k for k, v in flags.items() if not v])
    assert set(k.split(":")[0] for k in flags) == {"batch", "amax"}
    changed = [k for k in obs if obs[k] != base_obs.get(k)]
    print(f"[{arm}] observables that differ from the baseline: " + "; ".join(f"{k}: {base_obs.get(k)} -> {obs[k]}" for k in changed))
    if differs:
        assert any(k in changed for k in differs), (arm, {k: obs.get(k) for k in differs})
    else:
        assert literals, arm
    if literals:
        src = "".join(open(f).read() for f in glob.glob(os.path.join(REPO, "inverseproblemwithdiffusionmodel_amd", "csrc", "*.hip")) +
                      glob.glob(os.path.join(REPO, "inverseproblemwithdiffusionmodel_amd", "csrc", "*.h")))
        for name in literals:
            assert f'ipdm_env_int("{name}"' in src, f"{name} is no longer read by the native code: the arm would be a second baseline"
    same = [k for k in results if np.array_equal(results[k], base_results[k])]
    print(f"[{arm}] {len(same)} of {len(results)} results bit-identical to the baseline; differing: "
          + ", ".join(sorted(set(results) - set(same))[:12]))
    if identical:
        must = [k for k in results if re.search(identical, k)]
        assert must and all(k in same for k in must), (arm, sorted(set(must) - set(same)))


if __name__ == "__main__":
    _child(sys.argv[1])
