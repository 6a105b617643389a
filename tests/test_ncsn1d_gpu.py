"""The NCSN1D family on the GPU: the 1-D convolution kernel (csrc/conv1d.hip) against float64 torch.nn.functional.conv1d on the
CPU at every length it serves (12, 24, 48 and, in the `new_lengths` tests, 16, 32, 96), its maxima / batch-independence / range /
alignment contracts, every 1-D layer and network against the reference's own outputs (g33_ncsn1d, g34_ncsn1d_full; g34's
sequences also inside the production batches N = 512 and N = 256), the ALD2DTime trajectory with a 1-D temporal prior (g35_ald2dtime_1d), the
`IPDM_CONV1D=0` arm in a fresh child process and the 2D+time driver script with `--temporal_type Diffusion1D`.

Bounds: the kernel 2e-5 * max(1, max|want|) (the direct kernel's, test_2dtime_gpu.py:53); layers and tiny networks
2e-4 * max|ref| (the 3-D family's golden bound); the full-size network 2e-4 * max|ref| and NRMSE < 1e-4
(test_full_size_ncsn3d_shallow_vs_reference); the trajectory NRMSE and |SSIM - 1| < 1e-3 per frame
(test_ald2dtime_trajectory_golden).

Run as a script (`python tests/test_ncsn1d_gpu.py OUT.json`) this file is the child of the switch test: it runs the g34
forward and writes the error figures and the launch counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
if REPO not in sys.path:
    sys.path.insert(0, REPO)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from conftest import state_dict_from_golden  # noqa: E402
from oracle import metrics  # noqa: E402
from test_ncsn1d_host import cfg1d  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(64, 128), (128, 128), (128, 256), (256, 256), (256, 128), (128, 64)]
LENGTHS = [12, 24, 48]
TAPS = [(1, 1), (3, 1), (3, 2), (3, 4)]                     # (k, dilation)
# epilogue options: (bias, residual, act_out, raw, res_second, pool2)
EPILOGUES = {
    "bias": (True, False, "none", True, False, False),
    "plain": (False, False, "none", True, False, False),
    "bias_res": (True, True, "none", True, False, False),
    "res_elu_both": (True, True, "elu", True, False, False),
    "elu_only": (True, False, "elu", False, False, False),
    "copy_both": (False, True, "copy", True, False, False),
    "res_second": (True, True, "copy", True, True, False),
    "res_second_elu": (False, True, "elu", True, True, False),
    "pool": (True, False, "none", True, False, True),
    "pool_res_elu": (True, True, "elu", True, False, True),
    "pool_elu_only": (False, True, "elu", False, False, True),
}
EP_NAMES = list(EPILOGUES)


def _ops():
    from inverseproblemwithdiffusionmodel_amd import ops
    return ops


def _inputs(N, Cin, Cout, L, k, seed, pool2, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, L, generator=g) * scale
    x = x * torch.logspace(-1, 1, N).view(N, 1, 1)[torch.randperm(N, generator=g)]     # every sequence its own range
    w = torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    r = torch.randn(N, Cout, L // 2 if pool2 else L, generator=g)
    return x, w, b, r


def _want(x, w, b, r, d, ep):
    """float64 on the CPU -> (out, out_act), either None where the launch does not produce it"""
    bias, res, act, raw, res_second, pool2 = ep
    k = w.shape[2]
    y = F.conv1d(x.double(), w.double(), b.double() if bias else None, padding=d * (k // 2), dilation=d)
    if pool2:
        y = (y[:, :, ::2] + y[:, :, 1::2]) / 2.0
    full = y + r.double() if res else y
    out = y if res_second else full
    a = None
    if act == "elu":
        a = F.elu(full)
    elif act == "copy":
        a = full
    return (out if raw else None), a


def _run(x, w, b, r, d, ep, in_amax=True, want_amax=True):
    ops = _ops()
    bias, res, act, raw, res_second, pool2 = ep
    code = {"none": ops.ACT_NONE, "elu": ops.ACT_ELU, "copy": ops.ACT_COPY}[act]
    wq = ops.conv1d_weight(w.cuda())
    before = ops.CONV1D_LAUNCHES
    y = ops.conv1d(x if x.is_cuda else x.cuda(), wq, b.cuda() if bias else None, (r if r.is_cuda else r.cuda()) if res else None,
                   dilation=d, act_out=code, raw=raw, in_amax=in_amax, want_amax=want_amax, res_second=res_second, pool2=pool2)
    assert ops.CONV1D_LAUNCHES == before + 1
    return y if code != ops.ACT_NONE else (y, None)


def _check(got, want, what, rel_only=False):
    ops = _ops()
    for name, g_, w_ in (("out", got[0], want[0]), ("out_act", got[1], want[1])):
        assert (g_ is None) == (w_ is None), (what, name)
        if g_ is None:
            continue
        assert tuple(g_.shape) == tuple(w_.shape), (what, name)
        err = float((g_.cpu().double() - w_).abs().max())
        top = float(w_.abs().max())
        bound = 2e-5 * (top if rel_only else max(1.0, top))
        print(f"{what} {name}: max err {err:.3e} bound {bound:.3e} (max|want| {top:.3e})")
        assert err <= bound, (what, name, err, bound)
        am = ops.amax_of(g_)
        if am is not None:                                       # maxima: exact, per sequence
            assert torch.equal(ops.amax_value(am).cpu(), g_.abs().amax(dim=(1, 2)).cpu()), (what, name)


def _case(N, Cin, Cout, L, k, d, ep_name, seed):
    ep = EPILOGUES[ep_name]
    x, w, b, r = _inputs(N, Cin, Cout, L, k, seed, ep[5])
    got = _run(x, w, b, r, d, ep)
    ops = _ops()
    for t in got:
        if t is not None:
            assert ops.amax_of(t) is not None
    _check(got, _want(x, w, b, r, d, ep), f"N{N} {Cin}->{Cout} L{L} k{k} d{d} {ep_name}")


@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_conv1d_kernel_vs_float64_n5(Cin, Cout):
    """every census shape x length x (k, dilation) at N = 5 (a ragged tile at every length), the epilogues in rotation"""
    i = SHAPES.index((Cin, Cout))
    for li, L in enumerate(LENGTHS):
        for ti, (k, d) in enumerate(TAPS):
            _case(5, Cin, Cout, L, k, d, EP_NAMES[(i * 5 + li * 4 + ti) % len(EP_NAMES)], seed=1000 + i * 100 + li * 10 + ti)


@pytest.mark.parametrize("ep_name", EP_NAMES)
def test_conv1d_every_epilogue_both_tile_shapes(ep_name):
    """every epilogue option on the 128-channel tile (Cout = 256) and on the 64-channel one (Cout = 64), N = 5, k = 3, d = 1 / 2"""
    j = EP_NAMES.index(ep_name)
    _case(5, 128, 256, 24, 3, 1, ep_name, seed=2000 + j)
    _case(5, 128, 64, 12, 3, 2, ep_name, seed=2100 + j)
    _case(1, 64, 128, 48, 3, 4, ep_name, seed=2200 + j)


@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_conv1d_kernel_vs_float64_n1_n512(Cin, Cout):
    """N = 1 (one sequence in a tile of up to 16: a ragged tile) and N = 512 (the production batch: whole tiles only) for every
    census shape; lengths, taps and epilogues in rotation.  N = 5 above is ragged at every length."""
    i = SHAPES.index((Cin, Cout))
    for n_i, N in enumerate((1, 512)):
        L = LENGTHS[(i + n_i) % 3]
        k, d = TAPS[(i + 2 * n_i + 1) % 4]
        _case(N, Cin, Cout, L, k, d, EP_NAMES[(3 * i + 7 * n_i) % len(EP_NAMES)], seed=3000 + 10 * i + n_i)


NEW_LENGTHS = [16, 32, 96]             # 6, 3 and 1 sequences per 96-column group: the lengths LENGTHS does not run


def _new_length_plan(i):
    """the cases of census shape i at the new lengths -> [(N, L, k, d, epilogue name)]: N = 5 at every length x (k, dilation);
    N = 7 at every length (L = 96: two sequences per 64-channel workgroup, so the last one is half empty); N = 1 and N = 512 at
    one length each, so that every length meets both over the six shapes (L = 96 at N = 512 on the shapes with 128 inputs)"""
    plan = []
    for li, L in enumerate(NEW_LENGTHS):
        for ti, (k, d) in enumerate(TAPS):
            plan.append((5, L, k, d, EP_NAMES[(i * 5 + li * 4 + ti) % len(EP_NAMES)]))
        k, d = TAPS[(i + li) % 4]
        plan.append((7, L, k, d, EP_NAMES[(2 * i + 3 * li + 8) % len(EP_NAMES)]))
    for n_i, N in enumerate((1, 512)):
        k, d = TAPS[(i + 2 * n_i + 1) % 4]
        plan.append((N, NEW_LENGTHS[(i + 1 - n_i) % 3], k, d, EP_NAMES[(3 * i + 7 * n_i) % len(EP_NAMES)]))
    return plan


def test_new_length_plan_covers_what_it_should():
    """every new length meets every census shape, the four (k, dilation), N = 1, 5, 7, 512 and the epilogues pool, pool_res_elu,
    res_second and elu_only"""
    for L in NEW_LENGTHS:
        cases = [(i,) + c for i in range(len(SHAPES)) for c in _new_length_plan(i) if c[1] == L]
        assert {c[0] for c in cases} == set(range(len(SHAPES)))
        assert {c[1] for c in cases} == {1, 5, 7, 512}
        assert {(c[3], c[4]) for c in cases} == set(TAPS)
        assert {c[5] for c in cases} >= {"pool", "pool_res_elu", "res_second", "elu_only"}
        for i in range(len(SHAPES)):
            assert {(c[3], c[4]) for c in cases if c[0] == i and c[1] == 5} == set(TAPS)
    assert (7, 96) in {(c[0], c[1]) for c in _new_length_plan(SHAPES.index((128, 64)))}


@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_conv1d_kernel_vs_float64_new_lengths(Cin, Cout):
    """L = 16, 32, 96 (other LDS plane layouts, seam padding and pair-mean widths than 12 / 24 / 48): the same bound, the same
    exact maxima, and _run's launch counter shows the kernel took every case"""
    i = SHAPES.index((Cin, Cout))
    for n, (N, L, k, d, ep_name) in enumerate(_new_length_plan(i)):
        assert _ops().conv1d_pays(Cin, Cout, L, k, d)
        _case(N, Cin, Cout, L, k, d, ep_name, seed=4000 + 100 * i + n)


def test_conv1d_static_range_and_measured_maxima():
    """in_amax=None is the static range contract (|x| < 65504); in_amax=True measures; a producer's vector is taken as given"""
    ops = _ops()
    ep = EPILOGUES["bias_res"]
    x, w, b, r = _inputs(7, 128, 128, 24, 3, 41, False)
    want = _want(x, w, b, r, 1, ep)
    _check(_run(x, w, b, r, 1, ep, in_amax=None, want_amax=False), want, "static")
    xg = x.cuda()
    _check(_run(xg, w, b, r, 1, ep, in_amax=ops.absmax_per_image(xg)), want, "given maxima")
    y = ops.scale_shift_amax(xg, 2.0, -1.0)                       # the first layer's `2x - 1` as a producer
    assert torch.equal(y.cpu(), torch.from_numpy(np.float32(2.0) * x.numpy() + np.float32(-1.0)))
    assert torch.equal(ops.amax_value(ops.amax_of(y)).cpu(), y.abs().amax(dim=(1, 2)).cpu())


@pytest.mark.parametrize("Cout,L,d", [(128, 24, 1), (64, 12, 4), (256, 48, 2), (64, 96, 2), (256, 16, 4)])
def test_conv1d_bits_do_not_depend_on_the_batch(Cout, L, d):
    """a sequence's bits under a batch permutation, and alone versus inside N = 512"""
    ep = EPILOGUES["res_elu_both"]
    N = 512
    x, w, b, r = _inputs(N, 128, Cout, L, 3, 50 + d, False)
    xg, rg = x.cuda(), r.cuda()
    y, ya = _run(xg, w, b, rg, d, ep)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).cuda()
    yp, yap = _run(xg[perm].contiguous(), w, b, rg[perm].contiguous(), d, ep)
    assert torch.equal(yp, y[perm]) and torch.equal(yap, ya[perm])
    for n in (0, 3, 257, 511):
        y1, ya1 = _run(xg[n:n + 1].contiguous(), w, b, rg[n:n + 1].contiguous(), d, ep)
        assert torch.equal(y1[0], y[n]) and torch.equal(ya1[0], ya[n])
    yq = _run(xg, w, b, rg, d, EPILOGUES["pool_res_elu"][:1] + (False,) + EPILOGUES["pool_res_elu"][2:])
    y5 = _run(xg[:5].contiguous(), w, b, rg[:5].contiguous(), d, EPILOGUES["pool_res_elu"][:1] + (False,) + EPILOGUES["pool_res_elu"][2:])
    assert torch.equal(y5[0], yq[0][:5]) and torch.equal(y5[1], yq[1][:5])


def _rescaled(scale, cases):
    ep = EPILOGUES["plain"]
    for (Cin, Cout, L, k, d) in cases:
        x, w, b, r = _inputs(6, Cin, Cout, L, k, 60, False, scale=scale)
        _check(_run(x, w, b, r, d, ep), _want(x, w, b, r, d, ep), f"scale {scale:g} {Cin}->{Cout} L{L} k{k} d{d}", rel_only=True)


@pytest.mark.parametrize("scale", [1e-4, 1e5])
def test_conv1d_rescaled_inputs(scale):
    """inputs at 1e-4 and 1e5 times the unit range: the same bound, relative to the output range"""
    _rescaled(scale, [(128, 128, 24, 3, 1), (256, 128, 12, 3, 4), (64, 128, 48, 1, 1)])


@pytest.mark.parametrize("scale", [1e-4, 1e5])
def test_conv1d_rescaled_inputs_new_lengths(scale):
    _rescaled(scale, [(128, 128, 32, 3, 2), (128, 64, 96, 3, 1), (256, 256, 16, 1, 1)])


def _misaligned_views(off, cases):
    for (Cin, Cout, L, k, d, ep_name) in cases:
        ep = EPILOGUES[ep_name]
        x, w, b, r = _inputs(5, Cin, Cout, L, k, 70 + off, ep[5])
        xb = torch.empty(x.numel() + 4, device="cuda")
        rb = torch.empty(r.numel() + 4, device="cuda")
        xv, rv = xb[off:off + x.numel()].view(x.shape), rb[off:off + r.numel()].view(r.shape)
        xv.copy_(x)
        rv.copy_(r)
        assert xv.data_ptr() % 16 == 4 * off and rv.data_ptr() % 16 == 4 * off and xv.is_contiguous()
        _check(_run(xv, w, b, rv, d, ep), _want(x, w, b, r, d, ep), f"offset {4 * off} B {Cin}->{Cout} L{L} {ep_name}")


@pytest.mark.parametrize("off", [1, 2, 3])
def test_conv1d_misaligned_views(off):
    """`buf[off:]` views 4 / 8 / 12 bytes past a 16-byte boundary as input and residual: no IPDM_EINVAL, the aligned bound"""
    _misaligned_views(off, [(128, 128, 24, 3, 1, "res_elu_both"), (128, 64, 12, 3, 2, "pool_res_elu"),
                            (64, 128, 48, 1, 1, "res_second")])


@pytest.mark.parametrize("off", [1, 2, 3])
def test_conv1d_misaligned_views_new_lengths(off):
    _misaligned_views(off, [(128, 64, 96, 3, 2, "pool_res_elu"), (128, 256, 16, 3, 4, "res_second"), (64, 128, 32, 1, 1, "elu_only")])


def test_fallback_route_is_the_same_convolution():
    """shapes the kernel does not take (few channels, a length that does not divide 96) run as one-row images on the direct 2-D
    kernel: same convolution, same bound; and the standalone pair mean / MaxPool1d / linear resize against torch"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers1d
    ops = _ops()
    g = torch.Generator().manual_seed(80)
    for (Cin, Cout, L, k, d) in [(16, 4, 24, 3, 1), (6, 8, 10, 3, 2), (4, 16, 24, 1, 1), (128, 128, 10, 3, 4)]:
        conv = layers1d.Conv1d(Cin, Cout, k, dilation=d).cuda()
        x = torch.randn(3, Cin, L, generator=g)
        r = torch.randn(3, Cout, L, generator=g)
        assert not conv.conv1d_ok(x)
        before = (ops.CONV1D_LAUNCHES, ops.CONV1D_FALLBACKS)
        y = conv(x.cuda(), residual=r.cuda(), in_amax=True)
        assert (ops.CONV1D_LAUNCHES, ops.CONV1D_FALLBACKS) == (before[0], before[1] + 1)
        want = F.conv1d(x.double(), conv.weight.data.cpu().double(), conv.bias.data.cpu().double(), padding=d * (k // 2),
                        dilation=d) + r.double()
        assert y.shape == want.shape
        assert float((y.cpu().double() - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    x = torch.randn(3, 5, 24, generator=g)
    assert torch.equal(ops.meanpool1d2(x.cuda()).cpu(), (x[:, :, ::2] + x[:, :, 1::2]) / 2)
    assert torch.equal(ops.maxpool1d5(x.cuda()).cpu(), F.max_pool1d(x, 5, 1, 2))
    for Lo in (24, 48, 31):
        want = F.interpolate(x[:, :, :12].double(), size=Lo, mode="linear", align_corners=True)
        got = ops.linear1d(x[:, :, :12].contiguous().cuda(), Lo)
        assert got.shape == want.shape and float((got.cpu().double() - want).abs().max()) < 1e-5
    acc = torch.randn(3, 5, 24, generator=g)
    got = ops.linear1d(x[:, :, :12].contiguous().cuda(), 24, out=acc.cuda(), accumulate=True)
    want = acc.double() + F.interpolate(x[:, :, :12].double(), size=24, mode="linear", align_corners=True)
    assert float((got.cpu().double() - want).abs().max()) < 1e-5


# ---- the reference's own outputs ----------------------------------------------------------------------------------------------
def _act():
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers
    return layers._Act("elu")


def _close(y, ref, what):
    y = y.detach().cpu().numpy()
    assert y.shape == ref.shape, what
    err, top = float(np.abs(y - ref).max()), float(np.abs(ref).max())
    print(f"{what}: max|d| {err:.3e}  bound {2e-4 * top:.3e}")
    assert err <= 2e-4 * top, (what, err, 2e-4 * top)


def test_g33_layers(golden):
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers1d
    g = golden("g33_ncsn1d")
    x = torch.from_numpy(g["blk_x"]).cuda()
    xa, xb = torch.from_numpy(g["rf_xa"]).cuda(), torch.from_numpy(g["rf_xb"]).cuda()

    def load(m, prefix):
        sd = state_dict_from_golden(g, prefix)
        assert sorted(sd) == sorted(m.state_dict()), prefix
        m.load_state_dict(sd, strict=True)
        return m.cuda().eval()
    with torch.no_grad():
        _close(load(layers1d.InstanceNorm1dPlus(6), "in1d")(x), g["in1d_y"], "InstanceNorm1dPlus")
        _close(load(layers1d.CRPBlock(6, 2, _act()), "crp")(x.clone())[0], g["crp_y"], "CRPBlock")
        _close(load(layers1d.RCUBlock(6, 2, 2, _act()), "rcu")(x.clone())[0], g["rcu_y"], "RCUBlock")
        _close(load(layers1d.MSFBlock([6, 4], 5), "msf")([xa, xb], xa.shape[2:]), g["msf_y"], "MSFBlock")
        for name, (planes, feats, kw) in {"rf_start": ([6], 6, dict(start=True)), "rf_two": ([6, 4], 5, {}),
                                          "rf_end": ([6, 4], 6, dict(end=True))}.items():
            m = load(layers1d.RefineBlock(planes, feats, act=_act(), **kw), name)
            xs = [xa.clone()] if len(planes) == 1 else [xa.clone(), xb.clone()]
            _close(m(xs, xa.shape[2:]), g[name + "_y"], name)
        variants = {
            "rb_plain": dict(input_dim=6, output_dim=6, resample=None),
            "rb_pool": dict(input_dim=6, output_dim=8, resample="down"),
            "rb_dil_down": dict(input_dim=6, output_dim=8, resample="down", dilation=2),
            "rb_dil_same": dict(input_dim=6, output_dim=6, resample=None, dilation=4),
        }
        for name, kw in variants.items():
            _close(load(layers1d.ResidualBlock(act=_act(), **kw), name)(x.clone()), g[name + "_y"], name)


@pytest.mark.parametrize("prefix,cls,L", [("n1d", "NCSN1D", 24), ("n1d_deeper", "NCSN1DDeeper", 24),
                                          ("n1d_deepest", "NCSN1DDeepest", 32)])
def test_g33_tiny_networks(golden, prefix, cls, L):
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsn1d
    g = golden("g33_ncsn1d")
    net = getattr(ncsn1d, cls)(cfg1d(image_size=L, device="cuda"))
    net.load_state_dict(state_dict_from_golden(g, prefix), strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g[prefix + "_x"]).cuda(), torch.from_numpy(g[prefix + "_labels"]).cuda())
    assert y.shape == (3, 16, L)
    _close(y, g[prefix + "_y"], cls)


_G34 = []


def _g34_net():
    """-> (the g34 network: NCSN1D at the cine127_1d.yml size with synth_state_dict(seed 0) weights, the golden file); built once"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.models.ncsn1d import NCSN1D
    from inverseproblemwithdiffusionmodel_amd.synthetic import synth_state_dict
    if not _G34:
        g = np.load(os.path.join(TESTS, "golden", "g34_ncsn1d_full.npz"))
        net = NCSN1D(cfg1d(ngf=128, num_classes=400, sigma_begin=40, sigma_end=0.01, channels=64, image_size=24, device="cuda"))
        assert list(net.state_dict().keys()) == list(g["key_names"])
        net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=0), strict=False)
        _G34.append((net.cuda().eval(), g))
    return _G34[0]


def _g34_forward():
    """-> dict of figures and counters for the full-size forward against g34 (used here and by the child process)"""
    from inverseproblemwithdiffusionmodel_amd import ops
    net, g = _g34_net()
    x, labels = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["labels"]).cuda()
    with torch.no_grad():
        net(x, labels)                                           # (packs the weights)
        c0 = (ops.CONV1D_LAUNCHES, ops.CONV1D_FALLBACKS, ops.AMAX_MEASURED)
        y = net(x, labels).cpu().numpy()
        c1 = (ops.CONV1D_LAUNCHES, ops.CONV1D_FALLBACKS, ops.AMAX_MEASURED)
    ref = g["y"]
    n_convs = sum(1 for m in net.modules() if type(m).__name__ == "Conv2d")
    return dict(shape=list(y.shape), finite=bool(np.isfinite(y).all()), max_err=float(np.abs(y - ref).max()),
                max_ref=float(np.abs(ref).max()), nrmse=float(metrics.nrmse(y, ref)), launches=c1[0] - c0[0],
                fallbacks=c1[1] - c0[1], measured=c1[2] - c0[2], n_convs=n_convs, use_conv1d=bool(ops.USE_CONV1D))


def test_g34_full_size_default_path():
    """NCSN1D at the cine127_1d.yml size against the reference's forward; every convolution of the network is the 1-D kernel's
    (the counter shows it took them all) and no input was measured (the maxima travel from producer to consumer)"""
    r = _g34_forward()
    print(r)
    assert r["shape"] == [6, 64, 24] and r["finite"]
    assert r["max_err"] <= 2e-4 * r["max_ref"]
    assert r["nrmse"] < 1e-4
    assert r["use_conv1d"] and r["launches"] == r["n_convs"] and r["fallbacks"] == 0
    assert r["measured"] == 0


@pytest.mark.parametrize("N,pos", [(512, (0, 1, 255, 256, 510, 511)), (256, (0, 1, 127, 128, 254, 255))])
def test_g34_rows_inside_the_production_batch(N, pos):
    """the forward scripts/bench_ncsn1d.py times (N = 512: 65 536 planes at 128 channels, 131 072 at 256, so the glue folds its
    planes into chunks of 65 535; N = 256: 65 536 planes at 256 channels, the second chunk one plane) with g34's six sequences at
    both ends and across the middle of the batch: g34's bounds on those rows against the reference's output, every convolution
    the 1-D kernel's, no input measured, and a permuted batch gives bitwise the permuted output.  Whether the six rows have the
    bits of the N = 6 forward is printed (DESIGN.md 4.3a records the outcome); only the golden bound is asserted there."""
    from inverseproblemwithdiffusionmodel_amd import ops
    net, g = _g34_net()
    gen = torch.Generator().manual_seed(34 + N)
    x = torch.rand(N, 64, 24, generator=gen) * torch.logspace(-1, 1, N).view(N, 1, 1)[torch.randperm(N, generator=gen)]
    labels = torch.randint(0, 400, (N,), generator=gen)
    pos = torch.tensor(pos)
    x[pos], labels[pos] = torch.from_numpy(g["x"]), torch.from_numpy(g["labels"])
    xg, lg = x.cuda(), labels.cuda()
    with torch.no_grad():
        y6 = net(xg[pos.cuda()].contiguous(), lg[pos.cuda()].contiguous())      # (packs the weights on a first call)
        c0 = (ops.CONV1D_LAUNCHES, ops.CONV1D_FALLBACKS, ops.AMAX_MEASURED)
        y = net(xg, lg)
        c1 = (ops.CONV1D_LAUNCHES, ops.CONV1D_FALLBACKS, ops.AMAX_MEASURED)
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(6)).cuda()
        yp = net(xg[perm].contiguous(), lg[perm].contiguous())
    assert y.shape == (N, 64, 24) and bool(torch.isfinite(y).all())
    rows, ref = y[pos.cuda()].cpu().numpy(), g["y"]
    err, top, nrmse = float(np.abs(rows - ref).max()), float(np.abs(ref).max()), float(metrics.nrmse(rows, ref))
    print(f"N{N}: golden rows max err {err:.3e} (max|ref| {top:.3e}, bound {2e-4 * top:.3e}) nrmse {nrmse:.3e}; "
          f"bit-identical to the N = 6 forward: {torch.equal(y[pos.cuda()], y6)}")
    assert err <= 2e-4 * top
    assert nrmse < 1e-4
    n_convs = sum(1 for m in net.modules() if type(m).__name__ == "Conv2d")
    assert ops.USE_CONV1D and c1[0] - c0[0] == n_convs and c1[1] - c0[1] == 0
    assert c1[2] - c0[2] == 0
    assert torch.equal(yp, y[perm])
    err6 = float(np.abs(y6.cpu().numpy() - ref).max())
    assert err6 <= 2e-4 * top


def test_g34_full_size_conv1d_switched_off(tmp_path):
    """a fresh child process with IPDM_CONV1D=0: the same bounds on the one-row route, and the 1-D kernel took no launch"""
    out = str(tmp_path / "child.json")
    env = dict(os.environ, IPDM_CONV1D="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, f"child rc {p.returncode}\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}"
    with open(out) as f:
        r = json.load(f)
    print(r)
    assert r["shape"] == [6, 64, 24] and r["finite"]
    assert r["max_err"] <= 2e-4 * r["max_ref"]
    assert r["nrmse"] < 1e-4
    assert not r["use_conv1d"] and r["launches"] == 0 and r["fallbacks"] == r["n_convs"]


class _SeededNoise:
    def __init__(self, seed):
        self.g, self.calls, self.total = torch.Generator().manual_seed(seed), 0, 0.0

    def __call__(self, like):
        n = torch.randn(like.shape, generator=self.g, dtype=torch.float32)
        self.calls += 1
        self.total += float(n.double().sum())
        return n


@pytest.mark.parametrize("tag,shift", [("plain", False), ("shift", True)])
def test_g35_ald2dtime_with_1d_prior(golden, tag, shift):
    """the reference's ALD2DTime trajectory with the tiny NCSN1D as scorenet_T (4 x 4 patches as 16-channel sequences, T = 8)"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2, ncsn1d, ALD_optimizers, proximal_op
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import SENSE
    from test_scorenet_gpu import tiny_config
    T, H, W = 8, 32, 32
    g7, g17, g33, g = golden("g07_layers"), golden("g17_ald2dtime"), golden("g33_ncsn1d"), golden("g35_ald2dtime_1d")
    net2d = ncsnv2.NCSNv2Deepest(tiny_config())
    net2d.load_state_dict(state_dict_from_golden(g7, "net"), strict=True)
    net2d = net2d.cuda().eval()
    netT = ncsn1d.NCSN1D(cfg1d(image_size=T, device="cuda"))
    netT.load_state_dict(state_dict_from_golden(g33, "n1d"), strict=True)
    netT = netT.cuda().eval()
    op = SENSE("exp", 4, 8, 0.04, (1, H, W), seed=0)
    sigmas, sigmas_T = torch.from_numpy(g["sigmas"]).cuda(), torch.from_numpy(g["sigmas_T"]).cuda()
    params = dict(n_steps_each=2, step_lr=2e-5, denoise=False, final_only=True)
    meas = torch.from_numpy(g17["measurement"]).cuda()
    sampler = ALD_optimizers.ALD2DTime(proximal_op.get_proximal("L2Penalty")(op), netT, sigmas_T, (1, T, 1, H, W), net2d,
                                       sigmas, params, tiny_config(), meas, op, device=torch.device("cuda"))
    lamda_T, n_calls, n_sum = g[f"{tag}_meta"]
    noise = _SeededNoise(350)
    drawn = []
    real_randint = np.random.randint

    def randint(*a, **k):
        v = real_randint(*a, **k)
        drawn.append(np.array(v))
        return v
    np.random.seed(351)
    np.random.randint = randint
    try:
        x = sampler(save_dir=None, lr_scaled=1.0e5, mode_T="diffusion1d", lamda_T=float(lamda_T), if_random_shift=shift,
                    noise_fn=noise)[0].numpy()
    finally:
        np.random.randint = real_randint
    assert noise.calls == int(n_calls) and abs(noise.total - float(n_sum)) < 1e-3       # same stream as the reference run
    if shift:
        assert np.array_equal(np.stack(drawn), g["shift_shifts"]) and len(drawn) == 16
    else:
        assert not drawn
    ref = g[f"{tag}_x"]
    assert x.shape == ref.shape == (1, T, 1, H, W)
    print(f"{tag}: nrmse {metrics.nrmse(np.abs(x), np.abs(ref)):.3e}")
    assert metrics.nrmse(np.abs(x), np.abs(ref)) < 1e-3
    for t in range(T):
        assert abs(metrics.ssim(np.abs(x[0, t, 0]), np.abs(ref[0, t, 0])) - 1) < 1e-3


def test_cine_2d_time_script_with_1d_prior(tmp_path):
    """scripts/cine_SENSE_real_img_2d_time.py --temporal_type Diffusion1D at the size test_scripts_gpu.py runs this driver"""
    from test_scripts_gpu import run_script, _load
    d = str(tmp_path)
    out = run_script("cine_SENSE_real_img_2d_time.py", ["--R", 8, "--num_samples", 1, "--mode_T", "diffusion1d", "--lamda_T", 10.0,
                                                       "--image_size", 64, "--start_level", 996, "--n_levels", 2, "--save_dir", d,
                                                       "--temporal_type", "Diffusion1D"])
    assert "reconstruction time" in out
    rec = _load(d, "reconstructions.pt")
    assert rec.shape == (1, 24, 1, 64, 64) and rec.dtype == torch.complex64 and torch.isfinite(torch.view_as_real(rec)).all()


if __name__ == "__main__":
    res = _g34_forward()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
