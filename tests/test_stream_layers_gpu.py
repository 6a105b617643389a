"""The score network's first and last layer leave nothing for a second pass over their 128-channel tensors:
  * ops.conv3x3_fewout_fin (csrc/fewout_fin.hip): end_conv(act(InstanceNorm++(x))) from the RAW x and the coefficients, bit for bit
    what ops.affine_act -> ops.conv3x3_thin store (`IPDM_THIN_FIN`);
  * ops.conv3x3_thin(want_stats=True) (csrc/conv_thin.hip): the first layer's statistics partials for the InstanceNorm++ that reads
    it next (`IPDM_THIN_STATS`); the network's last refine block asks its last convolution for the same (`IPDM_END_STATS`);
  * one NCSNv2Deepest forward with the three switches on against all off, eagerly and as a replayed graph."""
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ELU = 1


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from inverseproblemwithdiffusionmodel_amd import ops
    return ops


def _traced(ops, fn):
    ops.CONV_TRACE = []
    try:
        with torch.no_grad():
            y = fn()
        return y, [{k: v for k, v in r.items() if k not in ("e0", "e1")} for r in ops.CONV_TRACE]
    finally:
        ops.CONV_TRACE = None


# ---- the last layer --------------------------------------------------------------------------------------------------------------
def _fewout_case(H, W, B=3, Cin=128, Cout=1, seed=51):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=gen) * 2 + 0.5
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.2
    b = torch.randn(Cout, generator=gen)
    coef = torch.randn(B, Cin, 3, generator=gen)
    coef[:, :, 1] = coef[:, :, 1] * 0.3 + 1.0
    # image 1: every normalised value below zero (|x - mu| * 0.1 stays under 2, the shift is -5): every ELU on the exponential side
    coef[1, :, 1] = 0.1
    coef[1, :, 2] = -5.0
    return x, w, b, coef


def _fewout_oracle(x, w, b, coef):
    xd, c = x.double(), coef.double()
    a = F.elu((xd - c[:, :, 0, None, None]) * c[:, :, 1, None, None] + c[:, :, 2, None, None])
    return a, F.conv2d(a, w.double(), b.double(), padding=1)


@pytest.mark.parametrize("Cout", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 8), (12, 20)])                # 12 x 20: five quads per row, no cross-lane halo
def test_fewout_fused_norm_input(ops, H, W, Cout):
    """against the separate passes (the parent's path, what IPDM_THIN_FIN=0 runs) bit for bit, and against float64 with the bound
    test_conv3x3_thin sets for a fused input affine: 4e-6 * max(1, max|ref|); both paths' errors are printed"""
    x, w, b, coef = _fewout_case(H, W, Cout=Cout)
    act64, want = _fewout_oracle(x, w, b, coef)
    assert float(act64[1].max()) < 0.0                          # the all-negative image
    xg, wg, bg, cg = x.cuda(), w.cuda(), b.cuda(), coef.cuda()
    assert ops.conv3x3_fewout_fin_ok(128, Cout, H, W, xg)
    parent = ops.conv3x3_thin(ops.affine_act(xg, cg, ELU), wg, bg)
    got = ops.conv3x3_fewout_fin(xg, wg, bg, cg, ELU)
    scale = max(1.0, float(want.abs().max()))
    e_new, e_par = float((got.cpu().double() - want).abs().max()), float((parent.cpu().double() - want).abs().max())
    print(f"fewout {H}x{W} Cout {Cout}: max error against float64, fused {e_new:.3e}, separate passes {e_par:.3e} (bound {4e-6 * scale:.3e})")
    assert torch.equal(got, parent)
    assert e_new <= 4e-6 * scale
    assert torch.equal(ops.conv3x3_fewout_fin(xg, wg, None, cg, ELU), ops.conv3x3_thin(ops.affine_act(xg, cg, ELU), wg, None))
    # a sample's result does not depend on the batch around it
    assert torch.equal(ops.conv3x3_fewout_fin(xg[1:2].contiguous(), wg, bg, cg[1:2].contiguous(), ELU), got[1:2])


def test_fewout_odd_channel_counts_and_ragged_strips(ops):
    """channel counts that leave the four channel groups and the two-channel trips uneven; H that is no multiple of the rows a
    thread owns"""
    for Cin, Cout, H, W in [(6, 1, 5, 8), (7, 2, 3, 12), (13, 3, 7, 16), (5, 1, 1, 4)]:
        x, w, b, coef = _fewout_case(H, W, B=2, Cin=Cin, Cout=Cout, seed=52)
        xg, wg, bg, cg = x.cuda(), w.cuda(), b.cuda(), coef.cuda()
        got = ops.conv3x3_fewout_fin(xg, wg, bg, cg, ELU)
        assert torch.equal(got, ops.conv3x3_thin(ops.affine_act(xg, cg, ELU), wg, bg)), (Cin, Cout, H, W)
        want = _fewout_oracle(x, w, b, coef)[1]
        assert (got.cpu().double() - want).abs().max() <= 4e-6 * max(1.0, float(want.abs().max()))


def test_fewout_unaligned_input_takes_the_separate_passes(ops):
    """a contiguous view off a 16-byte boundary: the layer says no, the entry says unsupported (never "invalid argument"), and
    the separate passes run -- CONV_TRACE shows the streaming kernel without the fused input"""
    from inverseproblemwithdiffusionmodel_amd import _lib
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import layers
    x, w, b, coef = _fewout_case(8, 8)
    conv = layers.Conv2d(128, 1, 3).cuda()
    conv.weight.data.copy_(w)
    conv.bias.data.copy_(b)
    cg = coef.cuda()
    buf = torch.zeros(x.numel() + 8).cuda()
    want = None
    for k in (0, 1, 2, 3):
        xm = buf[k:k + x.numel()].view(x.shape)
        xm.copy_(x)
        assert xm.data_ptr() % 16 == 4 * k
        assert conv.streams_norm_input(xm, ELU) == (k == 0)
        if k:
            with pytest.raises(_lib.IpdmUnsupported):
                ops.conv3x3_fewout_fin(xm, conv.weight.data, conv.bias.data, cg, ELU)
        run = (lambda: conv.stream_norm_input(xm, cg, ELU)) if k == 0 else (lambda: conv(ops.affine_act(xm, cg, ELU)))
        y, trace = _traced(ops, run)
        assert len(trace) == 1 and trace[0].get("thin") and bool(trace[0].get("fin")) == (k == 0), trace
        want = y if want is None else want
        assert torch.equal(y, want)


# ---- the first layer's statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 32), (24, 40)])              # 64 quads: one partial; 240 quads: four, the last one ragged
@pytest.mark.parametrize("Cin", [1, 3])
def test_fewin_statistics_partials(ops, H, W, Cin):
    """InstanceNorm++ coefficients from the partials against a pass over the stored tensor, with test_wino1d_statistics_epilogue's
    bounds; the partial counts cover the plane exactly; the stored tensor has the bits of the launch without the epilogue"""
    B, Cout = 2, 128
    gen = torch.Generator().manual_seed(53)
    x = torch.rand(B, Cin, H, W, generator=gen).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.3).cuda()
    b = (torch.randn(Cout, generator=gen) * 2).cuda()
    coef = torch.tensor([0.5, 2.0, 0.0]).repeat(B, Cin, 1).cuda()
    P = int(ops._lib.lib.ipdm_conv3x3_thin_stats_partials(Cin, Cout, H, W))
    assert P == (H * (W // 4) + 63) // 64
    y0 = ops.conv3x3_thin(x, w, b, coef)
    y1 = ops.conv3x3_thin(x, w, b, coef, want_stats=True)
    assert torch.equal(y0, y1) and hasattr(y1, "_ipdm_partials") and not hasattr(y0, "_ipdm_partials")
    part, tag = y1._ipdm_partials
    assert tuple(part.shape) == (B, Cout, P, 3) and tag == (y1._version, y1.data_ptr())
    assert float(part[..., 0].sum(dim=2).min()) == H * W == float(part[..., 0].sum(dim=2).max())
    alpha, gamma, beta = (torch.randn(Cout, generator=gen).cuda() for _ in range(3))
    c_part = ops.instnorm_plus_coef(y1, alpha, gamma, beta)
    assert not hasattr(y1, "_ipdm_partials")
    c_full = ops.instnorm_plus_coef(y0, alpha, gamma, beta)              # plane_stats_kernel on the written tensor
    print(f"fewin {Cin} -> {Cout} {H}x{W}: coefficients from partials against a pass: {float((c_part - c_full).abs().max() / c_full.abs().max()):.3e} (bound 2e-5)")
    assert (c_part - c_full).abs().max() <= 2e-5 * c_full.abs().max()
    yd = y0.double()
    mean = yd.mean(dim=(2, 3))
    rstd = 1.0 / torch.sqrt(yd.var(dim=(2, 3), unbiased=False) + 1e-5)
    assert (c_part[..., 0].double() - mean).abs().max() <= 1e-6 * mean.abs().max()
    assert ((c_part[..., 1] / gamma).double() / rstd - 1).abs().max() <= 1e-5
    # the few-output form has no such epilogue: the request is ignored
    assert int(ops._lib.lib.ipdm_conv3x3_thin_stats_partials(128, 1, H, W)) == 0


# ---- the whole network ------------------------------------------------------------------------------------------------------------
SWITCHES = ("THIN_STATS", "THIN_FIN", "END_STATS")


@pytest.fixture(scope="module")
def net32(ops):
    from inverseproblemwithdiffusionmodel_amd.ncsn.models import ncsnv2
    cfg = Namespace(device=torch.device("cuda"),
                    data=Namespace(channels=1, image_size=32, logit_transform=False, rescaled=False),
                    model=Namespace(ngf=128, num_classes=10, sigma_begin=1.0, sigma_end=0.01, sigma_dist="geometric",
                                    normalization="InstanceNorm++", nonlinearity="elu", spec_norm=False))
    torch.manual_seed(54)
    net = ncsnv2.NCSNv2Deepest(cfg).cuda().eval()
    gen = torch.Generator().manual_seed(55)
    return net, torch.rand(2, 1, 32, 32, generator=gen).cuda(), torch.tensor([1, 7]).cuda()


def _forward(ops, net32, **switches):
    net, x, labels = net32
    saved = {k: getattr(ops, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(ops, k, v)
        return _traced(ops, lambda: net(x, labels))
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def test_network_switches_on_against_off(ops, net32):
    """bit for bit but through the statistics: the fused last layer alone keeps every bit; with the partials on, the output moves
    no further than it does under IPDM_WINO1D_STATS (the existing switch between two sources of statistics), measured here"""
    off = {k: False for k in SWITCHES}
    y_off, t_off = _forward(ops, net32, **off)
    y_on, t_on = _forward(ops, net32)
    assert all(getattr(ops, k) for k in SWITCHES)                # the default
    assert len(t_on) == len(t_off)
    assert sum(1 for r in t_on if r.get("fin")) == 1 and not any(r.get("fin") for r in t_off)
    assert t_on[0].get("thin") and t_on[0].get("stats") and not t_off[0].get("stats")
    assert t_on[-2].get("stats") and not t_off[-2].get("stats")  # the last refine block's last convolution
    y_fin, _ = _forward(ops, net32, THIN_STATS=False, END_STATS=False)
    assert torch.equal(y_fin, y_off)
    y_w, _ = _forward(ops, net32, WINO1D_STATS=False, **off)
    bound = float((y_w - y_off).abs().max())
    moved = float((y_on - y_off).abs().max())
    print(f"network 2 x 32 x 32: new switches on against off {moved:.3e}; IPDM_WINO1D_STATS on against off {bound:.3e}; max|y| {float(y_off.abs().max()):.3e}")
    assert moved <= bound


def test_network_graph_replays_equal_eager(ops, net32):
    net, x, labels = net32
    with torch.no_grad():
        eager = net(x, labels).clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = net(x, labels)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
