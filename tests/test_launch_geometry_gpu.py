"""Launch geometry of the glue kernels and the small NCSN++ kernels (csrc/norm_act.hip, csrc/nn_extra.hip).

Part 1 -- plane counts across gridDim.y = 65 535.  A temporal step of the 1-D prior is 512 sequences of 128 / 256 channels
(DESIGN.md 4.3a): 65 536 / 131 072 (sequence, channel) planes, where the launchers fold the planes into chunks of 65 535
(affine_act, the tiled pools), leave the LDS resize for the grid-stride ones, refuse (affine_act_cat: the wrapper concatenates)
or reject (div_sigma, sample_axpy2, attention).  Every op runs at P = 65 535, 65 536, 65 537 and 131 073 planes of 1 x 24,
1 x 12, 1 x 10, 4 x 4 and 3 x 5 elements against float64 on the CPU.  Every plane has its own mean (spread over +-50) and its own
coefficient row, so a row or a pointer taken from the wrong plane or chunk misses by tens, not by round-off.  Two assertions per
op: (a) the bound of the op's existing test (named at each test); (b) planes 0, 65 534, 65 535, 65 536 and the last one have
the bits they have in a batch of a handful of planes, wherever both batches run the same kernel form (where the form changes
with the plane count the outcome is printed).
The resizes are judged against fp32 torch with the absolute 2e-6 of test_kernels_gpu.test_bilinear, which holds for values of
order one (an interpolation of values near 50 differs by ulps of 50 between two fp32 evaluations): their planes are unit normal,
where a wrong plane still misses by order one.

Part 4 -- attention, linear, sample_norm, sample_axpy2 called directly at ragged sizes.  No tolerance of theirs exists in the
project; the idiom of test_kernels_gpu.test_instnorm_plus_sizes: the same formula in fp32 torch on the CPU, both judged against
float64, and err_gpu <= max(2e-5 * max(1, max|want|), 2 * err_cpu) (the factor 2: another summation order).  Both errors are
printed for every case."""
import pytest
import torch
import torch.nn.functional as F

from oracle import scorenet

pytestmark = pytest.mark.gpu

PLANES = [65535, 65536, 65537, 131073]
SHAPES = [(1, 24), (1, 12), (1, 10), (4, 4), (3, 5)]
# (B, C) with B * C = P: C > 1 for InstanceNorm++ (a variance over one channel mean is NaN), B <= 65 535 for the per-image maxima
FACTOR = {65535: (21845, 3), 65536: (8192, 8), 65537: (1, 65537), 131073: (43691, 3)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from inverseproblemwithdiffusionmodel_amd import ops as _ops
    return _ops


def _probe(P):
    """the planes whose bits are compared with a small batch: either side of the fold, and the last one"""
    return sorted({p for p in (0, 65534, 65535, 65536, P - 1) if p < P})


def _planes(P, h, w, seed, spread=50.0):
    """-> (x [P, 1, h, w], the per-plane offsets [P]): every plane its own mean in +-spread and its own width"""
    g = torch.Generator().manual_seed(seed)
    off = (torch.rand(P, generator=g) * 2 - 1) * spread
    x = torch.randn(P, 1, h, w, generator=g) * (0.5 + 2.5 * torch.rand(P, 1, 1, 1, generator=g)) + off.view(P, 1, 1, 1)
    return x, off


def _rows(off, seed):
    """arbitrary coefficient rows [P, 1, 3] = (mu near the plane's own mean, scale in [0.5, 1.5], shift): another plane's row
    misses by |difference of the means| * scale, tens here"""
    g = torch.Generator().manual_seed(seed)
    P = off.numel()
    return torch.stack([off + 0.3 * torch.randn(P, generator=g), 0.5 + torch.rand(P, generator=g),
                        2.0 * torch.randn(P, generator=g)], dim=-1).view(P, 1, 3)


def _apply(x, coef):
    return (x - coef[..., 0, None, None]) * coef[..., 1, None, None] + coef[..., 2, None, None]


def _act_ref(v, code, ops):
    return {ops.ACT_ELU: F.elu, ops.ACT_RELU: F.relu, ops.ACT_LRELU02: lambda t: F.leaky_relu(t, 0.2),
            ops.ACT_SWISH: lambda t: t * torch.sigmoid(t)}.get(code, lambda t: t)(v)


def _act_codes(ops):
    return sorted(set(ops.ACT_CODES.values()) | {ops.ACT_COPY})


def _instnorm_ref(x, alpha, gamma, beta):
    """InstanceNorm++ (normalization.py:150-176; the conditional form :193-208 with per-image rows) in x's precision;
    alpha / gamma / beta broadcast against [B, C]"""
    means = x.mean(dim=(2, 3))
    m = means.mean(dim=-1, keepdim=True)
    v = means.var(dim=-1, keepdim=True)
    mn = (means - m) / torch.sqrt(v + 1e-5)
    h = F.instance_norm(x, eps=1e-5) + (mn * alpha)[..., None, None]
    out = (gamma * torch.ones_like(mn))[..., None, None] * h
    return out if beta is None else out + (beta * torch.ones_like(mn))[..., None, None]


def _misaligned(t, k=1):
    """a contiguous GPU copy of t that starts 4 * k bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    lead = (-buf.data_ptr() % 16) // t.element_size()
    v = buf[lead + k:lead + k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * k and v.is_contiguous()
    return v


def _norm_bound(got, want32, exact, what):
    """test_instnorm_plus_sizes: the kernel and the fp32 CPU evaluation against float64, max(2e-5, 2 * err_cpu)"""
    err_gpu = float((got.double() - exact).abs().max())
    err_cpu = float((want32.double() - exact).abs().max())
    print(f"{what}: err_gpu {err_gpu:.3e} err_cpu {err_cpu:.3e}")
    assert err_gpu <= max(2e-5, 2 * err_cpu), (what, err_gpu, err_cpu)
    return err_gpu


# ---- part 1: affine_act -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("P", PLANES)
def test_affine_act_across_the_fold(ops, P, hw):
    """every activation code with arbitrary per-plane rows and with instnorm_plus_coef's; a view 4 bytes off a 16-byte boundary
    (the scalar branch) gives the aligned bits; the probe planes have the bits of a batch of five"""
    h, w = hw
    x, off = _planes(P, h, w, seed=P % 1000 + 10 * h + w)
    coef = _rows(off, seed=7 + w)
    xg, cg = x.cuda(), coef.cuda()
    pre64, pre32 = _apply(x.double(), coef.double()), _apply(x, coef)
    idx = torch.tensor(_probe(P))
    xs, cs = x[idx].cuda(), coef[idx].cuda()
    xm = _misaligned(xg)
    for code in _act_codes(ops):
        got = ops.affine_act(xg, cg, code)
        _norm_bound(got.cpu(), _act_ref(pre32, code, ops), _act_ref(pre64, code, ops), f"affine_act P{P} {h}x{w} act{code} rows")
        assert torch.equal(ops.affine_act(xm, cg, code), got), ("misaligned view", code)
        assert torch.equal(ops.affine_act(xs, cs, code), got[idx.cuda()]), ("bits against a batch of five", code)
    # the coefficients InstanceNorm++ computes, on the (B, C) factorisation of P
    B, C = FACTOR[P]
    g = torch.Generator().manual_seed(3)
    al, ga, be = 1 + 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xb = x.view(B, C, h, w)
    xbg = xg.view(B, C, h, w)
    ci = ops.instnorm_plus_coef(xbg, al.cuda(), ga.cuda(), be.cuda())
    n64 = _instnorm_ref(xb.double(), al.double(), ga.double(), be.double())
    n32 = _instnorm_ref(xb, al, ga, be)
    cflat = ci.view(P, 1, 3)
    for code in _act_codes(ops):
        got = ops.affine_act(xbg, ci, code)
        _norm_bound(got.cpu(), _act_ref(n32, code, ops), _act_ref(n64, code, ops), f"affine_act P{P} {h}x{w} act{code} instnorm")
        assert torch.equal(ops.affine_act(xs, cflat[idx.cuda()].contiguous(), code), got.view(P, 1, h, w)[idx.cuda()]), code


# ---- part 1: InstanceNorm++ coefficients at the production batch ---------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("B,C", [(512, 128), (512, 256), (8193, 8)])
def test_instnorm_coefficients_at_the_production_batch(ops, B, C, hw):
    """instnorm_plus_coef and cond_instnorm_plus_coef at 65 536 / 131 072 / 65 544 planes against the float64 formula; the images
    that hold the probe planes have the coefficient bits they have in a batch of their own"""
    h, w = hw
    P = B * C
    x, _ = _planes(P, h, w, seed=B + C + 10 * h + w)
    x = x.view(B, C, h, w)
    xg = x.cuda()
    g = torch.Generator().manual_seed(5)
    al, ga, be = 1 + 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    coef = ops.instnorm_plus_coef(xg, al.cuda(), ga.cuda(), be.cuda())
    got = ops.affine_act(xg, coef, ops.ACT_NONE).cpu()
    _norm_bound(got, _instnorm_ref(x, al, ga, be), _instnorm_ref(x.double(), al.double(), ga.double(), be.double()),
                f"instnorm_plus_coef B{B} C{C} {h}x{w}")
    imgs = torch.tensor(sorted({p // C for p in _probe(P)}))
    small = ops.instnorm_plus_coef(x[imgs].cuda(), al.cuda(), ga.cuda(), be.cuda())
    assert torch.equal(small, coef[imgs.cuda()])
    if ops.dynamic_range():
        assert (got.abs().amax(dim=(1, 2, 3)) <= ops.amax_value(coef._ipdm_amax_bound).cpu()).all()
    # conditional: one embedding row per image, picked on the device
    nc = 7
    embed = 1.0 + 0.3 * torch.randn(nc, 3 * C, generator=g)
    embed[:, 2 * C:] = 0.5 * torch.randn(nc, C, generator=g)
    labels = torch.randint(0, nc, (B,), generator=g)
    e = embed[labels]
    cc = ops.cond_instnorm_plus_coef(xg, embed.cuda(), labels.cuda())
    got = ops.affine_act(xg, cc, ops.ACT_NONE).cpu()
    _norm_bound(got, _instnorm_ref(x, e[:, C:2 * C], e[:, :C], e[:, 2 * C:]),
                _instnorm_ref(x.double(), e[:, C:2 * C].double(), e[:, :C].double(), e[:, 2 * C:].double()),
                f"cond_instnorm_plus_coef B{B} C{C} {h}x{w}")
    small = ops.cond_instnorm_plus_coef(x[imgs].cuda(), embed.cuda(), labels[imgs].cuda())
    assert torch.equal(small, cc[imgs.cuda()])


# ---- part 1: pools ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("P", PLANES)
def test_maxpool5_across_the_fold(ops, P, hw):
    """exact (test_kernels_gpu.test_maxpool5); W % 4 == 0 is the strip form, the other widths and a misaligned view the tiled one
    and its fold; maxpool1d5 on the one-row shapes"""
    h, w = hw
    x, _ = _planes(P, h, w, seed=P % 1000 + h + 10 * w)
    want = F.max_pool2d(x, 5, 1, 2)
    xg = x.cuda()
    got = ops.maxpool5(xg)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.maxpool5(_misaligned(xg)).cpu(), want)                  # tiled form at every width
    idx = torch.tensor(_probe(P))
    assert torch.equal(ops.maxpool5(x[idx].cuda()), got[idx.cuda()])
    if h == 1:
        B, C = FACTOR[P]
        got1 = ops.maxpool1d5(xg.view(B, C, w))
        assert got1.shape == (B, C, w) and torch.equal(got1.cpu(), F.max_pool1d(x.view(B, C, w), 5, 1, 2))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("P", PLANES)
def test_affine_avgpool5_across_the_fold(ops, P, hw):
    """test_ncsn1_gpu.test_affine_avgpool5_kernel's bound (1e-5 * max(1, max|ref|) against float64) and its bit-equality of the
    strip and the tiled form; every plane its own coefficient row"""
    h, w = hw
    x, off = _planes(P, h, w, seed=P % 1000 + 3 * h + w)
    coef = _rows(off, seed=11 + h)
    xg, cg = x.cuda(), coef.cuda()
    ref = F.avg_pool2d(_apply(x.double(), coef.double()), 5, stride=1, padding=2, count_include_pad=True)
    got = ops.affine_avgpool5(xg, cg)
    err, top = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
    print(f"affine_avgpool5 P{P} {h}x{w}: err {err:.3e} bound {1e-5 * max(1.0, top):.3e}")
    assert err <= 1e-5 * max(1.0, top)
    assert torch.equal(ops.affine_avgpool5(_misaligned(xg), cg), got)              # tiled form, folded
    idx = torch.tensor(_probe(P))
    assert torch.equal(ops.affine_avgpool5(x[idx].cuda(), coef[idx].cuda()), got[idx.cuda()])


@pytest.mark.parametrize("P", PLANES)
def test_meanpools_across_the_fold(ops, P):
    """exact (test_kernels_gpu.test_meanpool2, test_ncsn1d_gpu's pair mean): 2 x 2 on 4 x 4 and 2 x 10 planes, pairs on the
    one-row lengths"""
    idx = torch.tensor(_probe(P))
    for (h, w) in [(4, 4), (2, 10)]:
        x, _ = _planes(P, h, w, seed=P % 1000 + h + w)
        got = ops.meanpool2(x.cuda())
        assert torch.equal(got.cpu(), scorenet.mean_pool2(x))
        assert torch.equal(ops.meanpool2(_misaligned(x.cuda())), got)
        assert torch.equal(ops.meanpool2(x[idx].cuda()), got[idx.cuda()])
    B, C = FACTOR[P]
    for L in (24, 12, 10):
        x = _planes(P, 1, L, seed=P % 1000 + L)[0].view(B, C, L)
        got = ops.meanpool1d2(x.cuda())
        assert got.shape == (B, C, L // 2) and torch.equal(got.cpu(), (x[:, :, ::2] + x[:, :, 1::2]) / 2)
        xs = x.view(P, 1, L)[idx]
        assert torch.equal(ops.meanpool1d2(xs.cuda()), got.view(P, 1, L // 2)[idx.cuda()])


# ---- part 1: resizes ----------------------------------------------------------------------------------------------------------
def _linear_want(x, Lo):
    B, C, L = x.shape
    return F.interpolate(x.view(B, C, 1, L), size=(1, Lo), mode="bilinear", align_corners=True).view(B, C, Lo)


@pytest.mark.parametrize("Li,Lo", [(12, 24), (24, 24), (12, 31)])
@pytest.mark.parametrize("P", PLANES)
def test_linear1d_across_the_grid_limit(ops, P, Li, Lo):
    """test_kernels_gpu.test_bilinear's bound (2e-6 against fp32 torch), plain and accumulated under ELU, with and without the
    maxima (exact, per image).  Up to 65 535 planes 12 -> 24 and 24 -> 24 are the LDS kernel's, above it bilinear4_kernel's:
    there the bits against the small batch are printed, everywhere else asserted."""
    B, C = FACTOR[P]
    g = torch.Generator().manual_seed(P % 1000 + Li + Lo)
    x = torch.randn(B, C, Li, generator=g)
    acc = torch.randn(B, C, Lo, generator=g)
    want = _linear_want(x, Lo)
    want_acc = F.elu(acc + want)
    xg = x.cuda()
    got = ops.linear1d(xg, Lo)
    err = float((got.cpu() - want).abs().max())
    assert ops.amax_of(got) is None
    ra = ops.linear1d(xg, Lo, want_amax=True)
    assert torch.equal(ra, got)
    assert torch.equal(ops.amax_value(ops.amax_of(ra)), ra.abs().amax(dim=(1, 2)))
    out = acc.clone().cuda()
    ops.linear1d(xg, Lo, out=out, accumulate=True, act=ops.ACT_ELU)
    err_acc = float((out.cpu() - want_acc).abs().max())
    out2 = acc.clone().cuda()
    r2 = ops.linear1d(xg, Lo, out=out2, accumulate=True, act=ops.ACT_ELU, want_amax=True)
    assert torch.equal(out2, out)
    assert torch.equal(ops.amax_value(ops.amax_of(r2)), out2.abs().amax(dim=(1, 2)))
    print(f"linear1d P{P} {Li}->{Lo}: err {err:.3e} accumulated+ELU {err_acc:.3e} (bound 2e-6)")
    assert err < 2e-6 and err_acc < 2e-6
    if Li == Lo:
        assert torch.equal(got.cpu(), x)                                           # identity resize is exact
    idx = torch.tensor(_probe(P))
    small = ops.linear1d(x.view(P, 1, Li)[idx].cuda(), Lo)
    same = torch.equal(small, got.view(P, 1, Lo)[idx.cuda()])
    osm = acc.view(P, 1, Lo)[idx].cuda()
    ops.linear1d(x.view(P, 1, Li)[idx].cuda(), Lo, out=osm, accumulate=True, act=ops.ACT_ELU)
    same_acc = torch.equal(osm, out.view(P, 1, Lo)[idx.cuda()])
    same_form = P <= 65535 or Li % 4 != 0 or Lo % 4 != 0
    print(f"linear1d P{P} {Li}->{Lo}: probe planes bit-equal to a batch of five: plain {same}, accumulated {same_acc} "
          f"({'same kernel form' if same_form else 'LDS kernel against bilinear4_kernel'})")
    if same_form:
        assert same and same_acc


@pytest.mark.parametrize("B", [65535, 65536])
def test_resize_maxima_either_side_of_the_wrapper_limit(ops, B):
    """C = 1, through linear1d, bilinear and trilinear: 65 535 images carry exact maxima; 65 536 carry none (the wrapper drops
    want_amax) and the values are still right"""
    g = torch.Generator().manual_seed(B % 100)
    x = torch.randn(B, 1, 12, generator=g)
    want = _linear_want(x, 24)
    r = ops.linear1d(x.cuda(), 24, want_amax=True)
    assert float((r.cpu() - want).abs().max()) < 2e-6
    x4 = x.view(B, 1, 1, 12).cuda()
    r4 = ops.bilinear(x4, (1, 24), want_amax=True)
    assert torch.equal(r4.view(B, 1, 24), r)
    x5 = x.view(B, 1, 1, 1, 12).cuda()
    r5 = ops.trilinear(x5, (1, 1, 24), want_amax=True)                             # (test_kernels_gpu.test_trilinear's bounds)
    want5 = F.interpolate(x.view(B, 1, 1, 1, 12).double(), size=(1, 1, 24), mode="trilinear", align_corners=True)
    assert float((r5.cpu().double() - want5).abs().max()) < 2e-5
    assert float((r5.cpu() - F.interpolate(x.view(B, 1, 1, 1, 12), size=(1, 1, 24), mode="trilinear",
                                           align_corners=True)).abs().max()) < 2e-6
    for t, dims in ((r, (1, 2)), (r4, (1, 2, 3)), (r5, (1, 2, 3, 4))):
        am = ops.amax_of(t)
        if B <= 65535:
            assert am is not None and torch.equal(ops.amax_value(am), t.abs().amax(dim=dims))
        else:
            assert am is None


# ---- part 1: the two-source GroupNorm past one grid.y -------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8191, 8193])
def test_groupnorm_act_cat_concatenation_fallback(ops, B):
    """B * (C1 + C2) = 65 528 is the two-source kernel's, 65 544 answers IPDM_EUNSUPPORTED and the wrapper concatenates:
    test_score_sde_gpu's bound (2e-5 * max(1, max|ref|) against float64 group_norm + swish) on both sides, maxima exact"""
    C1 = C2 = 4
    G = 2
    x, _ = _planes(B * (C1 + C2), 2, 2, seed=B)
    x = x.view(B, C1 + C2, 2, 2)
    g = torch.Generator().manual_seed(2)
    wt, bs = 1 + 0.3 * torch.randn(C1 + C2, generator=g), torch.randn(C1 + C2, generator=g)
    want = F.silu(F.group_norm(x.double(), G, wt.double(), bs.double(), eps=1e-6))
    x1, x2 = x[:, :C1].contiguous().cuda(), x[:, C1:].contiguous().cuda()
    got = ops.groupnorm_act_cat(x1, x2, wt.cuda(), bs.cuda(), G, act=ops.ACT_SWISH)
    err, top = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
    print(f"groupnorm_act_cat B{B}: err {err:.3e} bound {2e-5 * max(1.0, top):.3e}")
    assert got.shape == want.shape and err <= 2e-5 * max(1.0, top)
    got2, am = ops.groupnorm_act_cat(x1, x2, wt.cuda(), bs.cuda(), G, act=ops.ACT_SWISH, want_amax=True)
    assert float((got2.cpu().double() - want).abs().max()) <= 2e-5 * max(1.0, top)
    assert torch.equal(ops.amax_value(am).cpu(), x.abs().amax(dim=(1, 2, 3)))
    imgs = torch.tensor(sorted({p // (C1 + C2) for p in _probe(B * (C1 + C2))}))
    small = ops.groupnorm_act_cat(x1[imgs.cuda()].contiguous(), x2[imgs.cuda()].contiguous(), wt.cuda(), bs.cuda(), G,
                                  act=ops.ACT_SWISH)
    same = torch.equal(small, got[imgs.cuda()])
    print(f"groupnorm_act_cat B{B}: probe images bit-equal to the two-source kernel on a batch of their own: {same}")
    if B * (C1 + C2) <= 65535:
        assert same


# ---- part 1: grid-stride in x only ----------------------------------------------------------------------------------------------
def test_elementwise_at_the_production_element_count(ops):
    """add, act, scale_shift at 131 073 x 24 elements (test_kernels_gpu.test_elementwise's assertions)"""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(131073, 1, 1, 24, generator=g) * 2
    y = torch.randn(131073, 1, 1, 24, generator=g)
    xg = x.cuda()
    assert torch.equal(ops.add(xg, y.cuda()).cpu(), x + y)
    assert torch.equal(ops.scale_shift(xg, 2.0, -1.0).cpu(), 2 * x - 1.0)
    for name, fn in [("elu", F.elu), ("relu", F.relu), ("lrelu", lambda t: F.leaky_relu(t, 0.2)),
                     ("swish", lambda t: t * torch.sigmoid(t))]:
        got = ops.act(xg, ops.ACT_CODES[name])
        assert (got.cpu() - fn(x)).abs().max() < 1e-6, name
        idx = torch.tensor(_probe(131073)).cuda()
        assert torch.equal(ops.act(xg[idx].contiguous(), ops.ACT_CODES[name]), got[idx]), name


# ---- part 1: the documented limits ------------------------------------------------------------------------------------------------
def _idiom(got, want32, exact, what):
    """err_gpu <= max(2e-5 * max(1, max|want|), 2 * err_cpu), both errors printed"""
    err_gpu = float((got.double() - exact).abs().max())
    err_cpu = float((want32.double() - exact).abs().max())
    top = float(exact.abs().max())
    print(f"{what}: err_gpu {err_gpu:.3e} err_cpu {err_cpu:.3e} (max|want| {top:.3e})")
    assert torch.isfinite(got).all(), what
    assert err_gpu <= max(2e-5 * max(1.0, top), 2 * err_cpu), (what, err_gpu, err_cpu)
    return err_gpu, err_cpu


def test_sample_limits_raise_and_write_nothing(ops):
    """div_sigma, sample_axpy2 and attention take up to 65 535 samples: one more is an error and not a partly written result;
    one below the limit the result is right"""
    from inverseproblemwithdiffusionmodel_amd._lib import IpdmError
    g = torch.Generator().manual_seed(4)
    n = 65536
    x, y, z = (torch.randn(n, 1, generator=g) for _ in range(3))
    a, c = torch.randn(n, generator=g), torch.randn(n, generator=g)
    sig = 0.01 + torch.rand(50, generator=g)
    labels = torch.randint(0, 50, (n,), generator=g)
    xg, yg, zg, ag, cg, sg, lg = (t.cuda() for t in (x, y, z, a, c, sig, labels))
    mark = torch.full((n, 1), float("nan"), device="cuda")
    with pytest.raises(IpdmError):
        ops.div_sigma(xg, sg, lg, out=mark)
    with pytest.raises(IpdmError):
        ops.sample_axpy2(xg, yg, ag, zg, cg, out=mark)
    torch.cuda.synchronize()
    assert torch.isnan(mark).all()
    with pytest.raises(IpdmError):
        ops.attention(xg.view(n, 1, 1, 1), yg.view(n, 1, 1, 1), zg.view(n, 1, 1, 1), 1.0)
    m = n - 1
    assert torch.equal(ops.div_sigma(xg[:m].contiguous(), sg, lg[:m].contiguous()).cpu(), x[:m] / sig[labels[:m]].view(-1, 1))
    got = ops.sample_axpy2(xg[:m].contiguous(), yg[:m].contiguous(), ag[:m].contiguous(), zg[:m].contiguous(),
                           cg[:m].contiguous()).cpu()
    _idiom(got, x[:m] + a[:m, None] * y[:m] + c[:m, None] * z[:m],
           x[:m].double() + a[:m, None].double() * y[:m].double() + c[:m, None].double() * z[:m].double(), "sample_axpy2 65535 x 1")
    got = ops.attention(xg[:m].view(m, 1, 1, 1), yg[:m].view(m, 1, 1, 1), zg[:m].view(m, 1, 1, 1), 1.0).cpu()
    _idiom(got.view(m, 1), z[:m], z[:m].double(), "attention B65535 C1 N1")     # (one key: the softmax is 1, the result v)


# ---- part 4: nn_extra.hip called directly ---------------------------------------------------------------------------------------
def _attention_ref(q, k, v, scale):
    """softmax_j(scale * q[:, i] . k[:, j]) v[:, j] on [B, C, N] in the tensors' precision"""
    p = torch.softmax(torch.einsum("bci,bcj->bij", q, k) * scale, dim=-1)
    return torch.einsum("bij,bcj->bci", p, v)


@pytest.mark.parametrize("B,C,N", [(2, 1, 1), (2, 3, 63), (1, 65, 257), (2, 64, 256), (1, 130, 1025)])
def test_attention_vs_float64(ops, B, C, N):
    """distinct q, k, v (a swapped operand shows); scale = C ** -0.5, and a scale that puts the logits near +-200: the kernel
    subtracts the row maximum, so the result stays finite and inside the bound"""
    g = torch.Generator().manual_seed(B * 100 + C + N)
    q, k, v = (torch.randn(B, C, N, generator=g) for _ in range(3))
    logits = torch.einsum("bci,bcj->bij", q.double(), k.double())
    for scale in (C ** -0.5, 200.0 / float(logits.abs().max())):
        got = ops.attention(q.view(B, C, 1, N).cuda(), k.view(B, C, 1, N).cuda(), v.view(B, C, 1, N).cuda(), scale).cpu()
        assert got.shape == (B, C, 1, N)
        _idiom(got.view(B, C, N), _attention_ref(q, k, v, scale), _attention_ref(q.double(), k.double(), v.double(), scale),
               f"attention B{B} C{C} N{N} scale {scale:.3g} (max|logit| {float(logits.abs().max()) * scale:.1f})")


@pytest.mark.parametrize("In", [1, 63, 64, 65, 512])
def test_linear_vs_float64(ops, In):
    """one wave per output: ragged wave tails (In not a multiple of 64), B * Out = 21 outputs in workgroups of four (the last one
    not full) and a multiple of four; every act_in code, with and without bias"""
    g = torch.Generator().manual_seed(In)
    for (B, Out) in [(3, 7), (4, 6)]:
        x = torch.randn(B, In, generator=g) * 2
        wt, bias = torch.randn(Out, In, generator=g) / In ** 0.5, torch.randn(Out, generator=g)
        for code in _act_codes(ops):
            for b in (bias, None):
                got = ops.linear(x.cuda(), wt.cuda(), None if b is None else b.cuda(), act_in=code).cpu()
                want32 = F.linear(_act_ref(x, code, ops), wt, b)
                exact = F.linear(_act_ref(x.double(), code, ops), wt.double(), None if b is None else b.double())
                assert got.shape == (B, Out)
                _idiom(got, want32, exact, f"linear In{In} B{B} Out{Out} act{code} bias {b is not None}")


@pytest.mark.parametrize("elems", [1, 255, 257, 3 * 64 * 64])
@pytest.mark.parametrize("n", [1, 5])
def test_sample_norm_vs_float64(ops, n, elems):
    g = torch.Generator().manual_seed(n * 7 + elems)
    for scale in (1e-3, 1e3):
        x = torch.randn(n, elems, generator=g) * scale
        got = ops.sample_norm(x.cuda()).cpu()
        assert got.shape == (n,)
        _idiom(got, x.norm(dim=1), x.double().norm(dim=1), f"sample_norm n{n} elems{elems} scale {scale:g}")


@pytest.mark.parametrize("n,elems", [(3, 1), (5, 255), (2, 257), (3, 3 * 64 * 64 + 1), (2, 512 * 256 + 77)])
def test_sample_axpy2_vs_float64(ops, n, elems):
    """with and without z / c; sample sizes that are no multiple of 256, one past the 512 workgroups per sample"""
    g = torch.Generator().manual_seed(n + elems)
    x, y, z = (torch.randn(n, elems, generator=g) for _ in range(3))
    a, c = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) * 3
    xg, yg, zg, ag, cg = (t.cuda() for t in (x, y, z, a, c))

    def ref(x_, y_, z_, a_, c_):
        r = x_ + a_[:, None] * y_
        return r if z_ is None else r + c_[:, None] * z_
    got = ops.sample_axpy2(xg, yg, ag, zg, cg).cpu()
    _idiom(got, ref(x, y, z, a, c), ref(x.double(), y.double(), z.double(), a.double(), c.double()),
           f"sample_axpy2 n{n} elems{elems} with z, c")
    got = ops.sample_axpy2(xg, yg, ag).cpu()
    _idiom(got, ref(x, y, None, a, None), ref(x.double(), y.double(), None, a.double(), None),
           f"sample_axpy2 n{n} elems{elems} without z, c")
