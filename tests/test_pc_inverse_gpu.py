"""Predictor-corrector SENSE reconstruction on the GPU (sde/inverse.py): the per-sample coefficient kernel against
float64, the per-sample fused tails against the shared-record entry points called on each sample alone, the sampler
against the float64 restatement of tests/pc_helpers.py, its invariances (graph / eager, batch, split runs), data
consistency, the tiny NCSN++ end to end and the driver.

Run as a script (`python tests/test_pc_inverse_gpu.py OUTDIR`) this file is the child of the IPDM_SENSE_COILS=0 arm: the
one-workgroup-per-sample tail reads the per-sample records too, and the switch is read once per process.

Measured on one MI355X, max|x - x64| / max|x64| of the sampler against float64; the asserted bound is ten
times the observed value (margin for other cards and compiler versions) and never above the project's trajectory bar 1e-3:
    reverse_diffusion + langevin + gradient   6.2e-07
    ancestral_sampling + ald + cg             1.2e-06
    reverse_diffusion + langevin + projection 9.9e-07
    dc_weight = 0, ald, against sampling.get_pc_sampler on the [re | im] rows   3.7e-07"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
for p in (REPO, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import cg_helpers as cgh          # noqa: E402
import pc_helpers as pch          # noqa: E402

DEV = "cuda"
CHILD_TIMEOUT = 60
# observed error against float64 (module docstring); the bound asserted is min(10 * observed, 1e-3)
OBSERVED = {"rd_langevin_gradient": 6.2e-7, "as_ald_cg": 1.2e-6, "sc_projection": 9.9e-7, "pc_sampler": 3.7e-7}


def _bound(key):
    return min(10.0 * OBSERVED[key], 1e-3)


@pytest.fixture(scope="module")
def ops():
    from inverseproblemwithdiffusionmodel_amd import ops
    return ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


# ---- 1. the coefficient kernel ---------------------------------------------------------------------------------------
SNR, ALPHA, SEED, OFFSET, STEP_ID = 0.16, 0.9, 11, 5, 2 ** 32 + 7
RTOL = 2.0 ** -23            # double accumulation, coefficients in double, ONE rounding to float32 (2^-24) -- the issue's bound


def _coef_inputs(B, elems, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((2, B, elems)).astype(np.float32) * np.float32(3.0)
    nz = rng.standard_normal((2, B, elems)).astype(np.float32)
    return g, nz


def _coef_expected(g, z):
    """float64 from the same float32 inputs -> (step, noise_scale) [B]"""
    g, z = g.astype(np.float64), z.astype(np.float64)
    ng = np.sqrt((g ** 2).sum(axis=(0, 2)))
    nzn = np.sqrt((z ** 2).sum(axis=(0, 2)))
    with np.errstate(divide="ignore", invalid="ignore"):
        step = 2 * ALPHA * (SNR * nzn / ng) ** 2
    return step, np.sqrt(2 * step)


def _read(sample_sched):
    return sample_sched.cpu().numpy().view(pch.SCHED).reshape(-1)


@pytest.mark.parametrize("elems", [16, 256, 3840, 20480])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("philox", [False, True])
def test_langevin_coef_against_float64(ops, elems, B, philox):
    g, nz = _coef_inputs(B, elems, elems + B)
    g_re, g_im = dev(g[0]), dev(g[1])
    sched = torch.full((B, 32), 0xAB, dtype=torch.uint8, device=DEV)
    kw = dict(seed=SEED, sample_offset=OFFSET, step_id=STEP_ID, coef=0.25, sigma=1.5)
    if philox:
        z = np.stack([ops.philox_normal((B, elems), DEV, seed=SEED, sample_offset=OFFSET, step_id=STEP_ID, plane=p).cpu().numpy()
                      for p in (0, 1)])
        assert np.abs(z).max() > 1 and not np.array_equal(z[0], z[1])
    else:
        z = nz
        kw.update(noise_re=dev(nz[0]), noise_im=dev(nz[1]))
    ops.pc_langevin_coef(g_re, g_im, sched, SNR, ALPHA, **kw)
    r = _read(sched)
    step, ns = _coef_expected(g, z)
    print(f"elems {elems} B {B} philox {philox}: max rel err step {np.abs(r['step'] / step - 1).max():.3e} "
          f"noise_scale {np.abs(r['noise_scale'] / ns - 1).max():.3e}")
    assert (np.abs(r["step"].astype(np.float64) - step) <= RTOL * step).all()
    assert (np.abs(r["noise_scale"].astype(np.float64) - ns) <= RTOL * ns).all()
    assert (r["coef"] == np.float32(0.25)).all() and (r["sigma"] == 1.5).all() and (r["step_id"] == STEP_ID).all()
    assert (r["seg_scale"] == 0).all() and (r["reserved"] == 0).all()
    again = torch.zeros_like(sched)
    ops.pc_langevin_coef(g_re, g_im, again, SNR, ALPHA, **kw)
    assert torch.equal(again, sched)                                              # reproducible run to run
    if B == 3:                                                                    # a sample's record does not depend on its batch
        one = torch.zeros(1, 32, dtype=torch.uint8, device=DEV)
        kw1 = dict(kw, sample_offset=OFFSET + 2)
        if not philox:
            kw1.update(noise_re=dev(nz[0][2:]), noise_im=dev(nz[1][2:]))
        ops.pc_langevin_coef(dev(g[0][2:]), dev(g[1][2:]), one, SNR, ALPHA, **kw1)
        assert torch.equal(one[0], sched[2])


def test_langevin_coef_shared_record_zero_score_and_nan(ops):
    B, elems = 3, 256
    g, nz = _coef_inputs(B, elems, 3)
    g[:, 1] = 0.0                                                                 # sample 1: no score
    g[1, 2, 17] = np.nan                                                          # sample 2: a NaN in the imaginary plane
    shared = dev(pch.records([9.0], [9.0], [0.75], [STEP_ID + 1], sigma=2.5))
    sched = torch.zeros(B, 32, dtype=torch.uint8, device=DEV)
    ops.pc_langevin_coef(dev(g[0]), dev(g[1]), sched, SNR, 1.0, seed=SEED, sample_offset=OFFSET, step_id=3, dev_sched=shared,
                         coef=-1.0, sigma=-1.0)
    r = _read(sched)
    assert (r["step_id"] == STEP_ID + 1).all() and (r["coef"] == 0.75).all() and (r["sigma"] == 2.5).all()   # from the record
    assert r["step"][1] == 0.0 and r["noise_scale"][1] == 0.0
    assert np.isnan(r["step"][2]) and np.isnan(r["noise_scale"][2])
    z = np.stack([ops.philox_normal((B, elems), DEV, seed=SEED, sample_offset=OFFSET, step_id=STEP_ID + 1, plane=p).cpu().numpy()
                  for p in (0, 1)])                                               # keyed by the RECORD's step id
    gd, zd = g.astype(np.float64), z.astype(np.float64)
    want = 2 * (SNR * np.sqrt((zd[:, 0] ** 2).sum()) / np.sqrt((gd[:, 0] ** 2).sum())) ** 2
    assert np.isfinite(r["step"][0]) and abs(r["step"][0] - want) <= RTOL * want
    assert abs(r["noise_scale"][0] - np.sqrt(2 * want)) <= RTOL * np.sqrt(2 * want)
    g[:, 2] = np.inf                                                              # an infinite norm: NaN, never 0
    ops.pc_langevin_coef(dev(g[0]), dev(g[1]), sched, SNR, 1.0, seed=SEED, sample_offset=OFFSET, dev_sched=shared)
    assert np.isnan(_read(sched)["step"][2]) and np.isfinite(_read(sched)["step"][0])


def test_operand_checks_before_any_launch(ops):
    g = torch.zeros(2, 16, device=DEV)
    sched = torch.zeros(2, 32, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError):
        ops.pc_langevin_coef(g.double(), g, sched, 0.1)
    with pytest.raises(ValueError):
        ops.pc_langevin_coef(g.t(), g, sched, 0.1)
    with pytest.raises(ValueError, match="records"):
        ops.pc_langevin_coef(g, g, sched[:1], 0.1)
    with pytest.raises(ValueError):
        ops.pc_langevin_coef(g, g, sched, 0.1, noise_re=g)
    x = torch.zeros(2, 1, 16, 16, device=DEV)
    y = torch.zeros(2, 1, 16, 16, dtype=torch.complex64, device=DEV)
    m8 = torch.ones(1, 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="records"):
        ops.pc_singlecoil_step(x, x.clone(), x.clone(), x.clone(), y, m8, 2, sample_sched=sched[:1])
    with pytest.raises(ValueError, match="not both"):
        ops.pc_singlecoil_step(x, x.clone(), x.clone(), x.clone(), y, m8, 2, sample_sched=sched, dev_sched=sched[0])
    with pytest.raises(TypeError):
        ops.pc_singlecoil_step(x.double(), x.clone(), x.clone(), x.clone(), y, m8, 2, sample_sched=sched)
    v0 = x._version
    ops.pc_singlecoil_step(x, x.clone(), x.clone(), x.clone(), y, m8, 2, sample_sched=sched)
    assert x._version > v0                                                        # the state is marked written


# ---- 2. the per-sample tails -----------------------------------------------------------------------------------------
def _tail_case(H, W, n, B, complex_maps=False, mask2d=False, sets=1, seed=0):
    rng = np.random.default_rng(seed)
    c = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    shape = (sets, n, H, W) if sets > 1 else (n, H, W)
    maps = c(*shape) if complex_maps else (rng.random(shape).astype(np.float32) + np.float32(0.1))
    maps = (maps / np.sqrt((np.abs(maps) ** 2).sum(axis=-3, keepdims=True))).astype(maps.dtype)
    if mask2d:
        mask = (rng.random((1, H, W)) < 0.4)
        mask[:, H // 2 - 2:H // 2 + 2, W // 2 - 2:W // 2 + 2] = True
    else:
        mask = (rng.random((1, W)) < 0.4)
        mask[:, W // 2 - 2:W // 2 + 2] = True
    return dict(B=B, H=H, W=W, n=n, sets=sets, x=f(2, B, 1, H, W), g=f(2, B, 1, H, W), nz=f(2, B, 1, H, W), y=c(n, B, 1, H, W),
                ysc=c(B, 1, H, W), maps=maps, mask=mask.astype(np.uint8))


def _tail_records(B):
    """every sample its own record: different steps, noise scales, coefficients and step ids.  Sample 1 has coef = 0
    between non-zero neighbours: its workgroups alone take the tails' early return (no transform, stale work planes)"""
    b = np.arange(B)
    return pch.records(0.05 + 0.11 * b, 0.3 + 0.07 * b, np.where(b == 1, 0.0, 0.2 + 0.25 * (b % 3)), 40 + 3 * b)


def _run_tail(ops, kind, case, recs, rows, stride, philox, offset, new=True, **extra):
    """the tail `kind` on samples `rows` of the case -> (x_re, x_im).  stride 1: record b for sample b (new entry points
    only); stride 0: recs[0] shared.  new=False: the existing shared-record entry point."""
    B = len(rows)
    sl = lambda a, ax: dev(np.take(a, rows, axis=ax))
    x_re, x_im = sl(case["x"][0], 0), sl(case["x"][1], 0)
    g_re, g_im = sl(case["g"][0], 0), sl(case["g"][1], 0)
    kw = dict(seed=SEED, sample_offset=offset)
    if not philox:
        kw.update(noise_re=sl(case["nz"][0], 0), noise_im=sl(case["nz"][1], 0))
    recs = dev(recs)
    if stride == 1:
        kw["sample_sched"] = recs
    else:
        kw["dev_sched"] = recs[0]
    m8 = dev(case["mask"])
    H, W, n = case["H"], case["W"], case["n"]
    if kind.startswith("sc"):
        fn = ops.pc_singlecoil_step if new else ops.ald_singlecoil_step
        fn(x_re, x_im, g_re, g_im, sl(case["ysc"], 0), m8, int(kind[2:]), **kw)
        return x_re, x_im
    maps = case["maps"] if "set" not in extra else case["maps"][extra["set"]]
    sens, y = dev(maps), sl(case["y"], 1)
    if kind == "cg":
        fn = ops.pc_sense_cg_step if new else ops.ald_sense_cg_step
        fn(x_re, x_im, g_re, g_im, y, sens, m8, ops.sense_cg_workspace(B, n, H, W, DEV), max_iter=4, tol=0.0, **kw)
    else:
        fn = ops.pc_sense_step if new else ops.ald_sense_step
        fn(x_re, x_im, g_re, g_im, y, sens, m8, ops.sense_workspace(B, n, H, W, DEV), **kw)
    return x_re, x_im


def _check_tail(ops, kind, case, philox=True):
    """per-sample records through the new entry point == the existing entry point on each sample alone (B = 1,
    sample_offset = b, record b); stride 0 through the new entry point == the existing entry point on the batch"""
    B, S = case["B"], case["sets"]
    recs = _tail_records(B)
    rows = list(range(B))
    x_re, x_im = _run_tail(ops, kind, case, recs, rows, 1, philox, OFFSET)
    x0 = case["x"]
    assert not np.array_equal(x_re.cpu().numpy(), x0[0])
    for b in rows:
        extra = dict(set=b % S) if S > 1 else {}
        e_re, e_im = _run_tail(ops, kind, case, recs[b:b + 1], [b], 0, philox, OFFSET + b, new=False, **extra)
        assert torch.equal(x_re[b:b + 1], e_re) and torch.equal(x_im[b:b + 1], e_im), (kind, b)
    n_re, n_im = _run_tail(ops, kind, case, recs[2:3], rows, 0, philox, OFFSET)
    o_re, o_im = _run_tail(ops, kind, case, recs[2:3], rows, 0, philox, OFFSET, new=False)
    assert torch.equal(n_re, o_re) and torch.equal(n_im, o_im), kind
    return x_re, x_im


TAIL_CASES = {
    "16x16_real_line": dict(H=16, W=16, n=2, B=3),
    "48x80_complex_2d": dict(H=48, W=80, n=3, B=3, complex_maps=True, mask2d=True),
    "128x160_strips": dict(H=128, W=160, n=2, B=3),
    "two_map_sets": dict(H=16, W=32, n=2, B=4, sets=2, complex_maps=True),
}


@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_per_sample_sense_tail(ops, name):
    case = _tail_case(seed=len(name), **TAIL_CASES[name])
    if name == "128x160_strips":
        assert ops.kspace_size_class(128, 160) == ops.KSPACE_STRIPS
    _check_tail(ops, "sense", case, philox=True)
    if name == "16x16_real_line":
        _check_tail(ops, "sense", case, philox=False)


@pytest.mark.parametrize("name", ["16x16_real_line", "128x160_strips", "two_map_sets"])
def test_per_sample_cg_tail(ops, name):
    _check_tail(ops, "cg", _tail_case(seed=7 + len(name), **TAIL_CASES[name]))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("size", [(16, 16), (128, 160)])
def test_per_sample_singlecoil_tail(ops, mode, size):
    _check_tail(ops, f"sc{mode}", _tail_case(size[0], size[1], 1, 3, seed=mode))


def _child(outdir):
    """IPDM_SENSE_COILS=0: the one-workgroup-per-sample SENSE tail with per-sample records"""
    from inverseproblemwithdiffusionmodel_amd import ops
    assert os.environ.get("IPDM_SENSE_COILS") == "0"
    out = {}
    for name in ("16x16_real_line", "48x80_complex_2d", "two_map_sets"):
        x_re, _ = _check_tail(ops, "sense", _tail_case(seed=len(name), **TAIL_CASES[name]))
        out[name] = x_re.cpu().numpy()
    np.savez(os.path.join(outdir, "results.npz"), **out)
    with open(os.path.join(outdir, "ok.json"), "w") as f:
        json.dump({"ok": True}, f)


def test_per_sample_tail_one_workgroup_per_sample(ops, tmp_path):
    """a fresh child with IPDM_SENSE_COILS=0 (read once per process); same bits as the coil-parallel tail of this process"""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], env=dict(os.environ, IPDM_SENSE_COILS="0"),
                           cwd=REPO, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"child: timeout after {CHILD_TIMEOUT} s")
    assert p.returncode == 0, p.stderr[-3000:]
    with open(tmp_path / "ok.json") as f:
        assert json.load(f)["ok"]
    got = np.load(tmp_path / "results.npz")
    for name in got.files:
        x_re, _ = _run_tail(ops, "sense", _tail_case(seed=len(name), **TAIL_CASES[name]), _tail_records(TAIL_CASES[name]["B"]),
                            list(range(TAIL_CASES[name]["B"])), 1, True, OFFSET)
        assert np.array_equal(got[name], x_re.cpu().numpy()), name          # kspace.hip: "tuning / comparison; same bits"


# ---- 3. the sampler --------------------------------------------------------------------------------------------------
N_LV, H0, W0 = 8, 16, 16


def _problem(n_coils, B, seed=0):
    """-> dict: operator, measurement (device), float64 maps / mask / y, the Gaussian prior (mu rows, s0)"""
    from inverseproblemwithdiffusionmodel_amd.ncsn.linear_transforms.undersampling_fourier import (
        SENSE, RandomUndersamplingFourier)
    rng = np.random.default_rng(seed)
    mask = rng.random(W0) < 0.5
    mask[W0 // 2 - 2:W0 // 2 + 2] = True
    truth = (rng.random((B, 1, H0, W0)) * np.exp(1j * rng.standard_normal((B, 1, H0, W0)))).astype(np.complex64)
    if n_coils > 1:
        maps = rng.random((n_coils, H0, W0)) + 0.2
        op = SENSE("custom", n_coils, 2, 0.04, (1, H0, W0), seed=0, sens_maps=torch.from_numpy(maps), mask_mode="custom",
                   mask=torch.from_numpy(mask))
        maps64 = op.sens_dev("cpu").double().numpy()                                 # the float32 values the kernels read
        y = cgh.forward(truth, maps64, mask.astype(np.float64)).astype(np.complex64)
    else:
        op = RandomUndersamplingFourier(2, 0.04, (1, H0, W0), seed=0, mask_mode="custom", mask=torch.from_numpy(mask))
        maps64 = None
        y = (mask * cgh.fft2c(truth.astype(np.complex128))).astype(np.complex64)
    mu = rng.standard_normal((2 * B, 1, H0, W0)).astype(np.float32) * np.float32(0.5)
    return dict(op=op, y=y, maps=maps64, mask=mask.astype(np.float64), mu=mu, s0=0.7, B=B, n=n_coils, truth=truth)


def _sde():
    from inverseproblemwithdiffusionmodel_amd.sde import sde_lib
    return sde_lib.VESDE(0.01, 50.0, N_LV)


def _recorded_noise(n_updates, B, seed):
    nz = np.random.default_rng(seed).standard_normal((n_updates, 2, B, 1, H0, W0)).astype(np.float32)
    it = iter(nz.reshape(-1, B, 1, H0, W0))
    return nz, (lambda like: torch.from_numpy(next(it)))


SAMPLER_CASES = {
    "rd_langevin_gradient": dict(n=4, predictor="reverse_diffusion", corrector="langevin", dc="gradient", w=0.8),
    "as_ald_cg": dict(n=4, predictor="ancestral_sampling", corrector="ald", dc="cg", w=2.0),
    "sc_projection": dict(n=1, predictor="reverse_diffusion", corrector="langevin", dc="projection", w=0.7),
}


@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_sampler_against_float64(name):
    from inverseproblemwithdiffusionmodel_amd.sde import inverse
    c = SAMPLER_CASES[name]
    B = 2
    pb = _problem(c["n"], B, seed=3)
    sde = _sde()
    sampler = inverse.get_pc_inverse_sampler(sde, pb["op"], torch.from_numpy(pb["y"]), predictor=c["predictor"],
                                             corrector=c["corrector"], snr=SNR, n_steps=1, dc=c["dc"], dc_weight=c["w"],
                                             cg_iters=30, cg_tol=1e-7, device=DEV)
    rng = np.random.default_rng(5)
    x0 = (50.0 * (rng.standard_normal((B, 1, H0, W0)) + 1j * rng.standard_normal((B, 1, H0, W0)))).astype(np.complex64)
    nz, noise_fn = _recorded_noise(N_LV * 2, B, 9)
    model = pch.GaussianScore(dev(pb["mu"]), pb["s0"])
    x, nfe = sampler(model, x_init=torch.from_numpy(x0), noise_fn=noise_fn)
    assert nfe == 2 * N_LV and x.shape == (B, 1, H0, W0) and x.dtype == torch.complex64 and x.is_cuda
    sched = pch.schedule64(pch.vesde64(N=N_LV), c["predictor"], c["corrector"], SNR, 1e-5, True)
    y64 = pb["y"].astype(np.complex128)
    dc = {"gradient": lambda: pch.dc_gradient(pb["maps"], pb["mask"], y64, c["w"]),
          "cg": lambda: pch.dc_cg(pb["maps"], pb["mask"], y64, c["w"]),
          "projection": lambda: pch.dc_projection(pb["mask"], y64[0] if y64.ndim == 5 else y64, c["w"])}[c["dc"]]()
    mu_c = pb["mu"][:B].astype(np.float64) + 1j * pb["mu"][B:].astype(np.float64)
    want = pch.pc_reference(sched, sampler.slots, x0, pch.gaussian_score64(mu_c, pb["s0"]),
                            (z[0] + 1j * z[1].astype(np.float64) for z in nz), dc, SNR)
    err = np.abs(x.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"sampler {name}: max|x - x64| / max|x64| = {err:.3e}  (max|x64| = {np.abs(want).max():.3f})")
    assert np.isfinite(want).all() and np.abs(want - x0).max() > 1.0
    assert err <= _bound(name)


def _philox_run(pb, B, rows=None, offset=0, use_graph=True, **kw):
    """langevin + gradient with Philox noise and the Philox start state, on rows `rows` of the problem"""
    from inverseproblemwithdiffusionmodel_amd.sde import inverse
    rows = list(range(B)) if rows is None else rows
    y = torch.from_numpy(pb["y"][:, rows])
    mu = np.concatenate([pb["mu"][:pb["B"]][rows], pb["mu"][pb["B"]:][rows]])
    sampler = inverse.get_pc_inverse_sampler(_sde(), pb["op"], y, snr=SNR, n_steps=1, dc="gradient", dc_weight=0.9, device=DEV)
    return sampler(pch.GaussianScore(dev(mu), pb["s0"]), seed=SEED, sample_offset=offset, use_graph=use_graph, **kw)[0]


def test_graph_equals_eager_batch_and_split_invariance():
    pb = _problem(4, 3, seed=4)
    full = _philox_run(pb, 3)                                                     # warm-up level + 7 replayed levels
    assert torch.isfinite(torch.view_as_real(full)).all()
    assert torch.equal(full, _philox_run(pb, 3, use_graph=False))
    for b in range(3):                                                            # row b == the B = 1 run with sample_offset = b
        assert torch.equal(full[b:b + 1], _philox_run(pb, 1, rows=[b], offset=b)), b
    head = _philox_run(pb, 3, n_iters=3)
    tail = _philox_run(pb, 3, start_iter=3, x_init=head)
    assert torch.equal(tail, full)                                                # a split run continues the full run's bits
    assert not torch.equal(head, full)


def test_zero_weight_ald_matches_the_unconditional_pc_sampler():
    """dc_weight = 0 with corrector 'ald': no data consistency and no data-dependent step, i.e. sampling.get_pc_sampler on
    the [re | im] rows with the same recorded noise -- up to rounding (one fused update against two axpys)"""
    from inverseproblemwithdiffusionmodel_amd.sde import inverse, sampling
    B = 2
    pb = _problem(4, B, seed=6)
    sde = _sde()
    model = pch.GaussianScore(dev(pb["mu"]), pb["s0"])
    rng = np.random.default_rng(8)
    x0 = (50.0 * (rng.standard_normal((B, 1, H0, W0)) + 1j * rng.standard_normal((B, 1, H0, W0)))).astype(np.complex64)
    nz, noise_fn = _recorded_noise(N_LV * 2, B, 10)
    sampler = inverse.get_pc_inverse_sampler(sde, pb["op"], torch.from_numpy(pb["y"]), corrector="ald", snr=SNR, n_steps=1,
                                             dc="gradient", dc_weight=0.0, device=DEV)
    x, _ = sampler(model, x_init=torch.from_numpy(x0), noise_fn=noise_fn)
    rows = iter(nz.reshape(N_LV * 2, 2 * B, 1, H0, W0))                           # [re | im] rows of every update
    sampling.set_noise_source(lambda like: torch.from_numpy(next(rows)))
    try:
        ref = sampling.get_pc_sampler(sde, (2 * B, 1, H0, W0), sampling.ReverseDiffusionPredictor, sampling.AnnealedLangevinDynamics,
                                      lambda v: v, SNR, n_steps=1, continuous=True, denoise=True, eps=1e-5, device=DEV)
        r, _ = ref(model, x_init=torch.from_numpy(np.concatenate([x0.real, x0.imag])))
    finally:
        sampling.set_noise_source(None)
    want = torch.complex(r[:B], r[B:])
    err = float((x - want).abs().max() / want.abs().max())
    print(f"dc_weight 0, ald, against get_pc_sampler: max|x - ref| / max|ref| = {err:.3e}")
    assert err <= _bound("pc_sampler")


def test_projection_with_full_weight_reproduces_the_measurement(ops):
    """single coil, 'projection', lambda = 1: the sampled k-space of the result IS y (5e-6: test_kernels_gpu's
    tolerance for the projection operator)"""
    from inverseproblemwithdiffusionmodel_amd.sde import inverse
    pb = _problem(1, 2, seed=12)
    sampler = inverse.get_pc_inverse_sampler(_sde(), pb["op"], torch.from_numpy(pb["y"]), snr=SNR, dc="projection", dc_weight=1.0,
                                             device=DEV)
    x, _ = sampler(pch.GaussianScore(dev(pb["mu"]), pb["s0"]), seed=1)
    k = pb["op"](x)
    np.testing.assert_allclose(k.cpu().numpy(), pb["y"], atol=5e-6)
    assert np.abs(pb["y"]).max() > 1.0


def test_tiny_ncsnpp_end_to_end_graph_equals_eager():
    """the network path: stale activation maxima under capture or labels baked into the graph would split the two runs"""
    from test_score_sde_gpu import tiny_cfg
    from inverseproblemwithdiffusionmodel_amd import engine
    from inverseproblemwithdiffusionmodel_amd.models import ncsnpp
    from inverseproblemwithdiffusionmodel_amd.sde import sde_lib
    from inverseproblemwithdiffusionmodel_amd.synthetic import synth_state_dict
    cfg = tiny_cfg()
    cfg.data.num_channels = 1
    net = ncsnpp.NCSNpp(cfg)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=0), strict=False)
    net = net.to(DEV).eval()
    prob = engine.build_problem(torch.device(DEV), 2, R=8, H=32, W=32, num_sens=2, seed=0, scorenet=net,
                                cfg=engine.acdc_config(torch.device(DEV), 32))
    sde = sde_lib.VESDE(cfg.model.sigma_min, cfg.model.sigma_max, cfg.model.num_scales)
    sampler = engine.build_pc_sampler(prob, sde, snr=SNR, n_steps=1)
    a, nfe = sampler(net, n_iters=3, seed=2)
    b, _ = sampler(net, n_iters=3, seed=2, use_graph=False)
    assert nfe == 6 and a.shape == (2, 1, 32, 32)
    assert torch.isfinite(torch.view_as_real(a)).all()
    assert torch.equal(a, b)
    assert not torch.equal(a[0], a[1])                                            # two samples, two noise streams


def test_driver(tmp_path):
    out = tmp_path / "out"
    try:
        r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "acdc_SENSE_pc.py"), "--tiny", "--image_size", "32",
                            "--n_iters", "2", "--num_samples", "2", "--save_dir", str(out)], capture_output=True, text=True,
                           timeout=300, cwd=REPO)
    except subprocess.TimeoutExpired:
        pytest.fail("acdc_SENSE_pc.py: timeout")
    assert r.returncode == 0, r.stderr[-3000:]
    load = lambda name: torch.load(out / name, weights_only=False)
    rec, meas, maps = load("reconstructions.pt"), load("measurement.pt"), load("sens_maps.pt")
    assert rec.shape == (2, 1, 32, 32) and rec.is_complex() and torch.isfinite(torch.view_as_real(rec)).all()
    assert meas.shape == (4, 1, 1, 32, 32) and maps.shape == (4, 32, 32)
    assert "RMSE vs phantom" in r.stdout and os.path.exists(out / "original.pt")


if __name__ == "__main__":
    _child(sys.argv[1])
