"""Predictor-corrector sampling with a data-consistency step after every update: MRI reconstruction with the VE-SDE
score networks (NCSN++) of the score_sde half of this package.  Song et al., "Solving inverse problems in medical imaging
with score-based generative models" (ICLR 2022); Chung & Ye, "Score-based diffusion models for accelerated MRI"
(MedIA 2022).  ``sde/sampling.py`` stays the mirror of the reference's unconditional samplers; this module is new.

One level i, t_i from linspace(T, eps, N), runs the corrector n_steps times and the predictor once (the order of
``sampling.get_pc_sampler``); every update is ONE fused tail kernel, x += step * score + noise_scale * z ; x = DC(x),
on the complex state held as [real | imag] rows (2B, 1, H, W).  The schedule scalars come from a float64 host table
(``pc_schedule``) uploaded once; the Langevin corrector's step depends on the data and is formed on the device, per
sample, by ``ops.pc_langevin_coef``.

The step rule is PER COMPLEX SAMPLE: step_b = 2 (snr |z_b| / |score_b|)^2 with the norms of sample b's real and imaginary
planes together -- not score_sde's means over the batch.  A sample therefore does not depend on its batch: row b of a
batch equals the B = 1 run with sample_offset = b bit for bit, and a sharded run needs no all-reduce.  At B = 1 the rule
equals the mean rule applied to the complex sample."""
import numpy as np
import torch

from . import sde_lib
from .. import ops
from ..models.utils import get_score_fn
from ..ncsn.linear_transforms.undersampling_fourier import SENSE, RandomUndersamplingFourier
from ..ncsn.models.ALD_optimizers import SCHED_DTYPE

PREDICTORS = ("reverse_diffusion", "ancestral_sampling", "euler_maruyama", "none")
CORRECTORS = ("langevin", "ald", "none")
DC_CHOICES = {SENSE: ("gradient", "cg"), RandomUndersamplingFourier: ("projection", "closed_form")}
INIT_STEP_ID = -1      # Philox step id of the start state sigma_max * z: iterations use i * (n_steps + 1) + s >= 0


def pc_schedule(sde, predictor="reverse_diffusion", corrector="langevin", snr=0.16, eps=1e-5, denoise=True):
    """float64 schedule of the N levels -> dict of numpy arrays [N] (None where a stage is absent or data dependent):
    t, sigma = sigma(t_i), pred_step / pred_noise, corr_step / corr_noise.  With sigma_i = discrete_sigmas[k_i],
    k_i = floor(t_i (N - 1) / T) and sigma_{i-1} its lower neighbour (0 below the first):
      reverse_diffusion   step = sigma_i^2 - sigma_{i-1}^2, noise = sqrt(step)
      ancestral_sampling  the same step, noise = sqrt(sigma_{i-1}^2 step / sigma_i^2)
      euler_maruyama      step = g(t)^2 / N, noise = g(t) / sqrt(N), g = sigma(t) sqrt(2 log(sigma_max / sigma_min))
      corrector ald       step = 2 (snr sigma(t_i))^2, noise = sqrt(2 step)      (langevin: formed on the device)
    denoise: the last predictor update adds no noise (the reference's returned x_mean).
    k_i is taken in float64 here.  ``VESDE.discretize`` takes it in float32 on the device, where at N of about 2000 the
    margin i * eps of floor() is below one ulp of t_i (N - 1): a few levels of ``sampling.get_pc_sampler`` then use the
    neighbouring sigma.  This table is the deterministic float64 one."""
    N, T = sde.N, float(sde.T)
    t = np.linspace(T, eps, N)
    sig = sde.discrete_sigmas.detach().cpu().double().numpy()
    k = np.floor(t * (N - 1) / T).astype(np.int64)
    s = sig[k]
    adj = np.where(k == 0, 0.0, sig[np.maximum(k - 1, 0)])
    sigma_t = sde.sigma_min * (sde.sigma_max / sde.sigma_min) ** t
    out = dict(t=t, sigma=sigma_t, pred_step=None, pred_noise=None, corr_step=None, corr_noise=None)
    if predictor in ("reverse_diffusion", "ancestral_sampling"):
        step = s ** 2 - adj ** 2
        out["pred_step"] = step
        out["pred_noise"] = np.sqrt(step) if predictor == "reverse_diffusion" else np.sqrt(adj ** 2 * step / s ** 2)
    elif predictor == "euler_maruyama":
        g = sigma_t * np.sqrt(2 * (np.log(sde.sigma_max) - np.log(sde.sigma_min)))
        out["pred_step"], out["pred_noise"] = g ** 2 / N, g / np.sqrt(N)
    if out["pred_noise"] is not None and denoise:
        out["pred_noise"] = out["pred_noise"].copy()
        out["pred_noise"][N - 1] = 0.0
    if corrector == "ald":
        out["corr_step"] = 2 * (snr * sigma_t) ** 2
        out["corr_noise"] = np.sqrt(2 * out["corr_step"])
    return out


def pc_slots(predictor, corrector, n_steps):
    """the updates of one level, in order -> list of (kind, s): kind 'langevin' | 'ald' | 'predictor', s the update's
    offset in the level's n_steps + 1 Philox step ids (the predictor always takes the last)"""
    slots = [(corrector, s) for s in range(n_steps)] if corrector != "none" else []
    if predictor != "none":
        slots.append(("predictor", n_steps))
    return slots


def pc_records(sched, slots, n_steps, coef, start_iter, stop_iter):
    """ipdm_sched_t records of levels [start_iter, stop_iter) -> structured array [levels][len(slots)].  The Philox step id
    of update s of level i is i * (n_steps + 1) + s whatever slice of the schedule a call runs.  A langevin slot's record
    is the shared one its coefficient launch reads (coef, sigma, step_id): step and noise_scale are formed on the device."""
    lv = np.arange(start_iter, stop_iter)
    table = np.zeros((len(lv), len(slots)), dtype=SCHED_DTYPE)
    for j, (kind, s) in enumerate(slots):
        if kind == "predictor":
            table["step"][:, j], table["noise_scale"][:, j] = sched["pred_step"][lv], sched["pred_noise"][lv]
        elif kind == "ald":
            table["step"][:, j], table["noise_scale"][:, j] = sched["corr_step"][lv], sched["corr_noise"][lv]
        table["coef"][:, j] = coef
        table["sigma"][:, j] = sched["sigma"][lv]
        table["step_id"][:, j] = lv * (n_steps + 1) + s
    return table


def _check(sde, op, measurement, predictor, corrector, dc, dc_weight, n_steps, probability_flow):
    """every refusal, on the host, before any GPU work -> (dc, measurement as (n, B, 1, H, W) or, single coil,
    (B, 1, H, W), B, n_coils, H, W)"""
    if not isinstance(sde, sde_lib.VESDE):
        raise NotImplementedError(f"get_pc_inverse_sampler serves VESDE only (the fused tails have no scale on x); got "
                                  f"{type(sde).__name__}")
    if probability_flow:
        raise NotImplementedError("get_pc_inverse_sampler: probability_flow (the ODE predictor) with data consistency is not "
                                  "built")
    if predictor not in PREDICTORS:
        raise ValueError(f"predictor {predictor!r}: one of {PREDICTORS}")
    if corrector not in CORRECTORS:
        raise ValueError(f"corrector {corrector!r}: one of {CORRECTORS}")
    if isinstance(n_steps, bool) or int(n_steps) != n_steps or n_steps < 0:
        raise ValueError(f"n_steps must be an integer >= 0, got {n_steps}")
    if n_steps == 0 and corrector != "none":
        raise ValueError(f"n_steps = 0 runs no corrector: pass corrector='none' instead of {corrector!r}")
    legal = next((v for k, v in DC_CHOICES.items() if isinstance(op, k)), None)
    if legal is None:
        raise TypeError(f"get_pc_inverse_sampler: operator {type(op).__name__}: SENSE or RandomUndersamplingFourier")
    dc = legal[0] if dc is None else dc
    if dc not in sum(DC_CHOICES.values(), ()):
        raise ValueError(f"dc {dc!r}: one of {sum(DC_CHOICES.values(), ())}")
    if dc not in legal:
        raise ValueError(f"dc {dc!r} is not served by {type(op).__name__}: one of {legal}")
    w = float(dc_weight)
    if dc in ("gradient", "projection"):
        if not 0.0 <= w <= 1.0:
            raise ValueError(f"dc_weight {dc_weight} outside [0, 1] for dc={dc!r}")
    elif not 0.0 <= w < float("inf"):
        raise ValueError(f"dc_weight {dc_weight} must be finite and >= 0 for dc={dc!r}")
    if not isinstance(measurement, torch.Tensor) or not measurement.is_complex():
        raise TypeError("measurement: a complex tensor (n_coils, B, 1, H, W)")
    if isinstance(op, SENSE):
        if measurement.dim() != 5 or measurement.shape[0] != op.sens_maps.shape[-3]:
            raise ValueError(f"measurement {tuple(measurement.shape)}: expected (n_coils = {op.sens_maps.shape[-3]}, B, 1, H, W)")
        n_coils = measurement.shape[0]
    else:
        if measurement.dim() == 5 and measurement.shape[0] == 1:
            measurement = measurement[0]
        if measurement.dim() != 4:
            raise ValueError(f"measurement {tuple(measurement.shape)}: expected (B, 1, H, W) or (1, B, 1, H, W)")
        n_coils = 1
    B, H, W = measurement.shape[-4], measurement.shape[-2], measurement.shape[-1]
    if measurement.shape[-3] != 1 or B < 1:
        raise ValueError(f"measurement {tuple(measurement.shape)}: one channel and at least one image")
    if ops.kspace_size_class(H, W) == ops.KSPACE_NONE:
        raise ops._lib.IpdmUnsupported(f"get_pc_inverse_sampler: no k-space kernel for {H}x{W}; {ops.KSPACE_SIZE_RULE}")
    S = getattr(op, "n_map_sets", 1)
    if B % S:
        raise ValueError(f"a batch of {B} images is not a whole number of samples of {S} slices")
    return dc, measurement, B, n_coils, H, W


def get_pc_inverse_sampler(sde, op, measurement, predictor="reverse_diffusion", corrector="langevin", snr=0.16, n_steps=1,
                           dc=None, dc_weight=1.0, cg_iters=10, cg_tol=1e-5, continuous=True, denoise=True, eps=1e-5,
                           device="cuda", probability_flow=False):
    """-> sampler(model, x_init=None, start_iter=0, n_iters=None, seed=0, sample_offset=0, noise_fn=None, use_graph=True,
                  snapshot_its=None) -> (x, nfe), x complex64 (B, 1, H, W) on the device, nfe the score evaluations run.

    sde          a VESDE (anything else: NotImplementedError)
    op           SENSE (maps (n, H, W) or, a stack of slices, (S, n, H, W): row b is sample b // S of slice b % S) or
                 RandomUndersamplingFourier (single coil)
    measurement  (n, B, 1, H, W) complex k-space, as for the ALD sampler ((B, 1, H, W) also for a single coil)
    predictor    reverse_diffusion | ancestral_sampling | euler_maruyama | none;  corrector  langevin | ald | none
    dc           data consistency after every update; None picks the operator's first:
                 SENSE  'gradient'     x - l A^H(M A x - y), l = dc_weight in [0, 1]: one step, exact only for orthogonal
                                       coil images -- it ASSUMES RSS-normalised maps (sum_c |S_c|^2 = 1), for which
                                       l = 1 is the largest non-expansive step
                        'cg'           the exact proximal argmin |x - z|^2 / 2 + a |A x - y|^2 / 2, a = dc_weight >= 0,
                                       by cg_iters conjugate-gradient iterations (tolerance cg_tol); A^H y is formed once
                 single coil 'projection' F^-1[l y + (1 - l) M F x + (1 - M) F x], l = dc_weight in [0, 1]
                        'closed_form'  F^-1[(F x + a y) / (1 + a M)], a = dc_weight >= 0
    denoise      the last predictor update adds no noise (the reference's x_mean)

    The Langevin step is per complex sample, not score_sde's batch mean (module docstring).  Noise is Philox keyed by
    (seed, sample_offset + b, i * (n_steps + 1) + s, plane), so a run does not depend on sharding and a sliced run
    (start_iter, n_iters, x_init) continues the full run's bits; noise_fn(like) injects recorded noise instead (called for
    the real plane, then the imaginary plane, of every update in order).  x_init None starts from sigma_max * Philox
    normals with step id INIT_STEP_ID = -1, which no iteration uses.  use_graph: one level is captured into a hipGraph
    after a warm-up level and replayed; records and times are copied on-stream from device tables.  snapshot_its: levels
    of this call whose incoming state is kept in sampler.snapshots."""
    dc, measurement, B, n_coils, H, W = _check(sde, op, measurement, predictor, corrector, dc, dc_weight, n_steps,
                                               probability_flow)
    n_steps = int(n_steps)
    if dc == "cg":
        cg_iters, cg_tol = ops._check_cg_scalars(cg_iters, cg_tol, "get_pc_inverse_sampler")
    sched = pc_schedule(sde, predictor, corrector, snr, eps, denoise)
    slots = pc_slots(predictor, corrector, n_steps)
    sc_mode = {"projection": ops.SC_PROJECTION, "closed_form": ops.SC_CLOSED_FORM}.get(dc)
    N = sde.N

    def tail(st, score, j, per_sample):
        x = st["x"]
        nz = st["noise"]
        kw = dict(noise_re=None if nz is None else nz[j, 0], noise_im=None if nz is None else nz[j, 1], seed=st["seed"],
                  sample_offset=st["sample_offset"])
        if per_sample:
            kw["sample_sched"] = st["sample_sched"]
        else:
            kw["dev_sched"] = st["recs"][j]
        if dc == "cg":
            ops.pc_sense_cg_step(x[:B], x[B:], score[:B], score[B:], st["y"], st["sens"], st["mask"], st["work"], ahy=st["ahy"],
                                 max_iter=cg_iters, tol=cg_tol, iters_out=st["iters"], **kw)
        elif dc == "gradient":
            ops.pc_sense_step(x[:B], x[B:], score[:B], score[B:], st["y"], st["sens"], st["mask"], st["work"], **kw)
        else:
            ops.pc_singlecoil_step(x[:B], x[B:], score[:B], score[B:], st["y"], st["mask"], sc_mode, work=st["work"], **kw)

    def level(st):
        for j, (kind, _) in enumerate(slots):
            score = st["score_fn"](st["x"], st["t"])
            if score.dtype != torch.float32 or not score.is_contiguous():
                score = score.float().contiguous()
            if kind == "langevin":
                nz = st["noise"]
                ops.pc_langevin_coef(score[:B], score[B:], st["sample_sched"], snr, 1.0,
                                     noise_re=None if nz is None else nz[j, 0], noise_im=None if nz is None else nz[j, 1],
                                     seed=st["seed"], sample_offset=st["sample_offset"], dev_sched=st["recs"][j],
                                     work=st["coef_work"])
            tail(st, score, j, kind == "langevin")

    @torch.no_grad()
    def sampler(model, x_init=None, start_iter=0, n_iters=None, seed=0, sample_offset=0, noise_fn=None, use_graph=True,
                snapshot_its=None):
        dev = torch.device(device)
        i0 = int(start_iter)
        i1 = N if n_iters is None else min(N, i0 + int(n_iters))
        if not 0 <= i0 <= N:
            raise ValueError(f"start_iter {start_iter} outside the {N} levels")
        meas = measurement.to(dev).to(torch.complex64).contiguous()
        if x_init is None:
            shape = (B, 1, H, W)
            x = torch.cat([ops.philox_normal(shape, dev, seed=seed, sample_offset=sample_offset, step_id=INIT_STEP_ID, plane=p)
                           for p in (0, 1)], dim=0) * float(sde.sigma_max)
        else:
            if tuple(x_init.shape) != (B, 1, H, W) or not x_init.is_complex():
                raise ValueError(f"x_init: a complex tensor {(B, 1, H, W)}, got {tuple(x_init.shape)} {x_init.dtype}")
            x0 = x_init.to(dev)
            x = torch.cat([x0.real, x0.imag], dim=0).float()
        x = x.contiguous()
        n_lv = max(i1 - i0, 0)
        st = dict(x=x, y=meas, mask=op.mask_u8(dev), sens=op.sens_dev(dev) if sc_mode is None else None,
                  seed=int(seed), sample_offset=int(sample_offset), noise=None, ahy=None, iters=None,
                  score_fn=get_score_fn(sde, model, train=False, continuous=continuous),
                  t=torch.zeros(2 * B, dtype=torch.float32, device=dev),
                  recs=torch.zeros(max(len(slots), 1), SCHED_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                  sample_sched=torch.zeros(B, SCHED_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                  coef_work=ops.pc_langevin_coef_workspace(B, dev))
        if dc == "cg":
            st["ahy"] = op.conj_op(meas).to(torch.complex64).contiguous()
            st["iters"] = torch.zeros(B, dtype=torch.int32, device=dev)
            st["work"] = ops.sense_cg_workspace(B, n_coils, H, W, dev)
        else:
            st["work"] = ops.sense_workspace(B, n_coils, H, W, dev)
        if noise_fn is not None:
            st["noise"] = torch.empty(max(len(slots), 1), 2, B, 1, H, W, dtype=torch.float32, device=dev)
        sampler.snapshots = {}
        if n_lv == 0 or not slots:
            return torch.complex(x[:B], x[B:]), 0
        # every record and time of the run, uploaded once; a level copies its rows on-stream
        table = pc_records(sched, slots, n_steps, float(dc_weight), i0, i1)
        table_dev = torch.from_numpy(table.view(np.uint8).reshape(n_lv, len(slots), -1).copy()).to(dev)
        t_table = torch.from_numpy(np.repeat(sched["t"][i0:i1, None], 2 * B, axis=1).astype(np.float32)).to(dev)
        snap = set(snapshot_its or ())
        graph = None
        for k in range(n_lv):
            if k in snap:
                sampler.snapshots[k] = torch.complex(x[:B], x[B:]).to("cpu")
            st["recs"].copy_(table_dev[k], non_blocking=True)
            st["t"].copy_(t_table[k], non_blocking=True)
            if noise_fn is not None:
                for j in range(len(slots)):
                    st["noise"][j, 0].copy_(noise_fn(x[:B]).to(dev))
                    st["noise"][j, 1].copy_(noise_fn(x[B:]).to(dev))
            if not use_graph:
                level(st)
            elif graph is None:
                level(st)                                # warm-up (weight packing, LDS attributes, allocator)
                if k + 1 < n_lv:
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        level(st)
                    # (capture records, it does not run: level k + 1 is the first replay)
            else:
                graph.replay()
        return torch.complex(x[:B], x[B:]), n_lv * len(slots)

    sampler.snapshots = {}
    sampler.schedule = sched
    sampler.slots = slots
    sampler.dc = dc
    return sampler
