"""Synthetic inputs for the benchmark and the parity tests (no data or checkpoints ship with the
reference: SURVEY.md 8c/8d).

* ``synth_state_dict``  -- deterministic random-init weights for any score net, keyed by the
  reference's state-dict names, independent of module construction order.
* ``phantom_image``     -- 6-ellipse magnitude phantom with a smooth phase, mirroring what
  ``helpers/load_data.py:372-387`` (add_phase: bicubic upsampling of an N(0,1) 5x5 patch) produces.
* ``vd_mask_2d``        -- seeded variable-density 2-D (ky, kz) sampling mask with a fully sampled centre block.

Everything here is host-side torch-CPU so the very same tensors are produced on the build
container and on the GPU box.
"""
import hashlib
import math

import torch
import torch.nn.functional as F


def _key_generator(key: str, seed: int) -> torch.Generator:
    h = hashlib.sha256(f"{seed}:{key}".encode()).digest()
    return torch.Generator().manual_seed(int.from_bytes(h[:7], "little"))


def synth_state_dict(shapes, seed=0):
    """shapes: {state-dict key: shape tuple}.  Conv / linear weights ~ U(-b, b), b = 1/sqrt(fan_in)
    (the scale torch's default conv init gives), norm scales ~ N(1, 0.02), shifts ~ N(0, 0.02); a conditional
    InstanceNorm++ table (`*.embed.weight`, [num_classes, 3C]) has its gamma and alpha columns ~ N(1, 0.02), beta ~ N(0, 0.02)."""
    out = {}
    for key, shape in shapes.items():
        if key == "sigmas" or key.endswith(".sigmas"):
            continue
        g = _key_generator(key, seed)
        shape = tuple(shape)
        leaf = key.rsplit(".", 1)[-1]
        if key.endswith("embed.weight") and len(shape) == 2 and shape[1] % 3 == 0:
            # ConditionalInstanceNorm2dPlus table [num_classes, 3C] = [gamma | alpha | beta] (every NCSNv1 norm has bias=True):
            # scales ~ N(1, 0.02), shifts ~ N(0, 0.02), drawn as one tensor and shifted by column
            t = 0.02 * torch.randn(shape, generator=g)
            t[:, :2 * (shape[1] // 3)] += 1.0
        elif len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            b = 1.0 / math.sqrt(fan_in)
            t = (torch.rand(shape, generator=g) * 2 - 1) * b
        elif leaf in ("alpha", "gamma"):
            t = 1.0 + 0.02 * torch.randn(shape, generator=g)
        elif leaf == "weight":            # 1-D weight = affine norm scale
            t = 1.0 + 0.02 * torch.randn(shape, generator=g)
        else:                             # bias / beta
            t = 0.02 * torch.randn(shape, generator=g)
        out[key] = t.float()
    return out


def phantom_image(H=128, W=128, seed=0, n_ellipses=6, phase_patch=(5, 5)):
    """complex64 (1, 1, H, W): magnitude in [0, 1], smooth phase."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    mag = torch.zeros(H, W)
    for _ in range(n_ellipses):
        cx, cy = (torch.rand(2, generator=g) * 1.0 - 0.5).tolist()
        ax, ay = (torch.rand(2, generator=g) * 0.45 + 0.1).tolist()
        th = float(torch.rand(1, generator=g)) * math.pi
        val = float(torch.rand(1, generator=g)) * 0.6 + 0.2
        xr = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
        yr = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
        mag = mag + val * ((xr / ax) ** 2 + (yr / ay) ** 2 <= 1.0).float()
    mag = mag / mag.max().clamp_min(1e-6)
    patch = torch.randn(1, 1, *phase_patch, generator=g)
    phase = F.interpolate(patch, size=(H, W), mode="bicubic", align_corners=True)[0, 0]
    img = torch.polar(mag, phase).to(torch.complex64)
    return img[None, None]


def complex_coil_maps(n, H, W, seed=0):
    """complex128 (n, H, W) coil sensitivity maps for runs without external data: the magnitudes of the synthetic "exp"
    maps (SENSE("exp", ...): exp(-dist / 2l) around a seeded anchor) times a smooth seeded phase, a second-order
    polynomial in the normalised coordinates with coefficients drawn from N(0, 1) per coil; RSS-normalised (the phase has
    unit modulus, so the "exp" normalisation carries over)."""
    import numpy as np
    from .ncsn.linear_transforms.undersampling_fourier import SENSE
    mag = SENSE("exp", n, 8, 0.04, (1, H, W), seed=seed, mask_mode="uniform").sens_maps.numpy()
    rng = np.random.RandomState(seed)
    u = np.linspace(-1.0, 1.0, H)[:, None]
    v = np.linspace(-1.0, 1.0, W)[None, :]
    maps = np.empty((n, H, W), dtype=np.complex128)
    for i in range(n):
        a = rng.randn(6)
        phase = a[0] + a[1] * u + a[2] * v + a[3] * u * v + a[4] * u * u + a[5] * v * v
        maps[i] = mag[i] * np.exp(1j * np.pi * 0.5 * phase)
    maps /= np.sqrt((np.abs(maps) ** 2).sum(0))
    return torch.from_numpy(maps)


def vd_mask_2d(H, W, R, center_frac=0.04, seed=0, partial_fourier=None):
    """bool (1, 1, H, W) variable-density 2-D sampling mask (the (ky, kz) pattern of a 3-D acquisition), numpy only and a
    pure function of its arguments: a fully sampled centre block of max(2, round(center_frac * H)) by
    max(2, round(center_frac * W)) samples, the rest drawn without replacement with a density 1 / (1 + (d / 0.25)^2) of the
    normalised distance d from the centre, so that exactly round(H * W / R) samples are set (the block alone when it is
    larger than that).  partial_fourier=f then zeroes the last 1 - f of the rows."""
    import numpy as np
    if R < 1:
        raise ValueError(f"vd_mask_2d: R {R} < 1")
    if partial_fourier is not None and not 0.0 < partial_fourier <= 1.0:
        raise ValueError(f"vd_mask_2d: partial_fourier {partial_fourier} outside (0, 1]")
    rng = np.random.RandomState(seed)
    bh, bw = min(H, max(2, int(round(center_frac * H)))), min(W, max(2, int(round(center_frac * W))))
    mask = np.zeros((H, W), dtype=bool)
    r0, c0 = H // 2 - bh // 2, W // 2 - bw // 2
    mask[r0:r0 + bh, c0:c0 + bw] = True
    n_draw = int(round(H * W / R)) - bh * bw
    if n_draw > 0:
        u = (np.arange(H) - H // 2) / (H / 2.0)
        v = (np.arange(W) - W // 2) / (W / 2.0)
        d2 = u[:, None] ** 2 + v[None, :] ** 2
        p = 1.0 / (1.0 + d2 / 0.25 ** 2)
        p[mask] = 0.0
        p = (p / p.sum()).ravel()
        mask.ravel()[rng.choice(H * W, size=n_draw, replace=False, p=p)] = True
    if partial_fourier is not None:
        mask[int(round(partial_fourier * H)):] = False
    return torch.from_numpy(mask)[None, None]


def radial_trajectory(n_spokes, n_readout, H, W, golden_angle=True):
    """float64 (n_spokes * n_readout, 2) radial k-space trajectory, (k_y, k_x) in cycles per field of view: spokes through
    the centre, readout position t = (j - n_readout/2) / n_readout in [-1/2, 1/2), spoke i at angle i * pi (sqrt(5) - 1) / 2
    (golden angle) or i * pi / n_spokes (uniform); k_y = t sin(angle) H, k_x = t cos(angle) W, inside [-N/2, N/2]."""
    import numpy as np
    if any(isinstance(v, bool) or int(v) != v or v < 1 for v in (n_spokes, n_readout, H, W)):
        raise ValueError(f"radial_trajectory: positive integers expected, got {(n_spokes, n_readout, H, W)}")
    t = (np.arange(int(n_readout), dtype=np.float64) - n_readout / 2.0) / n_readout
    i = np.arange(int(n_spokes), dtype=np.float64)
    ang = i * (np.pi * (np.sqrt(5.0) - 1.0) / 2.0) if golden_angle else i * (np.pi / n_spokes)
    ky = t[None, :] * np.sin(ang)[:, None] * H
    kx = t[None, :] * np.cos(ang)[:, None] * W
    return torch.from_numpy(np.stack([ky.reshape(-1), kx.reshape(-1)], axis=1))


def radial_cine_trajectory(n_frames, spokes_per_frame, n_readout, H, W):
    """float64 (n_frames, spokes_per_frame * n_readout, 2): golden-angle radial cine.  The spoke index runs on across the
    frames -- frame t holds spokes t * spokes_per_frame ... (t + 1) * spokes_per_frame - 1 of
    ``radial_trajectory(n_frames * spokes_per_frame, ...)`` --, so every frame has a trajectory of its own."""
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or n_frames < 1:
        raise ValueError(f"radial_cine_trajectory: n_frames must be a positive integer, got {n_frames}")
    k = radial_trajectory(int(n_frames) * spokes_per_frame, n_readout, H, W)
    return k.reshape(int(n_frames), int(spokes_per_frame) * int(n_readout), 2).contiguous()


def radial_density(trajectory, H, W):
    """float64 (M,) ramp density compensation of a radial trajectory: w proportional to the normalised radius
    sqrt((k_y/H)^2 + (k_x/W)^2), the centre samples at half the smallest non-zero radius, normalised to sum w = H W.  For
    the zero-filled image only; the likelihood's weights stay 1.  A framed trajectory (T, M, 2) gives (T, M), every frame
    normalised on its own."""
    k = torch.as_tensor(trajectory, dtype=torch.float64)
    if k.dim() == 3 and k.shape[2] == 2 and k.shape[0] >= 1 and k.shape[1] >= 1:
        return torch.stack([radial_density(k[t], H, W) for t in range(k.shape[0])])
    if k.dim() != 2 or k.shape[1] != 2 or k.shape[0] < 1:
        raise ValueError(f"radial_density: trajectory {tuple(k.shape)} is not (M, 2)")
    r = torch.sqrt((k[:, 0] / H) ** 2 + (k[:, 1] / W) ** 2)
    pos = r[r > 0]
    floor = 0.5 * float(pos.min()) if pos.numel() else 1.0
    r = torch.where(r > 0, r, torch.full_like(r, floor))
    return r * (float(H * W) / float(r.sum()))
