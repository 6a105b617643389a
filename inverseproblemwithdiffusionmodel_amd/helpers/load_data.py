"""``load_config`` (mirror of the reference's ``helpers/load_data.py:301-321``): YAML -> nested Namespace,
``config.device`` injected, ``mode == "complex"`` switches to 2 channels.

Real-data front end (mirror of ``helpers/load_data.py:125-164`` load_cine, ``:167-226``
load_tissue_data / vol2slice / LoadDataNumpyDict, ``:241-283`` load_ACDC, ``:372-397`` add_phase): the on-disk formats
either side of the fast path -- ACDC slice ``.npz`` files (keys image, multiClassMasks, PD, T1, T2) and CINE ``.mat``
stacks (key ``imgs``, (H, W, T, N)).  The reference drives MONAI dictionary transforms; MONAI is not vendored (version
unpinned), so ``ScaleIntensityd`` / ``CropForegroundd`` / ``Resized`` / ``Resize`` are restated from their
published behaviour (min-max scaling, bounding box of ``image > 0``, ``torch.nn.functional.interpolate`` with the
transform's mode) -- PARITY UNPINNED for the exact resampled pixel values; training-time augmentation (RandRotated ...)
is out of scope.  Host-side data preparation: plain numpy / torch-CPU, nothing here runs per sampling step."""
import glob
import os
import random
from typing import Union

import numpy as np
import torch
import torch.nn.functional as F

from .utils import load_yml_file

_CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ncsn", "configs")
REGISTERED_DATA_CONFIG_FILENAME = {
    "MNIST": os.path.join(_CFG_DIR, "mnist.yml"),
    "CINE127": os.path.join(_CFG_DIR, "cine127.yml"),
    "CINE127_1D": os.path.join(_CFG_DIR, "cine127_1d.yml"),
    "ACDC": os.path.join(_CFG_DIR, "acdc.yml"),
}


def load_config(ds_name, mode="real-valued", device=None, **kwargs):
    assert mode in ["real-valued", "mag", "complex", "real-imag", "real-imag-random"]
    assert ds_name in REGISTERED_DATA_CONFIG_FILENAME.keys()
    if device is None:
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    cfg = load_yml_file(REGISTERED_DATA_CONFIG_FILENAME[ds_name])
    cfg.device = device
    if mode == "complex":
        cfg.data.channels = 2
    return cfg


# ---- real-data front end ----------------------------------------------------------------------------------------------
IMAGE_KEY, LABEL_KEY = "image", "label"          # monai.utils.CommonKeys.IMAGE / LABEL


def load_tissue_data(path_to_file):
    """one ACDC .npz: image intensity, multi-class segmentation, PD, T1, T2 ([1, N_slices, Nx, Ny] volumes or (1, H, W)
    slices written by vol2slice)"""
    data = np.load(path_to_file)
    return data["image"], data["multiClassMasks"], data["PD"], data["T1"], data["T2"]


def vol2slice(root_dir, save_dir):
    """save every slice of every volume .npz as its own .npz, all arrays (1, H, W)"""
    os.makedirs(save_dir, exist_ok=True)
    for filename in glob.glob(os.path.join(root_dir, "*.npz")):
        image, multi_class, PD, T1, T2 = load_tissue_data(filename)
        base = os.path.basename(filename)
        stem = base[:base.find(".npz")]
        for k in range(image.shape[1]):
            np.savez(os.path.join(save_dir, f"{stem}_{k}.npz"), image=image[:, k, ...], multiClassMasks=multi_class[:, k, ...],
                     PD=PD[:, k, ...], T1=T1[:, k, ...], T2=T2[:, k, ...])


class LoadDataNumpyDict:
    """filename -> {image (1, H, W) float32, label (1, H, W) int64 with the chosen classes merged to 1}"""

    def __init__(self, seg_labels: list):
        self.seg_labels = seg_labels

    def __call__(self, filename):
        image, label, _, _, _ = load_tissue_data(filename)
        label_out = np.zeros_like(label, dtype=np.int64)
        for seg_label in self.seg_labels:
            label_out[label == seg_label] = 1
        return {IMAGE_KEY: torch.tensor(image).float(), LABEL_KEY: torch.tensor(label_out).long()}


def _scale_intensity(img):
    """monai ScaleIntensity defaults: (x - min) / (max - min) -> [0, 1]"""
    lo, hi = img.min(), img.max()
    return (img - lo) / (hi - lo) if float(hi - lo) != 0.0 else img - lo


def _crop_foreground(data, source_key=IMAGE_KEY):
    """monai CropForegroundd defaults: bounding box of source > 0 over the spatial axes, margin 0"""
    fg = (data[source_key] > 0).any(dim=0)
    if not bool(fg.any()):
        return data
    rows, cols = torch.where(fg.any(dim=1))[0], torch.where(fg.any(dim=0))[0]
    r0, r1, c0, c1 = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
    return {k: v[:, r0:r1, c0:c1] for k, v in data.items()}


def _resize(img, size, mode):
    """monai Resize: torch.nn.functional.interpolate on (1, C, *spatial) with align_corners=None (True where asked)"""
    x = img[None].float()
    if mode in ("nearest", "area"):
        y = F.interpolate(x, size=size, mode=mode)
    else:
        y = F.interpolate(x, size=size, mode=mode, align_corners=False)
    return y[0].to(img.dtype) if mode == "nearest" else y[0]


class ACDCSliceDataset(torch.utils.data.Dataset):
    """what load_ACDC(if_aug=False) returns: ds[i] -> {image (1, 256, 256) float32 in [0, 1], label (1, 256, 256) int64}"""

    def __init__(self, filenames, seg_labels, spatial_size=(256, 256)):
        self.filenames, self.loader, self.spatial_size = list(filenames), LoadDataNumpyDict(seg_labels), spatial_size

    def __len__(self):
        return len(self.filenames)

    def __getitem__(self, idx):
        d = self.loader(self.filenames[idx])
        d[IMAGE_KEY] = _scale_intensity(d[IMAGE_KEY])
        d = _crop_foreground(d)
        return {IMAGE_KEY: _resize(d[IMAGE_KEY], self.spatial_size, "bilinear"),
                LABEL_KEY: _resize(d[LABEL_KEY], self.spatial_size, "nearest")}


def load_ACDC(root_dir, train_test_split=(0.8, 0.1), seg_labels=(3,), mode="train", seed=0, num_workers=4, if_aug=True):
    """file split exactly as the reference (glob order shuffled by random.seed(seed), 80/10/10); seg_label 3: left MYO.
    Training-time augmentation is not built: if_aug is accepted and ignored outside training."""
    assert mode in ["train", "val", "test"]
    all_filenames = glob.glob(os.path.join(root_dir, "*.npz"))
    random.seed(seed)
    random.shuffle(all_filenames)
    a = int(len(all_filenames) * train_test_split[0])
    b = int(len(all_filenames) * sum(train_test_split))
    filenames = {"train": all_filenames[:a], "val": all_filenames[a:b], "test": all_filenames[b:]}[mode]
    return ACDCSliceDataset(filenames, list(seg_labels))


def load_cine(root_dir, mode="train", img_key="imgs", flatten=True, flatten_type="spatial",
              resize_shape: Union[int, None] = None, resize_shape_T=None, win_size=2, **kwargs):
    """CINE .mat stack (H, W, T, N) -> per-volume min-max normalised TensorDataset: 'spatial' (N*T, 1, H0, W0) frames,
    'temporal' (N', win_size^2, T') patch time series (reshape_temporal_dim)"""
    import scipy.io as sio
    from .utils import reshape_temporal_dim
    assert mode in ["train", "val", "test"]
    assert flatten_type in ["spatial", "temporal"]
    if mode == "val":
        mode = "test"
    filename = glob.glob(os.path.join(root_dir, f"*{mode}*.mat"))[0]
    ds = sio.loadmat(filename)[img_key].transpose(3, 2, 0, 1)                      # (N, T, H, W)
    lo, hi = ds.min(axis=(1, 2, 3), keepdims=True), ds.max(axis=(1, 2, 3), keepdims=True)
    ds = (ds - lo) / (hi - lo)
    if flatten:
        N, T, H, W = ds.shape
        if flatten_type == "spatial":
            ds = torch.tensor(ds.reshape(-1, H, W))
            if resize_shape is not None and not (H == resize_shape and W == resize_shape):
                ds = _resize(ds, (resize_shape, resize_shape), "area")              # frames as channels, monai Resize default
            ds = ds[:, None, ...]
        else:
            size = (T if resize_shape_T is None else resize_shape_T, H if resize_shape is None else resize_shape,
                    W if resize_shape is None else resize_shape)
            ds = _resize(torch.tensor(ds), size, "area")                            # (N, T', H', W')
            ds = reshape_temporal_dim(ds, win_size, win_size)
    if isinstance(ds, np.ndarray):
        ds = torch.tensor(ds)
    return torch.utils.data.TensorDataset(ds)


def add_phase(imgs: torch.Tensor, init_shape: Union[tuple, int] = (5, 5), seed=None, mode="spatial"):
    """smooth random phase: N(0,1) patch of `init_shape` per image / channel, resized bicubic (spatial) or trilinear
    (2D+time) with align_corners=True, imgs * exp(i phase) -> complex64.  imgs (B, C, H, W) or (T, C, H, W)."""
    assert mode in ["spatial", "2D+time"]
    if seed is not None:
        torch.manual_seed(seed)
    if mode == "spatial":
        B, C, H, W = imgs.shape
        out = torch.empty(imgs.shape, dtype=torch.complex64, device=imgs.device)
        for i in range(B):
            patch = torch.randn(C, *init_shape, device=imgs.device)
            phase = F.interpolate(patch[None], size=(H, W), mode="bicubic", align_corners=True)[0]
            out[i] = imgs[i] * torch.exp(1j * phase)
        return out
    assert len(init_shape) == 3
    T, C, H, W = imgs.shape
    patch = torch.randn(C, *init_shape, device=imgs.device)
    phase = F.interpolate(patch[None], size=(T, H, W), mode="trilinear", align_corners=True)[0]     # (C, T, H, W)
    return imgs * torch.exp(1j * phase.permute(1, 0, 2, 3))


REGISTERED_DATA_ROOT_DIR = {}          # name -> directory; the reference hard-codes cluster paths (load_data.py:33-60)


def load_data(ds_name, mode="train", root_dir=None, **kwargs):
    """dispatcher (mirror of helpers/load_data.py:62-93 for the two on-disk datasets of the fast path)"""
    root = root_dir if root_dir is not None else REGISTERED_DATA_ROOT_DIR.get(ds_name)
    if root is None:
        raise FileNotFoundError(f"no data directory registered for {ds_name!r}: pass root_dir= or set "
                                "REGISTERED_DATA_ROOT_DIR (no data ships with the reference)")
    if ds_name == "ACDC":
        return load_ACDC(root, mode=mode, **kwargs)
    if ds_name == "CINE64":
        return load_cine(root, mode=mode, **kwargs)
    if ds_name == "CINE127":
        return load_cine(root, mode=mode, resize_shape=128, **kwargs)
    raise NotImplementedError(f"dataset {ds_name!r}: only the ACDC .npz and CINE .mat front ends are built")


def load_sens_maps(path):
    """coil sensitivity maps (n_coils, H, W), real or complex, from a ``.npy`` or ``.pt`` file -> host tensor
    (float64 / complex128), ready for ``SENSE("custom", ..., sens_maps=...)``"""
    import numpy as np
    import torch
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        maps = torch.from_numpy(np.load(path, allow_pickle=False))
    elif ext == ".pt":
        maps = torch.load(path, map_location="cpu")
        if isinstance(maps, np.ndarray):
            maps = torch.from_numpy(maps)
    else:
        raise ValueError(f"load_sens_maps: {path!r}: a .npy or .pt file")
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3:
        raise ValueError(f"load_sens_maps: {path!r} must hold one array of shape (n_coils, H, W)")
    if not (maps.is_complex() or maps.is_floating_point()):
        raise TypeError(f"load_sens_maps: {path!r} holds {maps.dtype}; real or complex floating maps expected")
    return maps.to(torch.complex128 if maps.is_complex() else torch.float64)


def load_kspace(path, cine=False, slices=False, noncartesian=False):
    """measured multi-coil k-space (n_coils, H, W) -- cine=True: 2D+time k-space (n_coils, T, H, W); slices=True: a stack
    of slices (S, n_coils, H, W); noncartesian=True: the samples of a trajectory (n_coils, M), in the order of
    ``load_trajectory``'s positions; noncartesian=True with cine=True: the samples of a framed trajectory (n_coils, T, M)
    -- from a ``.npy`` or ``.pt`` file -> host complex64 tensor, centred with orthonormal
    scale as ``SENSE.__call__`` produces it (``engine.build_problem(measurement=...)``, ``SENSE.from_cine_measurement``);
    any other rank or a real dtype is a ValueError"""
    if cine and slices:
        raise ValueError("load_kspace: cine=True or slices=True, not both (a cine volume is not served)")
    if noncartesian and slices:
        raise ValueError("load_kspace: noncartesian=True takes cine=True (n_coils, T, M) or neither cine=True nor slices=True "
                         "(n_coils, M); a stack of slices is not served")
    import numpy as np
    import torch
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        y = torch.from_numpy(np.load(path, allow_pickle=False))
    elif ext == ".pt":
        y = torch.load(path, map_location="cpu")
        if isinstance(y, np.ndarray):
            y = torch.from_numpy(y)
    else:
        raise ValueError(f"load_kspace: {path!r}: a .npy or .pt file")
    if noncartesian:
        if not isinstance(y, torch.Tensor) or y.dim() != (3 if cine else 2):
            raise ValueError(f"load_kspace: {path!r} must hold one array of shape {'(n_coils, T, M)' if cine else '(n_coils, M)'}")
    elif not isinstance(y, torch.Tensor) or y.dim() != (4 if cine or slices else 3):
        raise ValueError(f"load_kspace: {path!r} must hold one array of shape "
                         f"{'(n_coils, T, H, W)' if cine else '(S, n_coils, H, W)' if slices else '(n_coils, H, W)'}")
    if not y.is_complex():
        raise ValueError(f"load_kspace: {path!r} holds {y.dtype}; complex k-space expected")
    return y.to(torch.complex64).contiguous()


def load_trajectory(path, cine=False):
    """k-space trajectory (M, 2) = (k_y, k_x) in cycles per field of view -- cine=True: (T, M, 2), one trajectory per frame
    --, real, from a ``.npy`` or ``.pt`` file -> host float64 tensor for ``NonCartesianSENSE`` /
    ``engine.build_problem(trajectory=...)``; that it is finite and inside [-N/2, N/2] is checked where the image size is
    known"""
    import numpy as np
    import torch
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        k = torch.from_numpy(np.load(path, allow_pickle=False))
    elif ext == ".pt":
        k = torch.load(path, map_location="cpu")
        if isinstance(k, np.ndarray):
            k = torch.from_numpy(k)
    else:
        raise ValueError(f"load_trajectory: {path!r}: a .npy or .pt file")
    if cine:
        if not isinstance(k, torch.Tensor) or k.dim() != 3 or k.shape[2] != 2 or k.shape[0] < 1 or k.shape[1] < 1:
            raise ValueError(f"load_trajectory: {path!r} must hold one array of shape (T, M, 2) = (k_y, k_x) per frame and sample")
    elif not isinstance(k, torch.Tensor) or k.dim() != 2 or k.shape[1] != 2 or k.shape[0] < 1:
        raise ValueError(f"load_trajectory: {path!r} must hold one array of shape (M, 2) = (k_y, k_x) per sample")
    if k.is_complex() or not k.is_floating_point():
        raise TypeError(f"load_trajectory: {path!r} holds {k.dtype}; real floating positions expected")
    return k.to(torch.float64).contiguous()


def load_noise_cov(path):
    """coil noise covariance (n_coils, n_coils), real or complex, from a ``.npy`` or ``.pt`` file -> host tensor
    (float64 / complex128) for ``noise_cov=``; that it is Hermitian positive definite is checked where it is used
    (``ops.check_noise_cov``)"""
    import numpy as np
    import torch
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        psi = torch.from_numpy(np.load(path, allow_pickle=False))
    elif ext == ".pt":
        psi = torch.load(path, map_location="cpu")
        if isinstance(psi, np.ndarray):
            psi = torch.from_numpy(psi)
    else:
        raise ValueError(f"load_noise_cov: {path!r}: a .npy or .pt file")
    if not isinstance(psi, torch.Tensor) or psi.dim() != 2 or psi.shape[0] != psi.shape[1]:
        raise ValueError(f"load_noise_cov: {path!r} must hold one square matrix (n_coils, n_coils)")
    if not (psi.is_complex() or psi.is_floating_point()):
        raise TypeError(f"load_noise_cov: {path!r} holds {psi.dtype}; a real or complex floating matrix expected")
    return psi.to(torch.complex128 if psi.is_complex() else torch.float64)


def load_mask(path):
    """k-space sampling mask from a ``.npy`` or ``.pt`` file -> host tensor, dtype and shape as stored: a line mask
    ((W,), (1, 1, W), (T, 1, 1, W)) or a 2-D mask ((H, W), (1, 1, H, W), (T, 1, H, W)), bool, integer or real floating
    (non-zero = sampled), ready for ``SENSE(..., mask_mode="custom", mask=...)`` or ``op.random_under_fourier.mask = ...``"""
    import numpy as np
    import torch
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        mask = torch.from_numpy(np.load(path, allow_pickle=False))
    elif ext == ".pt":
        mask = torch.load(path, map_location="cpu")
    else:
        raise ValueError(f"load_mask: {path!r}: a .npy or .pt file")
    if not isinstance(mask, torch.Tensor) or not 1 <= mask.dim() <= 4:
        raise ValueError(f"load_mask: {path!r} must hold one array of 1 to 4 dims")
    if mask.is_complex():
        raise TypeError(f"load_mask: {path!r} holds {mask.dtype}; a bool, integer or real floating mask expected")
    return mask


def driver_mask(path, mask_2d, H, W, R, seed):
    """-> the mask a driver assigns to ``op.random_under_fourier.mask`` for --mask PATH or --mask_2d, None for the default
    line mask; a (T, H, W) stack from a file (per-frame 2-D masks) becomes (T, 1, H, W)"""
    if path and mask_2d:
        raise ValueError("--mask and --mask_2d exclude each other")
    if path:
        mask = load_mask(path)
        if mask.dim() == 3 and tuple(mask.shape[-2:]) == (H, W) and mask.shape[0] != 1:
            mask = mask[:, None]
        return mask
    if mask_2d:
        from ..synthetic import vd_mask_2d
        return vd_mask_2d(H, W, R, seed=seed if seed is not None else 0)
    return None


def add_sens_map_args(parser):
    """the drivers' coil-map flags: --sens_maps PATH (measured maps from a file) and --sens_phase (synthetic complex maps)"""
    parser.add_argument("--sens_maps", default=None,
                        help=".npy / .pt file with measured coil maps (num_sens, H, W), real or complex")
    parser.add_argument("--sens_phase", action="store_true",
                        help="synthetic COMPLEX coil maps: the exp magnitudes times a smooth seeded phase")


def driver_sens_maps(path, sens_phase, num_sens, H, W, seed):
    """-> (maps or None, num_sens): the RSS-normalised maps a driver assigns to ``op.sens_maps`` for --sens_maps PATH or
    --sens_phase, None for the default synthetic real maps; a file sets the coil count"""
    from ..ncsn.linear_transforms.undersampling_fourier import SENSE
    if path:
        maps = load_sens_maps(path)
        if tuple(maps.shape[-2:]) != (H, W):
            raise ValueError(f"--sens_maps {path!r}: maps {tuple(maps.shape)} for {H}x{W} images")
        return SENSE.rss_normalize(maps), int(maps.shape[0])
    if sens_phase:
        from ..synthetic import complex_coil_maps
        return complex_coil_maps(num_sens, H, W, seed), num_sens
    return None, num_sens


def add_maps_method_args(parser):
    """the drivers' choice of the coil-map estimator behind --estimate_maps"""
    parser.add_argument("--maps_method", choices=["walsh", "espirit"], default="walsh",
                        help="--estimate_maps: Walsh's adaptive estimator (default) or ESPIRiT (up to 16 coils and "
                             "n_coils * K^2 <= 432; more coils go through --coil_compress first)")
    parser.add_argument("--espirit_kernel", type=int, default=6, metavar="K", help="--maps_method espirit: kernel side, 3..8")
    parser.add_argument("--espirit_thresh", type=float, default=0.02, metavar="T",
                        help="--maps_method espirit: singular values of the calibration matrix above T * the largest span "
                             "the row space (noisy data may want another value)")
    parser.add_argument("--espirit_crop", type=float, default=0.8, metavar="C",
                        help="--maps_method espirit: the maps are zero where the eigenvalue of G(x) is at most C")


def driver_maps_method(a, estimate_maps, n_coils, H, W, region):
    """host-side check of add_maps_method_args' flags, before a score network is built or a GPU touched; every failure is a
    ``sys.exit``.  a: the parsed flags (Namespace or dict); n_coils: the coils the estimator sees (the virtual ones with
    --coil_compress); region: the calibration half-widths.  -> (method, kwargs for the estimator)"""
    import math
    import sys
    from .. import ops
    get = a.get if isinstance(a, dict) else lambda k: getattr(a, k)
    method = get("maps_method")
    if method == "walsh":
        return "walsh", {}
    if not estimate_maps:
        sys.exit("--maps_method espirit goes with --estimate_maps")
    k, t, c = get("espirit_kernel"), get("espirit_thresh"), get("espirit_crop")
    if not (math.isfinite(t) and 0.0 <= t < 1.0):
        sys.exit(f"--espirit_thresh {t}: a fraction of the largest singular value, 0 <= T < 1")
    if not (math.isfinite(c) and 0.0 <= c < 1.0):
        sys.exit(f"--espirit_crop {c}: an eigenvalue threshold, 0 <= C < 1")
    try:
        ops.espirit_check(n_coils, k, region[0], region[1], H, W, "--maps_method espirit")
    except (ValueError, NotImplementedError) as e:
        sys.exit(str(e))
    return "espirit", dict(ksize=k, sv_thresh=t, crop=c)


def add_self_calibrate_args(parser):
    """the drivers' non-Cartesian self-calibration flags (with --trajectory; --noise_cov, --calib_max and --maps_method are
    the flags the Cartesian calibration already has)"""
    parser.add_argument("--self_calibrate", action="store_true",
                        help="--trajectory: estimate the coil maps from the non-Cartesian samples themselves (the window of "
                             "samples about the k-space centre); --kspace PATH then needs no --sens_maps")
    parser.add_argument("--virtual_coils", type=int, default=None, metavar="N",
                        help="--self_calibrate: whiten (--noise_cov PATH) and compress the samples (up to 64 coils) to N <= 32 "
                             "virtual coils first; the maps are those of the virtual coils")


def driver_self_calibrate(a, trajectory, H, W, num_sens):
    """host-side check of --self_calibrate and its companions, before a score network is built or a GPU touched; every
    failure is a ``sys.exit``.  a: the parsed flags (Namespace or dict); trajectory: the checked trajectory, (M, 2) or
    (T, M, 2), None without --trajectory.  -> None without --self_calibrate, else Namespace(virtual_coils, noise_cov,
    calib_max, maps_method, maps_kwargs, region)"""
    import sys
    from argparse import Namespace
    from ..ncsn.linear_transforms.noncartesian import NonCartesianSENSE, calibration_window
    get = a.get if isinstance(a, dict) else lambda k: getattr(a, k)
    if not get("self_calibrate"):
        if get("virtual_coils") is not None:
            sys.exit("--virtual_coils N goes with --self_calibrate")
        return None
    if trajectory is None:
        sys.exit("--self_calibrate goes with --trajectory (Cartesian data: --estimate_maps, --coil_compress)")
    if get("sens_maps") or get("sens_phase"):
        sys.exit("--self_calibrate estimates the coil maps; it does not go with --sens_maps / --sens_phase")
    if get("noise_cov") and get("virtual_coils") is None:
        sys.exit("--noise_cov PATH goes with --virtual_coils N (whitening is part of the compression)")
    try:
        noise_cov = load_noise_cov(get("noise_cov")) if get("noise_cov") else None
        ah, aw, _ = calibration_window(trajectory, H, W, get("calib_max"))
    except (ValueError, TypeError) as e:
        sys.exit(f"--self_calibrate: {e}")
    n_est = num_sens if get("virtual_coils") is None else get("virtual_coils")
    maps_method, maps_kwargs = driver_maps_method(a, True, n_est, H, W, (ah, aw))
    try:
        _, noise_cov, _ = NonCartesianSENSE._check_calib(num_sens, get("virtual_coils"), noise_cov, H, W, ah, aw, maps_method,
                                                         dict(maps_kwargs), "--self_calibrate")
    except (ValueError, TypeError, NotImplementedError) as e:
        sys.exit(str(e))
    return Namespace(virtual_coils=get("virtual_coils"), noise_cov=noise_cov, calib_max=get("calib_max"), maps_method=maps_method,
                     maps_kwargs=maps_kwargs, region=(ah, aw))


def add_cine_measurement_args(parser):
    """the cine drivers' measured-data flags, with the meanings scripts/acdc_SENSE_real_img.py gives them"""
    parser.add_argument("--kspace", default=None,
                        help=".npy / .pt file with measured 2D+time multi-coil k-space (n_coils, T, H, W), complex, centred "
                             "with orthonormal scale; sets T and the coil count, needs --mask PATH and --estimate_maps")
    parser.add_argument("--estimate_maps", action="store_true",
                        help="estimate the coil maps from the calibration region of the time-averaged measurement")
    parser.add_argument("--calib_max", type=int, default=12, help="--estimate_maps: largest calibration half-width")
    parser.add_argument("--coil_compress", type=int, default=None, metavar="N",
                        help="whiten and compress the measurement (up to 64 coils) to N <= 32 virtual coils by PCA of the "
                             "calibration region of its time average: one matrix for all frames; needs --estimate_maps")
    parser.add_argument("--noise_cov", default=None,
                        help="--coil_compress: .npy / .pt file with the (n_coils, n_coils) coil noise covariance of the prescan")
    parser.add_argument("--kspace_scale", default="auto",
                        help="--kspace: factor on the measurement; auto: 1 / the peak of its composite calibration image")
    add_maps_method_args(parser)


def cine_measurement_requested(a):
    """whether any of add_cine_measurement_args' flags asks for the calibrated path (a: the parsed Namespace)"""
    return bool(a.kspace or a.estimate_maps or a.coil_compress is not None or a.noise_cov or a.maps_method != "walsh")


def driver_cine_checks(a, H, W, T, num_sens, mask):
    """host-side part of the cine drivers' calibrated path, run before a score network is built or a GPU touched: flag
    combinations, the measured file, the compression arguments and the composite calibration region; every failure is a
    ``sys.exit`` with the message scripts/acdc_SENSE_real_img.py gives.  a: the parsed flags (kspace, mask, sens_maps,
    sens_phase, estimate_maps, calib_max, coil_compress, noise_cov, kspace_scale, R, seed); mask: what driver_mask
    returned.  -> Namespace(kspace (n, T, H, W) or None, H, W, T, num_sens, noise_cov, kspace_scale (float or None))"""
    import sys
    from argparse import Namespace
    from .. import ops
    from ..ncsn.linear_transforms import undersampling_fourier as uf
    kspace = None
    if a.kspace:
        if not a.mask:
            sys.exit("--kspace PATH needs --mask PATH, the sampling mask of the acquisition")
        if a.sens_maps or a.sens_phase or not a.estimate_maps:
            sys.exit("--kspace PATH takes its coil maps from --estimate_maps (the time-averaged calibration region)")
        try:
            kspace = load_kspace(a.kspace, cine=True)
        except (ValueError, TypeError) as e:
            sys.exit(str(e))
        num_sens, T, H, W = (int(s) for s in kspace.shape)
    if a.noise_cov and a.coil_compress is None:
        sys.exit("--noise_cov PATH goes with --coil_compress N (whitening is part of the compression)")
    if a.coil_compress is not None and not a.estimate_maps:
        sys.exit("--coil_compress N needs --estimate_maps (the maps of the virtual coils come from the composite)")
    if ops.kspace_size_class(H, W) == ops.KSPACE_NONE:
        sys.exit(f"{H}x{W}: no k-space kernel for this size; {ops.KSPACE_SIZE_RULE}")
    noise_cov = None
    if a.coil_compress is not None:                                        # a bad N or a bad covariance fails here
        try:
            ops._coilcomp_counts(num_sens, a.coil_compress, "--coil_compress")
            if a.noise_cov:
                noise_cov = ops.check_noise_cov(load_noise_cov(a.noise_cov), num_sens, "--noise_cov")
        except (ValueError, TypeError, NotImplementedError) as e:
            sys.exit(str(e))
    if mask is None:
        mask = uf.RandomUndersamplingFourier(a.R, 0.04, (1, H, W), a.seed, mask_T=24 if T == 24 else 1).mask
    try:
        if kspace is not None:
            uf.SENSE._cine_operands(kspace, mask, "--kspace / --mask")
        region = uf.calibration_region(mask, H, W, a.calib_max, composite=True)
    except (ValueError, TypeError) as e:
        sys.exit(f"--estimate_maps / --coil_compress / --kspace: {e}")
    maps_method, maps_kwargs = driver_maps_method(a, a.estimate_maps, num_sens if a.coil_compress is None else a.coil_compress,
                                                  H, W, region)
    return Namespace(kspace=kspace, H=H, W=W, T=T, num_sens=num_sens, noise_cov=noise_cov,
                     kspace_scale=None if a.kspace_scale == "auto" else float(a.kspace_scale), maps_method=maps_method,
                     maps_kwargs=maps_kwargs)


def driver_cine_measurement(a, checked, op, frames, device):
    """GPU part of the cine drivers' calibrated path: the measurement -- the file's, or frames (T, C, H, W) simulated
    through `op` with its true maps -- calibrated by ``SENSE.from_cine_measurement`` (time-averaged composite, one
    compression matrix for all frames, maps of the composite).  checked: driver_cine_checks' result.
    -> (from_cine_measurement's Namespace with `measurement` scaled and `kspace_scale` added (None for simulated data),
    the operator to reconstruct with)"""
    from ..ncsn.linear_transforms.undersampling_fourier import SENSE
    if checked.kspace is not None:
        y, mask = checked.kspace.to(device), driver_mask(a.mask, False, checked.H, checked.W, a.R, a.seed)
    else:
        y = op(frames).reshape(op.num_sens, checked.T, checked.H, checked.W)
        mask = op.random_under_fourier.mask
    cal = SENSE.from_cine_measurement(y, mask, R=a.R, seed=a.seed, calib_max=a.calib_max, n_virtual=a.coil_compress,
                                      noise_cov=checked.noise_cov, method=checked.maps_method, **checked.maps_kwargs)
    cal.kspace_scale = None
    if checked.kspace is not None:
        cal.kspace_scale = checked.kspace_scale
        if cal.kspace_scale is None:
            if not cal.rss_max > 0.0:
                raise ValueError("--kspace: the calibration region of the time-averaged measurement holds no signal")
            cal.kspace_scale = 1.0 / cal.rss_max
        cal.measurement = cal.measurement * cal.kspace_scale
    return cal, cal.op
