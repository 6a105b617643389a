"""torch-tensor front end of the libipdm.so kernels: device memory, shapes and streams come from
PyTorch-ROCm (plumbing), all arithmetic happens in the hand-written HIP kernels (csrc/).

Every function requires GPU tensors and raises otherwise -- there is no CPU path.
"""
import contextlib
import ctypes
import os

import torch

from . import _lib
from ._lib import call, P

ACT_NONE, ACT_ELU, ACT_RELU, ACT_LRELU02, ACT_SWISH = 0, 1, 2, 3, 4
ACT_COPY = 5          # identity as an `act_out` code: "produce the second output, unactivated" (with res_second: conv + residual)
CONV_TRACE = None     # set to a list by engine.conv_census(): per-launch shapes + HIP events

ACT_CODES = {"none": ACT_NONE, None: ACT_NONE, "elu": ACT_ELU, "relu": ACT_RELU, "lrelu": ACT_LRELU02,
             "swish": ACT_SWISH}


def _gpu(t, dtype=None, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ipdm: {name} must be a GPU tensor (the HIP path has no CPU fallback); got "
                           f"{getattr(t, 'device', type(t))}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"ipdm: {name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return P(t.data_ptr()) if t is not None else P(0)


def _inplace_operand(t, dtype, name):
    """operand of an in-place / raw-pointer kernel: must already be a contiguous GPU tensor of the kernel's dtype
    (a silent .contiguous() copy would make the kernel update the copy; a wrong dtype would be read as raw memory)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ipdm: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"ipdm: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"ipdm: {name} must be contiguous (in-place kernel operand; call .contiguous() yourself and "
                         "keep the result)")
    return t


# One stream per device.  Two HSA queues on one card corrupt each other's packed-fp32 VALU results while certain MFMA kernels are
# resident (profiles/r03_shared_card_probe.txt; sharding.py), and kernels of ONE stream never overlap -- so the library refuses
# to be driven from a second eager stream of the same device.  Capture streams are exempt (torch.cuda.graph records on a side
# stream that never executes; a graph replays on the stream that launches it).  IPDM_ALLOW_MULTI_STREAM=1 lifts the check.
_STREAM_OF_DEVICE = {}


def _written(*tensors):
    """the kernels write through raw pointers, which torch's version counters never see: every op that stores into an EXISTING
    tensor reports it here, so that whatever was cached under (version, data_ptr) of that storage -- per-image maxima
    (`_ipdm_amax`), statistics partials (`_ipdm_partials`) -- goes stale for every alias (views share the counter).  Without this
    the sampler state, updated in place by the fused Langevin / proximal kernel, kept the maxima measured on its FIRST
    iteration: the segmentation network's first convolution then overflowed fp16 as the state grew (caught by
    test_guided_sense_trajectory_vs_oracle).  Host-side bookkeeping only; no launch."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def _stream():
    st = torch.cuda.current_stream()
    h = st.cuda_stream
    if _STREAM_OF_DEVICE.get(st.device_index, h) != h or st.device_index not in _STREAM_OF_DEVICE:
        _note_stream(st.device_index, h)
    return P(h)


def _note_stream(dev, h):
    if torch.cuda.is_current_stream_capturing():
        return
    first = _STREAM_OF_DEVICE.setdefault(dev, h)
    if first != h and os.environ.get("IPDM_ALLOW_MULTI_STREAM", "0") != "1":
        raise RuntimeError(
            f"ipdm: kernels were launched on stream {first:#x} of cuda:{dev} and now on stream {h:#x}: this library runs on ONE "
            "stream per device (two queues on one MI355X silently corrupt packed-fp32 results, "
            "profiles/r03_shared_card_probe.txt). Use one stream, or set IPDM_ALLOW_MULTI_STREAM=1 to take the risk.")


def _c64_as_f32(t):
    return torch.view_as_real(t)


# ---- StyleGAN2 ops -----------------------------------------------------------------------------
_FLOAT_SUFFIX = {torch.float32: "f32", torch.float16: "f16", torch.float64: "f64"}   # the reference's dispatch types


def _float_suffix(t, what):
    try:
        return _FLOAT_SUFFIX[t.dtype]
    except KeyError:
        raise TypeError(f"ipdm {what}: dtype {t.dtype} (float32 / float16 / float64, as the reference's "
                        "AT_DISPATCH_FLOATING_TYPES_AND_HALF)") from None


def upfirdn2d_raw(x, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """x [major, in_h, in_w, minor] -> [major, out_h, out_w, minor] (the reference extension's signature);
    float32 (the tuned kernels), float16 or float64 storage; the taps are cast to the input's dtype"""
    sfx = _float_suffix(x, "upfirdn2d")
    x = _gpu(x, x.dtype, "input")
    kernel = _gpu(kernel.to(x.dtype), x.dtype, "kernel")
    major, in_h, in_w, minor = x.shape
    kh, kw = kernel.shape
    out_h = (in_h * up_y + pad_y0 + pad_y1 - kh) // down_y + 1
    out_w = (in_w * up_x + pad_x0 + pad_x1 - kw) // down_x + 1
    out = torch.empty((major, out_h, out_w, minor), dtype=x.dtype, device=x.device)
    call(f"ipdm_upfirdn2d_{sfx}", _ptr(x), _ptr(kernel), _ptr(out), major, in_h, in_w, minor, kh, kw,
         up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, _stream())
    return out


def fused_bias_act_raw(x, bias, ref, act, grad, alpha, scale):
    sfx = _float_suffix(x, "fused_bias_act")
    x = _gpu(x, x.dtype, "input")
    bias = None if bias is None or bias.numel() == 0 else _gpu(bias.to(x.dtype), x.dtype, "bias")
    ref = None if ref is None or ref.numel() == 0 else _gpu(ref, x.dtype, "refer")
    step_b = 1
    for s in x.shape[2:]:
        step_b *= s
    y = torch.empty_like(x)
    call(f"ipdm_fused_bias_act_{sfx}", _ptr(x), _ptr(bias), _ptr(ref), _ptr(y), x.numel(), step_b,
         0 if bias is None else bias.numel(), act, grad, float(alpha), float(scale), _stream())
    return y


# ---- k-space --------------------------------------------------------------------------------
KSPACE_NONE, KSPACE_LDS, KSPACE_STRIPS = 0, 1, 2
KSPACE_SIZE_RULE = ("each side a power of two from 4, or a multiple of 16 of the form 2^a 3^b 5^c between 16 and 2048 "
                    "(e.g. 48, 80, 96, 144, 160, 192, 240, 288, 320, 384)")


def kspace_size_class(H, W):
    """which k-space kernels serve an H x W image (KSPACE_SIZE_RULE): KSPACE_NONE (0) no kernel -- the SENSE, single-coil
    and CG operators raise IpdmUnsupported --, KSPACE_LDS (1) whole image in LDS (H*W <= 16384), KSPACE_STRIPS (2) row /
    column strips.  Needs no GPU."""
    return int(_lib.lib.ipdm_kspace_size_class(int(H), int(W)))


def fft2c(x, inverse=False):
    x = _gpu(x, name="input")
    if x.dtype != torch.complex64:
        x = x.to(torch.complex64)
    H, W = x.shape[-2:]
    batch = x.numel() // (H * W) if H * W else 0
    out = torch.empty_like(x)
    ws_bytes = _lib.lib.ipdm_fft2c_workspace_bytes(batch, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if ws_bytes else None
    call("ipdm_fft2c_c64", _ptr(x), _ptr(out), batch, H, W, int(bool(inverse)), _ptr(ws), _stream())
    return out


def _mask_u8(mask, H, W, device):
    """host mask -> the kernels' uint8 table, by the reference's right-aligned broadcast of the mask against a
    (B, 1, H, W) stack (`mask * i2k_complex(X)`): last dim W, dim -2 either 1 (a line mask: sampled k-space columns) or H (a
    2-D mask), channel dim 1, dim -4 the number of planes T (image b uses plane b % T).
      line mask  (W,), (1, W), (1, 1, W), (T, 1, 1, W)   -> uint8 [T, W]
      2-D mask   (H, W), (1, 1, H, W), (T, 1, H, W)      -> uint8 [T, H, W]
    A shape that would not broadcast there raises ValueError; nothing is reshaped to fit."""
    m = torch.as_tensor(mask)
    if m.is_complex():
        raise TypeError(f"mask: bool, integer or real floating dtype, got {m.dtype}")
    shape = tuple(m.shape)
    if not 1 <= len(shape) <= 4:
        raise ValueError(f"mask {shape}: 1 to 4 dims, broadcastable against (B, 1, {H}, {W})")
    T, C, h, w = (1,) * (4 - len(shape)) + shape
    if w != W:
        raise ValueError(f"mask {shape}: last dim {w} != W {W}")
    if h not in (1, H):
        raise ValueError(f"mask {shape}: dim -2 is {h}; 1 (a line mask) or H = {H} (a 2-D mask)")
    if C != 1:
        raise ValueError(f"mask {shape}: channel dim {C} != 1")
    if T < 1:
        raise ValueError(f"mask {shape}: no planes")
    m = m.to(device=device).reshape((T, W) if h == 1 and H != 1 else (T, H, W))
    return (m != 0).to(torch.uint8).contiguous()


def _mask_t(mask_u8, H, W, what):
    """-> the C ABI's mask_t for a device mask: uint8 [mask_t, W] (line mask) gives mask_t, uint8 [T, H, W] (2-D mask)
    gives -T.  The kernels index the table by (b % T, r, c) through a raw pointer: dtype and shape are checked, never
    converted."""
    if not isinstance(mask_u8, torch.Tensor) or not mask_u8.is_cuda:
        raise RuntimeError(f"ipdm {what}: mask must be a GPU tensor (the HIP path has no CPU fallback)")
    if mask_u8.dtype != torch.uint8:
        raise TypeError(f"ipdm {what}: mask must be uint8 (ops._mask_u8 converts a host mask), got {mask_u8.dtype}")
    if not mask_u8.is_contiguous():
        raise ValueError(f"ipdm {what}: mask must be contiguous")
    shape = tuple(mask_u8.shape)
    if len(shape) == 2 and shape[0] >= 1 and shape[1] == W:
        return shape[0]
    if len(shape) == 3 and shape[0] >= 1 and shape[1:] == (H, W):
        return -shape[0]
    raise ValueError(f"ipdm {what}: mask {shape} is neither a line mask [mask_t, {W}] nor a 2-D mask [T, {H}, {W}]")


def _sens_entry(sens, real_name, csm_name, H, W, sets_name=None, B=None):
    """entry point for the coil maps' dtype: contiguous GPU [n, H, W], float32 (real maps) or complex64 (measured maps;
    the *_csm_* kernels).  Anything else -- float64, complex128, a strided view, a CPU tensor -- is refused, never
    converted: a complex tensor read by a real kernel is interleaved garbage.
    With sets_name the maps may also be [S, n, H, W], one set per slice (image b reads set b % S; ipdm.h): that form
    takes the *_sets_* entry point, whose extra arguments are _sens_tail(sens), and B must be a multiple of S."""
    if not isinstance(sens, torch.Tensor) or not sens.is_cuda:
        raise RuntimeError("ipdm: coil maps must be a GPU tensor (the HIP path has no CPU fallback)")
    if sens.dtype not in (torch.float32, torch.complex64):
        raise TypeError(f"ipdm: coil maps must be float32 or complex64, got {sens.dtype}")
    if not sens.is_contiguous():
        raise TypeError("ipdm: coil maps must be contiguous (call .contiguous() and keep the result)")
    if sets_name is not None and sens.dim() == 4:
        if tuple(sens.shape[-2:]) != (H, W) or sens.shape[0] < 1 or sens.shape[1] < 1:
            raise ValueError(f"ipdm: coil maps {tuple(sens.shape)} do not match [S, n_coils, {H}, {W}]")
        if B is not None and B % sens.shape[0]:
            raise ValueError(f"ipdm: a batch of {B} images is not a whole number of samples of {sens.shape[0]} map sets")
        return sets_name
    if sens.dim() != 3 or tuple(sens.shape[-2:]) != (H, W):
        raise ValueError(f"ipdm: coil maps {tuple(sens.shape)} do not match [n_coils, {H}, {W}]")
    return csm_name if sens.dtype == torch.complex64 else real_name


def _sens_tail(sens):
    """the arguments that follow `sens` in a *_sets_* entry point, (sens_complex, sens_sets); none for [n, H, W] maps"""
    return (int(sens.dtype == torch.complex64), sens.shape[0]) if sens.dim() == 4 else ()


def sense_forward(x, sens_f32, mask_u8):
    """sens_f32 None: single coil (S = 1), returns y with a leading axis of length 1; otherwise the coil maps [n, H, W]
    or [S, n, H, W] (image b reads set b % S), float32 or complex64"""
    x = _gpu(x, torch.complex64, "x")
    B = x.numel() // (x.shape[-1] * x.shape[-2])
    H, W = x.shape[-2:]
    fn = "ipdm_sense_forward_c64" if sens_f32 is None else _sens_entry(sens_f32, "ipdm_sense_forward_c64",
                                                                        "ipdm_sense_forward_csm_c64", H, W,
                                                                        "ipdm_sense_forward_sets_c64", B)
    n = 1 if sens_f32 is None else sens_f32.shape[-3]
    tail = () if sens_f32 is None else _sens_tail(sens_f32)
    y = torch.empty((n,) + tuple(x.shape), dtype=torch.complex64, device=x.device)
    mask_t = _mask_t(mask_u8, H, W, "sense_forward")
    call(fn, _ptr(x), _ptr(sens_f32), *tail, _ptr(mask_u8), mask_t, _ptr(y), B, n, H, W,
         _stream())
    return y


def sense_workspace(B, n_coils, H, W, device):
    """scratch tensor for the SENSE / single-coil operators at this size (None when the kernels need none)"""
    nbytes = _lib.lib.ipdm_sense_workspace_bytes(B, n_coils, H, W)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _check_work(work, B, n_coils, H, W, what):
    """the SENSE kernels write `work` as n_coils * B complex images: a short / foreign buffer is an out-of-bounds GPU write"""
    need = _lib.lib.ipdm_sense_workspace_bytes(B, n_coils, H, W)
    if need == 0:
        return
    if (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous()
            or work.numel() * 4 < need):
        raise ValueError(f"{what}: `work` must be a contiguous float32 GPU tensor of >= {need} bytes "
                         f"(ops.sense_workspace({B}, {n_coils}, {H}, {W}, device))")


def _large_image(H, W):
    return H * W > 16384


def sense_adjoint(s, sens_f32, mask_u8=None, apply_mask=False):
    s = _gpu(s, torch.complex64, "s")
    n = s.shape[0]
    H, W = s.shape[-2:]
    B = s[0].numel() // (H * W)
    fn = _sens_entry(sens_f32, "ipdm_sense_adjoint_c64", "ipdm_sense_adjoint_csm_c64", H, W,
                     "ipdm_sense_adjoint_sets_c64", B)
    if sens_f32.shape[-3] != n:
        raise ValueError(f"sense_adjoint: {n} coil images, {sens_f32.shape[-3]} coil maps")
    x = torch.empty(tuple(s.shape[1:]), dtype=torch.complex64, device=s.device)
    ws = sense_workspace(B, n, H, W, s.device) if _large_image(H, W) else None
    call(fn, _ptr(s), _ptr(sens_f32), *_sens_tail(sens_f32), _ptr(mask_u8),
         1 if mask_u8 is None else _mask_t(mask_u8, H, W, "sense_adjoint"), int(bool(apply_mask)), _ptr(x), _ptr(ws), B, n, H, W, _stream())
    return x


def sense_ssos(s):
    s = _gpu(s, torch.complex64, "s")
    n = s.shape[0]
    H, W = s.shape[-2:]
    B = s[0].numel() // (H * W)
    out = torch.empty(tuple(s.shape[1:]), dtype=torch.float32, device=s.device)
    ws = sense_workspace(B, n, H, W, s.device) if _large_image(H, W) else None
    call("ipdm_sense_ssos_c64", _ptr(s), _ptr(out), _ptr(ws), B, n, H, W, _stream())
    return out


def sense_l2prox(z_re, z_im, y, sens_f32, mask_u8, coef, out_re=None, out_im=None, work=None):
    z_re, z_im = _gpu(z_re, torch.float32, "z_re"), _gpu(z_im, torch.float32, "z_im")
    y = _gpu(y, torch.complex64, "y")
    H, W = z_re.shape[-2:]
    B = z_re.numel() // (H * W)
    fn = _sens_entry(sens_f32, "ipdm_sense_l2prox_f32", "ipdm_sense_l2prox_csm_f32", H, W, "ipdm_sense_l2prox_sets_f32", B)
    n = sens_f32.shape[-3]
    if y.numel() != n * B * H * W:
        raise ValueError("sense_l2prox: measurement does not match [n_coils, B, H, W]")
    out_re = torch.empty_like(z_re) if out_re is None else out_re
    out_im = torch.empty_like(z_im) if out_im is None else out_im
    work = sense_workspace(B, n, H, W, z_re.device) if work is None else work
    _check_work(work, B, n, H, W, "sense_l2prox")
    mask_t = _mask_t(mask_u8, H, W, "sense_l2prox")
    call(fn, _ptr(z_re), _ptr(z_im), _ptr(y), _ptr(sens_f32), *_sens_tail(sens_f32), _ptr(mask_u8), mask_t,
         float(coef), _ptr(out_re), _ptr(out_im), _ptr(work), B, n, H, W, _stream())
    _written(out_re, out_im)
    return out_re, out_im


def _fused_step(what, x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale, seed, sample_offset, step_id,
                dev_sched, sens=None, entries=None):
    """operand checks of a fused iteration tail, in the wrappers' order, and the 12 leading values of its C signature
    -> (fn, B, H, W, head).  entries: the (real, complex, map-sets) entry points of a SENSE step; None: single coil
    (fn None)"""
    for t, n in ((x_re, "x_re"), (x_im, "x_im"), (g_re, "g_re"), (g_im, "g_im")):
        _inplace_operand(t, torch.float32, n)
    H, W = x_re.shape[-2:]
    B = x_re.numel() // (H * W) if H * W else 0
    fn = _sens_entry(sens, entries[0], entries[1], H, W, entries[2], B) if entries else None
    _inplace_operand(y, torch.complex64, "y")
    if entries:
        for t, n in ((noise_re, "noise_re"), (noise_im, "noise_im")):
            if t is not None:
                _inplace_operand(t, torch.float32, n)
        if g_re.numel() != x_re.numel() or g_im.numel() != x_im.numel() or y.numel() != sens.shape[-3] * B * H * W:
            raise ValueError(f"{what}: operand sizes do not match the state")
    head = (_ptr(x_re), _ptr(x_im), _ptr(g_re), _ptr(g_im), _ptr(noise_re), _ptr(noise_im), float(step), float(noise_scale),
            int(seed), int(sample_offset), int(step_id), _ptr(dev_sched))
    return fn, B, H, W, head


def ald_sense_step(x_re, x_im, g_re, g_im, y, sens_f32, mask_u8, work, step=0.0, noise_scale=0.0, coef=0.0,
                   noise_re=None, noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None):
    """in place on x_re / x_im.  dev_sched: uint8/any device tensor holding an ipdm_sched_t.  sens_f32: the coil maps,
    [n, H, W] or [S, n, H, W] (image b reads set b % S), float32 or complex64."""
    fn, B, H, W, head = _fused_step("ald_sense_step", x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale, seed,
                                    sample_offset, step_id, dev_sched, sens_f32,
                                    ("ipdm_ald_sense_step_f32", "ipdm_ald_sense_step_csm_f32",
                                     "ipdm_ald_sense_step_sets_f32"))
    n = sens_f32.shape[-3]
    _check_work(work, B, n, H, W, "ald_sense_step")
    mask_t = _mask_t(mask_u8, H, W, "ald_sense_step")
    call(fn, *head, _ptr(y), _ptr(sens_f32), *_sens_tail(sens_f32), _ptr(mask_u8), mask_t, float(coef), _ptr(work), B, n,
         H, W, _stream())
    _written(x_re, x_im)


def sense_cg_workspace(B, n_coils, H, W, device):
    """scratch tensor of the conjugate-gradient proximal at this size (coil planes, r, p, A^H y, per-sample state)"""
    nbytes = _lib.lib.ipdm_sense_cg_workspace_bytes(B, n_coils, H, W)
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device) if nbytes else None


def _check_cg_scalars(max_iter, tol, what):
    """-> (max_iter, tol); checked before any tensor is looked at"""
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"{what}: max_iter must be an integer >= 1, got {max_iter}")
    tol = float(tol)
    if not (0.0 <= tol < float("inf")):
        raise ValueError(f"{what}: tol must be finite and >= 0, got {tol}")
    return int(max_iter), tol


def _check_cg_args(work, ahy, iters_out, B, n_coils, H, W, device, what):
    """-> (work, iters_out) checked: the kernels write `work` and `iters_out` through raw pointers"""
    need = _lib.lib.ipdm_sense_cg_workspace_bytes(B, n_coils, H, W)
    if work is None:
        work = sense_cg_workspace(B, n_coils, H, W, device)         # None for a size without a kernel: the call reports it
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous()
            or work.numel() * 4 < need):
        raise ValueError(f"{what}: `work` must be a contiguous float32 GPU tensor of >= {need} bytes "
                         f"(ops.sense_cg_workspace({B}, {n_coils}, {H}, {W}, device))")
    if ahy is not None:
        _inplace_operand(ahy, torch.complex64, "ahy")
        if ahy.numel() != B * H * W:
            raise ValueError(f"{what}: ahy {tuple(ahy.shape)} does not match the image batch [{B}, {H}, {W}]")
    if iters_out is None:
        iters_out = torch.zeros(B, dtype=torch.int32, device=device)
    else:
        _inplace_operand(iters_out, torch.int32, "iters_out")
        if iters_out.numel() < B:
            raise ValueError(f"{what}: iters_out holds {iters_out.numel()} < {B} entries")
    return work, iters_out


def sense_cgprox(z_re, z_im, y, sens_f32, mask_u8, a, max_iter=10, tol=1e-5, ahy=None, out_re=None, out_im=None, work=None,
                 iters_out=None):
    """exact SENSE proximal (I + a A^H A) x = z + a A^H y by conjugate gradients (ipdm.h, ipdm_sense_cgprox_f32)
    -> (out_re, out_im, iters): iters a device int32 [B], never synchronised here"""
    max_iter, tol = _check_cg_scalars(max_iter, tol, "sense_cgprox")
    z_re, z_im = _gpu(z_re, torch.float32, "z_re"), _gpu(z_im, torch.float32, "z_im")
    y = _gpu(y, torch.complex64, "y")
    H, W = z_re.shape[-2:]
    B = z_re.numel() // (H * W) if H * W else 0
    fn = _sens_entry(sens_f32, "ipdm_sense_cgprox_f32", "ipdm_sense_cgprox_csm_f32", H, W, "ipdm_sense_cgprox_sets_f32", B)
    n = sens_f32.shape[-3]
    if y.numel() != n * B * H * W:
        raise ValueError("sense_cgprox: measurement does not match [n_coils, B, H, W]")
    work, iters_out = _check_cg_args(work, ahy, iters_out, B, n, H, W, z_re.device, "sense_cgprox")
    out_re = torch.empty_like(z_re) if out_re is None else out_re
    out_im = torch.empty_like(z_im) if out_im is None else out_im
    mask_t = _mask_t(mask_u8, H, W, "sense_cgprox")
    call(fn, _ptr(z_re), _ptr(z_im), _ptr(y), _ptr(sens_f32), *_sens_tail(sens_f32), _ptr(mask_u8), mask_t, float(a), _ptr(ahy),
         max_iter, tol, _ptr(out_re), _ptr(out_im), _ptr(work), _ptr(iters_out), B, n, H, W, _stream())
    _written(out_re, out_im, iters_out)
    return out_re, out_im, iters_out


def ald_sense_cg_step(x_re, x_im, g_re, g_im, y, sens_f32, mask_u8, work, step=0.0, noise_scale=0.0, coef=0.0,
                      noise_re=None, noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None, ahy=None,
                      max_iter=10, tol=1e-5, iters_out=None):
    """ald_sense_step with the conjugate-gradient proximal; in place on x_re / x_im.  coef (dev_sched's coef field)
    carries a = alpha / lamda.  -> iters (device int32 [B])"""
    max_iter, tol = _check_cg_scalars(max_iter, tol, "ald_sense_cg_step")
    fn, B, H, W, head = _fused_step("ald_sense_cg_step", x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale, seed,
                                    sample_offset, step_id, dev_sched, sens_f32,
                                    ("ipdm_ald_sense_cg_step_f32", "ipdm_ald_sense_cg_step_csm_f32",
                                     "ipdm_ald_sense_cg_step_sets_f32"))
    nc = sens_f32.shape[-3]
    work, iters_out = _check_cg_args(work, ahy, iters_out, B, nc, H, W, x_re.device, "ald_sense_cg_step")
    mask_t = _mask_t(mask_u8, H, W, "ald_sense_cg_step")
    call(fn, *head, _ptr(y), _ptr(sens_f32), *_sens_tail(sens_f32), _ptr(mask_u8), mask_t, float(coef), _ptr(work), _ptr(ahy),
         max_iter, tol,
         _ptr(iters_out), B, nc, H, W, _stream())
    _written(x_re, x_im, iters_out)
    return iters_out


# ---- coil sensitivity maps from the calibration region (csrc/csm.hip) -----------------------------------------------
def csm_supported(n_coils, radius, H, W):
    """whether estimate_sens_maps has a kernel for this coil count (1..32), radius (1..4) and image size.  Needs no GPU."""
    return bool(_lib.lib.ipdm_csm_supported(int(n_coils), int(radius), int(H), int(W)))


def csm_workspace(B, n_coils, H, W, device):
    """scratch tensor of estimate_sens_maps (calibration images + RSS plane); None for a shape without a kernel"""
    nbytes = _lib.lib.ipdm_csm_workspace_bytes(B, n_coils, H, W)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _csm_measurement(y, what):
    """-> (n_coils, B, H, W) of a measurement (n, H, W), (n, B, H, W) or (n, B, 1, H, W): complex64, contiguous, on the GPU;
    read through a raw pointer, so never converted"""
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise RuntimeError(f"ipdm {what}: y must be a GPU tensor (the HIP path has no CPU fallback)")
    if y.dtype != torch.complex64:
        raise TypeError(f"ipdm {what}: y must be complex64, got {y.dtype}")
    if not y.is_contiguous():
        raise TypeError(f"ipdm {what}: y must be contiguous (call .contiguous() and keep the result)")
    shape = tuple(y.shape)
    if len(shape) == 3:
        return shape[0], 1, shape[1], shape[2]
    if len(shape) == 4 or (len(shape) == 5 and shape[2] == 1):
        return shape[0], shape[1], shape[-2], shape[-1]
    raise ValueError(f"ipdm {what}: y {shape} is none of (n, H, W), (n, B, H, W), (n, B, 1, H, W)")


def _csm_box(ah, aw):
    if any(isinstance(a, bool) or int(a) != a for a in (ah, aw)):
        raise ValueError(f"calibration half-widths must be integers, got ({ah}, {aw})")
    return int(ah), int(aw)


def csm_calib_images(y, ah, aw):
    """the estimator's low-resolution calibration images: ifft2c of y inside the box [H//2-ah, H//2+ah] x [W//2-aw, W//2+aw]
    under a separable raised-cosine window, zero outside it.  -> complex64 of y's shape"""
    n, B, H, W = _csm_measurement(y, "csm_calib_images")
    ah, aw = _csm_box(ah, aw)
    out = torch.empty_like(y)
    call("ipdm_csm_calib_images_c64", _ptr(y), ah, aw, _ptr(out), B, n, H, W, _stream())
    return out


def estimate_sens_maps(y, ah, aw, radius=2, power_iters=3, thresh=0.02, return_rss=False, *, out=None, work=None):
    """coil sensitivity maps from the fully sampled calibration box of multi-coil k-space y ((n, H, W), (n, B, H, W) or
    (n, B, 1, H, W) complex64; (ah, aw): SENSE's calibration_region): Walsh's adaptive estimator (ipdm.h,
    ipdm_csm_walsh_c64) -> maps of y's shape: unit RSS over the coils and coil 0 real and non-negative inside the support
    rss > thresh * rss_max, zero outside.  return_rss: -> (maps, rss (B, H, W) float32, rss_max (B,) float32) of the
    calibration images.  Asynchronous; no host synchronisation."""
    n, B, H, W = _csm_measurement(y, "estimate_sens_maps")
    ah, aw = _csm_box(ah, aw)
    if out is None:
        out = torch.empty_like(y)
    else:
        _inplace_operand(out, torch.complex64, "out")
        if out.numel() != y.numel():
            raise ValueError(f"estimate_sens_maps: out {tuple(out.shape)} does not match y {tuple(y.shape)}")
    need = _lib.lib.ipdm_csm_workspace_bytes(B, n, H, W)
    if work is None:
        work = csm_workspace(B, n, H, W, y.device)            # None for a shape without a kernel: the call reports it
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous()
            or work.numel() * 4 < need):
        raise ValueError(f"estimate_sens_maps: `work` must be a contiguous float32 GPU tensor of >= {need} bytes "
                         f"(ops.csm_workspace({B}, {n}, {H}, {W}, device))")
    rss = torch.empty((B, H, W), dtype=torch.float32, device=y.device) if return_rss else None
    rss_max = torch.empty(B, dtype=torch.float32, device=y.device)
    call("ipdm_csm_walsh_c64", _ptr(y), ah, aw, int(radius), int(power_iters), float(thresh), _ptr(out), _ptr(rss),
         _ptr(rss_max), _ptr(work), B, n, H, W, _stream())
    _written(out)
    return (out, rss, rss_max) if return_rss else out


# ---- coil compression and noise prewhitening (csrc/coilcomp.hip) ------------------------------------------------------
def coilcomp_supported(n_coils, n_virtual):
    """whether the coil-compression kernels serve n_coils (1..64) -> n_virtual (1..min(n_coils, 32)).  Needs no GPU."""
    return bool(_lib.lib.ipdm_coilcomp_supported(int(n_coils), int(n_virtual)))


def coilcomp_workspace(B, n_coils, device):
    """scratch tensor of coil_compress (the Gram matrices); None for a shape without a kernel"""
    nbytes = _lib.lib.ipdm_coilcomp_workspace_bytes(int(B), int(n_coils))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def _coilcomp_counts(n_coils, n_virtual, what):
    if isinstance(n_virtual, bool) or int(n_virtual) != n_virtual:
        raise ValueError(f"ipdm {what}: n_virtual must be an integer, got {n_virtual!r}")
    n_virtual = int(n_virtual)
    if n_virtual < 1 or n_virtual > n_coils:
        raise ValueError(f"ipdm {what}: n_virtual = {n_virtual} outside 1..n_coils = {n_coils}")
    if not coilcomp_supported(n_coils, n_virtual):
        raise _lib.IpdmUnsupported(f"ipdm {what}: {n_coils} -> {n_virtual} coils; the kernels serve 1..64 physical and "
                                   "1..32 virtual coils")
    return n_virtual


def check_noise_cov(noise_cov, n_coils, what="noise_cov"):
    """host-side check of a noise covariance: (n_coils, n_coils), real or complex, Hermitian positive definite (float64
    Cholesky) -> complex128 host tensor.  TypeError / ValueError before any launch."""
    import numpy as np
    if isinstance(noise_cov, torch.Tensor):
        noise_cov = noise_cov.detach().cpu().numpy()
    if not isinstance(noise_cov, np.ndarray):
        raise TypeError(f"{what}: a torch tensor or numpy array, got {type(noise_cov).__name__}")
    if noise_cov.dtype.kind not in "fc":
        raise TypeError(f"{what}: a real or complex floating dtype, got {noise_cov.dtype}")
    if noise_cov.ndim != 2 or noise_cov.shape != (n_coils, n_coils):
        raise ValueError(f"{what}: shape {noise_cov.shape}, expected ({n_coils}, {n_coils})")
    psi = noise_cov.astype(np.complex128)
    if not np.isfinite(psi).all():
        raise ValueError(f"{what}: not finite")
    scale = float(np.abs(psi).max())
    if not scale > 0 or float(np.abs(psi - psi.conj().T).max()) > 1e-5 * scale:
        raise ValueError(f"{what}: not Hermitian")
    psi = 0.5 * (psi + psi.conj().T)
    try:
        np.linalg.cholesky(psi)
    except np.linalg.LinAlgError:
        raise ValueError(f"{what}: not positive definite") from None
    return torch.from_numpy(psi)


def _noise_cov_dev(noise_cov, n_coils, device, what):
    if noise_cov is None:
        return None
    return check_noise_cov(noise_cov, n_coils, f"ipdm {what}: noise_cov").to(torch.complex64).to(device).contiguous()


def coil_gram(y, ah, aw, *, out=None):
    """Gram matrices of the calibration box [H//2-ah, H//2+ah] x [W//2-aw, W//2+aw] of multi-coil k-space y ((n, H, W),
    (n, B, H, W) or (n, B, 1, H, W) complex64): G_b[i][j] = sum y_i conj(y_j) -> (B, n, n) complex64, exactly Hermitian"""
    n, B, H, W = _csm_measurement(y, "coil_gram")
    ah, aw = _csm_box(ah, aw)
    if out is None:
        out = torch.empty((B, n, n), dtype=torch.complex64, device=y.device)
    else:
        _inplace_operand(out, torch.complex64, "out")
        if tuple(out.shape) != (B, n, n):
            raise ValueError(f"coil_gram: out {tuple(out.shape)}, expected {(B, n, n)}")
    call("ipdm_coil_gram_c64", _ptr(y), ah, aw, _ptr(out), B, n, H, W, _stream())
    _written(out)
    return out


def _c64_operand(t, name, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ipdm {what}: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.complex64:
        raise TypeError(f"ipdm {what}: {name} must be complex64, got {t.dtype}")
    if not t.is_contiguous():
        raise TypeError(f"ipdm {what}: {name} must be contiguous (call .contiguous() and keep the result)")
    return t


def coilcomp_matrix(gram, n_virtual, noise_cov=None, return_eig=False):
    """compression matrices from Gram matrices (B, n, n) or (n, n) complex64: with noise_cov psi = L L^H the Gram matrix
    is whitened (L^-1 G L^-H); A = U[:, :n_virtual]^H (L^-1) from its eigenvectors in descending order of the eigenvalues,
    every row turned so that its coil-0 entry is real and non-negative.  -> A (B, n_virtual, n) complex64; return_eig:
    -> (A, eig (B, n) float32 descending, status (B,) int32, 0 = fine).  noise_cov is checked on the host (TypeError /
    ValueError) before any launch."""
    _c64_operand(gram, "gram", "coilcomp_matrix")
    if gram.dim() == 2:
        gram = gram[None]
    if gram.dim() != 3 or gram.shape[1] != gram.shape[2]:
        raise ValueError(f"ipdm coilcomp_matrix: gram {tuple(gram.shape)}; (B, n, n) expected")
    B, n = gram.shape[0], gram.shape[1]
    n_virtual = _coilcomp_counts(n, n_virtual, "coilcomp_matrix")
    psi = _noise_cov_dev(noise_cov, n, gram.device, "coilcomp_matrix")
    A = torch.empty((B, n_virtual, n), dtype=torch.complex64, device=gram.device)
    eig = torch.empty((B, n), dtype=torch.float32, device=gram.device)
    status = torch.empty(B, dtype=torch.int32, device=gram.device)
    call("ipdm_coilcomp_matrix_c64", _ptr(gram), _ptr(psi), n_virtual, _ptr(A), _ptr(eig), _ptr(status), B, n, _stream())
    return (A, eig, status) if return_eig else A


def _coil_planes(y, what):
    """-> (n, B, P): y (n, B, ...) complex64 with any trailing pixel dims"""
    _c64_operand(y, "y", what)
    if y.dim() < 3:
        raise ValueError(f"ipdm {what}: y {tuple(y.shape)}; (n_coils, B, pixels...) expected")
    n, B = y.shape[0], y.shape[1]
    return n, B, (y.numel() // (n * B) if n * B else 0)


def coil_apply(y, A, out=None):
    """y'_v = sum_c A[v][c] y_c on every pixel: y (n, B, ...) complex64 (k-space, or coil maps (n, 1, H, W)), A
    (B, nv, n) per image or (nv, n) shared by the batch, complex64 -> (nv, B, ...) complex64.  out may not overlap y."""
    n, B, Pn = _coil_planes(y, "coil_apply")
    _c64_operand(A, "A", "coil_apply")
    if A.dim() not in (2, 3) or A.shape[-1] != n or (A.dim() == 3 and A.shape[0] != B):
        raise ValueError(f"ipdm coil_apply: A {tuple(A.shape)} does not match y {tuple(y.shape)}; (B, nv, n) or (nv, n) expected")
    nv = _coilcomp_counts(n, A.shape[-2], "coil_apply")
    shape = (nv,) + tuple(y.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.complex64, device=y.device)
    else:
        _c64_operand(out, "out", "coil_apply")
        if tuple(out.shape) != shape:
            raise ValueError(f"ipdm coil_apply: out {tuple(out.shape)}, expected {shape}")
    call("ipdm_coil_apply_c64", _ptr(y), _ptr(A), int(A.dim() == 3), _ptr(out), B, n, nv, Pn, _stream())
    _written(out)
    return out


def coil_compress(y, ah, aw, n_virtual, noise_cov=None, return_matrix=False, *, work=None):
    """whitening and compression of multi-coil k-space y ((n, H, W), (n, B, H, W) or (n, B, 1, H, W) complex64) to
    n_virtual virtual coils by PCA of its calibration box (ah, aw): Gram matrix, matrix and application in one call
    (ipdm.h, ipdm_coil_compress_c64) -> y' of y's shape with n_virtual coils; return_matrix: -> (y', A (B, n_virtual, n),
    eig (B, n), status (B,)).  Asynchronous; no host synchronisation."""
    n, B, H, W = _csm_measurement(y, "coil_compress")
    ah, aw = _csm_box(ah, aw)
    n_virtual = _coilcomp_counts(n, n_virtual, "coil_compress")
    psi = _noise_cov_dev(noise_cov, n, y.device, "coil_compress")
    need = _lib.lib.ipdm_coilcomp_workspace_bytes(B, n)
    if work is None:
        work = coilcomp_workspace(B, n, y.device)
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous()
            or work.numel() * 4 < need):
        raise ValueError(f"coil_compress: `work` must be a contiguous float32 GPU tensor of >= {need} bytes "
                         f"(ops.coilcomp_workspace({B}, {n}, device))")
    out = torch.empty((n_virtual,) + tuple(y.shape[1:]), dtype=torch.complex64, device=y.device)
    A = torch.empty((B, n_virtual, n), dtype=torch.complex64, device=y.device)
    eig = torch.empty((B, n), dtype=torch.float32, device=y.device)
    status = torch.empty(B, dtype=torch.int32, device=y.device)
    call("ipdm_coil_compress_c64", _ptr(y), ah, aw, n_virtual, _ptr(psi), _ptr(A), _ptr(eig), _ptr(status), _ptr(out), _ptr(work),
         B, n, H, W, _stream())
    return (out, A, eig, status) if return_matrix else out


# ---- geometric coil compression along the readout (csrc/gcc.hip) -------------------------------------------------------
GCC_MAX_WINDOW = 8


def gcc_supported(n_coils, n_virtual, H, W, win=2):
    """whether coil_compress_geometric has kernels for n_coils (1..64) -> n_virtual (1..min(n_coils, 32)), a readout side
    H (a power of two from 4 or a multiple of 16 of the form 2^a 3^b 5^c, at most 2048), W >= 1 and a window half-width
    0..8.  Needs no GPU."""
    return bool(_lib.lib.ipdm_gcc_supported(int(n_coils), int(n_virtual), int(H), int(W), int(win)))


def gcc_workspace(B, n_coils, n_virtual, H, W, device):
    """scratch tensor of coil_compress_geometric (hybrid data, Gram matrices, unaligned matrices); None when unserved"""
    nbytes = _lib.lib.ipdm_gcc_workspace_bytes(int(B), int(n_coils), int(n_virtual), int(H), int(W))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device) if nbytes else None


def gcc_window(win, what="gcc"):
    """host check of the window half-width: an integer 0..8"""
    if isinstance(win, bool) or not isinstance(win, (int, float)) or int(win) != win or not 0 <= win <= GCC_MAX_WINDOW:
        raise ValueError(f"ipdm {what}: window = {win!r} outside 0..{GCC_MAX_WINDOW} (readout positions on either side)")
    return int(win)


def gcc_check(n_coils, n_virtual, H, W, aw, win, what="gcc"):
    """host checks of a geometric compression, before any launch -> (n_virtual, win).  ValueError: a window outside 0..8, or
    one that holds fewer samples than virtual coils; IpdmUnsupported: coil counts or a readout side without a kernel."""
    win = gcc_window(win, what)
    n_virtual = _coilcomp_counts(n_coils, n_virtual, what)
    samples = (2 * win + 1) * (2 * int(aw) + 1)
    if samples < n_virtual:
        raise ValueError(f"ipdm {what}: the window holds {samples} samples per readout position ((2*{win}+1) rows x "
                         f"(2*{int(aw)}+1) calibration columns), fewer than the {n_virtual} virtual coils")
    if not gcc_supported(n_coils, n_virtual, H, W, win):
        raise _lib.IpdmUnsupported(f"ipdm {what}: no readout transform for H = {H}; {KSPACE_SIZE_RULE}")
    return n_virtual, win


def readout_fft(x, inverse=False, out=None):
    """centred orthonormal DFT (inverse=True: inverse DFT) along H of x (..., H, W) complex64, with fft2c's centring: the
    inverse transform of k-space along its fully sampled readout axis is the hybrid space whose row x is image row x.
    out may be x itself."""
    _c64_operand(x, "x", "readout_fft")
    if x.dim() < 2:
        raise ValueError(f"ipdm readout_fft: x {tuple(x.shape)}; (..., H, W) expected")
    H, W = x.shape[-2:]
    if out is None:
        out = torch.empty_like(x)
    else:
        _c64_operand(out, "out", "readout_fft")
        if tuple(out.shape) != tuple(x.shape):
            raise ValueError(f"ipdm readout_fft: out {tuple(out.shape)}, expected {tuple(x.shape)}")
    planes = x.numel() // (H * W) if H * W else 0
    call("ipdm_readout_fft_c64", _ptr(x), _ptr(out), int(bool(inverse)), planes, H, W, _stream())
    _written(out)
    return out


def gcc_gram(h, aw, win=2):
    """windowed Gram matrices of hybrid-space data h ((n, H, W) or (n, B, H, W) complex64): G_{b,x}[i][j] = sum over the
    rows [x-win, x+win] (clipped at the edges) and the columns [W//2-aw, W//2+aw] of h_i conj(h_j) -> (B, H, n, n)
    complex64, exactly Hermitian"""
    n, B, H, W = _csm_measurement(h, "gcc_gram")
    aw = _csm_box(0, aw)[1]
    win = gcc_window(win, "gcc_gram")
    out = torch.empty((B, H, n, n), dtype=torch.complex64, device=h.device)
    call("ipdm_gcc_gram_c64", _ptr(h), aw, win, _ptr(out), B, n, H, W, _stream())
    return out


def gcc_align(A, noise_cov=None, return_status=False):
    """alignment of per-position compression matrices A (B, H, nv, n) or (H, nv, n) complex64 along H: the centre row
    H // 2 is kept, every other position is turned onto its neighbour on the centre side by the unitary polar factor of
    A_x psi A_p^H (ipdm.h, ipdm_gcc_align_c64) -> the aligned matrices of A's shape; return_status: -> (A, status (B,)
    int32, the count of degenerate positions per image).  noise_cov is checked on the host before any launch."""
    _c64_operand(A, "A", "gcc_align")
    if A.dim() not in (3, 4):
        raise ValueError(f"ipdm gcc_align: A {tuple(A.shape)}; (B, H, nv, n) or (H, nv, n) expected")
    B = A.shape[0] if A.dim() == 4 else 1
    H, nv, n = A.shape[-3:]
    _coilcomp_counts(n, nv, "gcc_align")
    psi = _noise_cov_dev(noise_cov, n, A.device, "gcc_align")
    out = torch.empty_like(A)
    status = torch.empty(B, dtype=torch.int32, device=A.device)
    work = torch.empty(2 * B, dtype=torch.int32, device=A.device)
    call("ipdm_gcc_align_c64", _ptr(A), _ptr(psi), _ptr(out), _ptr(status), _ptr(work), B, H, n, nv, _stream())
    return (out, status) if return_status else out


def coil_apply_rows(y, A, out=None):
    """y'_v(x, c) = sum_k A[x][v][k] y_k(x, c), one matrix per row: y (n, H, W) or (n, B, H, W) complex64 (hybrid-space data,
    or coil maps in image space), A (B, H, nv, n) per image or (H, nv, n) shared by the batch -> (nv,) + y.shape[1:].
    out may not overlap y."""
    n, B, H, W = _csm_measurement(y, "coil_apply_rows")
    _c64_operand(A, "A", "coil_apply_rows")
    if A.dim() not in (3, 4) or A.shape[-1] != n or A.shape[-3] != H or (A.dim() == 4 and A.shape[0] != B):
        raise ValueError(f"ipdm coil_apply_rows: A {tuple(A.shape)} does not match y {tuple(y.shape)}; (B, H, nv, n) or "
                         "(H, nv, n) expected")
    nv = _coilcomp_counts(n, A.shape[-2], "coil_apply_rows")
    shape = (nv,) + tuple(y.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.complex64, device=y.device)
    else:
        _c64_operand(out, "out", "coil_apply_rows")
        if tuple(out.shape) != shape:
            raise ValueError(f"ipdm coil_apply_rows: out {tuple(out.shape)}, expected {shape}")
    call("ipdm_coil_apply_rows_c64", _ptr(y), _ptr(A), int(A.dim() == 4), _ptr(out), B, n, nv, H, W, _stream())
    _written(out)
    return out


def coil_compress_geometric(y, aw, n_virtual, win=2, noise_cov=None, return_matrix=False, *, work=None):
    """geometric coil compression of multi-coil k-space y ((n, H, W), (n, B, H, W) or (n, B, 1, H, W) complex64) whose
    axis H is fully sampled: one matrix per readout position from the calibration columns [W//2-aw, W//2+aw] and the rows
    [x-win, x+win] of the hybrid space, aligned along x (ipdm.h, ipdm_gcc_compress_c64) -> y' of y's shape with n_virtual
    coils; return_matrix: -> (y', A (B, H, n_virtual, n), eig (B, H, n), status (B,)).  Asynchronous; no host
    synchronisation."""
    n, B, H, W = _csm_measurement(y, "coil_compress_geometric")
    aw = _csm_box(0, aw)[1]
    n_virtual, win = gcc_check(n, n_virtual, H, W, aw, win, "coil_compress_geometric")
    psi = _noise_cov_dev(noise_cov, n, y.device, "coil_compress_geometric")
    need = _lib.lib.ipdm_gcc_workspace_bytes(B, n, n_virtual, H, W)
    if work is None:
        work = gcc_workspace(B, n, n_virtual, H, W, y.device)
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous()
            or work.numel() * 4 < need):
        raise ValueError(f"coil_compress_geometric: `work` must be a contiguous float32 GPU tensor of >= {need} bytes "
                         f"(ops.gcc_workspace({B}, {n}, {n_virtual}, {H}, {W}, device))")
    out = torch.empty((n_virtual,) + tuple(y.shape[1:]), dtype=torch.complex64, device=y.device)
    A = torch.empty((B, H, n_virtual, n), dtype=torch.complex64, device=y.device)
    eig = torch.empty((B, H, n), dtype=torch.float32, device=y.device)
    status = torch.empty(B, dtype=torch.int32, device=y.device)
    call("ipdm_gcc_compress_c64", _ptr(y), aw, win, n_virtual, _ptr(psi), _ptr(A), _ptr(eig), _ptr(status), _ptr(out),
         _ptr(work), B, n, H, W, _stream())
    return (out, A, eig, status) if return_matrix else out


# ---- ESPIRiT coil sensitivity maps from the calibration region (csrc/espirit.hip) ------------------------------------------
ESPIRIT_MAX_COILS, ESPIRIT_MAX_COLUMNS = 16, 432


def espirit_supported(n_coils, ksize, H, W):
    """whether espirit_maps has kernels for this coil count (1..16), kernel side (3..8, n_coils ksize^2 <= 432) and image
    size (every H, W up to 1024).  Needs no GPU."""
    return bool(_lib.lib.ipdm_espirit_supported(int(n_coils), int(ksize), int(H), int(W)))


def espirit_workspace(B, n_coils, ksize, device):
    """scratch tensor of espirit_kernels / espirit_maps (Gram matrix and eigenvectors, double); None without a kernel"""
    nbytes = _lib.lib.ipdm_espirit_workspace_bytes(int(B), int(n_coils), int(ksize))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device) if nbytes else None


def espirit_check(n_coils, ksize, ah, aw, H, W, what="espirit"):
    """host-side check of an ESPIRiT request, before any launch: ValueError for a calibration box with a side below ksize,
    IpdmUnsupported (naming n_virtual as the way out) for more coils or kernel columns than the kernels serve"""
    if isinstance(ksize, bool) or int(ksize) != ksize:
        raise ValueError(f"ipdm {what}: ksize must be an integer, got {ksize!r}")
    ksize = int(ksize)
    if ksize < 3 or ksize > 8:
        raise _lib.IpdmUnsupported(f"ipdm {what}: ksize = {ksize}; the kernels serve 3..8")
    if n_coils > ESPIRIT_MAX_COILS or n_coils * ksize * ksize > ESPIRIT_MAX_COLUMNS:
        raise _lib.IpdmUnsupported(f"ipdm {what}: {n_coils} coils with ksize = {ksize} make {n_coils * ksize * ksize} kernel "
                                   f"columns; the kernels serve up to {ESPIRIT_MAX_COILS} coils and n_coils ksize^2 <= "
                                   f"{ESPIRIT_MAX_COLUMNS}: compress the measurement first (n_virtual= / coil_compress=)")
    if 2 * ah + 1 < ksize or 2 * aw + 1 < ksize:
        raise ValueError(f"ipdm {what}: the calibration box {2 * ah + 1} x {2 * aw + 1} is smaller than ksize = {ksize}")
    if not espirit_supported(n_coils, ksize, H, W):
        raise _lib.IpdmUnsupported(f"ipdm {what}: no kernel for {n_coils} coils, ksize {ksize}, {H} x {W}")
    return ksize


def espirit_gram(y, ah, aw, ksize=6):
    """Gram matrix of the ESPIRiT calibration matrix of multi-coil k-space y ((n, H, W), (n, B, H, W) or (n, B, 1, H, W)
    complex64): every ksize x ksize patch of the box, columns in the order (coil, ty, tx) -> (B, M, M) complex128,
    M = n ksize^2, summed in double, exactly Hermitian"""
    n, B, H, W = _csm_measurement(y, "espirit_gram")
    ah, aw = _csm_box(ah, aw)
    M = n * int(ksize) ** 2
    out = torch.empty((B, M, M), dtype=torch.complex128, device=y.device)
    call("ipdm_espirit_gram_c64", _ptr(y), ah, aw, int(ksize), _ptr(out), B, n, H, W, _stream())
    return out


def _espirit_work(work, B, n, ksize, device, what):
    need = _lib.lib.ipdm_espirit_workspace_bytes(B, n, int(ksize))
    if work is None:
        return espirit_workspace(B, n, ksize, device)         # None for a shape without a kernel: the call reports it
    if (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float64 or not work.is_contiguous()
            or work.numel() * 8 < need):
        raise ValueError(f"{what}: `work` must be a contiguous float64 GPU tensor of >= {need} bytes "
                         f"(ops.espirit_workspace({B}, {n}, {ksize}, device))")
    return work


def espirit_kernels(y, ah, aw, ksize=6, sv_thresh=0.02, return_sweeps=False, *, work=None):
    """row space of the calibration matrix and its kernel correlation (ipdm.h, ipdm_espirit_kernels_c64) -> (K (B, n, n,
    2 ksize - 1, 2 ksize - 1) complex64, lam (B, M) float64 descending, rank (B,) int32, status (B,) int32: 0 = fine);
    return_sweeps: -> (..., sweeps (B,) int32, the Jacobi sweeps made).  Asynchronous; the rank is decided on the device."""
    n, B, H, W = _csm_measurement(y, "espirit_kernels")
    ah, aw = _csm_box(ah, aw)
    ksize = int(ksize)
    work = _espirit_work(work, B, n, ksize, y.device, "espirit_kernels")
    side = 2 * ksize - 1
    K = torch.empty((B, n, n, side, side), dtype=torch.complex64, device=y.device)
    lam = torch.empty((B, n * ksize * ksize), dtype=torch.float64, device=y.device)
    rank = torch.empty(B, dtype=torch.int32, device=y.device)
    status = torch.empty(B, dtype=torch.int32, device=y.device)
    sweeps = torch.empty(B, dtype=torch.int32, device=y.device)
    call("ipdm_espirit_kernels_c64", _ptr(y), ah, aw, ksize, float(sv_thresh), _ptr(K), _ptr(lam), _ptr(rank), _ptr(status),
         _ptr(sweeps), _ptr(work), B, n, H, W, _stream())
    return (K, lam, rank, status, sweeps) if return_sweeps else (K, lam, rank, status)


def espirit_pixel(K, H, W, crop=0.8, power_iters=30, status=None, shape=None):
    """the per-pixel stage alone: K (B, n, n, 2k-1, 2k-1) complex64 -> (maps (n, B, H, W) complex64 (or `shape`), eigval
    (B, H, W) float32)"""
    _c64_operand(K, "K", "espirit_pixel")
    if K.dim() != 5 or K.shape[1] != K.shape[2] or K.shape[3] != K.shape[4] or K.shape[3] % 2 == 0:
        raise ValueError(f"ipdm espirit_pixel: K {tuple(K.shape)}; (B, n, n, 2k-1, 2k-1) expected")
    B, n, ksize = K.shape[0], K.shape[1], (K.shape[3] + 1) // 2
    if status is not None:
        _inplace_operand(status, torch.int32, "status")
    maps = torch.empty(shape if shape is not None else (n, B, H, W), dtype=torch.complex64, device=K.device)
    eigval = torch.empty((B, H, W), dtype=torch.float32, device=K.device)
    call("ipdm_espirit_pixel_c64", _ptr(K), _ptr(status), ksize, float(crop), int(power_iters), _ptr(maps), _ptr(eigval), B, n,
         int(H), int(W), _stream())
    return maps, eigval


def espirit_maps(y, ah, aw, ksize=6, sv_thresh=0.02, crop=0.8, power_iters=30, return_eig=False, *, work=None):
    """ESPIRiT coil sensitivity maps from the fully sampled calibration box of multi-coil k-space y ((n, H, W), (n, B, H, W)
    or (n, B, 1, H, W) complex64; (ah, aw): SENSE's calibration_region), one map set (ipdm.h, ipdm_espirit_c64) -> maps of
    y's shape: unit norm over the coils and coil 0 real and non-negative where the eigenvalue of G(x) exceeds crop, exactly
    zero elsewhere.  return_eig: -> (maps, eigval (B, H, W) float32, rank (B,) int32, status (B,) int32; a non-zero status
    marks an image whose decomposition failed: its maps are zeros).  Every H, W up to 1024 (the pixel stage is a direct DFT
    of the kernel taps).  Asynchronous; no host synchronisation."""
    n, B, H, W = _csm_measurement(y, "espirit_maps")
    ah, aw = _csm_box(ah, aw)
    ksize = int(ksize)
    work = _espirit_work(work, B, n, ksize, y.device, "espirit_maps")
    side = 2 * ksize - 1
    maps = torch.empty_like(y)
    eigval = torch.empty((B, H, W), dtype=torch.float32, device=y.device)
    K = torch.empty((B, n, n, side, side), dtype=torch.complex64, device=y.device)
    lam = torch.empty((B, n * ksize * ksize), dtype=torch.float64, device=y.device)
    rank = torch.empty(B, dtype=torch.int32, device=y.device)
    status = torch.empty(B, dtype=torch.int32, device=y.device)
    call("ipdm_espirit_c64", _ptr(y), ah, aw, ksize, float(sv_thresh), float(crop), int(power_iters), _ptr(maps), _ptr(eigval),
         _ptr(K), _ptr(lam), _ptr(rank), _ptr(status), _ptr(work), B, n, H, W, _stream())
    return (maps, eigval, rank, status) if return_eig else maps


# ---- mask-weighted time average of 2D+time k-space (csrc/kspace_tavg.hip) ------------------------------------------------
TAVG_MAX_FRAMES = 4096


def _cine_measurement(y, what):
    """-> (n_coils, B, T, H, W, batched) of a cine measurement (n, T, H, W), (n, B, T, H, W) or (n, B, T, 1, H, W):
    complex64, contiguous, on the GPU; read through a raw pointer, so never converted"""
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise RuntimeError(f"ipdm {what}: y must be a GPU tensor (the HIP path has no CPU fallback)")
    if y.dtype != torch.complex64:
        raise TypeError(f"ipdm {what}: y must be complex64, got {y.dtype}")
    if not y.is_contiguous():
        raise TypeError(f"ipdm {what}: y must be contiguous (call .contiguous() and keep the result)")
    shape = tuple(y.shape)
    if len(shape) == 4:
        return shape[0], 1, shape[1], shape[2], shape[3], False
    if len(shape) == 5 or (len(shape) == 6 and shape[3] == 1):
        return shape[0], shape[1], shape[2], shape[-2], shape[-1], True
    raise ValueError(f"ipdm {what}: y {shape} is none of (n, T, H, W), (n, B, T, H, W), (n, B, T, 1, H, W)")


def kspace_time_average(y, mask_u8, return_count=False, *, out=None):
    """the time-averaged composite of a cine measurement y ((n, T, H, W), (n, B, T, H, W) or (n, B, T, 1, H, W) complex64)
    under its per-frame sampling mask (a device table of ops._mask_u8; frame t of image b uses plane (b*T + t) % planes, as
    the SENSE operators on the flattened (B*T) stack): ybar = (sum of y over the frames that sampled the pixel) / count,
    exactly 0 where no frame did; y is read at sampled positions only (ipdm.h, ipdm_kspace_tavg_c64).  -> ybar with T
    dropped, (n, H, W) or (n, B, H, W) complex64; return_count: -> (ybar, count (B, H, W) int32).  Asynchronous; no host
    synchronisation."""
    n, B, T, H, W, batched = _cine_measurement(y, "kspace_time_average")
    mask_t = _mask_t(mask_u8, H, W, "kspace_time_average")
    if min(n, T, H, W) < 1:
        raise ValueError(f"ipdm kspace_time_average: y {tuple(y.shape)} has an empty dimension")
    if T > TAVG_MAX_FRAMES:
        raise _lib.IpdmUnsupported(f"ipdm kspace_time_average: T = {T} frames; the kernel serves 1..{TAVG_MAX_FRAMES}")
    shape = (n, B, H, W) if batched else (n, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.complex64, device=y.device)
    else:
        _c64_operand(out, "out", "kspace_time_average")
        if tuple(out.shape) != shape:
            raise ValueError(f"ipdm kspace_time_average: out {tuple(out.shape)}, expected {shape}")
    count = torch.empty((B, H, W), dtype=torch.int32, device=y.device) if return_count else None
    call("ipdm_kspace_tavg_c64", _ptr(y), _ptr(mask_u8), mask_t, _ptr(out), _ptr(count), B, T, n, H, W, _stream())
    _written(out)
    return (out, count) if return_count else out


SC_L2PENALTY, SC_CLOSED_FORM, SC_PROJECTION = 0, 1, 2


def singlecoil_prox(z_re, z_im, y, mask_u8, coef, mode, out_re=None, out_im=None, work=None):
    """single-coil data consistency on planar real / imaginary planes (modes: ipdm.h, ipdm_singlecoil_prox_f32)"""
    z_re, z_im = _gpu(z_re, torch.float32, "z_re"), _gpu(z_im, torch.float32, "z_im")
    y = _gpu(y, torch.complex64, "y")
    H, W = z_re.shape[-2:]
    B = z_re.numel() // (H * W)
    if y.numel() != B * H * W:
        raise ValueError(f"singlecoil_prox: measurement {tuple(y.shape)} does not match the image batch {tuple(z_re.shape)}")
    out_re = torch.empty_like(z_re) if out_re is None else out_re
    out_im = torch.empty_like(z_im) if out_im is None else out_im
    if work is None and _large_image(H, W):
        work = sense_workspace(B, 1, H, W, z_re.device)
    if work is not None or _large_image(H, W):
        _check_work(work, B, 1, H, W, "singlecoil_prox")
    mask_t = _mask_t(mask_u8, H, W, "singlecoil_prox")
    call("ipdm_singlecoil_prox_f32", _ptr(z_re), _ptr(z_im), _ptr(y), _ptr(mask_u8), mask_t, float(coef),
         int(mode), _ptr(out_re), _ptr(out_im), _ptr(work), B, H, W, _stream())
    _written(out_re, out_im)
    return out_re, out_im


def ald_singlecoil_step(x_re, x_im, g_re, g_im, y, mask_u8, mode, step=0.0, noise_scale=0.0, coef=0.0, noise_re=None,
                        noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None, work=None):
    """in place on x_re / x_im (contiguous float32 GPU planes)"""
    _, B, H, W, head = _fused_step("ald_singlecoil_step", x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale,
                                   seed, sample_offset, step_id, dev_sched)
    if work is None and _large_image(H, W):
        work = sense_workspace(B, 1, H, W, x_re.device)
    if work is not None or _large_image(H, W):
        _check_work(work, B, 1, H, W, "ald_singlecoil_step")
    mask_t = _mask_t(mask_u8, H, W, "ald_singlecoil_step")
    call("ipdm_ald_singlecoil_step_f32", *head, _ptr(y), _ptr(mask_u8), mask_t, float(coef), int(mode), _ptr(work), B, H, W,
         _stream())
    _written(x_re, x_im)


def langevin_step(x, g, step=0.0, noise_scale=0.0, noise=None, seed=0, sample_offset=0, step_id=0, dev_sched=None):
    """x += step*g + noise_scale*noise in place; x [n_samples, ...]."""
    _inplace_operand(x, torch.float32, "x")
    _inplace_operand(g, torch.float32, "g")
    if noise is not None:
        _inplace_operand(noise, torch.float32, "noise")
        if noise.numel() != x.numel():
            raise ValueError("langevin_step: noise does not match x")
    if g.numel() != x.numel():
        raise ValueError("langevin_step: g does not match x")
    n_samples = x.shape[0]
    call("ipdm_langevin_step_f32", _ptr(x), _ptr(g), _ptr(noise), float(step), float(noise_scale), int(seed),
         int(sample_offset), int(step_id), _ptr(dev_sched), n_samples, x.numel() // max(n_samples, 1), _stream())
    _written(x)
    return x


def philox_normal(shape, device, seed=0, sample_offset=0, step_id=0, plane=0):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    n_samples = shape[0]
    call("ipdm_philox_normal_f32", _ptr(out), int(seed), int(sample_offset), int(step_id), int(plane), n_samples,
         out.numel() // max(n_samples, 1), _stream())
    return out


# ---- predictor-corrector sampling with data consistency: one schedule record per sample (ipdm.h) ---------------------
SCHED_BYTES = 32                                 # sizeof(ipdm_sched_t)


def _sched_records(t, n, name, what):
    """a device tensor holding at least n ipdm_sched_t records (the kernels read / write it through a raw pointer)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ipdm: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    if t.numel() * t.element_size() < n * SCHED_BYTES:
        raise ValueError(f"{what}: {name} holds {t.numel() * t.element_size()} bytes < {n} records of {SCHED_BYTES} bytes")
    if t.data_ptr() % 8:
        raise ValueError(f"{what}: {name} must be 8-byte aligned")
    return t


def pc_langevin_coef(g_re, g_im, sample_sched, snr, alpha=1.0, noise_re=None, noise_im=None, seed=0, sample_offset=0,
                     step_id=0, dev_sched=None, coef=0.0, sigma=0.0, work=None):
    """Langevin-corrector step of every complex sample, on the device (ipdm.h, ipdm_pc_langevin_coef_f32): record b of
    sample_sched receives step = 2 alpha (snr |z_b| / |g_b|)^2 and noise_scale = sqrt(2 step), z the injected noise or
    (noise None) the Philox normals the following per-sample tail will draw with the same (seed, sample_offset,
    step_id); coef, sigma and step_id come from the device record dev_sched when given.  g_re / g_im: [B, ...]."""
    for t, n in ((g_re, "g_re"), (g_im, "g_im")):
        _inplace_operand(t, torch.float32, n)
    if (noise_re is None) != (noise_im is None):
        raise ValueError("pc_langevin_coef: noise_re and noise_im come together")
    B = g_re.shape[0] if g_re.dim() else 0
    elems = g_re.numel() // max(B, 1)
    if g_im.numel() != g_re.numel() or B < 1 or elems < 1:
        raise ValueError("pc_langevin_coef: g_re / g_im must be two equal non-empty [B, ...] planes")
    if B > 65535:
        raise ValueError(f"pc_langevin_coef: {B} samples exceed the 65535 of one launch")
    for t, n in ((noise_re, "noise_re"), (noise_im, "noise_im")):
        if t is not None:
            _inplace_operand(t, torch.float32, n)
            if t.numel() != g_re.numel():
                raise ValueError(f"pc_langevin_coef: {n} does not match the score")
    _sched_records(sample_sched, B, "sample_sched", "pc_langevin_coef")
    if dev_sched is not None:
        _sched_records(dev_sched, 1, "dev_sched", "pc_langevin_coef")
    snr, alpha = float(snr), float(alpha)
    if not (snr >= 0.0 and alpha >= 0.0 and snr < float("inf") and alpha < float("inf")):
        raise ValueError(f"pc_langevin_coef: snr and alpha must be finite and >= 0, got {snr}, {alpha}")
    need = _lib.lib.ipdm_pc_langevin_coef_workspace_bytes(B)
    if work is None:
        work = torch.empty(need // 8, dtype=torch.float64, device=g_re.device)
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float64 or not work.is_contiguous()
            or work.numel() * 8 < need):
        raise ValueError(f"pc_langevin_coef: `work` must be a contiguous float64 GPU tensor of >= {need} bytes")
    call("ipdm_pc_langevin_coef_f32", _ptr(g_re), _ptr(g_im), _ptr(noise_re), _ptr(noise_im), snr, alpha, int(seed),
         int(sample_offset), int(step_id), _ptr(dev_sched), float(coef), float(sigma), _ptr(sample_sched), _ptr(work), B, elems,
         _stream())
    _written(sample_sched)
    return sample_sched


def pc_langevin_coef_workspace(B, device):
    return torch.empty(_lib.lib.ipdm_pc_langevin_coef_workspace_bytes(B) // 8, dtype=torch.float64, device=device)


def _pc_head(what, head, B, dev_sched, sample_sched):
    """the leading C arguments of a per-sample tail: _fused_step's head with (records, stride) in place of dev_sched.
    sample_sched given: sample b reads record b; otherwise dev_sched (or the host scalars) serves every sample"""
    if sample_sched is not None:
        if dev_sched is not None:
            raise ValueError(f"{what}: pass sample_sched (a record per sample) or dev_sched (one shared record), not both")
        _sched_records(sample_sched, B, "sample_sched", what)
        return head[:-1] + (_ptr(sample_sched), 1)
    if dev_sched is not None:
        _sched_records(dev_sched, 1, "dev_sched", what)
    return head + (0,)


def _pc_sens_tail(sens):
    return (int(sens.dtype == torch.complex64), sens.shape[0] if sens.dim() == 4 else 1)


def pc_sense_step(x_re, x_im, g_re, g_im, y, sens_f32, mask_u8, work, step=0.0, noise_scale=0.0, coef=0.0, noise_re=None,
                  noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None, sample_sched=None):
    """ald_sense_step with a schedule record per sample: sample b takes step, noise_scale, coef and step_id from record b
    of sample_sched (ipdm_sched_t[B] on the device, e.g. written by pc_langevin_coef).  sample_sched None: dev_sched or
    the scalars, ald_sense_step's bits.  In place on x_re / x_im."""
    name = "ipdm_pc_sense_step_f32"
    fn, B, H, W, head = _fused_step("pc_sense_step", x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale, seed,
                                    sample_offset, step_id, dev_sched, sens_f32, (name, name, name))
    head = _pc_head("pc_sense_step", head, B, dev_sched, sample_sched)
    n = sens_f32.shape[-3]
    _check_work(work, B, n, H, W, "pc_sense_step")
    mask_t = _mask_t(mask_u8, H, W, "pc_sense_step")
    call(fn, *head, _ptr(y), _ptr(sens_f32), *_pc_sens_tail(sens_f32), _ptr(mask_u8), mask_t, float(coef), _ptr(work), B, n,
         H, W, _stream())
    _written(x_re, x_im)


def pc_sense_cg_step(x_re, x_im, g_re, g_im, y, sens_f32, mask_u8, work, step=0.0, noise_scale=0.0, coef=0.0, noise_re=None,
                     noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None, sample_sched=None, ahy=None,
                     max_iter=10, tol=1e-5, iters_out=None):
    """ald_sense_cg_step with a schedule record per sample (pc_sense_step).  -> iters (device int32 [B])"""
    max_iter, tol = _check_cg_scalars(max_iter, tol, "pc_sense_cg_step")
    name = "ipdm_pc_sense_cg_step_f32"
    fn, B, H, W, head = _fused_step("pc_sense_cg_step", x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale, seed,
                                    sample_offset, step_id, dev_sched, sens_f32, (name, name, name))
    head = _pc_head("pc_sense_cg_step", head, B, dev_sched, sample_sched)
    nc = sens_f32.shape[-3]
    work, iters_out = _check_cg_args(work, ahy, iters_out, B, nc, H, W, x_re.device, "pc_sense_cg_step")
    mask_t = _mask_t(mask_u8, H, W, "pc_sense_cg_step")
    call(fn, *head, _ptr(y), _ptr(sens_f32), *_pc_sens_tail(sens_f32), _ptr(mask_u8), mask_t, float(coef), _ptr(work),
         _ptr(ahy), max_iter, tol, _ptr(iters_out), B, nc, H, W, _stream())
    _written(x_re, x_im, iters_out)
    return iters_out


def pc_singlecoil_step(x_re, x_im, g_re, g_im, y, mask_u8, mode, step=0.0, noise_scale=0.0, coef=0.0, noise_re=None,
                       noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None, sample_sched=None, work=None):
    """ald_singlecoil_step with a schedule record per sample (pc_sense_step); in place on x_re / x_im"""
    _, B, H, W, head = _fused_step("pc_singlecoil_step", x_re, x_im, g_re, g_im, y, noise_re, noise_im, step, noise_scale,
                                   seed, sample_offset, step_id, dev_sched)
    for t, n in ((noise_re, "noise_re"), (noise_im, "noise_im")):
        if t is not None:
            _inplace_operand(t, torch.float32, n)
    if g_re.numel() != x_re.numel() or g_im.numel() != x_im.numel() or y.numel() != B * H * W:
        raise ValueError("pc_singlecoil_step: operand sizes do not match the state")
    head = _pc_head("pc_singlecoil_step", head, B, dev_sched, sample_sched)
    if work is None and _large_image(H, W):
        work = sense_workspace(B, 1, H, W, x_re.device)
    if work is not None or _large_image(H, W):
        _check_work(work, B, 1, H, W, "pc_singlecoil_step")
    mask_t = _mask_t(mask_u8, H, W, "pc_singlecoil_step")
    call("ipdm_pc_singlecoil_step_f32", *head, _ptr(y), _ptr(mask_u8), mask_t, float(coef), int(mode), _ptr(work), B, H, W,
         _stream())
    _written(x_re, x_im)


# ---- non-Cartesian SENSE (csrc/kspace_nc.hip, the Toeplitz chain of kspace_large.hip) ---------------------
NC_SIZE_RULE = "the padded grid 2H x 2W must be a served k-space size: " + KSPACE_SIZE_RULE + ", for 2H and 2W"


def nc_supported(H, W):
    """whether the non-Cartesian operators serve an H x W image (NC_SIZE_RULE: kspace_size_class(2H, 2W) != 0).  Needs no
    GPU."""
    return bool(_lib.lib.ipdm_nc_supported(int(H), int(W)))


def _nc_unsupported(H, W, what):
    if not nc_supported(H, W):
        raise _lib.IpdmUnsupported(f"{what}: no non-Cartesian kernel for {H}x{W}: {NC_SIZE_RULE}")


def _nc_operand(t, dtype, name, what):
    """operand read through a raw pointer: a contiguous GPU tensor of exactly this dtype, never converted"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"ipdm {what}: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"ipdm {what}: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise TypeError(f"ipdm {what}: {name} must be contiguous (call .contiguous() and keep the result)")
    return t


def _nc_traj(traj, weights, what):
    """-> (M, T) of a device trajectory float64 [M, 2] (T None; weights float32 [M], optional) or of one trajectory per
    frame [T, M, 2] (weights [T, M]): image row b reads frame b % T"""
    _nc_operand(traj, torch.float64, "trajectory", what)
    if traj.dim() == 3 and traj.shape[2] == 2 and traj.shape[0] >= 1 and traj.shape[1] >= 1:
        T, M = traj.shape[0], traj.shape[1]
    elif traj.dim() != 2 or traj.shape[1] != 2 or traj.shape[0] < 1:
        raise ValueError(f"ipdm {what}: trajectory {tuple(traj.shape)} is not (M, 2)" + (" or (T, M, 2)" if traj.dim() > 2 else ""))
    else:
        T, M = None, traj.shape[0]
    if weights is not None:
        _nc_operand(weights, torch.float32, "weights", what)
        if T is not None and tuple(weights.shape) != (T, M):
            raise ValueError(f"ipdm {what}: weights {tuple(weights.shape)} do not match the {T} frames of {M} samples")
        if T is None and tuple(weights.shape) != (M,):
            raise ValueError(f"ipdm {what}: weights {tuple(weights.shape)} do not match the {M} samples")
    return M, T


def _nc_frames(B, T, what):
    """a batch of B rows over T frame sets (row b reads set b % T): refused on the host unless T divides B"""
    if T is not None and B % T != 0:
        raise ValueError(f"ipdm {what}: B = {B} image rows are not a multiple of the T = {T} frames (row b reads frame b % T)")


def _nc_traj_frames(traj, B, what):
    """the B % T refusal of a framed trajectory [T, M, 2], from the shapes alone: before any operand is looked at"""
    if isinstance(traj, torch.Tensor) and traj.dim() == 3 and traj.shape[2] == 2 and traj.shape[0] >= 1:
        _nc_frames(B, traj.shape[0], what)


def _nc_rows(t):
    """-> (B, H, W) of an image batch [..., H, W] (None where it is no tensor of two or more dimensions)"""
    if not isinstance(t, torch.Tensor) or t.dim() < 2:
        return None
    H, W = t.shape[-2:]
    return (t.numel() // (H * W) if H * W else 0), H, W


def _nc_sens(sens, H, W, what):
    """-> n_coils of complex64 maps [n, H, W] (None: 1, S = 1)"""
    if sens is None:
        return 1
    _nc_operand(sens, torch.complex64, "coil maps", what)
    if sens.dim() != 3 or tuple(sens.shape[-2:]) != (H, W) or sens.shape[0] < 1:
        raise ValueError(f"ipdm {what}: coil maps {tuple(sens.shape)} do not match [n_coils, {H}, {W}]")
    return sens.shape[0]


def _nc_table_work(nbytes, device):
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def ndft_forward(x, traj, sens=None):
    """exact non-uniform DFT of images at the trajectory's samples (ipdm.h, ipdm_ndft_forward_c64).
    sens [n, H, W]: x [B, H, W] (or [B, 1, H, W]) -> y [n, B, M] = A x;  sens None: x [n, B, H, W] coil images -> [n, B, M].
    traj [M, 2], or [T, M, 2]: row b at the samples of frame b % T (ipdm_ndft_forward_sets_c64)"""
    what = "ndft_forward"
    if _nc_rows(x) is not None and (sens is not None or x.dim() >= 3):
        _nc_traj_frames(traj, _nc_rows(x)[0] // (1 if sens is not None else max(x.shape[0], 1)), what)
    _nc_operand(x, torch.complex64, "x", what)
    M, T = _nc_traj(traj, None, what)
    H, W = x.shape[-2:]
    n = _nc_sens(sens, H, W, what)
    if sens is None:
        if x.dim() < 3:
            raise ValueError(f"ipdm {what}: without coil maps x is [n_coils, B, H, W], got {tuple(x.shape)}")
        n = x.shape[0]
        B = x.numel() // (n * H * W)
    else:
        B = x.numel() // (H * W)
    _nc_frames(B, T, what)
    _nc_unsupported(H, W, what)
    y = torch.empty((n, B, M), dtype=torch.complex64, device=x.device)
    work = _nc_table_work(_lib.lib.ipdm_ndft_workspace_bytes((T or 1) * M, H, W), x.device)
    if T is None:
        call("ipdm_ndft_forward_c64", _ptr(x), _ptr(sens), _ptr(traj), _ptr(y), _ptr(work), B, n, M, H, W, _stream())
    else:
        call("ipdm_ndft_forward_sets_c64", _ptr(x), _ptr(sens), _ptr(traj), T, _ptr(y), _ptr(work), B, n, M, H, W, _stream())
    return y


def ndft_adjoint(y, traj, H, W, sens=None, weights=None):
    """adjoint of ndft_forward, the samples weighted first.  y [n, B, M] -> sens [n, H, W]: A^H W y [B, H, W]; sens None: the
    coil images [n, B, H, W].  traj [T, M, 2] (weights [T, M]): row b from the samples of frame b % T"""
    what = "ndft_adjoint"
    if isinstance(y, torch.Tensor) and y.dim() == 3:
        _nc_traj_frames(traj, y.shape[1], what)
    _nc_operand(y, torch.complex64, "y", what)
    M, T = _nc_traj(traj, weights, what)
    if y.dim() != 3 or y.shape[-1] != M:
        raise ValueError(f"ipdm {what}: y {tuple(y.shape)} is not [n_coils, B, {M}]")
    n, B = y.shape[0], y.shape[1]
    _nc_frames(B, T, what)
    if sens is not None and _nc_sens(sens, H, W, what) != n:
        raise ValueError(f"ipdm {what}: {n} coil signals, {sens.shape[0]} coil maps")
    _nc_unsupported(H, W, what)
    x = torch.empty((B, H, W) if sens is not None else (n, B, H, W), dtype=torch.complex64, device=y.device)
    work = _nc_table_work(_lib.lib.ipdm_ndft_workspace_bytes((T or 1) * M, H, W), y.device)
    if T is None:
        call("ipdm_ndft_adjoint_c64", _ptr(y), _ptr(sens), _ptr(traj), _ptr(weights), _ptr(x), _ptr(work), B, n, M, H, W, _stream())
    else:
        call("ipdm_ndft_adjoint_sets_c64", _ptr(y), _ptr(sens), _ptr(traj), T, _ptr(weights), _ptr(x), _ptr(work), B, n, M, H, W,
             _stream())
    return x


def toeplitz_psf(traj, H, W, weights=None):
    """the real spectrum P [2H, 2W] (float32) of the trajectory's Toeplitz kernel: A^H W A = crop F^-1 P F pad.
    traj [T, M, 2] (weights [T, M]) -> [T, 2H, 2W], one spectrum per frame"""
    what = "toeplitz_psf"
    M, T = _nc_traj(traj, weights, what)
    _nc_unsupported(H, W, what)
    psf = torch.empty((2 * H, 2 * W) if T is None else (T, 2 * H, 2 * W), dtype=torch.float32, device=traj.device)
    work = _nc_table_work(_lib.lib.ipdm_toeplitz_psf_workspace_bytes(M, H, W), traj.device)
    if T is None:
        call("ipdm_toeplitz_psf_f32", _ptr(traj), _ptr(weights), _ptr(psf), _ptr(work), M, H, W, _stream())
    else:
        call("ipdm_toeplitz_psf_sets_f32", _ptr(traj), T, _ptr(weights), _ptr(psf), _ptr(work), M, H, W, _stream())
    return psf


def _nc_psf_frames(psf, x, what):
    """-> T of a psf [T, 2H, 2W] for the image batch x (row b reads set b % T), None of the one-set form [2H, 2W].  Shapes
    alone: a psf of neither form and B % T != 0 are refused here, before any operand is looked at"""
    rows = _nc_rows(x)
    if rows is None or not isinstance(psf, torch.Tensor) or psf.dim() < 3:
        return None
    B, H, W = rows
    if psf.dim() != 3 or tuple(psf.shape[1:]) != (2 * H, 2 * W) or psf.shape[0] < 1:
        raise ValueError(f"ipdm {what}: psf {tuple(psf.shape)} is neither [{2 * H}, {2 * W}] nor [T, {2 * H}, {2 * W}]")
    _nc_frames(B, psf.shape[0], what)
    return psf.shape[0]


def _nc_psf(psf, H, W, T, what):
    _nc_operand(psf, torch.float32, "psf", what)
    if T is None and tuple(psf.shape) != (2 * H, 2 * W):
        raise ValueError(f"ipdm {what}: psf {tuple(psf.shape)} is not [{2 * H}, {2 * W}]")


def toeplitz_normal(v, psf, sens=None):
    """A^H W A v by the Toeplitz chain.  v complex64 [B, H, W] (or [B, 1, H, W]) -> the same shape.  psf [2H, 2W], or
    [T, 2H, 2W]: row b with the spectrum of frame b % T"""
    what = "toeplitz_normal"
    T = _nc_psf_frames(psf, v, what)
    _nc_operand(v, torch.complex64, "v", what)
    H, W = v.shape[-2:]
    B = v.numel() // (H * W) if H * W else 0
    n = _nc_sens(sens, H, W, what)
    _nc_psf(psf, H, W, T, what)
    _nc_unsupported(H, W, what)
    out = torch.empty_like(v)
    work = torch.empty(_lib.lib.ipdm_toeplitz_workspace_bytes(B, n, H, W) // 4, dtype=torch.float32, device=v.device)
    if T is None:
        call("ipdm_toeplitz_normal_c64", _ptr(v), _ptr(sens), _ptr(psf), _ptr(out), _ptr(work), B, n, H, W, _stream())
    else:
        call("ipdm_toeplitz_normal_sets_c64", _ptr(v), _ptr(sens), _ptr(psf), T, _ptr(out), _ptr(work), B, n, H, W, _stream())
    return out


def nc_sense_cg_workspace(B, n_coils, H, W, device):
    """scratch tensor of the non-Cartesian conjugate-gradient proximal (the Toeplitz chain's rows, T v, r, p, state)"""
    nbytes = _lib.lib.ipdm_nc_sense_cg_workspace_bytes(B, n_coils, H, W)
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device) if nbytes else None


def _nc_cg_args(work, ahy, iters_out, B, n_coils, H, W, device, what):
    need = _lib.lib.ipdm_nc_sense_cg_workspace_bytes(B, n_coils, H, W)
    if work is None:
        work = nc_sense_cg_workspace(B, n_coils, H, W, device)
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float32 or not work.is_contiguous()
            or work.numel() * 4 < need):
        raise ValueError(f"{what}: `work` must be a contiguous float32 GPU tensor of >= {need} bytes "
                         f"(ops.nc_sense_cg_workspace({B}, {n_coils}, {H}, {W}, device))")
    if ahy is None:
        raise ValueError(f"{what}: ahy = A^H W y is required (ops.ndft_adjoint): the iterations never apply A")
    _inplace_operand(ahy, torch.complex64, "ahy")
    if ahy.numel() != B * H * W:
        raise ValueError(f"{what}: ahy {tuple(ahy.shape)} does not match the image batch [{B}, {H}, {W}]")
    if iters_out is None:
        iters_out = torch.zeros(B, dtype=torch.int32, device=device)
    else:
        _inplace_operand(iters_out, torch.int32, "iters_out")
        if iters_out.numel() < B:
            raise ValueError(f"{what}: iters_out holds {iters_out.numel()} < {B} entries")
    return work, iters_out


def nc_sense_cgprox(z_re, z_im, ahy, sens, psf, a, max_iter=10, tol=1e-5, out_re=None, out_im=None, work=None, iters_out=None):
    """exact non-Cartesian SENSE proximal (I + a A^H W A) x = z + a ahy by conjugate gradients (sense_cgprox with the
    Toeplitz operator; ahy = ndft_adjoint(y, ...), psf = toeplitz_psf(...)) -> (out_re, out_im, iters).  psf [T, 2H, 2W]: row
    b solves with the spectrum of frame b % T"""
    what = "nc_sense_cgprox"
    max_iter, tol = _check_cg_scalars(max_iter, tol, what)
    T = _nc_psf_frames(psf, z_re, what)
    z_re, z_im = _nc_operand(z_re, torch.float32, "z_re", what), _nc_operand(z_im, torch.float32, "z_im", what)
    H, W = z_re.shape[-2:]
    B = z_re.numel() // (H * W) if H * W else 0
    if z_im.shape != z_re.shape:
        raise ValueError(f"{what}: z_re {tuple(z_re.shape)} and z_im {tuple(z_im.shape)} differ")
    n = _nc_sens(sens, H, W, what)
    _nc_psf(psf, H, W, T, what)
    _nc_unsupported(H, W, what)
    work, iters_out = _nc_cg_args(work, ahy, iters_out, B, n, H, W, z_re.device, what)
    out_re = torch.empty_like(z_re) if out_re is None else _inplace_operand(out_re, torch.float32, "out_re")
    out_im = torch.empty_like(z_im) if out_im is None else _inplace_operand(out_im, torch.float32, "out_im")
    if T is None:
        call("ipdm_nc_sense_cgprox_f32", _ptr(z_re), _ptr(z_im), _ptr(sens), _ptr(psf), float(a), _ptr(ahy), max_iter, tol,
             _ptr(out_re), _ptr(out_im), _ptr(work), _ptr(iters_out), B, n, H, W, _stream())
    else:
        call("ipdm_nc_sense_cgprox_sets_f32", _ptr(z_re), _ptr(z_im), _ptr(sens), _ptr(psf), T, float(a), _ptr(ahy), max_iter,
             tol, _ptr(out_re), _ptr(out_im), _ptr(work), _ptr(iters_out), B, n, H, W, _stream())
    _written(out_re, out_im, iters_out)
    return out_re, out_im, iters_out


def ald_nc_sense_cg_step(x_re, x_im, g_re, g_im, ahy, sens, psf, work, step=0.0, noise_scale=0.0, coef=0.0, noise_re=None,
                         noise_im=None, seed=0, sample_offset=0, step_id=0, dev_sched=None, sample_sched=None, max_iter=10,
                         tol=1e-5, iters_out=None):
    """ald_sense_cg_step for the non-Cartesian operator: Langevin update, then nc_sense_cgprox, in place on x_re / x_im.
    sample_sched: a schedule record per sample (pc_sense_step).  psf [T, 2H, 2W]: row b with the spectrum of frame b % T.
    -> iters (device int32 [B])"""
    what = "ald_nc_sense_cg_step"
    max_iter, tol = _check_cg_scalars(max_iter, tol, what)
    T = _nc_psf_frames(psf, x_re, what)
    for t, nm in ((x_re, "x_re"), (x_im, "x_im"), (g_re, "g_re"), (g_im, "g_im")):
        _inplace_operand(t, torch.float32, nm)
    for t, nm in ((noise_re, "noise_re"), (noise_im, "noise_im")):
        if t is not None:
            _inplace_operand(t, torch.float32, nm)
    if (noise_re is None) != (noise_im is None):
        raise ValueError(f"{what}: pass both noise planes or neither")
    H, W = x_re.shape[-2:]
    B = x_re.numel() // (H * W) if H * W else 0
    if any(t.numel() != x_re.numel() for t in (x_im, g_re, g_im)) or any(
            t is not None and t.numel() != x_re.numel() for t in (noise_re, noise_im)):
        raise ValueError(f"{what}: operand sizes do not match the state")
    n = _nc_sens(sens, H, W, what)
    _nc_psf(psf, H, W, T, what)
    _nc_unsupported(H, W, what)
    head = (_ptr(x_re), _ptr(x_im), _ptr(g_re), _ptr(g_im), _ptr(noise_re), _ptr(noise_im), float(step), float(noise_scale),
            int(seed), int(sample_offset), int(step_id), _ptr(dev_sched))
    head = _pc_head(what, head, B, dev_sched, sample_sched)
    work, iters_out = _nc_cg_args(work, ahy, iters_out, B, n, H, W, x_re.device, what)
    if T is None:
        call("ipdm_ald_nc_sense_cg_step_f32", *head, _ptr(sens), _ptr(psf), float(coef), _ptr(work), _ptr(ahy), max_iter, tol,
             _ptr(iters_out), B, n, H, W, _stream())
    else:
        call("ipdm_ald_nc_sense_cg_step_sets_f32", *head, _ptr(sens), _ptr(psf), T, float(coef), _ptr(work), _ptr(ahy), max_iter,
             tol, _ptr(iters_out), B, n, H, W, _stream())
    _written(x_re, x_im, iters_out)
    return iters_out


# ---- non-Cartesian self-calibration (csrc/nc_calib.hip) ----------------------------------------------------
NC_GRAM_CHUNK = 1024                             # samples per partial sum of nc_coil_gram (csrc/nc_calib.hip, NCG_CHUNK)


def nc_coil_gram_workspace(B, n_coils, M, device):
    """scratch tensor of nc_coil_gram (the double partial sums per chunk of NC_GRAM_CHUNK samples); None for a shape without
    a kernel"""
    nbytes = _lib.lib.ipdm_nc_coil_gram_workspace_bytes(int(B), int(n_coils), int(M))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device) if nbytes else None


def _nc_samples(y, what):
    """-> (n, B, M) of non-Cartesian samples y [n, B, M] complex64"""
    _nc_operand(y, torch.complex64, "y", what)
    if y.dim() != 3 or min(y.shape[0], y.shape[2]) < 1:
        raise ValueError(f"ipdm {what}: y {tuple(y.shape)} is not [n_coils, B, M]")
    return tuple(y.shape)


def _nc_window(weights, M, what):
    if weights is not None:
        _nc_operand(weights, torch.float32, "weights", what)
        if tuple(weights.shape) != (M,):
            raise ValueError(f"ipdm {what}: weights {tuple(weights.shape)} do not match the {M} samples")


def nc_coil_gram(y, weights=None, *, out=None, work=None):
    """weighted Gram matrices of non-Cartesian samples y [n, B, M] complex64 (1..64 coils): G_b[i][j] = sum_m w_m y_i conj(y_j)
    with weights [M] float32 >= 0 (None: 1; ``calibration_window``'s) -> (B, n, n) complex64, exactly Hermitian; y is read
    only where w_m > 0 (ipdm.h, ipdm_nc_coil_gram_c64).  The result goes to ``coilcomp_matrix`` as ``coil_gram``'s does."""
    what = "nc_coil_gram"
    n, B, M = _nc_samples(y, what)
    _nc_window(weights, M, what)
    if n > 64:
        raise _lib.IpdmUnsupported(f"ipdm {what}: {n} coils; the kernel serves 1..64")
    if out is None:
        out = torch.empty((B, n, n), dtype=torch.complex64, device=y.device)
    else:
        _inplace_operand(out, torch.complex64, "out")
        if tuple(out.shape) != (B, n, n):
            raise ValueError(f"ipdm {what}: out {tuple(out.shape)}, expected {(B, n, n)}")
    need = _lib.lib.ipdm_nc_coil_gram_workspace_bytes(B, n, M)
    if work is None:
        work = nc_coil_gram_workspace(B, n, M, y.device)
    elif (not isinstance(work, torch.Tensor) or not work.is_cuda or work.dtype != torch.float64 or not work.is_contiguous()
            or work.numel() * 8 < need):
        raise ValueError(f"ipdm {what}: `work` must be a contiguous float64 GPU tensor of >= {need} bytes "
                         f"(ops.nc_coil_gram_workspace({B}, {n}, {M}, device))")
    call("ipdm_nc_coil_gram_c64", _ptr(y), _ptr(weights), _ptr(out), _ptr(work), B, n, M, _stream())
    _written(out)
    return out


def nc_calib_images(y, traj, H, W, weights, lam=1e-2, max_iter=40, tol=1e-4, return_iters=False):
    """low-resolution calibration images of non-Cartesian samples: y [n, B, M] complex64 at traj [M, 2] float64, weights [M]
    float32 the calibration window (``calibration_window``) -> x [n, B, H, W] complex64, per coil the regularised inverse
        (A^H W A + lam t0 I) x_c = A^H W y_c,   t0 = sum(w) / (H W)
    of the windowed samples: no density compensation, any trajectory the operator accepts.  One ``toeplitz_psf``, one
    ``ndft_adjoint`` and one ``nc_sense_cgprox`` call with the n B coil images as batch rows, one unit map, z = 0 and
    a = 1 / (lam t0).  tol = 0 runs max_iter iterations.  return_iters: -> (x, iters int32 [n, B]).  sum(w) is read back
    once (the solver's `a` is a host scalar)."""
    what = "nc_calib_images"
    n, B, M = _nc_samples(y, what)
    _nc_operand(traj, torch.float64, "trajectory", what)
    if tuple(traj.shape) != (M, 2):
        raise ValueError(f"ipdm {what}: trajectory {tuple(traj.shape)} is not ({M}, 2), one position per sample")
    if weights is None:
        raise ValueError(f"ipdm {what}: weights, the calibration window of the trajectory, are required")
    _nc_window(weights, M, what)
    lam = float(lam)
    if not (lam > 0.0 and lam < float("inf")):
        raise ValueError(f"ipdm {what}: lam must be positive and finite, got {lam}")
    max_iter, tol = _check_cg_scalars(max_iter, tol, what)
    H, W = int(H), int(W)
    _nc_unsupported(H, W, what)
    t0 = float(weights.sum(dtype=torch.float64)) / (H * W)
    if not t0 > 0.0:
        raise ValueError(f"ipdm {what}: the weights are all zero")
    psf = toeplitz_psf(traj, H, W, weights)
    ahy = ndft_adjoint(y, traj, H, W, None, weights).reshape(n * B, H, W)
    z = torch.zeros((n * B, H, W), dtype=torch.float32, device=y.device)
    x_re, x_im, iters = nc_sense_cgprox(z, z, ahy, None, psf, 1.0 / (lam * t0), max_iter=max_iter, tol=tol)
    x = torch.complex(x_re, x_im).reshape(n, B, H, W)
    return (x, iters.reshape(n, B)) if return_iters else x


def nc_calib_kspace(y, traj, H, W, weights, lam=1e-2, max_iter=40, tol=1e-4, return_iters=False):
    """Cartesian calibration k-space of non-Cartesian samples: ``fft2c`` of ``nc_calib_images`` -> [n, B, H, W] complex64, which
    ``estimate_sens_maps`` and ``espirit_maps`` take as it is, with the box of ``calibration_window``"""
    if kspace_size_class(H, W) == KSPACE_NONE:
        raise _lib.IpdmUnsupported(f"ipdm nc_calib_kspace: no k-space kernel for {H}x{W}; {KSPACE_SIZE_RULE}")
    x, iters = nc_calib_images(y, traj, H, W, weights, lam, max_iter, tol, return_iters=True)
    k = fft2c(x)
    return (k, iters) if return_iters else k


# ---- segmentation-likelihood guidance glue ----------------------------------------------------------
def zero_insert2(x):
    """(..., H, W) -> (..., 2H, 2W): x at the even positions, zeros elsewhere"""
    x = _gpu(x, torch.float32, "x")
    H, W = x.shape[-2:]
    out = torch.empty(tuple(x.shape[:-2]) + (2 * H, 2 * W), dtype=torch.float32, device=x.device)
    call("ipdm_zero_insert2_f32", _ptr(x), _ptr(out), x.numel() // (H * W), H, W, _stream())
    return out


def subsample2(x, offset=(0, 0), size=None):
    """(..., H, W) -> (..., Ho, Wo): x[..., 2i + oy, 2j + ox]; default: the even positions, (H/2, W/2)"""
    x = _gpu(x, torch.float32, "x")
    H, W = x.shape[-2:]
    oy, ox = offset
    Ho, Wo = ((H - oy + 1) // 2, (W - ox + 1) // 2) if size is None else size
    out = torch.empty(tuple(x.shape[:-2]) + (Ho, Wo), dtype=torch.float32, device=x.device)
    call("ipdm_subsample2_f32", _ptr(x), _ptr(out), x.numel() // (H * W), H, W, oy, ox, Ho, Wo, _stream())
    return out


def conv2d_stride2_valid(x, wt, bias=None, ksize=3, in_amax=None):
    """F.conv2d(x, w, stride=2, padding=0) for an odd kernel on the stride-1 MFMA kernel: the 'same' convolution sampled at
    (k//2, k//2) + 2(i, j).  wt: the packed weight of the same layer (conv_weight)."""
    H, W = x.shape[-2:]
    full = conv2d(x, wt, bias, in_amax=in_amax)
    o = ksize // 2
    return subsample2(full, (o, o), ((H - ksize) // 2 + 1, (W - ksize) // 2 + 1))


def in_prelu_fwd(x, slope, eps=1e-5):
    """InstanceNorm (no affine) + PReLU(one slope) on (B, C, H, W) -> (xhat, y, rstd (B*C,))"""
    x = _gpu(x, torch.float32, "x")
    B, C = x.shape[:2]
    hw = x.numel() // max(B * C, 1)
    xhat, y = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(B * C, dtype=torch.float32, device=x.device)
    call("ipdm_in_prelu_fwd_f32", _ptr(x), _ptr(slope), _ptr(xhat), _ptr(y), _ptr(rstd), B * C, hw, float(eps), _stream())
    return xhat, y, rstd


def in_prelu_bwd(gy, xhat, rstd, slope, eps=1e-5):
    """input-gradient of in_prelu_fwd from what it saved; eps: the forward's (planes of two pixels need it, seg_ops.hip)"""
    gy = _gpu(gy, torch.float32, "gy")
    B, C = gy.shape[:2]
    gx = torch.empty_like(gy)
    call("ipdm_in_prelu_bwd_eps_f32", _ptr(gy), _ptr(xhat), _ptr(rstd), _ptr(slope), _ptr(gx), B * C,
         gy.numel() // max(B * C, 1), float(eps), _stream())
    return gx


def seg_loglh_grad(logits, label):
    """d/dlogits of sum log softmax(logits, dim=1)[label]: logits (B, C, H, W) f32, label (B, 1, H, W) int64"""
    logits = _gpu(logits, torch.float32, "logits")
    label = _gpu(label, torch.int64, "label")
    B, C = logits.shape[:2]
    hw = logits.numel() // max(B * C, 1)
    if label.numel() != B * hw:
        raise ValueError(f"seg_loglh_grad: label {tuple(label.shape)} does not match logits {tuple(logits.shape)}")
    g = torch.empty_like(logits)
    call("ipdm_seg_loglh_grad_f32", _ptr(logits), _ptr(label), _ptr(g), B, C, hw, _stream())
    return g


def axpy_sched(y, x, scale=0.0, dev_sched=None, mask=None):
    """y += scale * x (* mask, broadcast over y's leading copies) in place; dev_sched: the device ipdm_sched_t whose
    seg_scale replaces `scale` (graph replay)"""
    _inplace_operand(y, torch.float32, "y")
    _inplace_operand(x, torch.float32, "x")
    if x.numel() != y.numel():
        raise ValueError("axpy_sched: x does not match y")
    period = 0
    if mask is not None:
        _inplace_operand(mask, torch.int64, "mask")
        period = mask.numel()
        if y.numel() % period:
            raise ValueError("axpy_sched: mask does not tile y")
    call("ipdm_axpy_sched_f32", _ptr(y), _ptr(x), _ptr(mask), period, _ptr(dev_sched), float(scale), y.numel(), _stream())
    _written(y)
    return y


# ---- on-device reporting ------------------------------------------------------------------------
def magnitude(x):
    x = _gpu(x, torch.complex64, "x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("ipdm_magnitude_c64", _ptr(x), _ptr(out), x.numel(), _stream())
    return out


def posterior_moment_planes(samples):
    """samples (n, ..., H, W) complex64 -> (7, ..., H, W) float64 partial sums over the n samples:
    sum |x|, sum |x|^2, sum angle, sum angle^2, sum Re, sum Im, sum |angle|"""
    samples = _gpu(samples, torch.complex64, "samples")
    n = samples.shape[0]
    hw = samples[0].numel() if n else 0
    planes = torch.empty((7,) + tuple(samples.shape[1:]), dtype=torch.float64, device=samples.device)
    call("ipdm_posterior_moments_c64", _ptr(samples), _ptr(planes), n, hw, _stream())
    return planes


def tv_value(x):
    """x (n, ..., H, W) complex64 -> (n',) float64 total variation per image (n' = all leading dims flattened)"""
    x = _gpu(x, torch.complex64, "x")
    H, W = x.shape[-2:]
    n = x.numel() // (H * W)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    call("ipdm_tv_c64", _ptr(x), _ptr(out), n, H, W, _stream())
    return out


def tv_grad(x):
    """gradient of sum-of-moduli total variation w.r.t. the complex image (torch autograd's convention)"""
    x = _gpu(x, torch.complex64, "x")
    H, W = x.shape[-2:]
    g = torch.empty_like(x)
    call("ipdm_tv_grad_c64", _ptr(x), _ptr(g), x.numel() // (H * W), H, W, _stream())
    return g


def nrmse(img, ref):
    """per-image ||img - ref|| / ||img|| (the reference's argument order); img (n, ...), ref same shape or one image"""
    img, ref = _gpu(img, torch.float32, "img"), _gpu(ref, torch.float32, "ref")
    n = img.shape[0]
    elems = img[0].numel()
    bcast = ref.numel() == elems
    if not bcast and ref.numel() != img.numel():
        raise ValueError(f"nrmse: reference {tuple(ref.shape)} does not match {tuple(img.shape)}")
    out = torch.empty(n, dtype=torch.float64, device=img.device)
    call("ipdm_nrmse_f32", _ptr(img), _ptr(ref), _ptr(out), n, elems, int(bcast), _stream())
    return out


def ssim(img, ref, data_range=2.0):
    """per-image mean SSIM of single-channel images (n, H, W) (or (n, 1, H, W)) against ref (same shape or one image)"""
    img, ref = _gpu(img, torch.float32, "img"), _gpu(ref, torch.float32, "ref")
    H, W = img.shape[-2:]
    n = img.numel() // (H * W)
    bcast = ref.numel() == H * W
    if not bcast and ref.numel() != img.numel():
        raise ValueError(f"ssim: reference {tuple(ref.shape)} does not match {tuple(img.shape)}")
    out = torch.empty(n, dtype=torch.float64, device=img.device)
    call("ipdm_ssim_f32", _ptr(img), _ptr(ref), _ptr(out), n, H, W, int(bcast), float(data_range), _stream())
    return out


# ---- per-image activation maxima: the f16x2 family's DYNAMIC RANGE without a pass over the tensor ------------------
# An f16x2 convolution scales every image of its input into fp16's range by an exact power of two derived from an upper bound of
# that image's max |x| (`in_amax`, conv_kernel.h hx_dynamic_scale) -- then ANY fp32 input is in range and values down to 2^-17 of
# the bound keep all 22 significand bits.  The bounds come from the PRODUCERS: convolution epilogues and the resize kernels
# accumulate the exact maxima of what they store with one atomic max per wave (`want_amax`), InstanceNorm++ / GroupNorm hand over
# a bound computed from their coefficients, and pooling / activation / gather kernels pass their input's bound on (they never
# increase |x|).  Maxima ride on the tensors as `_ipdm_amax = (amax [B], (version, data_ptr))`: a tensor written in place since
# loses them, and a consumer that finds none MEASURES its input (ipdm_absmax_f32: one extra pass, counted in AMAX_MEASURED so that
# tests can assert the hot path never does).  IPDM_HX2_DYNAMIC=0 restores round 3's static contract (|x| < 65504) for A/B runs.
HX2_DYNAMIC = os.environ.get("IPDM_HX2_DYNAMIC", "1") != "0"
AMAX_MEASURED = 0                               # fallback absmax passes since import (diagnostics / tests)


def dynamic_range(impl=None):
    """True when convolutions should produce and consume per-image maxima (the f16x2 family with the dynamic range on);
    impl: the kernel family in use where it is not CONV_IMPL (the score_sde networks: impl_unbounded())"""
    return HX2_DYNAMIC and (CONV_IMPL if impl is None else impl) == "hx2"


AMAX_WAYS, AMAX_SLOT = 8, 128                    # include/ipdm.h "maxima vectors": [B][AMAX_SLOT] floats, 8 ways per image, 16 floats apart


def amax_value(am):
    """maxima vector [B, AMAX_SLOT] -> per-image values [B] (the max over an image's ways)"""
    return am.view(am.shape[0], AMAX_WAYS, AMAX_SLOT // AMAX_WAYS)[:, :, 0].amax(dim=1)


class _AmaxArena:
    """zeroed [slots][B][AMAX_SLOT] float32 block: ONE fill per block instead of one per vector (atomic-max ways start at zero)"""

    def __init__(self, B, device, slots):
        self.B, self.device, self.used, self.slots = B, device, 0, slots
        self.buf = torch.zeros((slots, B, AMAX_SLOT), dtype=torch.float32, device=device)

    def take(self):
        if self.used == self.slots:
            return None
        self.used += 1
        return self.buf[self.used - 1]


_ARENAS = []                                    # stack of active amax_scope()s


class amax_scope:
    """`with ops.amax_scope():` around one network evaluation: the zeroed slots of every producer inside come out of a few large
    blocks (one fill kernel per 256 slots).  Allocated INSIDE the scope, so a forward captured into a hipGraph re-zeroes its
    slots on every replay.  Without a scope every slot is its own torch.zeros (correct, one more launch each)."""

    def __enter__(self):
        _ARENAS.append({})
        return self

    def __exit__(self, *exc):
        _ARENAS.pop()
        return False


def amax_slot(B, device):
    """a zeroed maxima vector (float32 [B, AMAX_SLOT]) for a producer's atomic maxima"""
    if _ARENAS:
        blocks = _ARENAS[-1]
        key = (int(B), str(device))
        a = blocks.get(key)
        slot = a.take() if a is not None else None
        if slot is None:
            blocks[key] = a = _AmaxArena(int(B), device, 128)
            slot = a.take()
        return slot
    return torch.zeros((int(B), AMAX_SLOT), dtype=torch.float32, device=device)


def tag_amax(t, amax):
    """attach per-image maxima (or an upper bound of them) to tensor t as it is NOW"""
    if t is not None and amax is not None:
        t._ipdm_amax = (amax, (t._version, t.data_ptr()))
    return t


def amax_of(t):
    """the maxima attached to t, or None (never attached, or t was written in place since)"""
    hit = getattr(t, "_ipdm_amax", None)
    if hit is None:
        return None
    amax, tag = hit
    if tag != (t._version, t.data_ptr()) or amax.shape[0] != t.shape[0]:
        return None
    return amax


def carry_amax(src, dst):
    """dst = f(src) with |f(x)| <= max |src| everywhere (pooling, activations, gathers, views): src's bound bounds dst"""
    return tag_amax(dst, amax_of(src))


def in_amax_for(x, impl=None, always=False):
    """the `in_amax` argument for a convolution reading x: None (static contract / other kernel families), the maxima attached to
    x, or -- where nothing is attached -- a MEASUREMENT (ipdm_absmax_f32: one pass, counted in AMAX_MEASURED), which is then
    attached to x so that its other consumers find it.  always: dynamic whenever the family is f16x2 (the score_sde networks,
    whose raw streams overflow the static contract: HX2_DYNAMIC does not apply to them)"""
    fam = CONV_IMPL if impl is None else impl
    if fam != "hx2" or not (always or HX2_DYNAMIC) or os.environ.get("IPDM_AMAX_CONSUME", "1") == "0":
        return None
    am = amax_of(x)
    if am is not None:
        return am
    global AMAX_MEASURED
    AMAX_MEASURED += 1
    am = absmax_per_image(x)
    tag_amax(x, am)
    return am


# ---- score-network glue -----------------------------------------------------------------------
# the producing convolution's epilogue hands the plane statistics over as partials (conv2d_wino_bx3(want_stats=True) hangs
# them on its result as `_ipdm_partials`), so that InstanceNorm++ does not read the tensor a second time
USE_STATS_EPILOGUE = os.environ.get("IPDM_STATS_EPILOGUE", "1") != "0"


def instnorm_plus_coef(x, alpha, gamma, beta):
    """x [B, C, *spatial] (2-D images or 3-D volumes: the statistics run over all spatial positions)"""
    x = _gpu(x, torch.float32, "x")
    B, C = x.shape[:2]
    coef = torch.empty((B, C, 3), dtype=torch.float32, device=x.device)
    hw = x.numel() // max(B * C, 1)
    # dynamic range: an upper bound of max |normalised value| per image, from the coefficients (affine_act passes it on)
    bound = torch.empty((B, AMAX_SLOT), dtype=torch.float32, device=x.device) if dynamic_range() else None
    if bound is not None:
        coef._ipdm_amax_bound = bound
    part = getattr(x, "_ipdm_partials", None)
    if part is not None:
        del x._ipdm_partials             # single use: whatever touches the tensor afterwards cannot meet stale statistics
        part, tag = part
        if tag != (x._version, x.data_ptr()):        # written in place since the convolution produced it: read the tensor
            part = None
    if part is not None and USE_STATS_EPILOGUE and tuple(part.shape[:2]) == (B, C):
        call("ipdm_instnorm_plus_coef_partials_f32", _ptr(part), int(part.shape[2]), _ptr(alpha), _ptr(gamma), _ptr(beta),
             _ptr(coef), B, C, hw, _ptr(bound), _stream())
        return coef
    call("ipdm_instnorm_plus_coef_f32", _ptr(x), _ptr(alpha), _ptr(gamma), _ptr(beta), _ptr(coef), B, C, hw, _ptr(bound),
         _stream())
    return coef


def cond_instnorm_plus_coef(x, embed, labels, bias=True):
    """ConditionalInstanceNorm2dPlus coefficients: x [B, C, *spatial], embed [num_classes, 3C] ([gamma | alpha | beta]; bias=False:
    [num_classes, 2C]), labels int64 [B] on the device -- read by the kernel, so a captured graph follows labels written in place.
    A label outside [0, num_classes) gives NaN coefficients (the host cannot check inside a graph).  -> coef [B, C, 3], as
    instnorm_plus_coef (statistics from the producing convolution's partials where they ride on x)."""
    x = _gpu(x, torch.float32, "x")
    embed = _gpu(embed, torch.float32, "embed")
    labels = _gpu(labels, torch.int64, "labels")
    B, C = x.shape[:2]
    if embed.dim() != 2 or embed.shape[1] != (3 if bias else 2) * C:
        raise ValueError(f"ipdm cond_instnorm_plus_coef: embed {tuple(embed.shape)} is not [num_classes, {3 if bias else 2}*{C}]")
    if labels.shape != (B,):
        raise ValueError(f"ipdm cond_instnorm_plus_coef: labels {tuple(labels.shape)} for a batch of {B}")
    coef = torch.empty((B, C, 3), dtype=torch.float32, device=x.device)
    hw = x.numel() // max(B * C, 1)
    bound = torch.empty((B, AMAX_SLOT), dtype=torch.float32, device=x.device) if dynamic_range() else None
    if bound is not None:
        coef._ipdm_amax_bound = bound
    nc = int(embed.shape[0])
    part = getattr(x, "_ipdm_partials", None)
    if part is not None:
        del x._ipdm_partials             # single use, as in instnorm_plus_coef
        part, tag = part
        if tag != (x._version, x.data_ptr()):
            part = None
    if part is not None and USE_STATS_EPILOGUE and tuple(part.shape[:2]) == (B, C):
        call("ipdm_cond_instnorm_plus_coef_partials_f32", _ptr(part), int(part.shape[2]), _ptr(embed), _ptr(labels), nc,
             int(bool(bias)), _ptr(coef), B, C, hw, _ptr(bound), _stream())
        return coef
    call("ipdm_cond_instnorm_plus_coef_f32", _ptr(x), _ptr(embed), _ptr(labels), nc, int(bool(bias)), _ptr(coef), B, C, hw,
         _ptr(bound), _stream())
    return coef


def affine_act(x, coef, act=ACT_NONE, out=None):
    x = _gpu(x, torch.float32, "x")
    B, C = x.shape[:2]
    out = torch.empty_like(x) if out is None else out
    call("ipdm_affine_act_f32", _ptr(x), _ptr(coef), _ptr(out), B, C, x.numel() // max(B * C, 1), act, _stream())
    _written(out)
    return tag_amax(out, getattr(coef, "_ipdm_amax_bound", None))     # (every activation code shrinks |.|)


def act(x, code, out=None):
    x = _gpu(x, torch.float32, "x")
    out = torch.empty_like(x) if out is None else out
    call("ipdm_act_f32", _ptr(x), _ptr(out), x.numel(), code, _stream())
    am = amax_of(x)                                 # (every activation code shrinks |.|: the input's bound holds, in place too)
    _written(out)
    return tag_amax(out, am)


def scale_shift(x, a, b, out=None):
    x = _gpu(x, torch.float32, "x")
    out = torch.empty_like(x) if out is None else out
    call("ipdm_scale_shift_f32", _ptr(x), _ptr(out), x.numel(), float(a), float(b), _stream())
    _written(out)
    return out


def add(x, y, out=None):
    x, y = _gpu(x, torch.float32, "x"), _gpu(y, torch.float32, "y")
    if x.shape != y.shape:
        raise ValueError(f"ipdm add: shapes differ {tuple(x.shape)} vs {tuple(y.shape)}")
    out = torch.empty_like(x) if out is None else out
    call("ipdm_add_f32", _ptr(x), _ptr(y), _ptr(out), x.numel(), _stream())
    _written(out)
    return out


def div_sigma(x, sigmas, labels=None, out=None):
    """x[b] / sigmas[labels[b]]  (labels None: x[b] / sigmas[b])"""
    x = _gpu(x, torch.float32, "x")
    labels = None if labels is None else _gpu(labels, torch.int64, "labels")
    sigmas = _gpu(sigmas, torch.float32, "sigmas")
    out = torch.empty_like(x) if out is None else out
    B = x.shape[0]
    call("ipdm_div_sigma_f32", _ptr(x), _ptr(sigmas), _ptr(labels), _ptr(out), B, x.numel() // max(B, 1), _stream())
    _written(out)
    return out


def maxpool5(x):
    x = _gpu(x, torch.float32, "x")
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    call("ipdm_maxpool5_f32", _ptr(x), _ptr(out), B * C, H, W, _stream())
    return carry_amax(x, out)


def affine_avgpool5(x, coef):
    """avg_pool2d((x - coef[..., 0]) * coef[..., 1] + coef[..., 2], 5, stride 1, padding 2, count_include_pad=True) in one pass
    (CondCRPBlock's norm + pool).  The normalisation's bound rides on the result: an average cannot exceed its terms' bound."""
    x = _gpu(x, torch.float32, "x")
    B, C, H, W = x.shape
    bound = getattr(coef, "_ipdm_amax_bound", None)
    coef = _gpu(coef, torch.float32, "coef")
    if tuple(coef.shape) != (B, C, 3):
        raise ValueError(f"ipdm affine_avgpool5: coef {tuple(coef.shape)} for x {tuple(x.shape)}")
    out = torch.empty_like(x)
    call("ipdm_affine_avgpool5_f32", _ptr(x), _ptr(coef), _ptr(out), B * C, H, W, _stream())
    return tag_amax(out, bound)


def meanpool2(x):
    x = _gpu(x, torch.float32, "x")
    B, C, H, W = x.shape
    out = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    call("ipdm_meanpool2_f32", _ptr(x), _ptr(out), B * C, H, W, _stream())
    return carry_amax(x, out)


def bilinear(x, size, out=None, accumulate=False, act=ACT_NONE, want_amax=False):
    """want_amax: the per-image maxima of what is written ride on the result (tag_amax)"""
    x = _gpu(x, torch.float32, "x")
    B, C, H, W = x.shape
    oh, ow = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((B, C, oh, ow), dtype=torch.float32, device=x.device)
        accumulate = False
    slot = amax_slot(B, x.device) if want_amax and B <= 65535 else None
    call("ipdm_bilinear_f32", _ptr(x), _ptr(out), B * C, H, W, oh, ow, int(bool(accumulate)), act, C, _ptr(slot), _stream())
    _written(out)
    return tag_amax(out, slot)


def trilinear(x, size, out=None, accumulate=False, act=ACT_NONE, want_amax=False):
    """F.interpolate(x, size, mode='trilinear', align_corners=True) of (B, C, D, H, W), optionally accumulated into out"""
    x = _gpu(x, torch.float32, "x")
    B, C, D, H, W = x.shape
    od, oh, ow = (int(v) for v in size)
    if out is None:
        out = torch.empty((B, C, od, oh, ow), dtype=torch.float32, device=x.device)
        accumulate = False
    slot = amax_slot(B, x.device) if want_amax and B <= 65535 else None
    call("ipdm_trilinear_f32", _ptr(x), _ptr(out), B * C, D, H, W, od, oh, ow, int(bool(accumulate)), act, C, _ptr(slot),
         _stream())
    _written(out)
    return tag_amax(out, slot)


# ---- NCSN++ / predictor-corrector extras --------------------------------------------------------
def stats_partials_of(x):
    """the statistics partials [B, C, P, 3] the producing convolution's epilogue hung on x (conv2d_wino_bx3(want_stats=True)), or
    None -- also None when x was written since (the tag is its (version, data_ptr))"""
    part = getattr(x, "_ipdm_partials", None)
    if part is None or not USE_STATS_EPILOGUE:
        return None
    part, tag = part
    if tag != (x._version, x.data_ptr()) or tuple(part.shape[:2]) != tuple(x.shape[:2]):
        return None
    return part


def groupnorm_coef(x, weight, bias, groups, eps=1e-6, want_amax=False):
    """-> coef [B, C, 3]; want_amax: -> (coef, per-image max |x| [B]) -- the maxima come out of the statistics pass (planes in
    registers) plus one tiny reduction; where that pass is not the single-read kernel the input is measured separately.
    Where x carries its producer's statistics partials (stats_partials_of) the coefficients come from those: x is not read."""
    x = _gpu(x, torch.float32, "x")
    B, C, H, W = x.shape
    coef = torch.empty((B, C, 3), dtype=torch.float32, device=x.device)
    part = None if want_amax else stats_partials_of(x)
    if part is not None:
        call("ipdm_groupnorm_coef_partials_f32", _ptr(part), C, _ptr(None), 0, int(part.shape[2]), _ptr(weight), _ptr(bias),
             _ptr(coef), B, groups, float(eps), _stream())
        return coef
    if want_amax:
        planes = torch.empty((B, C), dtype=torch.float32, device=x.device)
        try:
            call("ipdm_groupnorm_coef_f32", _ptr(x), _ptr(weight), _ptr(bias), _ptr(coef), B, C, H * W, groups, float(eps),
                 _ptr(planes), _stream())
            return coef, absmax_per_image(planes)
        except _lib.IpdmUnsupported:
            pass
    call("ipdm_groupnorm_coef_f32", _ptr(x), _ptr(weight), _ptr(bias), _ptr(coef), B, C, H * W, groups, float(eps),
         _ptr(None), _stream())
    return (coef, absmax_per_image(x)) if want_amax else coef


def groupnorm_act_cat(x1, x2, weight, bias, groups, eps=1e-6, act=ACT_NONE, want_amax=False):
    """act(GroupNorm(torch.cat([x1, x2], dim=1))) without materialising the concatenation of the RAW tensors; falls back to
    the concatenation where the two-source kernels do not apply.  want_amax: -> (out, per-image max over BOTH tensors [B])"""
    x1, x2 = _gpu(x1, torch.float32, "x1"), _gpu(x2, torch.float32, "x2")
    B, C1, H, W = x1.shape
    C2 = x2.shape[1]
    if tuple(x2.shape) != (B, C2, H, W):
        raise ValueError(f"groupnorm_act_cat: {tuple(x1.shape)} vs {tuple(x2.shape)}")
    coef = torch.empty((B, C1 + C2, 3), dtype=torch.float32, device=x1.device)
    out = torch.empty((B, C1 + C2, H, W), dtype=torch.float32, device=x1.device)
    planes = torch.empty((B, C1 + C2), dtype=torch.float32, device=x1.device) if want_amax else None
    p1, p2 = (None, None) if want_amax else (stats_partials_of(x1), stats_partials_of(x2))
    if p1 is not None and p2 is not None and p1.shape[2] == p2.shape[2]:       # both producers left their statistics: no read
        try:
            call("ipdm_groupnorm_coef_partials_f32", _ptr(p1), C1, _ptr(p2), C2, int(p1.shape[2]), _ptr(weight), _ptr(bias),
                 _ptr(coef), B, groups, float(eps), _stream())
            call("ipdm_affine_act_cat_f32", _ptr(x1), C1, _ptr(x2), C2, _ptr(coef), _ptr(out), B, H * W, act, _stream())
            return out
        except _lib.IpdmUnsupported:
            pass
    try:
        call("ipdm_groupnorm_coef_cat_f32", _ptr(x1), C1, _ptr(x2), C2, _ptr(weight), _ptr(bias), _ptr(coef), B, H * W, groups,
             float(eps), _ptr(planes), _stream())
        call("ipdm_affine_act_cat_f32", _ptr(x1), C1, _ptr(x2), C2, _ptr(coef), _ptr(out), B, H * W, act, _stream())
        return (out, absmax_per_image(planes)) if want_amax else out
    except _lib.IpdmUnsupported:
        x = torch.cat([x1, x2], dim=1)
        if want_amax:
            c, am = groupnorm_coef(x, weight, bias, groups, eps, want_amax=True)
            return affine_act(x, c, act), am
        return affine_act(x, groupnorm_coef(x, weight, bias, groups, eps), act)


def linear(x, weight, bias=None, act_in=ACT_NONE):
    x = _gpu(x, torch.float32, "x")
    B, In = x.shape
    Out = weight.shape[0]
    y = torch.empty((B, Out), dtype=torch.float32, device=x.device)
    call("ipdm_linear_f32", _ptr(x), _ptr(weight), _ptr(bias), _ptr(y), B, In, Out, act_in, _stream())
    return y


def attention(q, k, v, scale):
    q, k, v = (_gpu(t, torch.float32, n) for t, n in ((q, "q"), (k, "k"), (v, "v")))
    B, C, H, W = q.shape
    out = torch.empty_like(q)
    call("ipdm_attention_f32", _ptr(q), _ptr(k), _ptr(v), _ptr(out), B, C, H * W, float(scale), _stream())
    return out


def axpby(x, y, a, b, out=None):
    x, y = _gpu(x, torch.float32, "x"), _gpu(y, torch.float32, "y")
    if x.shape != y.shape:
        raise ValueError(f"ipdm axpby: shapes differ {tuple(x.shape)} vs {tuple(y.shape)}")
    out = torch.empty_like(x) if out is None else out
    call("ipdm_axpby_f32", _ptr(x), _ptr(y), _ptr(out), x.numel(), float(a), float(b), _stream())
    _written(out)
    return out


def sample_axpy2(x, y, a, z=None, c=None, out=None):
    """x + a[:,None]*y (+ c[:,None]*z): per-sample float32 device vectors a, c"""
    x = _gpu(x, torch.float32, "x")
    n = x.shape[0]
    out = torch.empty_like(x) if out is None else out
    a = _gpu(a.to(torch.float32), torch.float32, "a")
    c = None if c is None else _gpu(c.to(torch.float32), torch.float32, "c")
    call("ipdm_sample_axpy2_f32", _ptr(x), _ptr(y), _ptr(z), _ptr(a), _ptr(c), _ptr(out), n,
         x.numel() // max(n, 1), _stream())
    _written(out)
    return out


def sample_norm(x):
    x = _gpu(x, torch.float32, "x")
    n = x.shape[0]
    norms = torch.empty(n, dtype=torch.float32, device=x.device)
    call("ipdm_sample_norm_f32", _ptr(x), _ptr(norms), n, x.numel() // max(n, 1), _stream())
    return norms


# ---- convolution ------------------------------------------------------------------------------
def conv_pack_weight(w):
    """[Cout, Cin, k, k] -> [k*k, Cin, Cout]; a 5-D [Cout, Cin, 3, 3, 3] kernel -> [27, Cin, Cout]"""
    w = _gpu(w, torch.float32, "weight")
    if w.dim() == 5:
        Cout, Cin = w.shape[:2]
        kk = w.shape[2] * w.shape[3] * w.shape[4]
        if kk not in (1, 27):
            raise ValueError("3-D kernels must be 1x1x1 or 3x3x3")
        wt = torch.empty((kk, Cin, Cout), dtype=torch.float32, device=w.device)
        call("ipdm_conv_pack_weight_f32", _ptr(w), _ptr(wt), Cout, Cin, 27 if kk == 27 else 1, _stream())
        return wt
    Cout, Cin, k, k2 = w.shape
    assert k == k2
    wt = torch.empty((k * k, Cin, Cout), dtype=torch.float32, device=w.device)
    call("ipdm_conv_pack_weight_f32", _ptr(w), _ptr(wt), Cout, Cin, k, _stream())
    return wt


def conv_wino_weight(w):
    """[Cout, Cin, 3, 3] -> Winograd-domain weights U = G g G^T, [16, Cin, Cout]"""
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin = w.shape[:2]
    U = torch.empty((16, Cin, Cout), dtype=torch.float32, device=w.device)
    call("ipdm_conv_wino_weight_f32", _ptr(w), _ptr(U), Cout, Cin, _stream())
    return U


def conv_wino_supported(Cin, Cout, H, W, dilation=1):
    return bool(_lib.lib.ipdm_conv2d_wino_supported(Cin, Cout, H, W, dilation))


def _wino_residual(residual):
    """residual of a Winograd launch (2-D and 1-D kernels): their epilogues fetch it as pairs of columns, so it must start on
    an 8-byte boundary.  A contiguous view at 4 bytes past one (a legal argument) is COPIED to a fresh tensor here -- a read-only
    operand, the copy is never written -- so the same kernel runs and the result's bits do not depend on where the caller's
    residual happened to lie; the native entries answer such a pointer with IPDM_EUNSUPPORTED."""
    if residual is None:
        return None
    residual = _gpu(residual, torch.float32, "residual")
    return residual.clone() if residual.data_ptr() % 8 else residual


# The frame the convolution wrappers share: _conv_outputs (the output pair and its maxima slots), _need_both (res_second),
# _trace_open / _conv_done (the CONV_TRACE bracket, the maxima tags and the return convention), _chunks (the batch loop).
def _conv_outputs(x, shape, raw, act_out, who=None, out=None, want_amax=False, amax_cap=65535):
    """-> (out, out_act, slot_o, slot_a): the raw result (raw; the caller's `out=` where given) and the activated copy (act_out),
    fresh float32 tensors of `shape`, and -- want_amax -- a zeroed maxima vector for each of the two that exists (out's first: the
    arena hands slots out in sequence).  who: the wrapper's name where it refuses raw=False without act_out itself.
    amax_cap: batches above it get no maxima (the kernels' grid limit); conv1d passes None -- it has no cap"""
    want_act = act_out != ACT_NONE
    if who and not raw and not want_act:
        raise ValueError(f"{who}: raw=False needs act_out")
    B = x.shape[0]
    want_amax = (bool(want_amax) and (amax_cap is None or B <= amax_cap) and os.environ.get("IPDM_AMAX_PRODUCE", "1") != "0")
    slot_o = amax_slot(B, x.device) if want_amax and raw else None
    slot_a = amax_slot(B, x.device) if want_amax and want_act else None
    if not raw:
        out = None
    elif out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    out_act = torch.empty(shape, dtype=torch.float32, device=x.device) if want_act else None
    return out, out_act, slot_o, slot_a


def _need_both(who, res_second, residual, act_out, raw, how=" (act_out, e.g. ACT_COPY; raw=True)"):
    if res_second and (residual is None or act_out == ACT_NONE or not raw):
        raise ValueError(f"{who}: res_second needs a residual and both outputs{how}")


def _trace_open():
    """-> the recorded start event of this call's CONV_TRACE record (None: no census is running)"""
    if CONV_TRACE is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _conv_done(e0, out, out_act, slot_o=None, slot_a=None, **record):
    """the tail of a wrapper: closes the CONV_TRACE bracket (`record`: the shape keys of the census), hangs the maxima on the
    results and returns them as every wrapper does -- out, or (out, out_act) where an activated copy was asked for"""
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        CONV_TRACE.append(dict(record, n_out=int(out is not None) + int(out_act is not None), e0=e0, e1=e1))
    tag_amax(out, slot_o)
    tag_amax(out_act, slot_a)
    return out if out_act is None else (out, out_act)


def _chunks(B, nb):
    """the batch loop of the kernels with 32-bit buffer offsets: B images as launches of nb at most -> per launch (its images,
    cut), where cut(t) is that launch's slice t[b0:b1] of a per-image operand (None stays None)"""
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        yield b1 - b0, lambda t: None if t is None else t[b0:b1]


def conv2d_wino(x, U, bias=None, residual=None, act_out=ACT_NONE, raw=True, dilation=1):
    """3x3 / dilation-1 convolution through the Winograd F(2x2,3x3) kernel (same output options as conv2d).
    A residual that does not start on an 8-byte boundary is copied first (_wino_residual: the epilogue fetches pairs)."""
    x = _gpu(x, torch.float32, "x")
    residual = _wino_residual(residual)
    B, Cin, H, W = x.shape
    Cout = U.shape[2]
    out, out_act, _, _ = _conv_outputs(x, (B, Cout, H, W), raw, act_out)
    e0 = _trace_open()
    call("ipdm_conv2d_wino_f32", _ptr(x), _ptr(U), _ptr(bias), _ptr(residual), _ptr(out), _ptr(out_act), act_out,
         B, Cin, Cout, H, W, dilation, _stream())
    return _conv_done(e0, out, out_act, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=3, dil=dilation, wino=True, res=residual is not None)


def conv3d(x, wt, bias=None, coef=None, act=ACT_NONE, residual=None, dilation=1, act_out=ACT_NONE, raw=True, in_amax=None,
           want_amax=False, res_second=False):
    """x [B,Cin,D,H,W]; wt packed [27 or 1, Cin, Cout]; same fused input/output options as conv2d"""
    if isinstance(wt, PackedBx3) and wt.kk == 36:                # conv_wino1d_weight3d: the 1-D Winograd kernel's volume form
        if coef is not None or act != ACT_NONE or dilation != 1:
            raise ValueError("conv3d: the 1-D Winograd blob serves undilated launches without a fused input")
        return conv3d_wino1d(x, wt, bias, residual, act_out=act_out, raw=raw, in_amax=in_amax, want_amax=want_amax,
                             res_second=res_second)
    if isinstance(wt, PackedBx3):
        return conv_bx3(x, wt, bias, coef, act, residual, dilation, act_out=act_out, raw=raw, in_amax=in_amax,
                        want_amax=want_amax, res_second=res_second)
    if res_second:
        raise _lib.IpdmUnsupported("conv3d: res_second exists on the split-operand kernels only")
    x = _gpu(x, torch.float32, "x")
    B, Cin, D, H, W = x.shape
    kk, Cin_w, Cout = wt.shape
    if Cin_w != Cin:
        raise ValueError(f"conv3d: weight Cin {Cin_w} != input Cin {Cin}")
    k = {1: 1, 27: 3}[kk]
    out, out_act, _, _ = _conv_outputs(x, (B, Cout, D, H, W), raw, act_out)
    e0 = _trace_open()
    call("ipdm_conv3d_f32", _ptr(x), _ptr(wt), _ptr(bias), _ptr(coef), act, _ptr(residual), _ptr(out), _ptr(out_act),
         act_out, B, Cin, Cout, D, H, W, k, dilation, _stream())
    return _conv_done(e0, out, out_act, B=B * D, Cin=Cin, Cout=Cout, H=H, W=W, k=k, dil=dilation, taps3d=kk, res=residual is not None)


def maxpool3d5(x):
    x = _gpu(x, torch.float32, "x")
    B, C, D, H, W = x.shape
    out = torch.empty_like(x)
    call("ipdm_maxpool3d5_f32", _ptr(x), _ptr(out), B * C, D, H, W, _stream())
    return carry_amax(x, out)


def temporal_taps(x, mode):
    """x [B,C,D,H,T] -> [B,4C,D,H,T'] (mode 0: T' = T/2 strided-conv taps; mode 1: T' = 2T transposed-conv taps)"""
    x = _gpu(x, torch.float32, "x")
    B, C, D, H, T = x.shape
    T_out = T // 2 if mode == 0 else T * 2
    out = torch.empty((B, 4 * C, D, H, T_out), dtype=torch.float32, device=x.device)
    call("ipdm_temporal_taps_f32", _ptr(x), _ptr(out), B * C, D * H, T, T_out, mode, _stream())
    return carry_amax(x, out)


def conv2d(x, wt, bias=None, coef=None, act=ACT_NONE, residual=None, dilation=1, pool2=False, out=None,
           act_out=ACT_NONE, raw=True, in_amax=None, out_scale=1.0, want_amax=False, res_second=False):
    """x [B,Cin,H,W]; wt packed [k*k,Cin,Cout].  Input side: optional InstanceNorm++ coefficients / activation.
    Output side: bias, residual add; act_out != NONE additionally returns the activated copy act_out(result)
    (raw=False: ONLY the activated copy is produced).  Returns out, or (out, out_act) when act_out is set
    (out is None when raw=False)."""
    if isinstance(wt, PackedBx3):
        if pool2:
            raise _lib.IpdmUnsupported("conv2d: pool2 epilogue is not fused")
        return conv_bx3(x, wt, bias, coef, act, residual, dilation, out=out, act_out=act_out, raw=raw, in_amax=in_amax,
                        out_scale=out_scale, want_amax=want_amax, res_second=res_second)
    if out_scale != 1.0 or (bias is not None and bias.dim() == 2) or res_second:
        raise _lib.IpdmUnsupported("conv2d: per-image bias / out_scale exist on the split-operand kernels only")
    x = _gpu(x, torch.float32, "x")
    B, Cin, H, W = x.shape
    kk, Cin_w, Cout = wt.shape
    if Cin_w != Cin:
        raise ValueError(f"conv2d: weight Cin {Cin_w} != input Cin {Cin}")
    k = {1: 1, 9: 3}[kk]
    oh, ow = (H // 2, W // 2) if pool2 else (H, W)
    out, out_act, _, _ = _conv_outputs(x, (B, Cout, oh, ow), raw, act_out, "conv2d", out)
    e0 = _trace_open()
    call("ipdm_conv2d_f32", _ptr(x), _ptr(wt), _ptr(bias), _ptr(coef), act, _ptr(residual), _ptr(out), _ptr(out_act),
         act_out, B, Cin, Cout, H, W, k, dilation, int(bool(pool2)), _stream())
    _written(out)
    return _conv_done(e0, out, out_act, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=k, dil=dilation, res=residual is not None)


USE_THIN_CONV = os.environ.get("IPDM_THIN_CONV", "1") != "0"


def conv3x3_thin_ok(Cin, Cout, H, W, x=None):
    """3x3, dilation 1, no fused input norm / residual / second output, and a thin side: the streaming kernels.
    x: the tensor the layer is about to read -- the kernels move float4 rows, so an input off a 16-byte boundary (a contiguous
    view into a larger buffer) is not theirs; the caller's next branch (the matrix-core kernels) takes it"""
    if x is not None and x.data_ptr() % 16:
        return False
    return USE_THIN_CONV and bool(_lib.lib.ipdm_conv3x3_thin_supported(int(Cin), int(Cout), int(H), int(W)))


# the streaming layers leave nothing for a second pass (IPDM_THIN_STATS, IPDM_THIN_FIN; 0: the separate passes, launch for launch):
# the first layer hands its statistics partials to the InstanceNorm++ that reads it next, as the Winograd epilogues do ...
THIN_STATS = os.environ.get("IPDM_THIN_STATS", "1") != "0"
# ... and the last layer takes act(InstanceNorm++(x)) as (raw x, coefficients): no normalised tensor written and read back
THIN_FIN = os.environ.get("IPDM_THIN_FIN", "1") != "0"
# the network's last refine block is normalised next: its last convolution takes the statistics epilogue (IPDM_END_STATS)
END_STATS = os.environ.get("IPDM_END_STATS", "1") != "0"


def conv3x3_thin_stats_ok(Cin, Cout, H, W, x=None):
    """True where conv3x3_thin(want_stats=True) writes statistics partials (the few-input-channel form, IPDM_THIN_STATS)"""
    return (THIN_STATS and USE_STATS_EPILOGUE and conv3x3_thin_ok(Cin, Cout, H, W, x)
            and int(_lib.lib.ipdm_conv3x3_thin_stats_partials(int(Cin), int(Cout), int(H), int(W))) > 0)


def conv3x3_fewout_fin_ok(Cin, Cout, H, W, x, act=ACT_ELU):
    """True where conv3x3_fewout_fin takes the layer: a thin output side, ELU, 16-byte rows (IPDM_THIN_FIN; IPDM_THIN_CONV=0
    switches every streaming layer off, this one included)"""
    return (THIN_FIN and act == ACT_ELU and x.dim() == 4 and Cout <= 3 < Cin and conv3x3_thin_ok(Cin, Cout, H, W, x)
            and bool(_lib.lib.ipdm_conv3x3_fewout_fin_supported(int(Cin), int(Cout), int(H), int(W))))


def conv3x3_fewout_fin(x, weight, bias, coef, act=ACT_ELU):
    """last layer of a score network on act(InstanceNorm++(x)): x [B,Cin,H,W] RAW, coef [B,Cin,3] from instnorm_plus_coef,
    weight [Cout,Cin,3,3], Cout <= 3.  The bits of conv3x3_thin(affine_act(x, coef, act), weight, bias) in one pass over x.
    Raises IpdmUnsupported outside conv3x3_fewout_fin_ok()."""
    x = _gpu(x, torch.float32, "x")
    weight = _gpu(weight, torch.float32, "weight")
    coef = _gpu(coef, torch.float32, "coef")
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, Cin, 3, 3):
        raise ValueError(f"conv3x3_fewout_fin: weight {tuple(weight.shape)} does not match input channels {Cin}")
    if tuple(coef.shape) != (B, Cin, 3):
        raise ValueError(f"conv3x3_fewout_fin: coef {tuple(coef.shape)} != {(B, Cin, 3)}")
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    e0 = _trace_open()
    call("ipdm_conv3x3_fewout_fin_f32", _ptr(x), _ptr(weight), _ptr(bias), _ptr(coef), act, _ptr(out), B, Cin, Cout, H, W, _stream())
    return _conv_done(e0, out, None, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=3, dil=1, res=False, thin=True, fin=True)


def conv3x3_thin(x, weight, bias=None, coef=None, want_stats=False):
    """first / last layer of a score network: x [B,Cin,H,W], weight [Cout,Cin,3,3] (the reference's layout), Cin <= 3 or
    Cout <= 3; coef [B,Cin,3]: input affine (x - c0) * c1 + c2 inside the image (Cin <= 3 form).
    want_stats: the result feeds an InstanceNorm++ -- where conv3x3_thin_stats_ok(), the statistics partials [B, Cout, P, 3] ride
    on it as `_ipdm_partials` (as conv2d_wino_bx3(want_stats=True)); the stored bits do not change.
    Raises IpdmUnsupported for a shape outside conv3x3_thin_ok() and for an x that is not 16-byte aligned."""
    x = _gpu(x, torch.float32, "x")
    weight = _gpu(weight, torch.float32, "weight")
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    if tuple(weight.shape) != (Cout, Cin, 3, 3):
        raise ValueError(f"conv3x3_thin: weight {tuple(weight.shape)} does not match input channels {Cin}")
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    e0 = _trace_open()
    if coef is not None:
        coef = _gpu(coef, torch.float32, "coef")
        if tuple(coef.shape) != (B, Cin, 3):
            raise ValueError(f"conv3x3_thin: coef {tuple(coef.shape)} != {(B, Cin, 3)}")
    if want_stats and conv3x3_thin_stats_ok(Cin, Cout, H, W, x):
        P = int(_lib.lib.ipdm_conv3x3_thin_stats_partials(Cin, Cout, H, W))
        part = torch.empty((B, Cout, P, 3), dtype=torch.float32, device=x.device)
        call("ipdm_conv3x3_thin_stats_f32", _ptr(x), _ptr(weight), _ptr(bias), _ptr(coef), _ptr(out), _ptr(part), B, Cin, Cout, H, W,
             _stream())
        out._ipdm_partials = (part, (out._version, out.data_ptr()))
        return _conv_done(e0, out, None, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=3, dil=1, res=False, thin=True, stats=True)
    call("ipdm_conv3x3_thin_f32", _ptr(x), _ptr(weight), _ptr(bias), _ptr(coef), _ptr(out), B, Cin, Cout, H, W, _stream())
    return _conv_done(e0, out, None, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=3, dil=1, res=False, thin=True)


# ---- fp32 convolution on the 16-bit matrix cores (exactly split operands) ---------------------------------------
# Which kernel family the modules use (conv_weight()):
#   "hx2" (default): operands as two fp16 pieces, three fp16 MFMAs per product (csrc/conv_kernel.h) -- fp32-faithful
#                    for |activation| < 65504, NaN (never a wrong finite value) beyond
#   "bx3":           operands as three bf16 pieces, six bf16 MFMAs per product -- the whole fp32 exponent range
#   "f32":           the fp32-MFMA direct kernel + fp32 Winograd (conv.hip / conv_wino.hip)
CONV_IMPL = os.environ.get("IPDM_CONV_IMPL", "hx2")
SPLIT_IMPLS = ("hx2", "bx3")
if CONV_IMPL not in SPLIT_IMPLS + ("f32",):
    raise ValueError(f"IPDM_CONV_IMPL={CONV_IMPL!r}: expected 'hx2', 'bx3' or 'f32'")


def split_impl():
    """True when the modules run the split-operand kernels (conv_bx3.hip / conv_wino_bx3.hip)"""
    return CONV_IMPL in SPLIT_IMPLS


def impl_unbounded():
    """kernel family for networks whose convolution inputs are NOT bounded by a per-plane normalisation (NCSN++: GroupNorm'ed
    blocks but raw progressive / skip streams -- 1.7e5 in the full-size golden forward g22): the f16x2 family's STATIC range
    contract (|x| < 65504) does not hold there; these networks run it with the DYNAMIC range instead (`unbounded_amax()`:
    one ipdm_absmax_f32 pass per convolution input, every image scaled into fp16's range by an exact power of two).
    IPDM_CONV_IMPL_UNBOUNDED overrides the family (e.g. bx3: three bf16 pieces, the whole fp32 exponent range, no extra pass)."""
    env = os.environ.get("IPDM_CONV_IMPL_UNBOUNDED")
    if env:
        if env not in SPLIT_IMPLS + ("f32",):
            raise ValueError(f"IPDM_CONV_IMPL_UNBOUNDED={env!r}")
        return env
    return CONV_IMPL


def unbounded_amax():
    """the `in_amax` argument those networks pass to their convolutions: True (measure the input) on the f16x2 family"""
    return True if impl_unbounded() == "hx2" else None


class PackedWeightCache:
    """Packed copies of ONE parameter, one entry per (kernel family, layout), each tagged with the parameter's
    (version counter, storage pointer, device).  In-place optimiser steps and `copy_` on the parameter bump the version;
    a write through `.data` (the reference's EMA swap, helpers/utils.py:161-170) does not: modules clear the cache in
    their load_state_dict hook, and anything else that writes `.data` must call the module's invalidate()."""

    def __init__(self):
        self._entries = {}

    def clear(self):
        self._entries.clear()

    def get(self, weight, kind, build):
        tag = (weight._version, weight.data_ptr(), str(weight.device))
        hit = self._entries.get(kind)
        if hit is None or hit[0] != tag:
            hit = (tag, build(weight.data))
            self._entries[kind] = hit
        return hit[1]


class PackedWeightMixin:
    """for conv modules holding `self.weight`: `self._cache` + invalidate() + the load_state_dict hook"""

    def invalidate(self):
        self._cache.clear()

    def _load_from_state_dict(self, *args, **kwargs):
        self._cache.clear()
        return super()._load_from_state_dict(*args, **kwargs)


def conv_weight(w, impl=None):
    """pack a convolution weight for the selected kernel family (impl: override CONV_IMPL); pass the result to conv2d / conv3d"""
    impl = CONV_IMPL if impl is None else impl
    return conv_bx3_weight(w, fmt=impl) if impl in SPLIT_IMPLS else conv_pack_weight(w)


class PackedBx3:
    """weights split into 16-bit pieces and laid out as MFMA A-fragments: fmt "bx3" = three bf16 pieces
    (ipdm_conv_bx3_pack_weight), "hx2" = two fp16 pieces + per-output-channel inverse scales (ipdm_conv_hx2_pack_weight)"""
    __slots__ = ("blob", "Cout", "Cin", "kk", "fmt")

    def __init__(self, blob, Cout, Cin, kk, fmt="bx3"):
        self.blob, self.Cout, self.Cin, self.kk, self.fmt = blob, Cout, Cin, kk, fmt


def absmax_per_image(x):
    """per-image max |x| of an activation tensor as a maxima vector (float32 [B, AMAX_SLOT]; amax_value() -> [B]): the `in_amax`
    of the f16x2 convolutions' dynamic range where no producer handed the maxima over"""
    x = _gpu(x, torch.float32, "x")
    B = x.shape[0]
    out = torch.empty((B, AMAX_SLOT), dtype=torch.float32, device=x.device)
    call("ipdm_absmax_f32", _ptr(x), _ptr(out), B, x.numel() // max(B, 1), _stream())
    return out


def _conv_ext(fmt, in_amax, x, fused_input, bias_per_image=False, out_scale=1.0, Cout=0, out_amax=None, act_amax=None,
              res_second=False):
    """-> the `ext` argument of the split-operand entry points (NULL when every extra is at its default).
    in_amax (hx2 blobs only): None -> static range contract; True -> measure the input here; a tensor -> as given (a fused input
    normalisation / activation makes the raw maximum meaningless: ignored).  bias_per_image: bias is [B, Cout].  out_scale:
    result = (conv + bias + residual) * out_scale.  out_amax / act_amax: zeroed maxima vectors for what is stored.  res_second:
    the residual enters the second output only (out = conv + bias, out_act = act_out(conv + bias + residual))."""
    amax_ptr = None
    if fmt == "hx2" and in_amax is not None and not fused_input:
        if in_amax is True:
            in_amax = absmax_per_image(x)
        if (tuple(in_amax.shape) != (x.shape[0], AMAX_SLOT) or in_amax.dtype != torch.float32 or not in_amax.is_cuda
                or not in_amax.is_contiguous()):
            raise ValueError(f"in_amax: expected a maxima vector -- contiguous float32 GPU tensor [{x.shape[0]}, {AMAX_SLOT}] "
                             "(ops.absmax_per_image / a producer's tag)")
        amax_ptr = in_amax.data_ptr()
        _KEEP.append(in_amax)                    # (the kernel reads it asynchronously: keep the tensor alive until the call returns)
    if (amax_ptr is None and not bias_per_image and out_scale == 1.0 and out_amax is None and act_amax is None
            and not res_second):
        return P(0)
    ext = _lib.ConvExt(amax_ptr, int(Cout) if bias_per_image else 0, float(out_scale), int(bool(res_second)),
                       None if out_amax is None else out_amax.data_ptr(), None if act_amax is None else act_amax.data_ptr())
    _KEEP.append(ext)
    del _KEEP[:-8]
    return ctypes.byref(ext)


_KEEP = []                                       # last few ext structs / amax tensors (host structs are read during the call)


def conv_hx2_weight(w):
    return conv_bx3_weight(w, fmt="hx2")


def conv_bx3_weight(w, fmt="bx3"):
    """[Cout, Cin, k, k] (k = 1 or 3) or [Cout, Cin, 3, 3, 3] / [Cout, Cin, 1, 1, 1] -> PackedBx3"""
    if fmt not in SPLIT_IMPLS:
        raise ValueError(f"conv_bx3_weight: fmt {fmt!r}")
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin = w.shape[:2]
    kk = 1
    for n in w.shape[2:]:
        kk *= int(n)
    if w.dim() == 5:
        if kk not in (1, 27):
            raise ValueError("3-D kernels must be 1x1x1 or 3x3x3")
        k = 27 if kk == 27 else 1
    else:
        k = {1: 1, 9: 3}[kk]
    nbytes = getattr(_lib.lib, f"ipdm_conv_{fmt}_weight_bytes")(Cout, Cin, k)
    blob = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    call(f"ipdm_conv_{fmt}_pack_weight", _ptr(w), _ptr(blob), Cout, Cin, k, _stream())
    return PackedBx3(blob, Cout, Cin, kk, fmt)


def conv_bx3(x, wq, bias=None, coef=None, act=ACT_NONE, residual=None, dilation=1, out=None, act_out=ACT_NONE, raw=True,
             in_amax=None, out_scale=1.0, want_amax=False, res_second=False):
    """2-D ([B,Cin,H,W]) or 3-D ([B,Cin,D,H,W]) convolution, same options / return convention as conv2d / conv3d.
    res_second (needs residual, act_out (ACT_COPY = none) and raw): -> (conv + bias, act_out(conv + bias + residual)).
    in_amax (hx2 blobs only): None = static range contract |x| < 65504, True = measure the input (ipdm_absmax_f32) and scale every
    image into fp16's range, or the per-image maxima themselves"""
    x = _gpu(x, torch.float32, "x")
    bias_per_image = bias is not None and bias.dim() == 2
    if bias_per_image and (tuple(bias.shape) != (x.shape[0], wq.Cout) or bias.stride(1) != 1):
        raise ValueError(f"conv_bx3: per-image bias {tuple(bias.shape)} != {(x.shape[0], wq.Cout)} (rows may be strided, not columns)")
    _need_both("conv_bx3", res_second, residual, act_out, raw)
    if wq.Cin != x.shape[1]:
        raise ValueError(f"conv_bx3: weight Cin {wq.Cin} != input Cin {x.shape[1]}")
    vol = x.dim() == 5
    k = {1: 1, 9: 3, 27: 3}[wq.kk]
    if (wq.kk == 27) != (vol and k == 3):
        raise ValueError("conv_bx3: kernel / input rank mismatch")
    shape = (x.shape[0], wq.Cout) + tuple(x.shape[2:])
    out, out_act, slot_o, slot_a = _conv_outputs(x, shape, raw, act_out, "conv_bx3", out, want_amax)
    ext = _conv_ext(wq.fmt, in_amax, x, coef is not None or act != ACT_NONE, bias_per_image, out_scale,
                    bias.stride(0) if bias_per_image else 0, slot_o, slot_a, res_second)
    e0 = _trace_open()
    if vol:
        B, Cin, D, H, W = x.shape
    else:
        B, Cin, H, W = x.shape
        D = 1
    ksplit = _lib.lib.ipdm_conv_bx3_splitk(B, D, Cin, wq.Cout, H, W, k, dilation) if B else 1
    if ksplit > 1:        # too few tiles to fill the chip: deal the K loop to several workgroups per tile
        work = torch.empty((ksplit,) + shape, dtype=torch.float32, device=x.device)
        call(f"ipdm_conv_{wq.fmt}_splitk_f32", _ptr(x), _ptr(wq.blob), _ptr(bias), _ptr(coef), act, _ptr(residual), _ptr(out),
             _ptr(out_act), act_out, B, Cin, wq.Cout, D, H, W, k, dilation, int(vol), ksplit, _ptr(work), ext, _stream())
    elif vol:
        call(f"ipdm_conv3d_{wq.fmt}_f32", _ptr(x), _ptr(wq.blob), _ptr(bias), _ptr(coef), act, _ptr(residual), _ptr(out),
             _ptr(out_act), act_out, B, Cin, wq.Cout, D, H, W, k, dilation, ext, _stream())
    else:
        call(f"ipdm_conv2d_{wq.fmt}_f32", _ptr(x), _ptr(wq.blob), _ptr(bias), _ptr(coef), act, _ptr(residual), _ptr(out),
             _ptr(out_act), act_out, B, Cin, wq.Cout, H, W, k, dilation, ext, _stream())
    _written(out)                                   # (a caller's `out=` tensor: whatever was cached on it is stale)
    return _conv_done(e0, out, out_act, slot_o, slot_a, B=B * D, Cin=Cin, Cout=wq.Cout, H=H, W=W, k=k, dil=dilation, bx3=True,
                      fmt=wq.fmt, res=residual is not None, taps3d=wq.kk if vol else None)


def conv_wino_bx3_weight(w, fmt="bx3"):
    """[Cout, Cin, 3, 3] -> Winograd-domain weights, split into 16-bit pieces in MFMA fragment order (PackedBx3, kk=16)"""
    if fmt not in SPLIT_IMPLS:
        raise ValueError(f"conv_wino_bx3_weight: fmt {fmt!r}")
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin = w.shape[:2]
    nbytes = getattr(_lib.lib, f"ipdm_conv_wino_{fmt}_weight_bytes")(Cout, Cin)
    blob = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    call(f"ipdm_conv_wino_{fmt}_pack_weight", _ptr(w), _ptr(blob), Cout, Cin, _stream())
    return PackedBx3(blob, Cout, Cin, 16, fmt)


def conv_wino_hx2_weight(w):
    return conv_wino_bx3_weight(w, fmt="hx2")


def conv_wino1d_weight(w):
    """[Cout, Cin, 3, 3] -> weights of the 1-D Winograd kernel (F(2,3) along x, the filter's rows as K; f16x2 pieces; PackedBx3, kk=12)"""
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin = w.shape[:2]
    blob = torch.empty(_lib.lib.ipdm_conv_wino1d_weight_bytes(Cout, Cin), dtype=torch.uint8, device=w.device)
    call("ipdm_conv_wino1d_pack_weight", _ptr(w), _ptr(blob), Cout, Cin, _stream())
    return PackedBx3(blob, Cout, Cin, 12, "hx2")


def conv_wino1d_pool_weight(w):
    """[Cout, Cin, 3, 3] -> weights of the 1-D Winograd kernel's folded ConvMeanPool form: the 2x2 mean's two rows summed into a
    4-row filter (16 positions; PackedBx3, kk=16, fmt "w1dp") -- for conv2d_wino_bx3(pool2=True) only"""
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"conv_wino1d_pool_weight: weight {tuple(w.shape)}")
    blob = torch.empty(_lib.lib.ipdm_conv_wino1d_pool_weight_bytes(Cout, Cin), dtype=torch.uint8, device=w.device)
    call("ipdm_conv_wino1d_pack_weight_pool", _ptr(w), _ptr(blob), Cout, Cin, _stream())
    return PackedBx3(blob, Cout, Cin, 16, "w1dp")


def conv_wino1d_weight3d(w):
    """[Cout, Cin, 3, 3, 3] -> weights of the 1-D Winograd kernel's volume form (36 positions: depth tap x filter row x position)"""
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"conv_wino1d_weight3d: weight {tuple(w.shape)}")
    blob = torch.empty(_lib.lib.ipdm_conv_wino1d_weight_bytes3d(Cout, Cin), dtype=torch.uint8, device=w.device)
    call("ipdm_conv_wino1d_pack_weight3d", _ptr(w), _ptr(blob), Cout, Cin, _stream())
    return PackedBx3(blob, Cout, Cin, 36, "hx2")


def conv3d_wino1d(x, U, bias=None, residual=None, act_out=ACT_NONE, raw=True, in_amax=None, want_amax=False, res_second=False):
    """3x3x3 'same' convolution of x [B, Cin, D, H, W] on the 1-D Winograd kernel (same output options as conv3d).
    A residual that does not start on an 8-byte boundary is copied first (_wino_residual: the epilogue fetches pairs)."""
    x = _gpu(x, torch.float32, "x")
    B, Cin, D, H, W = x.shape
    if U.kk != 36 or U.Cin != Cin:
        raise ValueError("conv3d_wino1d: weight blob does not match the input")
    _need_both("conv3d_wino1d", res_second, residual, act_out, raw, how="")
    Cout = U.Cout
    if residual is not None and tuple(residual.shape) != (B, Cout, D, H, W):
        raise ValueError(f"conv3d_wino1d: residual {tuple(residual.shape)} != output {(B, Cout, D, H, W)}")
    residual = _wino_residual(residual)
    amax_t = None
    if in_amax is not None:
        amax_t = absmax_per_image(x) if in_amax is True else in_amax
    out, out_act, slot_o, slot_a = _conv_outputs(x, (B, Cout, D, H, W), raw, act_out, want_amax=want_amax)
    e0 = _trace_open()
    nb = max(1, (0x3fffffff - 1) // (Cin * D * H * W * 4))       # images per launch inside the buffer descriptor's reach
    for n, cut in _chunks(B, nb):
        ext = _conv_ext("hx2", cut(amax_t), cut(x), False, False, 1.0, 0, cut(slot_o), cut(slot_a), res_second)
        call("ipdm_conv3d_wino1d_f32", _ptr(cut(x)), _ptr(U.blob), _ptr(bias), _ptr(cut(residual)), _ptr(cut(out)), _ptr(cut(out_act)),
             act_out, n, Cin, Cout, D, H, W, ext, _stream())
    return _conv_done(e0, out, out_act, slot_o, slot_a, B=B * D, Cin=Cin, Cout=Cout, H=H, W=W, k=3, dil=1, wino=True, bx3=True,
                      fmt="hx2", wino1d=True, res=residual is not None, taps3d=27)


def wino1d_vol_pays(Cin, Cout, D, H, W, dilation=1):
    """3x3x3 layers the 1-D Winograd kernel's volume form takes from the direct kernel (layer shape only)"""
    return (WINO1D and WINO1D_VOL and CONV_IMPL == "hx2" and dilation == 1
            and bool(_lib.lib.ipdm_conv3d_wino1d_supported(int(Cin), int(Cout), int(D), int(H), int(W))))


WINO1D_VOL = os.environ.get("IPDM_WINO1D_VOL", "1") != "0"          # 0: config 4's 3x3x3 layers stay on the direct kernel (A/B)
WINO1D = os.environ.get("IPDM_WINO1D", "1") != "0"          # 0: the 2-D Winograd kernel everywhere (A/B, fallback)
WINO1D_STATS = os.environ.get("IPDM_WINO1D_STATS", "1") != "0"      # the launches with a statistics epilogue too (tuning)
# InstanceNorm++ + ELU of the input inside the 1-D kernel's producer instead of the affine + activation pass: built, tested, and
# measured SLOWER on MI355X (17.24 -> 17.68 ms per iteration, same box: +1.1 ms of convolution for 0.8 ms of passes removed -- the
# exponentials and selects in a 256-register kernel cost more than 8 bytes per element at the HBM roof), so off by default
WINO1D_FIN = os.environ.get("IPDM_WINO1D_FIN", "0") != "0"
# ConvMeanPool on the 1-D kernel: the 2x2 mean's rows folded into a 4-row filter (conv_wino1d_pool_weight: 16 of the direct form's
# 36 multiply-adds instead of 24); 0: the 12-position blob and the epilogue that averages four convolution outputs
W1D_POOLFOLD = os.environ.get("IPDM_W1D_POOLFOLD", "1") != "0"
_POOL_FORM_OFFER = None


@contextlib.contextmanager
def offer_pool_form(get):
    """ConvMeanPool.fused's choice of the folded form: inside the block, a conv2d_wino_bx3(pool2=True) of a 12-position blob with a
    plain input launches the folded form on get()'s blob (Conv2d.packed_wino1d_pool) instead.  The offer travels beside the call,
    not in it: what the layer modules hand to this module, and what a 12-position blob hands to the native entry, are pinned
    (tests/golden/g39, g40) and stay as they are.  get = None: no offer."""
    global _POOL_FORM_OFFER
    prev, _POOL_FORM_OFFER = _POOL_FORM_OFFER, get
    try:
        yield
    finally:
        _POOL_FORM_OFFER = prev


def wino1d_pays(Cin, Cout, H, W, dilation=1):
    """layers the 1-D Winograd kernel takes from the 2-D one (a function of the layer SHAPE only): f16x2 family, undilated,
    at least 128 output channels in blocks of 128, rows of 32 pixels or more"""
    return (WINO1D and CONV_IMPL == "hx2" and dilation == 1
            and bool(_lib.lib.ipdm_conv2d_wino1d_supported(int(Cin), int(Cout), int(H), int(W))))


def conv_wino_split_weight(w, impl=None):
    """Winograd-domain weights for the selected split family (CONV_IMPL = "hx2" / "bx3")"""
    impl = CONV_IMPL if impl is None else impl
    return conv_wino_bx3_weight(w, fmt=impl if impl in SPLIT_IMPLS else "bx3")


def conv_wino_bx3_supported(Cin, Cout, H, W, dilation=1):
    return bool(_lib.lib.ipdm_conv2d_wino_bx3_supported(Cin, Cout, H, W, dilation))


def conv2d_wino_bx3(x, U, bias=None, residual=None, act_out=ACT_NONE, raw=True, dilation=1, pool2=False, want_stats=False,
                    in_amax=None, out_scale=1.0, want_amax=False, res_second=False, coef=None, act=ACT_NONE):
    """3x3 convolution through the split-bf16 Winograd kernel (same output options as conv2d).
    res_second (needs residual, act_out (ACT_COPY = none) and raw): -> (conv + bias, act_out(conv + bias + residual)).
    pool2: the ConvMeanPool form -- outputs (and the residual) are [B, Cout, H/2, W/2] 2x2 means of the convolution;
    raises IpdmUnsupported where the pooled epilogue is not built (small / odd images).  A conv_wino1d_pool_weight blob
    (fmt "w1dp") runs the 1-D kernel's folded pooled form and serves nothing else (ValueError without pool2 or with coef).
    want_stats: the result feeds an InstanceNorm++ -- where the statistics epilogue exists for this shape, its partials
    [B, Cout, P, 3] are hung on the raw result as `_ipdm_partials` (instnorm_plus_coef picks them up).
    x may be any contiguous tensor (off a 16-byte boundary: the dword-staged forms, no statistics epilogue, no split-K).
    A residual that does not start on an 8-byte boundary is copied first (_wino_residual: the epilogue fetches pairs)."""
    x = _gpu(x, torch.float32, "x")
    B, Cin, H, W = x.shape
    if _POOL_FORM_OFFER is not None and pool2 and U.kk == 12 and U.fmt == "hx2" and coef is None and act == ACT_NONE:
        offered = _POOL_FORM_OFFER()
        if (offered.fmt, offered.Cout, offered.Cin) != ("w1dp", U.Cout, U.Cin):
            raise ValueError("conv2d_wino_bx3: the offered pool form does not match the weight blob")
        U = offered
    fold = U.fmt == "w1dp"               # conv_wino1d_pool_weight: the 1-D kernel's folded pooled form, an f16x2 launch
    if fold and (not pool2 or U.kk != 16):
        raise ValueError("conv2d_wino_bx3: the folded pool blob (conv_wino1d_pool_weight) serves pool2=True launches only")
    fmt = "hx2" if fold else U.fmt
    amax_t = None
    if fmt == "hx2" and in_amax is not None:
        if in_amax is True and coef is not None:
            raise ValueError("conv2d_wino_bx3: with a fused input the maxima are the coefficient kernel's bound, not max |x|")
        amax_t = absmax_per_image(x) if in_amax is True else in_amax
    bias_per_image = bias is not None and bias.dim() == 2
    if bias_per_image and (tuple(bias.shape) != (B, U.Cout) or bias.stride(1) != 1):
        raise ValueError(f"conv2d_wino_bx3: per-image bias {tuple(bias.shape)} != {(B, U.Cout)} (rows may be strided, not columns)")
    one_d = U.kk == 12 or fold           # conv_wino1d_weight: 1-D Winograd along x (conv_wino1d.hip), plain epilogues only
    if U.kk not in (12, 16) or U.Cin != Cin:
        raise ValueError("conv2d_wino_bx3: weight blob does not match the input")
    if one_d and (dilation != 1 or fmt != "hx2"):
        raise ValueError("conv2d_wino_bx3: the 1-D Winograd blob serves undilated f16x2 launches only")
    if coef is not None or act != ACT_NONE:
        # fused input act(InstanceNorm++(x)) (coef from instnorm_plus_coef): the 1-D kernel's producer applies it to the raw rows
        if not one_d or fold or coef is None or act != ACT_ELU:
            raise ValueError("conv2d_wino_bx3: a fused input (coef + ACT_ELU) is the 1-D Winograd kernel's only (12-position blob)")
        coef = _gpu(coef, torch.float32, "coef")
        if tuple(coef.shape) != (B, Cin, 3):
            raise ValueError(f"conv2d_wino_bx3: coef {tuple(coef.shape)} != {(B, Cin, 3)}")
    _need_both("conv2d_wino_bx3", res_second, residual, act_out, raw)
    Cout = U.Cout
    oh, ow = (H // 2, W // 2) if pool2 else (H, W)
    if residual is not None and tuple(residual.shape) != (B, Cout, oh, ow):
        raise ValueError(f"conv2d_wino_bx3: residual {tuple(residual.shape)} != output {(B, Cout, oh, ow)}")
    residual = _wino_residual(residual)
    out, out_act, slot_o, slot_a = _conv_outputs(x, (B, Cout, oh, ow), raw, act_out, want_amax=want_amax)
    e0 = _trace_open()
    nb = wino_bx3_max_batch(Cin, H, W, dilation)
    # 16-pixel layers with few channel tiles: two K halves + a fixed-order reduction
    ksplit = 1 if one_d or pool2 or x.data_ptr() % 16 or (WBX3_CO32 and fmt == "hx2") else wino_bx3_splitk(Cin, Cout, H, W, dilation)
    part = None
    if ksplit == 1 and want_stats and raw and USE_STATS_EPILOGUE and x.data_ptr() % 16 == 0:
        P = (int(_lib.lib.ipdm_conv2d_wino1d_stats_partials(Cin, Cout, H, W)) if one_d else
             int(_lib.lib.ipdm_conv2d_wino_bx3_stats_partials(Cin, Cout, H, W, dilation, int(bool(pool2)))))
        if P > 0:
            part = torch.empty((B, Cout, P, 3), dtype=torch.float32, device=x.device)
    for n, cut in _chunks(B, nb):        # one launch unless the batch outgrows the kernel's 32-bit buffer offsets
        head = (_ptr(cut(x)), _ptr(U.blob), _ptr(cut(bias) if bias_per_image else bias))
        outs = (_ptr(cut(residual)), _ptr(cut(out)), _ptr(cut(out_act)), act_out, n, Cin, Cout, H, W)
        ext = _conv_ext(fmt, cut(amax_t), cut(x), False, bias_per_image, out_scale, bias.stride(0) if bias_per_image else 0,
                        cut(slot_o), cut(slot_a), res_second)
        if ksplit > 1:
            work = torch.empty((ksplit, n, Cout, H, W), dtype=torch.float32, device=x.device)
            call(f"ipdm_conv2d_wino_{U.fmt}_splitk_f32", *head, *outs, dilation, ksplit, _ptr(work), ext, _stream())
        elif one_d:                      # (+ fused input, no dilation)
            stats = () if part is None else (_ptr(cut(part)),)
            call("ipdm_conv2d_wino1d_f32" if part is None else "ipdm_conv2d_wino1d_stats_f32", *head, _ptr(cut(coef)), act, *outs,
                 2 if fold else int(bool(pool2)), *stats, ext, _stream())
        else:
            args = head + outs + (dilation, int(bool(pool2)))
            if part is not None:
                try:
                    call(f"ipdm_conv2d_wino_{U.fmt}_stats_f32", *args, _ptr(cut(part)), ext, _stream())
                    continue
                except _lib.IpdmUnsupported:         # e.g. IPDM_WBX3_DMA4=0: no statistics epilogue on that kernel form
                    part = None
            call(f"ipdm_conv2d_wino_{U.fmt}_f32", *args, ext, _stream())
    if part is not None:
        out._ipdm_partials = (part, (out._version, out.data_ptr()))
    # (the folded form executes 16 / 36 of the direct multiply-adds, the 2-D Winograd factor: counted as `wino`, not `wino1d`)
    form = dict(pool2=False, ksplit=ksplit) if ksplit > 1 else dict(pool2=bool(pool2), wino1d=one_d and not fold, stats=part is not None)
    if fold:
        form["w1d_fold"] = True
    return _conv_done(e0, out, out_act, slot_o, slot_a, B=B, Cin=Cin, Cout=Cout, H=H, W=W, k=3, dil=dilation, wino=True, bx3=True,
                      fmt=fmt, res=residual is not None, **form)


# f16x2 family: the 16-pixel layers whose split-K rule says "two K halves" run as ONE launch of 32-channel workgroups instead
# (conv_wino_bx3.hip: CO32, and for 16 x 16 images HALF -- the native launcher's choice, ops.wino_hx2_form; -0.35 % per iteration and
# 28 reduction launches fewer; 0: the split-K form)
WBX3_CO32 = os.environ.get("IPDM_WBX3_CO32", "1") != "0"


def wino_bx3_pays(Cin, Cout, H, W, dilation=1, B=None):
    """dispatch rule measured on MI355X (scripts/bench_conv.py): the split-bf16 Winograd kernel beats the direct
    split-bf16 kernel wherever it is eligible, except on undilated images of 16 pixels or less with fewer than 512
    output channels (one 8x8-tile workgroup per (image, channel tile): at the production batch only the 512-channel
    layers fill the chip; with 256 channels the direct kernel's finer tiles tie).
    The rule depends on the LAYER SHAPE ONLY -- never on the batch -- so that a sample's bits do not depend on how many
    other samples share its GPU (sharding.py's invariance; `B` is accepted and ignored for old call sites)."""
    if W <= 16 and dilation == 1:
        if wino_bx3_splitk(Cin, Cout, H, W, dilation) > 1:      # ... unless the layer runs as two K halves (shape rule too)
            return True
        if H > 16 or Cout < 512 or Cin < 32:
            return False
    return conv_wino_bx3_supported(Cin, Cout, H, W, dilation)


def wino_bx3_splitk(Cin, Cout, H, W, dilation=1):
    """K parts of the Winograd launch for this layer shape (1 = plain launch); never a function of the batch"""
    return int(_lib.lib.ipdm_conv2d_wino_bx3_splitk(int(Cin), int(Cout), int(H), int(W), int(dilation)))


WINO_FORM_OTHER, WINO_FORM_CO32, WINO_FORM_HALF, WINO_FORM_POLY = 0, 1, 2, 3      # include/ipdm.h IPDM_WINO_FORM_*


def wino_hx2_form(Cin, Cout, H, W, dilation=1):
    """the instantiation the f16x2 family's plain Winograd call runs for this layer shape (WINO_FORM_*; the native rule, a
    function of the shape only); None where the kernel does not apply"""
    f = int(_lib.lib.ipdm_conv2d_wino_hx2_form(int(Cin), int(Cout), int(H), int(W), int(dilation)))
    return None if f < 0 else f


def wino_bx3_max_batch(Cin, H, W, dilation=1):
    """images per launch the Winograd kernel's 32-bit buffer offsets reach (larger batches run as several launches)"""
    reach = 0x1fffffff if (W < 32 or dilation > 1) else 0x3fffffff
    return max(1, (reach - 1) // (Cin * H * W * 4))


def adam_ascent(x, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """one torch.optim.Adam step in place on x with param.grad = -g (x, g, m, v: same-shaped float32 GPU tensors)"""
    for t, n in ((x, "x"), (g, "g"), (m, "m"), (v, "v")):
        _inplace_operand(t, torch.float32, n)
        if t.numel() != x.numel():
            raise ValueError(f"adam_ascent: {n} does not match x")
    call("ipdm_adam_ascent_f32", _ptr(x), _ptr(g), _ptr(m), _ptr(v), x.numel(), float(lr), float(betas[0]), float(betas[1]),
         float(eps), int(step), _stream())
    _written(x, m, v)
    return x


# ---- 1-D convolution of (N, C, L) sequences: the temporal score networks NCSN1D* (csrc/conv1d.hip) --------------------------
# The f16x2 arithmetic of the direct kernels on a GEMM whose columns are the flattened (sequence, t) positions: K = k * Cin with no
# dead taps, whole sequences per column tile, one power-of-two input scale per SEQUENCE (the maxima vectors have one slot per
# sequence here).  Dispatch is a function of the layer shape only (conv1d_pays): every other 1-D convolution -- few channels,
# lengths that do not divide 96, other kernel families, IPDM_CONV1D=0 -- runs as the one-row image (N, C, 1, L) on the direct 2-D
# kernel with the filter in the middle row of a 3 x 3 one, which is the same convolution (conv1d_rows).
USE_CONV1D = os.environ.get("IPDM_CONV1D", "1") != "0"
CONV1D_LAUNCHES = 0                              # launches of the 1-D kernel since import (diagnostics / tests)
CONV1D_FALLBACKS = 0                             # 1-D convolutions that ran as one-row images on the 2-D kernels


def conv1d_pays(Cin, Cout, L, k, dilation=1):
    """True when the 1-D kernel takes a layer of this shape (a rule of the shape and of IPDM_CONV1D / IPDM_CONV_IMPL alone).
    Measured on the MI355X at N = 512 (profiles/ncsn1d_ab.txt): 1.4x to 5.8x faster than the one-row form per launch on every
    census shape, none slower -- so every served shape takes the kernel."""
    return (USE_CONV1D and CONV_IMPL == "hx2"
            and bool(_lib.lib.ipdm_conv1d_hx2_supported(int(Cin), int(Cout), int(L), int(k), int(dilation))))


# ---- which kernel runs a layer ------------------------------------------------------------------------------------------------
ROUTE_THIN, ROUTE_WINO_F32, ROUTE_WINO1D, ROUTE_WINO_SPLIT = "thin", "wino_f32", "wino1d", "wino_split"
ROUTE_WINO1D_VOL, ROUTE_SEQ, ROUTE_ROWS, ROUTE_DIRECT2D, ROUTE_DIRECT3D = "wino1d_vol", "conv1d", "rows", "direct2d", "direct3d"


def conv_route(site, ndim, k, dilation, Cin, Cout, size, aligned, impl, winograd=True, fuse_pool=True, full_range=False,
               coef=False, coef_bound=False, act=ACT_NONE, residual=False, out=False, act_out=ACT_NONE, raw=True, want_stats=False):
    """-> the ROUTE_* of one layer call; None: "no fused pooled launch" (site "pool" only).  The ONE place that decides: the
    modules ask, switch on the answer and forward their arguments.  Pure host code, no tensor: size = x.shape[2:], aligned = x
    starts on a 16-byte boundary, coef / residual / out = "one is given", coef_bound = the coefficients carry their bound
    (`_ipdm_amax_bound`).  The switches of this module are read at call time.  The sites differ, on purpose or not:
    site: "ncsn" = Conv2d.forward, "pool" = ConvMeanPool.fused (a pooled launch or None), "sde" = Conv.forward (score_sde networks)
    impl: the kernel family -- "ncsn" / "pool" pass CONV_IMPL, "sde" passes impl_unbounded(); wino1d_pays tests CONV_IMPL all the same
    winograd: "ncsn" / "pool" pass their USE_WINOGRAD; "sde" passes nothing (it does not consult the switch)
    fuse_pool: "pool" passes its FUSE_POOL; read by no other site
    coef / act / out / act_out / raw / full_range: "sde" has none of them and passes nothing; "pool" passes coef, act, act_out
    want_stats: gates the 1-D kernel at "ncsn" only; "pool" demands WINO1D_STATS outright, "sde" has no statistics gate"""
    plain_in = not coef and act == ACT_NONE
    if ndim == 1:
        seq = plain_in and not full_range and conv1d_pays(Cin, Cout, size[0], k, dilation)
        if site == "pool":
            return ROUTE_SEQ if fuse_pool and k == 3 and size[0] % 2 == 0 and seq else None
        return ROUTE_SEQ if seq else ROUTE_ROWS
    H, W = size[0], size[1]
    wino = winograd and impl in SPLIT_IMPLS and ndim == 2 and k == 3

    def one_d():                                         # the 1-D Winograd kernel instead of the 2-D one, statistics gate apart
        return (impl == "hx2" and aligned and act_out in (ACT_NONE, ACT_ELU, ACT_COPY) and wino1d_pays(Cin, Cout, H, W, dilation))
    if site == "pool":
        if not (fuse_pool and wino and dilation == 1 and H % 2 == 0 and W % 2 == 0 and wino_bx3_pays(Cin, Cout, H, W, 1)):
            return None
        if one_d() and WINO1D_STATS:
            return ROUTE_WINO1D                          # (with coef: the fused input -- whatever `act` says)
        return None if coef else ROUTE_WINO_SPLIT        # a fused input is the 1-D kernel's only; `act` alone is not looked at
    if (site == "ncsn" and coef and act == ACT_ELU and not out and WINO1D_FIN and wino and len(size) == 2 and aligned
            and (not dynamic_range(impl) or coef_bound) and wino1d_pays(Cin, Cout, H, W, dilation)):
        return ROUTE_WINO1D                              # act(InstanceNorm++(x)) as (raw x, coefficients): Conv2d.fuses_input
    if (ndim == 2 and k == 3 and dilation == 1 and act == ACT_NONE and not residual and not out and act_out == ACT_NONE and raw
            and len(size) == 2 and (Cin <= 3 or (Cout <= 3 and not coef)) and aligned and conv3x3_thin_ok(Cin, Cout, H, W)):
        return ROUTE_THIN                                # ("sde" writes min(Cin, Cout) <= 3: the same without a coef)
    if (site == "ncsn" and winograd and impl == "f32" and ndim == 2 and k == 3 and plain_in and not out
            and conv_wino_supported(Cin, Cout, H, W, dilation)):
        return ROUTE_WINO_F32
    if wino and plain_in and not out and wino_bx3_pays(Cin, Cout, H, W, dilation):
        stats_ok = site == "sde" or WINO1D_STATS or not (want_stats and raw and USE_STATS_EPILOGUE)
        return ROUTE_WINO1D if one_d() and stats_ok else ROUTE_WINO_SPLIT
    if (ndim == 3 and k == 3 and dilation == 1 and plain_in and not out and len(size) == 3 and aligned
            and act_out in (ACT_NONE, ACT_ELU, ACT_COPY) and wino1d_vol_pays(Cin, Cout, *size)):
        return ROUTE_WINO1D_VOL
    return ROUTE_DIRECT3D if ndim == 3 else ROUTE_DIRECT2D


class PackedConv1d:
    """[Cout, Cin, k] weights as f16x2 MFMA A-fragments + per-output-channel inverse scales (ipdm_conv1d_hx2_pack_weight)"""
    __slots__ = ("blob", "Cout", "Cin", "k")

    def __init__(self, blob, Cout, Cin, k):
        self.blob, self.Cout, self.Cin, self.k = blob, Cout, Cin, k


def conv1d_weight(w):
    """[Cout, Cin, k] (k = 1 or 3; Cin % 16 == 0, Cout % 32 == 0) -> PackedConv1d"""
    w = _gpu(w, torch.float32, "weight")
    if w.dim() != 3:
        raise ValueError(f"conv1d_weight: expected [Cout, Cin, k], got {tuple(w.shape)}")
    Cout, Cin, k = (int(v) for v in w.shape)
    nbytes = _lib.lib.ipdm_conv1d_hx2_weight_bytes(Cout, Cin, k)
    if nbytes < 0:
        raise _lib.IpdmUnsupported(f"conv1d_weight: no 1-D kernel for a [{Cout}, {Cin}, {k}] filter")
    blob = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    call("ipdm_conv1d_hx2_pack_weight", _ptr(w), _ptr(blob), Cout, Cin, k, _stream())
    return PackedConv1d(blob, Cout, Cin, k)


def conv1d_rows_weight(w, impl=None):
    """[Cout, Cin, k] -> the direct 2-D kernels' packed weight of the SAME convolution on one-row images: the filter in the
    middle row of a 3 x 3 one (k = 1: a 1 x 1 filter)"""
    w = _gpu(w, torch.float32, "weight")
    Cout, Cin, k = (int(v) for v in w.shape)
    if k == 1:
        return conv_weight(w.reshape(Cout, Cin, 1, 1), impl=impl)
    w2 = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float32, device=w.device)
    w2[:, :, 1, :] = w
    return conv_weight(w2, impl=impl)


def as_rows(x):
    """(N, C, L) -> the one-row image view (N, C, 1, L); the per-sequence maxima ride along"""
    return carry_amax(x, x.view(x.shape[0], x.shape[1], 1, x.shape[2]))


def as_seq(x):
    """(N, C, 1, L) -> (N, C, L), a view; the maxima ride along"""
    return carry_amax(x, x.view(x.shape[0], x.shape[1], x.shape[3]))


def conv1d_rows(x, wt, bias=None, coef=None, act=ACT_NONE, residual=None, dilation=1, act_out=ACT_NONE, raw=True, in_amax=None,
                want_amax=False, res_second=False):
    """the fallback / A-B arm: x (N, Cin, L) as one-row images on conv2d (wt from conv1d_rows_weight); conv2d's conventions"""
    global CONV1D_FALLBACKS
    CONV1D_FALLBACKS += 1
    x = _gpu(x, torch.float32, "x")
    res = None if residual is None else as_rows(_gpu(residual, torch.float32, "residual"))
    y = conv2d(as_rows(x), wt, bias, coef, act, res, dilation, act_out=act_out, raw=raw, in_amax=in_amax, want_amax=want_amax,
               res_second=res_second)
    if act_out != ACT_NONE:
        return (None if y[0] is None else as_seq(y[0])), as_seq(y[1])
    return as_seq(y)


def conv1d(x, wq, bias=None, residual=None, dilation=1, act_out=ACT_NONE, raw=True, in_amax=None, want_amax=False,
           res_second=False, pool2=False):
    """x (N, Cin, L) float32, wq a PackedConv1d.  Output side as conv2d: bias, residual, act_out != NONE additionally returns the
    activated copy (raw=False: only that one; ACT_COPY + res_second: (conv + bias, conv + bias + residual)).  pool2: the pair
    mean of ConvMeanPool -- results and residual are (N, Cout, L / 2).  in_amax: None (static range contract), True (measure) or
    a maxima vector with one slot per sequence; want_amax: the per-sequence maxima of what is stored ride on the results."""
    global CONV1D_LAUNCHES
    x = _gpu(x, torch.float32, "x")
    if x.dim() != 3 or x.shape[1] != wq.Cin:
        raise ValueError(f"conv1d: input {tuple(x.shape)} for a filter with Cin {wq.Cin}")
    N, Cin, L = (int(v) for v in x.shape)
    if pool2 and L % 2:
        raise ValueError("conv1d: the pair mean needs an even length")
    shape = (N, wq.Cout, L // 2 if pool2 else L)
    out, out_act, slot_o, slot_a = _conv_outputs(x, shape, raw, act_out, "conv1d", None, want_amax, amax_cap=None)
    _need_both("conv1d", res_second, residual, act_out, raw)
    if residual is not None:
        residual = _gpu(residual, torch.float32, "residual")
        if tuple(residual.shape) != shape:
            raise ValueError(f"conv1d: residual {tuple(residual.shape)} != {shape}")
    ext = _conv_ext("hx2", in_amax, x, False, False, 1.0, 0, slot_o, slot_a, res_second)
    e0 = _trace_open()
    call("ipdm_conv1d_hx2_f32", _ptr(x), _ptr(wq.blob), _ptr(bias), _ptr(residual), _ptr(out), _ptr(out_act), act_out, N, Cin,
         wq.Cout, L, wq.k, int(dilation), int(bool(pool2)), ext, _stream())
    CONV1D_LAUNCHES += 1
    return _conv_done(e0, out, out_act, slot_o, slot_a, B=N, Cin=Cin, Cout=wq.Cout, H=1, W=L, k=wq.k, dil=dilation, conv1d=True,
                      res=residual is not None)


def meanpool1d2(x):
    """(..., L) -> (..., L / 2): y[j] = (x[2j] + x[2j+1]) / 2 (ConvMeanPool's tail along one axis); the maxima ride along"""
    x = _gpu(x, torch.float32, "x")
    L = int(x.shape[-1])
    if L % 2:
        raise ValueError("meanpool1d2: the length must be even")
    out = torch.empty(tuple(x.shape[:-1]) + (L // 2,), dtype=torch.float32, device=x.device)
    call("ipdm_meanpool1d2_f32", _ptr(x), _ptr(out), x.numel() // L, L, _stream())
    return carry_amax(x, out)


def scale_shift_amax(x, a, b):
    """a * x + b whose per-image (dim 0) maxima ride on the result: the `2x - 1` in front of a score network's first convolution
    as a PRODUCER of that convolution's in_amax (no measuring pass)"""
    x = _gpu(x, torch.float32, "x")
    B = int(x.shape[0])
    out = torch.empty_like(x)
    slot = amax_slot(B, x.device)
    call("ipdm_scale_shift_amax_f32", _ptr(x), _ptr(out), _ptr(slot), B, x.numel() // max(B, 1), float(a), float(b), _stream())
    return tag_amax(out, slot)


def maxpool1d5(x):
    """MaxPool1d(5, 1, 2) of (N, C, L): the 5 x 5 max-pool on one-row images (its padding is -inf: the same maxima)"""
    return as_seq(maxpool5(as_rows(x)))


def linear1d(x, size, out=None, accumulate=False, act=ACT_NONE, want_amax=False):
    """F.interpolate(x, size, mode='linear', align_corners=True) of (N, C, L), optionally accumulated into out: the bilinear
    kernel on one-row images (its row ratio at 1 -> 1 is taken as 0)"""
    x = _gpu(x, torch.float32, "x")
    out4 = None if out is None else out.view(out.shape[0], out.shape[1], 1, out.shape[2])
    return as_seq(bilinear(as_rows(x), (1, int(size)), out=out4, accumulate=accumulate, act=act, want_amax=want_amax))
