"""Operators of the hot path as calls into libmdx.so on torch CUDA (ROCm) tensors.

torch is plumbing only: device memory, the current HIP stream, and (elsewhere)
torch.distributed.  Every function here hands raw device pointers to the C ABI
(include/mdx.h); nothing computes with torch ops and nothing falls back to the CPU.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import MDX_DIM_MAJOR, MDX_ROW_MAJOR, POOL_KINDS, check

_vp = ctypes.c_void_p


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """Handle of torch's current HIP stream (launches are enqueued there; nothing synchronises)."""
    if _raw_stream is not None:           # a few hundred ns instead of building a torch.cuda.Stream object
        return _vp(_raw_stream(torch.cuda.current_device()))
    return _vp(torch.cuda.current_stream().cuda_stream)


class _Here:
    """No-op context: the tensor's device is already the current one (the common case; a real
    ``torch.cuda.device`` guard costs a few microseconds per launch, and the trunk epilogue launches ~100 times per image)."""
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_HERE = _Here()


def _on(t):
    """Context in which ``t``'s device is current, so that ``_stream()`` and the launch use the device the pointers
    live on (a caller may pass ``device=cuda:1`` without ``set_device``; the reference's torch ops follow the tensor)."""
    idx = t.device.index
    if idx is None or idx == torch.cuda.current_device():
        return _HERE
    return torch.cuda.device(idx)


def _dev(t, dtype, what, contiguous=True):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA/ROCm tensor: the MI355X path has no CPU fallback" % what)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (what, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return _vp(t.data_ptr())


def _rows(t, what):
    """(pointer, row stride) of a 2-D fp32 CUDA matrix whose rows are contiguous (a row slice of a larger matrix is fine)."""
    p = _dev(t, torch.float32, what, contiguous=False)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
        raise ValueError("%s must be a 2-d matrix with contiguous rows" % what)
    return p, t.stride(0)


def _center(center, d, dtype=torch.float32):
    """Pointer of the optional ``center`` vector of ``d`` elements; None without one."""
    if center is None:
        return None
    cp = _dev(center, dtype, "center")
    if center.numel() != d:
        raise ValueError("center has %d elements, expected %d" % (center.numel(), d))
    return cp


def _layout(t, layout, what):
    """(n, d) of a 2-D descriptor matrix under the given layout name."""
    if t.dim() != 2:
        raise ValueError("%s must be 2-D" % what)
    if layout in ("DN", "dim_major", MDX_DIM_MAJOR):
        return t.shape[1], t.shape[0], MDX_DIM_MAJOR
    if layout in ("ND", "row_major", MDX_ROW_MAJOR):
        return t.shape[0], t.shape[1], MDX_ROW_MAJOR
    raise ValueError("unknown layout %r" % (layout,))


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ extraction

def pool_l2n(feat, kind="gem", p=3.0, pool_eps=1e-6, l2n_eps=1e-6):
    """[B,C,H,W] feature maps -> [B,C] pooled (+ L2-normalised unless l2n_eps is None).

    ``self.norm(self.pool(o))`` of cirtorch/networks/imageretrievalnet.py:108.  fp16 maps (the ``precision: f16`` trunk) go to
    ``mdx_pool_l2n_f16``: fp32 out, the bits of the fp32 call on ``feat.float()``."""
    if feat.dim() != 4:
        raise ValueError("feature map must be [B,C,H,W]")
    half = isinstance(feat, torch.Tensor) and feat.dtype == torch.float16
    fp = _dev(feat, torch.float16 if half else torch.float32, "feature map")
    B, C, H, W = feat.shape
    out = torch.empty((B, C), dtype=torch.float32, device=feat.device)
    fn, name = (_lib.lib().mdx_pool_l2n_f16, "mdx_pool_l2n_f16") if half else (_lib.lib().mdx_pool_l2n, "mdx_pool_l2n")
    with _on(feat):
        check(fn(fp, B, C, H, W, POOL_KINDS[kind], float(p), float(pool_eps), -1.0 if l2n_eps is None else float(l2n_eps),
                 _vp(out.data_ptr()), _stream()), name)
    return out


def rmac(feat, regions, eps=1e-6):
    """R-MAC pooling ``[B,C,H,W] -> [B,C]`` over the given regions (``[(row0, col0, height, width), ...]``, the whole map
    first): ``sum_r l2n(max over region r)`` -- ``LF.rmac`` (functional.py:26-72) through ``mdx_rmac``."""
    fp = _dev(feat, torch.float32, "feature map")
    if feat.dim() != 4:
        raise ValueError("feature map must be [B,C,H,W]")
    B, C, H, W = feat.shape
    n = len(regions)
    if not 1 <= n <= 64:
        raise ValueError("1..64 regions supported, got %d" % n)
    flat = (ctypes.c_int32 * (4 * n))(*[int(v) for reg in regions for v in reg])
    out = torch.empty((B, C), dtype=torch.float32, device=feat.device)
    ws = _workspace(_lib.lib().mdx_rmac_workspace(B, C, n), feat.device)
    with _on(feat):
        check(_lib.lib().mdx_rmac(fp, B, C, H, W, flat, n, float(eps), _vp(ws.data_ptr()), ws.numel(), _vp(out.data_ptr()), _stream()),
              "mdx_rmac")
    return out


def roipool(feat, regions, kind="gem", p=3.0, pool_eps=1e-6):
    """Regional pooling ``[B,C,H,W] -> [B,R,C]``: the pooling ``kind`` of every region ``(row0, col0, height, width)``, no
    normalisation -- ``LF.roipool`` (functional.py:75-121) through ``mdx_roipool``."""
    fp = _dev(feat, torch.float32, "feature map")
    if feat.dim() != 4:
        raise ValueError("feature map must be [B,C,H,W]")
    B, C, H, W = feat.shape
    n = len(regions)
    if not 1 <= n <= 64:
        raise ValueError("1..64 regions supported, got %d" % n)
    flat = (ctypes.c_int32 * (4 * n))(*[int(v) for reg in regions for v in reg])
    out = torch.empty((B, n, C), dtype=torch.float32, device=feat.device)
    with _on(feat):
        check(_lib.lib().mdx_roipool(fp, B, C, H, W, flat, n, POOL_KINDS[kind], float(p), float(pool_eps), _vp(out.data_ptr()), _stream()),
              "mdx_roipool")
    return out


def region_sum(vecs, l2n_eps=None):
    """``[B,R,C] -> [B,C]``: sum over the regions in order; ``l2n_eps`` not None: each region vector L2-normalised first."""
    vp = _dev(vecs, torch.float32, "region vectors")
    if vecs.dim() != 3:
        raise ValueError("region vectors must be [B,R,C]")
    B, R, C = vecs.shape
    out = torch.empty((B, C), dtype=torch.float32, device=vecs.device)
    with _on(vecs):
        check(_lib.lib().mdx_region_sum(vp, B, R, C, -1.0 if l2n_eps is None else float(l2n_eps), _vp(out.data_ptr()), _stream()),
              "mdx_region_sum")
    return out


def l2n_rows_(x, bias=None, eps=1e-6):
    """In place ``(x + bias) / (||x + bias|| + eps)`` per row of a [R,D] matrix."""
    xp = _dev(x, torch.float32, "x")
    if x.dim() != 2:
        raise ValueError("x must be [R,D]")
    bp = _dev(bias, torch.float32, "bias") if bias is not None else None
    if bias is not None and bias.numel() != x.shape[1]:
        raise ValueError("bias length %d != D %d" % (bias.numel(), x.shape[1]))
    with _on(x):
        check(_lib.lib().mdx_l2n_rows(xp, x.shape[0], x.shape[1], bp, float(eps), _stream()), "mdx_l2n_rows")
    return x


def ms_aggregate(vecs, msp=1.0):
    """Per-scale descriptors (list of [D] or [D,1] tensors) -> aggregated [D].

    mdir/components/data/wrapper.py:109-119."""
    if not 1 <= len(vecs) <= 8:
        raise ValueError("1..8 scales supported, got %d" % len(vecs))
    flat = [v.reshape(-1) for v in vecs]
    D = flat[0].numel()
    ptrs = (ctypes.c_void_p * len(flat))()
    for i, v in enumerate(flat):
        if v.numel() != D:
            raise ValueError("scale %d has %d elements, expected %d" % (i, v.numel(), D))
        ptrs[i] = _dev(v, torch.float32, "scale descriptor").value
    out = torch.empty(D, dtype=torch.float32, device=flat[0].device)
    with _on(flat[0]):
        check(_lib.lib().mdx_ms_aggregate(ptrs, len(flat), D, float(msp), _vp(out.data_ptr()), _stream()),
              "mdx_ms_aggregate")
    return out


def ms_aggregate_batch(mats, msp=1.0):
    """Per-scale descriptor MATRICES (list of ``[B,D]`` tensors, one row per image) -> aggregated ``[B,D]`` in one
    launch (``mdx_ms_aggregate_batch``)."""
    if not 1 <= len(mats) <= 8:
        raise ValueError("1..8 scales supported, got %d" % len(mats))
    B, D = mats[0].shape
    ptrs = (ctypes.c_void_p * len(mats))()
    for i, v in enumerate(mats):
        if tuple(v.shape) != (B, D):
            raise ValueError("scale %d is %s, expected %s" % (i, tuple(v.shape), (B, D)))
        ptrs[i] = _dev(v, torch.float32, "scale descriptors").value
    out = torch.empty((B, D), dtype=torch.float32, device=mats[0].device)
    with _on(mats[0]):
        check(_lib.lib().mdx_ms_aggregate_batch(ptrs, len(mats), B, D, float(msp), _vp(out.data_ptr()), _stream()),
              "mdx_ms_aggregate_batch")
    return out


def pool_multi(feats, kind="gem", p=3.0, pool_eps=1e-6):
    """The feature maps of one pyramid (list of ``[B,C,H_s,W_s]``, same B and C) -> pooled ``[S,B,C]`` in ONE launch
    (``mdx_pool_multi``); no normalisation.  All fp32, or all fp16 (``mdx_pool_multi_f16``: fp32 out, the bits of the fp32
    call on the maps' ``.float()``); mixed maps are refused."""
    if not 1 <= len(feats) <= 8:
        raise ValueError("1..8 scales supported, got %d" % len(feats))
    if feats[0].dim() != 4:
        raise ValueError("feature maps must be [B,C,H,W]")
    B, C = feats[0].shape[:2]
    S = len(feats)
    half = feats[0].dtype == torch.float16
    if any(f.dtype != feats[0].dtype for f in feats):
        raise ValueError("the maps of one pool_multi call must share a dtype, got %s" % [str(f.dtype) for f in feats])
    ptrs = (ctypes.c_void_p * S)()
    hs, ws = (ctypes.c_int * S)(), (ctypes.c_int * S)()
    for i, f in enumerate(feats):
        if f.dim() != 4 or tuple(f.shape[:2]) != (B, C):
            raise ValueError("map %d is %s, expected [%d,%d,H,W]" % (i, tuple(f.shape), B, C))
        ptrs[i] = _dev(f, torch.float16 if half else torch.float32, "feature map").value
        hs[i], ws[i] = f.shape[2], f.shape[3]
    out = torch.empty((S, B, C), dtype=torch.float32, device=feats[0].device)
    fn, name = (_lib.lib().mdx_pool_multi_f16, "mdx_pool_multi_f16") if half else (_lib.lib().mdx_pool_multi, "mdx_pool_multi")
    with _on(feats[0]):
        check(fn(ptrs, S, B, C, hs, ws, POOL_KINDS[kind], float(p), float(pool_eps), _vp(out.data_ptr()), _stream()), name)
    return out


def l2n_aggregate(pooled, l2n_eps=1e-6, msp=1.0):
    """Pooled ``[S,B,D]`` -> aggregated descriptors ``[B,D]`` in ONE launch (``mdx_l2n_aggregate``): L2N of every
    scale's row, power mean over the scales, renormalisation."""
    if pooled.dim() != 3 or not 1 <= pooled.shape[0] <= 8:
        raise ValueError("pooled must be [S,B,D] with 1..8 scales")
    S, B, D = pooled.shape
    out = torch.empty((B, D), dtype=torch.float32, device=pooled.device)
    with _on(pooled):
        check(_lib.lib().mdx_l2n_aggregate(_dev(pooled, torch.float32, "pooled"), S, B, D, float(l2n_eps), float(msp),
                                           _vp(out.data_ptr()), _stream()), "mdx_l2n_aggregate")
    return out


def u8_to_chw(images, mean, std):
    """uint8 ``[B,H,W,C]`` device images -> normalised fp32 ``[B,C,H,W]`` (``mdx_u8_to_chw``):
    ``(u / 255 - mean) / std``, the scenarios' ``pil2np | totensor | normalize``."""
    if not (images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.is_contiguous()):
        raise ValueError("u8_to_chw expects a contiguous uint8 [B,H,W,C] CUDA/ROCm tensor (no CPU fallback)")
    b, h, w, c = images.shape
    if len(mean) != c or len(std) != c:
        raise ValueError("mean / std need %d values" % c)
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=images.device)
    if images.numel() == 0:
        return out
    arr = ctypes.c_float * c
    with _on(images):
        check(_lib.lib().mdx_u8_to_chw(images.data_ptr(), b, h, w, c, arr(*[float(v) for v in mean]),
                                       arr(*[float(v) for v in std]), out.data_ptr(), _stream()), "mdx_u8_to_chw")
    return out


def clahe_u8_to_chw(images, clip_limit, grid, mean, std, return_intermediates=False):
    """uint8 RGB ``[B,H,W,3]`` device images -> CLAHE on the Lab lightness -> normalised fp32 ``[B,3,H,W]``
    (``mdx_clahe_u8_to_chw``): the scenarios' ``pil2np | apply_clahe | totensor | normalize``.  ``grid``: int or
    ``(tiles_x, tiles_y)``.  ``return_intermediates``: also the uint8 lightness ``[B,H,W]``, the LUTs
    ``[B,tiles_y,tiles_x,256]`` and the equalised lightness ``[B,H,W]`` the kernels left in the workspace (tests)."""
    if not (images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.is_contiguous() and images.shape[3] == 3):
        raise ValueError("clahe_u8_to_chw expects a contiguous uint8 [B,H,W,3] CUDA/ROCm tensor (no CPU fallback)")
    b, h, w, _ = images.shape
    tx, ty = (int(grid), int(grid)) if not isinstance(grid, (tuple, list)) else (int(grid[0]), int(grid[1]))
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean / std need 3 values")
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=images.device)
    need = _lib.lib().mdx_clahe_workspace(b, h, w, tx, ty)
    ws = _workspace(need, images.device)
    if images.numel():
        arr = ctypes.c_float * 3
        with _on(images):
            check(_lib.lib().mdx_clahe_u8_to_chw(images.data_ptr(), b, h, w, int(clip_limit), tx, ty, arr(*[float(v) for v in mean]),
                                                 arr(*[float(v) for v in std]), ws.data_ptr(), ws.numel(), out.data_ptr(), _stream()),
                  "mdx_clahe_u8_to_chw")
    if return_intermediates:
        plane, tables = -(-(b * h * w) // 256) * 256, -(-(b * ty * tx * 256) // 256) * 256
        return (out, ws[:b * h * w].view(b, h, w), ws[plane:plane + b * ty * tx * 256].view(b, ty, tx, 256),
                ws[plane + tables:plane + tables + b * h * w].view(b, h, w))
    return out


def _photometric_args(images, mean, std, who):
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4
            and images.is_contiguous() and images.shape[3] == 3):
        raise ValueError("%s expects a contiguous uint8 [B,H,W,3] CUDA/ROCm tensor (no CPU fallback)" % who)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean / std need 3 values")
    b, h, w, _ = images.shape
    arr = ctypes.c_float * 3
    return b, h, w, arr(*[float(v) for v in mean]), arr(*[float(v) for v in std])


def _photometric_regions(ws, b, h, w):
    """Views of the workspace regions of include/mdx_photometric.h: x, x' (or log2 x), counts, fp, gamma, solver info."""
    n = b * h * w
    plane = -(-(4 * n) // 256) * 256
    small = -(-(8 * b) // 256) * 256
    at = 4 * plane
    return (ws[:4 * n].view(torch.float32).view(b, h, w), ws[plane:plane + 4 * n].view(torch.float32).view(b, h, w),
            ws[at:at + 1024 * b].view(torch.int32).view(b, 256), ws[at + 1024 * b:at + 3072 * b].view(torch.float64).view(b, 256),
            ws[at + 3072 * b:at + 3072 * b + 8 * b].view(torch.float64),
            ws[at + 3072 * b + small:at + 3072 * b + small + 8 * b].view(torch.int32).view(b, 2))


def histmatch_u8_to_chw(images, mean, std, target_cdf=None, return_intermediates=False):
    """uint8 RGB ``[B,H,W,3]`` device images -> histogram matching of the Lab lightness -> normalised fp32 ``[B,3,H,W]``
    (``mdx_histmatch_u8_to_chw``): the scenarios' ``pil2np | match_histogram:<eq or name> | totensor | normalize``.
    ``target_cdf``: None for ``eq`` (global histogram equalisation), or a float64 device tensor of the 256 cumulative values of the
    target histogram (``datasets.register_histogram``).  ``return_intermediates``: also the lightness ``[B,H,W]`` f32, the counts
    ``[B,256]`` int32, the table ``fp`` ``[B,256]`` f64 and the mapped lightness ``[B,H,W]`` f32 the kernels left in the workspace."""
    b, h, w, mean_c, std_c = _photometric_args(images, mean, std, "histmatch_u8_to_chw")
    cdf_p = None
    if target_cdf is not None:
        cdf_p = _dev(target_cdf, torch.float64, "target_cdf")
        if target_cdf.numel() != 256 or target_cdf.device != images.device:
            raise ValueError("target_cdf must hold 256 values on the images' device")
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=images.device)
    ws = _workspace(_lib.lib().mdx_photometric_workspace(b, h, w), images.device)
    if images.numel():
        with _on(images):
            check(_lib.lib().mdx_histmatch_u8_to_chw(images.data_ptr(), b, h, w, cdf_p, mean_c, std_c, ws.data_ptr(), ws.numel(),
                                                     out.data_ptr(), _stream()), "mdx_histmatch_u8_to_chw")
    if return_intermediates:
        x, mapped, counts, fp, _, _ = _photometric_regions(ws, b, h, w)
        return out, x, counts, fp, mapped
    return out


def gamma_u8_to_chw(images, target, mean, std, return_intermediates=False):
    """uint8 RGB ``[B,H,W,3]`` device images -> gamma equalisation of the Lab lightness (per image the gamma in [0.1, 10] with
    ``mean(x ** gamma) = target``) -> normalised fp32 ``[B,3,H,W]`` (``mdx_gamma_u8_to_chw``): the scenarios'
    ``pil2np | gamma_equalize:<target> | totensor | normalize``.  ``return_intermediates``: also the lightness ``[B,H,W]`` f32 and
    gamma ``[B]`` f64 the kernels left in the workspace; ``return_intermediates="solver"``: after them int32 ``[B,2]``, the secant
    steps taken and 1 where the fallback decided."""
    b, h, w, mean_c, std_c = _photometric_args(images, mean, std, "gamma_u8_to_chw")
    target = float(target)
    if not 0.0 < target < 1.0:
        raise ValueError("gamma_u8_to_chw: target %r must satisfy 0 < target < 1" % (target,))
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=images.device)
    ws = _workspace(_lib.lib().mdx_photometric_workspace(b, h, w), images.device)
    if images.numel():
        with _on(images):
            check(_lib.lib().mdx_gamma_u8_to_chw(images.data_ptr(), b, h, w, target, mean_c, std_c, ws.data_ptr(), ws.numel(),
                                                 out.data_ptr(), _stream()), "mdx_gamma_u8_to_chw")
    if return_intermediates:
        x, _, _, _, gamma, info = _photometric_regions(ws, b, h, w)
        return (out, x, gamma, info) if return_intermediates == "solver" else (out, x, gamma)
    return out


def bilinear_pyramid(x, scales):
    """``[F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False) for s in scales]`` for an fp32
    ``[B,C,H,W]`` device tensor, all levels in ONE launch (``mdx_bilinear_pyramid``); a scale of exactly 1 returns ``x``."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bilinear_pyramid expects a contiguous fp32 [B,C,H,W] CUDA/ROCm tensor (no CPU fallback)")
    import math
    b, c, h, w = x.shape
    todo = [(i, float(s)) for i, s in enumerate(scales) if float(s) != 1.0]
    out = [x] * len(scales)
    if not todo:
        return out
    if len(todo) > 8:
        raise ValueError("at most 8 scaled levels")
    sc = (ctypes.c_double * len(todo))(*[s for _, s in todo])
    ptrs = (ctypes.c_void_p * len(todo))()
    for k, (i, s) in enumerate(todo):
        out[i] = torch.empty((b, c, int(math.floor(h * s)), int(math.floor(w * s))), dtype=torch.float32, device=x.device)
        ptrs[k] = out[i].data_ptr()
    with _on(x):
        check(_lib.lib().mdx_bilinear_pyramid(x.data_ptr(), b, c, h, w, len(todo), sc, ptrs, _stream()), "mdx_bilinear_pyramid")
    return out


def resample_u8(images, axis, bounds, taps):
    """One pass of Pillow's 8-bit resampling on uint8 ``[B,H,W,C]`` device images: along the width (``axis=1``) or the
    height (``axis=0``), with device taps ``bounds`` int32 ``[out,2]`` and ``taps`` int32 ``[out,ksize]``
    (``mdx_resample_u8``; the taps come from ``mdir_amd.resample``)."""
    if not (images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.is_contiguous()):
        raise ValueError("resample_u8 expects a contiguous uint8 [B,H,W,C] CUDA/ROCm tensor (no CPU fallback)")
    if axis not in (0, 1):
        raise ValueError("axis must be 0 (height) or 1 (width)")
    b, h, w, c = images.shape
    out_len, ksize = taps.shape
    if tuple(bounds.shape) != (out_len, 2) or bounds.dtype != torch.int32 or taps.dtype != torch.int32 \
            or bounds.device != images.device or taps.device != images.device:
        raise ValueError("bounds / taps must be int32 [out,2] / [out,ksize] on the images' device")
    out = torch.empty((b, h, out_len, c) if axis == 1 else (b, out_len, w, c), dtype=torch.uint8, device=images.device)
    with _on(images):
        check(_lib.lib().mdx_resample_u8(images.data_ptr(), b, h, w, c, axis, out_len, _dev(bounds, torch.int32, "bounds"),
                                         _dev(taps, torch.int32, "taps"), ksize, out.data_ptr(), _stream()), "mdx_resample_u8")
    return out


def bn_act_(x, running_mean, running_var, weight=None, bias=None, eps=1e-5, residual=None, relu=True):
    """In place on a convolution output ``x [N,C,H,W]``: inference batch-norm, ``+ residual``, ReLU
    in one pass (``mdx_bn_act``); returns ``x``.  Called ~100 times per image by a launch-bound trunk,
    so the checks are kept to what protects the raw pointers.  An fp16 ``x`` (with an fp16 residual; the statistics stay fp32)
    goes to ``mdx_bn_act_f16``: the same fp32 arithmetic on the upcast elements, rounded once to fp16."""
    half = x.dtype == torch.float16
    if not (x.is_cuda and (half or x.dtype == torch.float32) and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bn_act_ expects a contiguous fp32 (or fp16) [N,C,H,W] CUDA/ROCm tensor (no CPU fallback)")
    n, c, h, w = x.shape
    ptrs = []
    for name, t in (("running_mean", running_mean), ("running_var", running_var), ("weight", weight), ("bias", bias)):
        if t is None:
            ptrs.append(None)
            continue
        if t.numel() != c or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
            raise ValueError("%s must be %d contiguous fp32 values on %s" % (name, c, x.device))
        ptrs.append(t.data_ptr())
    if (ptrs[0] is None) != (ptrs[1] is None):
        raise ValueError("running_mean and running_var must both be given or both be None")
    rp = None
    if residual is not None:
        if residual.shape != x.shape or residual.dtype != x.dtype or residual.device != x.device \
                or not residual.is_contiguous():
            raise ValueError("residual must be contiguous %s and shaped like x" % ("fp16" if half else "fp32"))
        rp = residual.data_ptr()
    if x.numel() == 0:
        return x
    fn, name = (_lib.lib().mdx_bn_act_f16, "mdx_bn_act_f16") if half else (_lib.lib().mdx_bn_act, "mdx_bn_act")
    with _on(x):
        check(fn(x.data_ptr(), rp, n, c, h * w, ptrs[0], ptrs[1], ptrs[2], ptrs[3], float(eps), 1 if relu else 0, _stream()), name)
    return x


ACT_NONE, ACT_RELU, ACT_LEAKY = _lib.MDX_ACT_NONE, _lib.MDX_ACT_RELU, _lib.MDX_ACT_LEAKY


def bn_act_into(x, out_view, running_mean=None, running_var=None, weight=None, bias=None, eps=1e-5, act=ACT_RELU, slope=0.0):
    """Inference batch-norm / conv bias and an activation of a convolution output ``x [N,C,H,W]`` in one pass, written into
    ``out_view`` (``mdx_bn_act_into``, include/mdx_unet.h); returns ``out_view``.  ``out_view`` is ``x`` itself (in place) or a
    channel slice ``buf[:, c0:c0 + C]`` of a contiguous ``[N, Ctot, H, W]`` tensor: same shape as ``x``, contiguous planes one
    after the other, any distance between images.  ``act``: ``ACT_NONE``, ``ACT_RELU``, ``ACT_LEAKY`` (with ``slope``).  Unlike
    ``bn_act_`` nothing is added after the ``fmaf``, so a -0 stays -0."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bn_act_into expects a contiguous fp32 [N,C,H,W] CUDA/ROCm tensor (no CPU fallback)")
    n, c, h, w = x.shape
    if not (isinstance(out_view, torch.Tensor) and out_view.shape == x.shape and out_view.dtype == x.dtype
            and out_view.device == x.device):
        raise ValueError("out_view must be an fp32 tensor shaped like x on %s" % (x.device,))
    if act not in (ACT_NONE, ACT_RELU, ACT_LEAKY):
        raise ValueError("act=%r (ACT_NONE, ACT_RELU or ACT_LEAKY)" % (act,))
    ptrs = []
    for name, t in (("running_mean", running_mean), ("running_var", running_var), ("weight", weight), ("bias", bias)):
        if t is None:
            ptrs.append(None)
            continue
        if t.numel() != c or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
            raise ValueError("%s must be %d contiguous fp32 values on %s" % (name, c, x.device))
        ptrs.append(t.data_ptr())
    if (ptrs[0] is None) != (ptrs[1] is None):
        raise ValueError("running_mean and running_var must both be given or both be None")
    if x.numel() == 0:
        return out_view
    hw = h * w
    sn, sc, sh, sw = out_view.stride()
    # a channel slice: the planes of one image follow one another as in x (a size-1 dimension's stride is arbitrary in torch)
    if (w > 1 and sw != 1) or (h > 1 and sh != w) or (c > 1 and sc != hw) or (n > 1 and sn < c * hw):
        raise ValueError("out_view is not a channel slice of a contiguous [N,Ctot,H,W] tensor: strides %s for shape %s"
                         % ((sn, sc, sh, sw), tuple(x.shape)))
    stride = sn if n > 1 else c * hw
    with _on(x):
        check(_lib.lib().mdx_bn_act_into(x.data_ptr(), out_view.data_ptr(), n, c, hw, stride, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                         float(eps), int(act), float(slope), _stream()), "mdx_bn_act_into")
    return out_view


def conv1x1_transpose_weights(weight):
    """``[Cout, Cin(,1,1)]`` convolution weights -> the ``[Cin, Cout]`` copy ``conv1x1_bn_act`` reads (made once)."""
    w = weight.reshape(weight.shape[0], -1)
    wp = _dev(w, torch.float32, "weight")
    wt = torch.empty((w.shape[1], w.shape[0]), dtype=torch.float32, device=w.device)
    with _on(w):
        check(_lib.lib().mdx_conv1x1_transpose_weights(wp, w.shape[0], w.shape[1], wt.data_ptr(), _stream()),
              "mdx_conv1x1_transpose_weights")
    return wt


def conv1x1_supported(cin, cout):
    return cin % 16 == 0 and cout % 64 == 0


def conv1x1_bn_act(x, weight_t, running_mean, running_var, weight=None, bias=None, eps=1e-5, residual=None, relu=True):
    """1x1 convolution + inference batch-norm (+ residual) (+ ReLU) in one kernel (``mdx_conv1x1_bn_act``).
    ``x [N,Cin,H,W]`` contiguous fp32; ``weight_t [Cin,Cout]`` from ``conv1x1_transpose_weights``; returns ``[N,Cout,H,W]``."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("conv1x1_bn_act expects a contiguous fp32 [N,C,H,W] CUDA/ROCm tensor (no CPU fallback)")
    n, cin, h, w = x.shape
    if weight_t.dim() != 2 or weight_t.shape[0] != cin or weight_t.dtype != torch.float32 or weight_t.device != x.device \
            or not weight_t.is_contiguous():
        raise ValueError("weight_t must be contiguous fp32 [Cin=%d, Cout] on %s" % (cin, x.device))
    cout = weight_t.shape[1]
    ptrs = []
    for name, t in (("running_mean", running_mean), ("running_var", running_var), ("weight", weight), ("bias", bias)):
        if t is None:
            ptrs.append(None)
            continue
        if t.numel() != cout or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
            raise ValueError("%s must be %d contiguous fp32 values on %s" % (name, cout, x.device))
        ptrs.append(t.data_ptr())
    rp = None
    if residual is not None:
        if tuple(residual.shape) != (n, cout, h, w) or residual.dtype != torch.float32 or residual.device != x.device \
                or not residual.is_contiguous():
            raise ValueError("residual must be contiguous fp32 [%d,%d,%d,%d]" % (n, cout, h, w))
        rp = residual.data_ptr()
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    with _on(x):
        check(_lib.lib().mdx_conv1x1_bn_act(x.data_ptr(), weight_t.data_ptr(), n, cin, cout, h * w, ptrs[0], ptrs[1], ptrs[2],
                                            ptrs[3], float(eps), rp, 1 if relu else 0, out.data_ptr(), _stream()),
              "mdx_conv1x1_bn_act")
    return out


# ----------------------------------------------------------------------- index

def quantize_i8(vecs, layout="ND"):
    """``(codes int8 [N, D], scales fp32 [N])``: the int8 quantisation of an ``MDX_I8`` shard (``mdx_quantize_i8``; the
    values ``DescriptorIndex(vecs, layout, storage="i8")`` holds for the same rows, bit for bit).  ``vecs`` is a device tensor,
    ``[N, D]`` (layout "ND") or ``[D, N]`` (layout "DN")."""
    vp = _dev(vecs, torch.float32, "vecs")
    n, d, lay = _layout(vecs, layout, "vecs")
    if n == 0 or d == 0:
        raise ValueError("vecs must be non-empty, got %d x %d" % (n, d))
    codes = torch.empty((n, d), dtype=torch.int8, device=vecs.device)
    scales = torch.empty(n, dtype=torch.float32, device=vecs.device)
    with torch.cuda.device(vecs.device):
        check(_lib.lib().mdx_quantize_i8(vp, n, d, lay, _vp(codes.data_ptr()), _vp(scales.data_ptr()), _stream()), "mdx_quantize_i8")
    return codes, scales


class DescriptorIndex:
    """A resident, re-tiled shard of descriptors (``mdx_index``).

    ``vecs`` is a device tensor, ``[D,N]`` (layout "DN", the reference's
    ``extract_vectors`` output) or ``[N,D]`` (layout "ND")."""

    def __init__(self, vecs, layout="DN", row_offset=0, storage="f32"):
        """``storage="f16"`` keeps the shard (and each call's queries) in fp16 and uses the fp16
        MFMA with fp32 accumulation: half the HBM bytes, ~1e-3 relative score error.

        ``storage="i8"`` keeps every row as int8 codes and one fp32 scale (a quarter of the fp32 bytes) and multiplies on
        the int8 MFMA with exact int32 accumulation.  The scores are defined to the bit (``include/mdx.h`` ``MDX_I8``): a row
        ``x`` (a query: ``q - center``) has ``a = max|x|``, codes ``clamp(rint(x * (127/a)), -127, 127)`` and scale ``a/127``
        (all fp32, round to nearest even; ``a == 0``: zero codes and scale), and
        ``score = float(sum_k c_q,k c_i,k) * (scale_i * scale_q)``; :func:`quantize_i8` returns the codes and scales.
        ``d`` <= 133 120; split-precision ``compute`` modes and the direct-store exchange need an fp32 shard."""
        self._h = None
        self.storage = storage
        vp = _dev(vecs, torch.float32, "vecs")
        n, d, lay = _layout(vecs, layout, "vecs")
        self._h = ctypes.c_void_p()
        self.device = vecs.device
        self.n, self.d, self.row_offset = n, d, int(row_offset)
        with torch.cuda.device(self.device):
            # the tiles live in PyTorch's caching allocator: hipMalloc + hipFree of an 8 GB shard cost ~190 ms per index, a
            # block of the pool nothing after the first use
            need = _lib.lib().mdx_index_bytes(n, d, _lib.STORAGE[storage])
            self._tiles = torch.empty(need, dtype=torch.uint8, device=self.device)
            check(_lib.lib().mdx_index_create_in(ctypes.byref(self._h), vp, n, d, lay, self.row_offset, _lib.STORAGE[storage],
                                                 _vp(self._tiles.data_ptr()), need, _stream()), "mdx_index_create_in")
            # the source tensor may be freed by the caller right after: finish the re-tiling first
            torch.cuda.current_stream().synchronize()

    @property
    def device_bytes(self):
        b = ctypes.c_int64()
        check(_lib.lib().mdx_index_info(self._h, None, None, None, ctypes.byref(b)), "mdx_index_info")
        return b.value

    def scores(self, queries, qlayout="DN", center=None, out=None, compute="chain"):
        """fp32 ``[nq, n]``: row q = similarities of query q to every shard row.

        The transpose of ``np.dot(vecs.T, qvecs)`` (cirscore.py:69).  ``compute="chain"`` (default): the exact k-ordered
        fp32 fma chain; ``"split3"``: the labelled split-precision mode on the same fp32 shard (three bf16 pieces per
        operand, six products on the bf16 MFMA, fp32 accumulation: HBM-bound instead of fp32-MFMA-bound; scores within
        the summation-order bound 2e-6 of the chain, ``include/mdx.h`` ``MDX_F32_SPLIT3``); ``"split2"``: the second labelled
        mode, block floating point with two fp16 pieces and three products (``MDX_F32_SPLIT2``): for data of ordinary dynamic
        range (L2-normalised descriptors), 0.63 of the exact kernel's time."""
        if self._h is None:
            raise RuntimeError("index is closed")
        nq, d, lay = _layout(queries, qlayout, "queries")
        if d != self.d:
            raise ValueError("query dimension %d != index dimension %d" % (d, self.d))
        qp = _dev(queries, torch.float32, "queries")
        cp = _center(center, d)
        if out is None:
            out = torch.empty((nq, self.n), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (nq, self.n):
            raise ValueError("out must be [%d,%d]" % (nq, self.n))
        if compute not in _lib.COMPUTE:
            raise ValueError("compute %r (one of %s)" % (compute, sorted(_lib.COMPUTE)))
        mode = _lib.COMPUTE[compute]
        if mode != _lib.MDX_F32_CHAIN and self.storage != "f32":
            raise ValueError("compute=%r multiplies an fp32 shard; this one is stored as %s" % (compute, self.storage))
        need = _lib.lib().mdx_scores_workspace_ex(nq, d, mode)
        ws = _workspace(need, self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_scores_ex(self._h, qp, nq, lay, cp, _dev(out, torch.float32, "out"),
                                           _vp(ws.data_ptr()), need, mode, _stream()), "mdx_scores_ex")
        return out

    def scores_p2p(self, queries, p2p, qlayout="DN", center=None):
        """The similarity of ``scores`` with the ROUTED epilogue (``mdx_scores_p2p``): query q's scores against this shard's
        rows go straight to row ``q - qlo_owner`` of the owner rank's receive buffer, at columns ``row_offset ..`` -- the
        direct-store exchange of a row-sharded database (:class:`P2P`).  Nothing is returned: ``p2p.close_step()`` hands
        out this rank's ``[nq_mine, n_total]`` matrix once every rank has written its part."""
        if self._h is None:
            raise RuntimeError("index is closed")
        nq, d, lay = _layout(queries, qlayout, "queries")
        if d != self.d:
            raise ValueError("query dimension %d != index dimension %d" % (d, self.d))
        if self.storage != "f32":
            raise ValueError("the direct-store exchange multiplies an fp32 shard; this one is stored as %s" % self.storage)
        qp = _dev(queries, torch.float32, "queries")
        cp = _dev(center, torch.float32, "center") if center is not None else None
        need = _lib.lib().mdx_scores_workspace(nq, d)
        ws = _workspace(need, self.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_scores_p2p(self._h, qp, nq, lay, cp, p2p._h, _vp(ws.data_ptr()), need, _stream()), "mdx_scores_p2p")

    def i8_bounds(self):
        """Device tensor (float64 ``[4]``, the bytes of ``mdx_i8_bounds``) of this int8 shard: ``S_max``, ``S_min`` (smallest
        nonzero scale), ``L_max = max scale_i ||c_i||_1`` and the out-of-contract flag (:func:`unpack_i8_bounds` reads it on the
        host).  Reduced once per index (``mdx_index_i8_bounds``) and kept; what :func:`rescore_certify` needs."""
        if self._h is None:
            raise RuntimeError("index is closed")
        if self.storage != "i8":
            raise ValueError("i8_bounds needs an int8 shard; this one is stored as %s" % self.storage)
        if getattr(self, "_i8_bounds", None) is None:
            b = torch.empty(4, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                check(_lib.lib().mdx_index_i8_bounds(self._h, _vp(b.data_ptr()), _stream()), "mdx_index_i8_bounds")
            self._i8_bounds = b
        return self._i8_bounds

    def close(self):
        self._i8_bounds = None
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, None
            check(_lib.lib().mdx_index_destroy(h), "mdx_index_destroy")
            # back to the pool -- after every kernel that may still read the tiles, on whatever stream it was launched
            # (what the library's own hipFree guaranteed by being device-synchronous; here without its ~100 ms)
            if self._tiles is not None and self._tiles.is_cuda:
                torch.cuda.synchronize(self._tiles.device)
            self._tiles = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------- ranking

def rank_workspace_bytes(n, nq):
    return _lib.lib().mdx_rank_workspace(n, nq)


def rank_full(scores, id_offset=0, out=None, workspace=None):
    """int64 ``[nq, n]``: row q = ids best to worst (transpose of cirscore.py:70)."""
    sp = _dev(scores, torch.float32, "scores")
    nq, n = scores.shape
    need = rank_workspace_bytes(n, nq)
    ws = workspace if workspace is not None else _workspace(need, scores.device)
    if out is None:
        out = torch.empty((nq, n), dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        check(_lib.lib().mdx_rank_full(sp, n, nq, int(id_offset), _dev(out, torch.int64, "ranks"),
                                       _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_rank_full")
    return out


MAX_RANK_SEGMENTS = 32


def rank_full_segments(blocks, id_offset=0, out=None, workspace=None):
    """``rank_full`` of scores that lie in column blocks: ``blocks[g]`` is ``[nq, w_g]`` and row q of the problem is
    the blocks' rows q side by side (the peer blocks of the multi-GPU exchange).  No concatenated copy is made:
    the first pass of the sort reads the blocks in place (``mdx_rank_full_segments``)."""
    if not 1 <= len(blocks) <= MAX_RANK_SEGMENTS:
        raise ValueError("1..%d blocks supported, got %d" % (MAX_RANK_SEGMENTS, len(blocks)))
    nq = blocks[0].shape[0]
    ptrs = (ctypes.c_void_p * len(blocks))()
    widths = (ctypes.c_int64 * len(blocks))()
    for g, b in enumerate(blocks):
        if b.dim() != 2 or b.shape[0] != nq:
            raise ValueError("block %d is %s, expected [%d, w]" % (g, tuple(b.shape), nq))
        ptrs[g] = _dev(b, torch.float32, "score block").value
        widths[g] = b.shape[1]
    n = sum(int(b.shape[1]) for b in blocks)
    dev = blocks[0].device
    ws = workspace if workspace is not None else _workspace(rank_workspace_bytes(n, nq), dev)
    if out is None:
        out = torch.empty((nq, n), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().mdx_rank_full_segments(ptrs, widths, len(blocks), nq, int(id_offset), _dev(out, torch.int64, "ranks"),
                                                _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_rank_full_segments")
    return out


def scores_rowmajor(db, queries, qlayout="DN", center=None, out=None):
    """fp32 ``[nq, n]`` similarities of ``queries`` against the rows of ``db`` -- a row-major ``[n, d]`` fp32 CUDA matrix that
    is multiplied ONCE and read where it lies (``mdx_scores_rowmajor``): no index build, no second copy of the database.
    Bit-identical to ``DescriptorIndex(db, "ND").scores(queries, qlayout, center)`` (same kernels, same k order).
    ``d`` must be a multiple of 4 (rows are fetched in 16-byte pieces); other shapes: build a :class:`DescriptorIndex`."""
    dp = _dev(db, torch.float32, "db")
    if db.dim() != 2:
        raise ValueError("db: a 2-d [n, d] matrix")
    n, d = db.shape
    nq, dq, lay = _layout(queries, qlayout, "queries")
    if dq != d:
        raise ValueError("query dimension %d != database dimension %d" % (dq, d))
    qp = _dev(queries, torch.float32, "queries")
    cp = _center(center, d)
    if out is None:
        out = torch.empty((nq, n), dtype=torch.float32, device=db.device)
    elif tuple(out.shape) != (nq, n):
        raise ValueError("out must be [%d,%d]" % (nq, n))
    need = _lib.lib().mdx_scores_workspace(nq, d)
    ws = _workspace(need, db.device)
    with torch.cuda.device(db.device):
        check(_lib.lib().mdx_scores_rowmajor(dp, n, d, qp, nq, lay, cp, _dev(out, torch.float32, "out"), _vp(ws.data_ptr()), need,
                                             _stream()), "mdx_scores_rowmajor")
    return out


def topk(scores, k, id_offset=0, workspace=None):
    """(ids int64 [nq,k], scores fp32 [nq,k]) of the k best rows per query."""
    sp = _dev(scores, torch.float32, "scores")
    nq, n = scores.shape
    need = rank_workspace_bytes(n, nq)
    ws = workspace if workspace is not None else _workspace(need, scores.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    vals = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    with torch.cuda.device(scores.device):
        check(_lib.lib().mdx_topk(sp, n, nq, int(k), int(id_offset), _vp(ids.data_ptr()), _vp(vals.data_ptr()),
                                  _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_topk")
    return ids, vals


def rank_route(n):
    """``"SMALL"``, ``"PACKED"`` or ``"KV"``: the kernels ``rank_full`` would run now for rows of ``n`` scores on the current
    device (``mdx_rank_route``: host arithmetic, nothing is launched).  Before anything was ranked on the device the form a
    wave ranks with is unknown and the answer is the one for ballots: never ``"SMALL"``."""
    rc = _lib.lib().mdx_rank_route(int(n), None)
    check(min(rc, 0), "mdx_rank_route")
    return _lib.RANK_ROUTES[rc]


def topk_route(n, nq, k, workspace_bytes=None):
    """``"SAMPLED"``, ``"SELECT"`` or ``"SORT"``: the route ``topk`` takes for ``[nq, n]`` scores and ``k`` (``mdx_topk_route``),
    with the workspace ``topk`` itself allocates unless ``workspace_bytes`` is given."""
    if workspace_bytes is None:
        workspace_bytes = rank_workspace_bytes(n, nq)
    rc = _lib.lib().mdx_topk_route(int(n), int(nq), int(k), int(workspace_bytes))
    check(min(rc, 0), "mdx_topk_route")
    return _lib.TOPK_ROUTES[rc]


RESCORE_MAX_K = 4096              # include/mdx.h MDX_RESCORE_MAX_K: one query's shortlist is sorted in LDS


def rescore(rows, queries, ids, qlayout="ND", center=None):
    """``(ids int64 [nq, K], scores fp32 [nq, K])``: the exact fp32 chain scores of each query's shortlist ``ids`` (int64
    ``[nq, K]``, unique within a query, ``K <= 4096``) against ``rows`` (fp32 ``[n, d]`` on the device, rows contiguous at any
    stride), sorted by :func:`rank_full`'s order (``mdx_rescore``).  Every score is bit-identical to
    ``DescriptorIndex(rows, "ND").scores(queries, qlayout, center)`` at the same id; an id outside ``[0, n)`` scores NaN and
    sorts last."""
    rp, ld = _rows(rows, "rows")
    n, d = rows.shape
    nq, dq, lay = _layout(queries, qlayout, "queries")
    if dq != d:
        raise ValueError("query dimension %d != rows dimension %d" % (dq, d))
    qp = _dev(queries, torch.float32, "queries")
    cp = _center(center, d)
    _dev(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[0] != nq:
        raise ValueError("ids must be [%d, K], got %s" % (nq, tuple(ids.shape)))
    K = ids.shape[1]
    if n < 1 or d < 1 or nq < 1 or not 1 <= K <= RESCORE_MAX_K:
        raise ValueError("rescore: n=%d d=%d nq=%d must be >= 1 and K=%d in [1, %d]" % (n, d, nq, K, RESCORE_MAX_K))
    out_ids = torch.empty((nq, K), dtype=torch.int64, device=rows.device)
    out_scores = torch.empty((nq, K), dtype=torch.float32, device=rows.device)
    h = _lib.lib()
    need = h.mdx_rescore_workspace(nq, K, d)
    ws = _workspace(need, rows.device)
    with _on(rows):
        check(h.mdx_rescore(rp, n, d, ld, qp, nq, lay, cp, _vp(ids.data_ptr()), K, _vp(out_ids.data_ptr()),
                            _vp(out_scores.data_ptr()), _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_rescore")
    return out_ids, out_scores


def unpack_i8_bounds(bounds):
    """The values of :meth:`DescriptorIndex.i8_bounds` on the host: ``{"s_max", "s_min", "l_max": float, "flag": int}``."""
    raw = bounds.cpu().numpy()
    return {"s_max": float(raw[0]), "s_min": float(raw[1]), "l_max": float(raw[2]),
            "flag": int(raw[3:4].view(np.int32)[0])}


def rescore_certify(scores, t, queries, bounds, n, qlayout="ND", center=None):
    """``(depth int32 [nq], upper fp32 [nq])`` (``mdx_rescore_certify``, the proof in ``include/mdx.h``): the first ``depth[q]``
    entries of :func:`rescore`'s sorted output for the shortlist ``topk(int8 scores, K)`` are, bit for bit, the first entries
    of the exact fp32 ranking.  ``scores`` fp32 ``[nq, K]`` (rescore's sorted scores), ``t`` fp32 ``[nq]`` (the K-th int8
    shortlist score, ``top_scores[:, K-1]``), ``queries`` / ``center`` those of the int8 scores, ``bounds`` of
    :meth:`DescriptorIndex.i8_bounds`, ``n`` the index's rows.  ``upper`` is the bound U_q every row outside the shortlist
    stays under."""
    _dev(scores, torch.float32, "scores")
    if scores.dim() != 2:
        raise ValueError("scores must be [nq, K]")
    nq, K = scores.shape
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] != nq:
        raise ValueError("t must be a [%d] tensor" % nq)
    t = t.contiguous()
    tp = _dev(t, torch.float32, "t")
    nqq, d, lay = _layout(queries, qlayout, "queries")
    if nqq != nq:
        raise ValueError("queries hold %d queries, scores %d" % (nqq, nq))
    qp = _dev(queries, torch.float32, "queries")
    cp = _center(center, d)
    bp = _dev(bounds, torch.float64, "bounds")
    if bounds.numel() != 4:
        raise ValueError("bounds: the float64 [4] tensor of DescriptorIndex.i8_bounds()")
    if not 1 <= K <= min(int(n), RESCORE_MAX_K):
        raise ValueError("K=%d must be in [1, min(n=%d, %d)]" % (K, n, RESCORE_MAX_K))
    upper = torch.empty(nq, dtype=torch.float32, device=scores.device)
    depth = torch.empty(nq, dtype=torch.int32, device=scores.device)
    with _on(scores):
        check(_lib.lib().mdx_rescore_certify(_vp(scores.data_ptr()), nq, K, tp, qp, d, lay, cp, bp, int(n), _vp(upper.data_ptr()),
                                             _vp(depth.data_ptr()), _stream()), "mdx_rescore_certify")
    return depth, upper


# ------------------------------------------------------------- range search and self-join

JOIN_BLOCK = 128                  # include/mdx.h MDX_JOIN_BLOCK: rows per block side of the join kernel
_MAX_ITEMS = (1 << 31) - 1        # pairs, rows and capacities of one call stay below 2^31


def _tau(threshold):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not math.isfinite(threshold):
        raise ValueError("threshold must be a finite number, got %r" % (threshold,))
    with np.errstate(over="ignore"):
        t = float(np.float32(threshold))
    if not math.isfinite(t):
        raise ValueError("threshold %r is outside the fp32 range" % (threshold,))
    return t


def _join_operands(who, a, stats_a, b, stats_b, a_lo, a_hi):
    for name, ix in (("a", a), ("b", b)):
        if not isinstance(ix, DescriptorIndex) or ix._h is None:
            raise ValueError("%s: %s must be an open DescriptorIndex" % (who, name))
        if ix.storage != "i8":
            raise ValueError("%s: pruning needs int8 indexes (%s is %s)" % (who, name, ix.storage))
    if a.d != b.d:
        raise ValueError("%s: dimensions %d and %d differ" % (who, a.d, b.d))
    a_hi = a.n if a_hi is None else int(a_hi)
    a_lo = int(a_lo)
    if not (0 <= a_lo < a_hi <= a.n) or a_lo % JOIN_BLOCK:
        raise ValueError("%s: rows [%d, %d) of %d, the first a multiple of %d" % (who, a_lo, a_hi, a.n, JOIN_BLOCK))
    for name, st, ix in (("stats_a", stats_a, a), ("stats_b", stats_b, b)):
        _dev(st, torch.float32, name)
        if tuple(st.shape) != (ix.n, 4):
            raise ValueError("%s must be join_stats of its index: [%d, 4]" % (name, ix.n))
    return a_lo, a_hi


def _capacity(value):
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= _MAX_ITEMS:
        raise ValueError("capacity must be an integer in [0, 2^31), got %r" % (value,))
    return value


def _pair_rows(rows_a, rows_b, m, m_lo, who):
    """The operands of a resolve: (pointer, stride) of both row matrices, their dimension, and m, m_lo as checked ints."""
    ap, lda = _rows(rows_a, "rows_a")
    bp, ldb = _rows(rows_b, "rows_b")
    if rows_a.shape[1] != rows_b.shape[1]:
        raise ValueError("rows_a and rows_b differ in dimension")
    m, m_lo = int(m), int(m_lo)
    if m < 1 or m_lo < 0 or m > _MAX_ITEMS:
        raise ValueError("%s: m=%d must be in [1, 2^31) and m_lo=%d >= 0" % (who, m, m_lo))
    return ap, lda, bp, ldb, rows_a.shape[1], m, m_lo


def center_rows(queries, qlayout="ND", center=None):
    """fp32 ``[nq, d]`` row-major: ``queries - center`` (one fp32 subtraction per element; a copy without ``center``) --
    the query rows ``x_q`` of a range search (``mdx_center_rows``)."""
    qp = _dev(queries, torch.float32, "queries")
    nq, d, lay = _layout(queries, qlayout, "queries")
    if nq < 1 or d < 1:
        raise ValueError("queries must be non-empty, got %d x %d" % (nq, d))
    cp = _center(center, d)
    out = torch.empty((nq, d), dtype=torch.float32, device=queries.device)
    with _on(queries):
        check(_lib.lib().mdx_center_rows(qp, nq, d, lay, cp, _vp(out.data_ptr()), _stream()), "mdx_center_rows")
    return out


def join_stats(index, rows):
    """fp32 ``[n, 4]``: the per-row factors ``{p, q, r, w}`` of the pruning bound (``mdx_join_stats``, include/mdx.h) of an int8
    ``index`` and the fp32 rows ``[n, d]`` it was built from (rows contiguous, any stride)."""
    if not isinstance(index, DescriptorIndex) or index._h is None:
        raise ValueError("join_stats: an open DescriptorIndex is needed")
    if index.storage != "i8":
        raise ValueError("join_stats: pruning needs an int8 index (an %s one has no bound)" % index.storage)
    rp, ld = _rows(rows, "rows")
    if tuple(rows.shape) != (index.n, index.d):
        raise ValueError("rows must be the index's [%d, %d] rows, got %s" % (index.n, index.d, tuple(rows.shape)))
    stats = torch.empty((index.n, 4), dtype=torch.float32, device=rows.device)
    with _on(rows):
        check(_lib.lib().mdx_join_stats(index._h, rp, ld, _vp(stats.data_ptr()), _stream()), "mdx_join_stats")
    return stats


def join_candidates(a, stats_a, b, stats_b, threshold, a_lo=0, a_hi=None, symmetric=False, capacity=1 << 20):
    """``(pairs uint64-as-int64 [min(count, capacity)], count)``: the candidates ``i << 32 | j`` of the join kernel
    (``mdx_join_candidates``) for rows ``[a_lo, a_hi)`` of int8 index ``a`` against every row of ``b`` (``symmetric``: a is b,
    j > i).  ``count`` may exceed ``capacity``: then call again with ``capacity >= count``.  Synchronises the stream (reads
    the count)."""
    tau = _tau(threshold)
    a_lo, a_hi = _join_operands("join_candidates", a, stats_a, b, stats_b, a_lo, a_hi)
    if symmetric and a is not b:
        raise ValueError("join_candidates: the self-join joins one index with itself")
    _capacity(capacity)
    pairs = torch.empty(max(capacity, 1), dtype=torch.int64, device=a.device)
    count = torch.zeros(1, dtype=torch.int64, device=a.device)
    with _on(pairs):
        check(_lib.lib().mdx_join_candidates(a._h, _vp(stats_a.data_ptr()), b._h, _vp(stats_b.data_ptr()), a_lo, a_hi, int(bool(symmetric)),
                                             tau, _vp(pairs.data_ptr()), capacity, _vp(count.data_ptr()), _stream()), "mdx_join_candidates")
    c = int(count.item())
    return pairs[:min(c, capacity)], c


def join_resolve(rows_a, rows_b, pairs, threshold, m_lo, m):
    """``(offsets int64 [m + 1], ids int64 [hits], scores fp32 [hits])``: the exact chains of the candidate ``pairs`` (int64
    ``i << 32 | j``, unique, rows i in ``[m_lo, m_lo + m)``) of ``rows_a`` x ``rows_b``, the hits ``>= threshold`` and their CSR
    over rows ``m_lo ..`` in rank order (``mdx_join_resolve``).  Synchronises the stream (reads the hits)."""
    tau = _tau(threshold)
    ap, lda, bp, ldb, d, m, m_lo = _pair_rows(rows_a, rows_b, m, m_lo, "join_resolve")
    dev = rows_a.device
    P = pairs.numel()
    if P == 0:
        return (torch.zeros(m + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev))
    _dev(pairs, torch.int64, "pairs")
    if P > _MAX_ITEMS:
        raise ValueError("join_resolve: %d pairs, at most 2^31 - 1 per call" % P)
    h = _lib.lib()
    need = h.mdx_join_resolve_workspace(P, m)
    ws = _workspace(need, dev)
    offsets = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ids = torch.empty(P, dtype=torch.int64, device=dev)
    scores = torch.empty(P, dtype=torch.float32, device=dev)
    with _on(rows_a):
        check(h.mdx_join_resolve(ap, lda, bp, ldb, d, _vp(pairs.data_ptr()), P, tau, m_lo, m, _vp(offsets.data_ptr()),
                                 _vp(ids.data_ptr()), _vp(scores.data_ptr()), _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_join_resolve")
    hits = int(offsets[m].item())
    return offsets, ids[:hits], scores[:hits]


# ------------------------------------------------------------- exact kNN join

KNN_JOIN_MAX_K = 64               # include/mdx.h MDX_KNN_JOIN_MAX_K: the k largest bounds of 128 rows are kept in LDS
KNN_MAX_SLICES = 64


def _knn_k(who, k, nb=None):
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("%s: k must be an integer >= 1, got %r" % (who, k))
    if k > KNN_JOIN_MAX_K:
        raise ValueError("%s: k=%d, at most KNN_JOIN_MAX_K = %d neighbours per row" % (who, k, KNN_JOIN_MAX_K))
    if nb is not None and k > nb:
        raise ValueError("%s: k=%d > the %d rows of b" % (who, k, nb))
    return k


def knn_bounds(a, stats_a, b, stats_b, lo, hi, k, slices=0):
    """fp32 ``[hi - lo]``: the thresholds ``t_i`` of the exact kNN join (``mdx_knn_bounds``, include/mdx.h "exact kNN join") of
    rows ``[lo, hi)`` of int8 index ``a`` against every row of ``b`` -- a lower bound of each row's exact k-th score, the k-th
    largest of its per-pair lower bounds (-inf where fewer than k pairs have one).  ``slices``: 0 = automatic, or 1 .. 64
    slices of b's row blocks per block of a; every value gives the same bits."""
    lo, hi = _join_operands("knn_bounds", a, stats_a, b, stats_b, lo, hi)
    k = _knn_k("knn_bounds", k, b.n)
    if isinstance(slices, bool) or not isinstance(slices, int) or not 0 <= slices <= KNN_MAX_SLICES:
        raise ValueError("knn_bounds: slices must be 0 (automatic) or an integer in [1, %d], got %r" % (KNN_MAX_SLICES, slices))
    h = _lib.lib()
    t = torch.empty(hi - lo, dtype=torch.float32, device=a.device)
    ws = _workspace(h.mdx_knn_bounds_workspace(hi - lo, k, b.n, slices), a.device)
    with _on(t):
        check(h.mdx_knn_bounds(a._h, _vp(stats_a.data_ptr()), b._h, _vp(stats_b.data_ptr()), lo, hi, k, slices, _vp(t.data_ptr()),
                               _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_knn_bounds")
    return t


def join_candidates_rows(a, stats_a, b, stats_b, taus, a_lo=0, a_hi=None, capacity=1 << 20):
    """:func:`join_candidates` (not symmetric) with the threshold of row i read from ``taus`` (fp32 ``[a_hi - a_lo]`` on the
    device; -inf or NaN keeps every pair of the row) (``mdx_join_candidates_rows``): ``(pairs, count)`` as there.  Synchronises
    the stream (reads the count)."""
    a_lo, a_hi = _join_operands("join_candidates_rows", a, stats_a, b, stats_b, a_lo, a_hi)
    tp = _dev(taus, torch.float32, "taus")
    if taus.dim() != 1 or taus.shape[0] != a_hi - a_lo or not taus.is_contiguous():
        raise ValueError("taus must be a contiguous [%d] tensor, one threshold per row" % (a_hi - a_lo))
    _capacity(capacity)
    pairs = torch.empty(max(capacity, 1), dtype=torch.int64, device=a.device)
    count = torch.zeros(1, dtype=torch.int64, device=a.device)
    with _on(pairs):
        check(_lib.lib().mdx_join_candidates_rows(a._h, _vp(stats_a.data_ptr()), b._h, _vp(stats_b.data_ptr()), a_lo, a_hi, tp,
                                                  _vp(pairs.data_ptr()), capacity, _vp(count.data_ptr()), _stream()),
              "mdx_join_candidates_rows")
    c = int(count.item())
    return pairs[:min(c, capacity)], c


def knn_resolve(rows_a, rows_b, pairs, m_lo, m, k):
    """``(ids int64 [m, k], scores fp32 [m, k], counts int32 [m])``: the exact chains of the candidate ``pairs`` (int64
    ``i << 32 | j``, unique, rows i in ``[m_lo, m_lo + m)``) of ``rows_a`` x ``rows_b`` and the first ``k`` of every row in rank
    order (``mdx_knn_resolve``); ``counts``: the candidates of each row -- where that is below k (thresholds that were not
    :func:`knn_bounds`') the tail is id -1 / score NaN."""
    ap, lda, bp, ldb, d, m, m_lo = _pair_rows(rows_a, rows_b, m, m_lo, "knn_resolve")
    k = _knn_k("knn_resolve", k)
    _dev(pairs, torch.int64, "pairs")
    P = pairs.numel()
    if not 1 <= P <= _MAX_ITEMS:
        raise ValueError("knn_resolve: %d pairs, between 1 and 2^31 - 1 per call" % P)
    dev = rows_a.device
    h = _lib.lib()
    ws = _workspace(h.mdx_knn_resolve_workspace(P, m), dev)
    ids = torch.empty((m, k), dtype=torch.int64, device=dev)
    scores = torch.empty((m, k), dtype=torch.float32, device=dev)
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    with _on(rows_a):
        check(h.mdx_knn_resolve(ap, lda, bp, ldb, d, _vp(pairs.data_ptr()), P, m_lo, m, k, _vp(ids.data_ptr()), _vp(scores.data_ptr()),
                                _vp(counts.data_ptr()), _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_knn_resolve")
    return ids, scores, counts


# ------------------------------------------------------------- near-duplicate groups

GROUPS_MAX_T = 8                  # include/mdx.h MDX_GROUPS_MAX_T: thresholds (levels of the forest) of one pass
GROUPS_GAVE_UP, GROUPS_OUT_OF_RANGE = 1, 2       # the flags of status[3]


def _taus(thresholds):
    """The thresholds of a groups call as a ctypes float array (the C ABI reads them on the host) and their number."""
    if isinstance(thresholds, (bool, int, float)):
        thresholds = [thresholds]
    if not isinstance(thresholds, (list, tuple)) or not 1 <= len(thresholds) <= GROUPS_MAX_T:
        raise ValueError("thresholds: a number or a sequence of 1 to GROUPS_MAX_T = %d numbers, got %r" % (GROUPS_MAX_T, thresholds))
    vals = [_tau(t) for t in thresholds]
    return (ctypes.c_float * len(vals))(*vals), len(vals)


def _forest(parent, status):
    """(parent pointer, status pointer, T, n) of a forest as :func:`groups_init` makes it."""
    pp = _dev(parent, torch.int32, "parent")
    sp = _dev(status, torch.int64, "status")
    if parent.dim() != 2 or parent.shape[0] < 1 or parent.shape[0] > GROUPS_MAX_T or parent.shape[1] < 1:
        raise ValueError("parent must be the int32 [T, n] forest of groups_init, got %s" % (tuple(parent.shape),))
    if status.dim() != 1 or status.shape[0] != 4:
        raise ValueError("status must be the int64 [4] words of groups_init, got %s" % (tuple(status.shape),))
    return pp, sp, parent.shape[0], parent.shape[1]


def groups_init(levels, n, device):
    """``(parent int32 [levels, n], status int64 [4])``: a forest of singletons, ``parent[t, i] = i``, and zeroed counters
    (``mdx_groups_init``, include/mdx.h "near-duplicate groups")."""
    for name, v, hi in (("levels", levels, GROUPS_MAX_T), ("n", n, _MAX_ITEMS)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError("groups_init: %s must be an integer in [1, %d], got %r" % (name, hi, v))
    parent = torch.empty((levels, n), dtype=torch.int32, device=device)
    status = torch.empty(4, dtype=torch.int64, device=device)
    with _on(parent):
        check(_lib.lib().mdx_groups_init(_vp(parent.data_ptr()), levels, n, _vp(status.data_ptr()), _stream()), "mdx_groups_init")
    return parent, status


def groups_union_pairs(rows, pairs, thresholds, parent, status):
    """Unites, in every level t of ``parent`` whose ``thresholds[t]`` the exact chain of the pair reaches, the two rows of each of
    ``pairs`` (int64 ``i << 32 | j`` as :func:`join_candidates` writes them, any order, duplicates allowed) of ``rows`` fp32
    ``[n, d]`` (``mdx_groups_union_pairs``).  Enqueues only."""
    rp, ld = _rows(rows, "rows")
    tv, T = _taus(thresholds)
    pp, sp, levels, n = _forest(parent, status)
    if levels != T or rows.shape[0] != n:
        raise ValueError("groups_union_pairs: %d thresholds and %d rows for a forest of [%d, %d]" % (T, rows.shape[0], levels, n))
    kp = _dev(pairs, torch.int64, "pairs")
    P = pairs.numel()
    if pairs.dim() != 1 or not 1 <= P <= _MAX_ITEMS:
        raise ValueError("groups_union_pairs: pairs must be a 1-d tensor of 1 to 2^31 - 1 pairs, got %s" % (tuple(pairs.shape),))
    with _on(rows):
        check(_lib.lib().mdx_groups_union_pairs(rp, ld, rows.shape[1], kp, P, tv, T, pp, n, sp, _stream()), "mdx_groups_union_pairs")


def groups_union_dense(scores, row_base, col_base, thresholds, parent, status):
    """The same for a dense fp32 score block ``[m, ncols]`` (rows contiguous, any stride) whose entry (r, c) is the pair
    ``(row_base + r, col_base + c)``: an edge of level t iff ``s >= thresholds[t]`` and the column's row id is the larger
    (``mdx_groups_union_dense``).  Enqueues only."""
    sp_, ld = _rows(scores, "scores")
    tv, T = _taus(thresholds)
    pp, sp, levels, n = _forest(parent, status)
    m, ncols = scores.shape
    for name, v in (("row_base", row_base), ("col_base", col_base)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError("groups_union_dense: %s must be an integer >= 0, got %r" % (name, v))
    if levels != T or m < 1 or ncols < 1 or row_base + m > n or col_base + ncols > n:
        raise ValueError("groups_union_dense: %d thresholds, rows [%d, +%d) x columns [%d, +%d) for a forest of [%d, %d]"
                         % (T, row_base, m, col_base, ncols, levels, n))
    with _on(scores):
        check(_lib.lib().mdx_groups_union_dense(sp_, m, ncols, ld, row_base, col_base, tv, T, pp, n, sp, _stream()), "mdx_groups_union_dense")


def groups_labels(parent):
    """int64 ``[T, n]``: the label of every row in every level, the smallest id of its group (``mdx_groups_labels``); a buffer
    of its own, ``parent`` is left as it is."""
    pp = _dev(parent, torch.int32, "parent")
    if parent.dim() != 2 or parent.shape[0] < 1 or parent.shape[0] > GROUPS_MAX_T or parent.shape[1] < 1:
        raise ValueError("parent must be the int32 [T, n] forest of groups_init, got %s" % (tuple(parent.shape),))
    T, n = parent.shape
    labels = torch.empty((T, n), dtype=torch.int64, device=parent.device)
    with _on(parent):
        check(_lib.lib().mdx_groups_labels(pp, T, n, _vp(labels.data_ptr()), _stream()), "mdx_groups_labels")
    return labels


def groups_status(status):
    """``{"chains", "edges", "hooks", "flags"}`` of a forest's status words.  Synchronises the stream (reads them)."""
    _dev(status, torch.int64, "status")
    if status.dim() != 1 or status.shape[0] != 4:
        raise ValueError("status must be the int64 [4] words of groups_init, got %s" % (tuple(status.shape),))
    chains, edges, hooks, flags = (int(v) for v in status.cpu().tolist())
    return {"chains": chains, "edges": edges, "hooks": hooks, "flags": flags}


def range_select(scores, threshold, diag=None, capacity=None):
    """``(offsets int64 [m + 1], ids int64 [hits], scores fp32 [hits])``: the deterministic threshold compaction of an fp32 score
    matrix ``[m, n]`` (rows contiguous, any stride) into the CSR of include/mdx.h (``mdx_range_select``): hits ``s >= threshold``,
    for ``diag`` not None only ``j > diag + r`` in row r (the upper triangle of a self-join block whose first row is ``diag``).
    Synchronises the stream; with ``capacity`` too small for the hits it runs again at their exact number."""
    tau = _tau(threshold)
    sp, ld = _rows(scores, "scores")
    m, n = scores.shape
    if m < 1 or n < 1 or m > _MAX_ITEMS:
        raise ValueError("range_select: scores must be non-empty, got %d x %d" % (m, n))
    if diag is not None and (isinstance(diag, bool) or not isinstance(diag, int) or diag < 0):
        raise ValueError("diag must be None or an integer >= 0, got %r" % (diag,))
    cap = _capacity(1 << 16 if capacity is None else capacity)
    h = _lib.lib()
    dev = scores.device
    offsets = torch.empty(m + 1, dtype=torch.int64, device=dev)
    while True:
        need = h.mdx_range_select_workspace(m, cap)
        ws = _workspace(need, dev)
        ids = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        vals = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
        with _on(scores):
            check(h.mdx_range_select(sp, m, n, ld, tau, -1 if diag is None else int(diag), _vp(offsets.data_ptr()), _vp(ids.data_ptr()),
                                     _vp(vals.data_ptr()), cap, _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_range_select")
        hits = int(offsets[m].item())
        if hits <= cap:
            return offsets, ids[:hits], vals[:hits]
        if hits > _MAX_ITEMS:
            raise ValueError("range_select: %d hits, more than one call holds (2^31 - 1)" % hits)
        cap = hits


def knn_aggregate(rows, ids, sims, alpha, self_rows=None, eps=1e-6, out=None):
    """fp32 ``[nq, d]``: row q = the L2-normalised ``self_rows[q] + sum_j w_j rows[ids[q, j]]`` with
    ``w_j = sims[q, j] ** alpha`` for a positive similarity and 0 otherwise (``mdx_knn_aggregate``; the contract, its
    summation order and its bit-determinism are in ``include/mdx.h``).  ``ids`` int64 and ``sims`` fp32 are ``[nq, k]``
    (what :func:`topk` returns); an id outside ``[0, n)`` contributes nothing.  ``rows``, ``self_rows`` and ``out`` may be
    row slices of larger matrices; ``out`` must not overlap ``rows`` or ``self_rows``."""
    rp, ld = _rows(rows, "rows")
    n, d = rows.shape
    ip = _dev(ids, torch.int64, "ids")
    sp = _dev(sims, torch.float32, "sims")
    if ids.dim() != 2 or tuple(sims.shape) != tuple(ids.shape):
        raise ValueError("ids and sims must both be [nq, k], got %s and %s" % (tuple(ids.shape), tuple(sims.shape)))
    nq, k = ids.shape
    selfp, ld_self = None, d
    if self_rows is not None:
        selfp, ld_self = _rows(self_rows, "self_rows")
        if tuple(self_rows.shape) != (nq, d):
            raise ValueError("self_rows must be [%d,%d], got %s" % (nq, d, tuple(self_rows.shape)))
    if out is None:
        out = torch.empty((nq, d), dtype=torch.float32, device=rows.device)
    elif tuple(out.shape) != (nq, d):
        raise ValueError("out must be [%d,%d]" % (nq, d))
    op, ld_out = _rows(out, "out")
    with _on(rows):
        check(_lib.lib().mdx_knn_aggregate(rp, n, d, ld, ip, sp, nq, k, selfp, ld_self, float(alpha), float(eps), op, ld_out,
                                           _stream()), "mdx_knn_aggregate")
    return out


DIFFUSION_MAX_NQ = 256        # queries per mdx_diffusion launch (64 lanes x float4)


def _finite(x, what, lo=0.0, hi=None):
    """``x`` as a float, ValueError unless it is a finite real number in ``[lo, hi)`` (``hi`` None: no upper bound)."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < lo or (hi is not None and x >= hi):
        raise ValueError("%s must be a finite number in [%g, %s), got %r" % (what, lo, "inf" if hi is None else "%g" % hi, x))
    return float(x)


def knn_graph(ids, sims, gamma):
    """The normalised mutual kNN graph of diffusion (``mdx_knn_graph``; the definition is in ``include/mdx.h``) from the
    database's own top-k lists: ``ids`` int64 and ``sims`` fp32 ``[N, k]`` (what :func:`topk` returns for every row against
    the whole database).  Returns ``(cols int32 [N, k], vals fp32 [N, k], counts int32 [N])``, row i's edges first in list
    order.  An id outside ``[0, N)`` is no edge."""
    gamma = _finite(gamma, "gamma")
    ip = _dev(ids, torch.int64, "ids")
    sp = _dev(sims, torch.float32, "sims")
    if ids.dim() != 2 or tuple(sims.shape) != tuple(ids.shape):
        raise ValueError("ids and sims must both be [N, k], got %s and %s" % (tuple(ids.shape), tuple(sims.shape)))
    n, k = ids.shape
    if n < 1 or k < 1:
        raise ValueError("ids must be a non-empty [N, k], got %s" % (tuple(ids.shape),))
    h = _lib.lib()
    cols = torch.empty((n, k), dtype=torch.int32, device=ids.device)
    vals = torch.empty((n, k), dtype=torch.float32, device=ids.device)
    counts = torch.empty((n,), dtype=torch.int32, device=ids.device)
    nbytes = h.mdx_knn_graph_workspace(n)
    ws = _workspace(nbytes, ids.device)
    with _on(ids):
        check(h.mdx_knn_graph(ip, sp, n, k, gamma, _vp(cols.data_ptr()), _vp(vals.data_ptr()), _vp(counts.data_ptr()),
                              _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_knn_graph")
    return cols, vals, counts


def diffusion(graph, scores, seed_ids, seed_sims, gamma, alpha, iters, tol, out=None, return_residual=False):
    """Diffusion scores ``[nq, N]`` (``mdx_diffusion``: CG on ``(I - alpha S) f = y``, the definition in ``include/mdx.h``):
    ``f_j`` where positive, else ``scores - 3``.  ``graph`` is ``(cols, vals, counts)`` of :func:`knn_graph` or an object
    with those attributes; ``scores`` the first-stage ``[nq, N]`` scores (rows contiguous; a row slice is fine);
    ``seed_ids`` int64 / ``seed_sims`` fp32 ``[nq, kq]`` (:func:`topk` of the scores).  ``out`` may be ``scores`` (in
    place).  More than 256 queries run in groups of 256, which gives the same bits (a query's outputs do not depend on the
    other queries of a launch).  With ``return_residual``: ``(out, residual fp32 [nq], steps int32 [nq])``."""
    cols, vals, counts = graph if isinstance(graph, tuple) else (graph.cols, graph.vals, graph.counts)
    gamma = _finite(gamma, "gamma")
    alpha = _finite(alpha, "alpha", 0.0, 1.0)
    tol = _finite(tol, "tol")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError("iters must be an integer >= 1, got %r" % (iters,))
    _dev(cols, torch.int32, "cols")
    _dev(vals, torch.float32, "vals")
    _dev(counts, torch.int32, "counts")
    if cols.dim() != 2 or tuple(vals.shape) != tuple(cols.shape) or tuple(counts.shape) != (cols.shape[0],):
        raise ValueError("graph: cols / vals [N, k] and counts [N] expected, got %s, %s, %s"
                         % (tuple(cols.shape), tuple(vals.shape), tuple(counts.shape)))
    n, k = cols.shape
    sp, ld = _rows(scores, "scores")
    nq = scores.shape[0]
    if scores.shape[1] != n:
        raise ValueError("scores must be [nq, %d], got %s" % (n, tuple(scores.shape)))
    _dev(seed_ids, torch.int64, "seed_ids")
    _dev(seed_sims, torch.float32, "seed_sims")
    if seed_ids.dim() != 2 or tuple(seed_sims.shape) != tuple(seed_ids.shape) or seed_ids.shape[0] != nq:
        raise ValueError("seed_ids and seed_sims must both be [%d, kq], got %s and %s"
                         % (nq, tuple(seed_ids.shape), tuple(seed_sims.shape)))
    kq = seed_ids.shape[1]
    if out is None:
        out = torch.empty((nq, n), dtype=torch.float32, device=scores.device)
    elif tuple(out.shape) != (nq, n):
        raise ValueError("out must be [%d,%d]" % (nq, n))
    _, ld_out = _rows(out, "out")
    residual = torch.empty((nq,), dtype=torch.float32, device=scores.device) if return_residual else None
    steps = torch.empty((nq,), dtype=torch.int32, device=scores.device) if return_residual else None
    h = _lib.lib()
    group = min(nq, DIFFUSION_MAX_NQ)
    nbytes = h.mdx_diffusion_workspace(n, group)
    ws = _workspace(nbytes, scores.device)
    with _on(scores):
        for q0 in range(0, nq, group):
            q1 = min(nq, q0 + group)
            check(h.mdx_diffusion(_vp(cols.data_ptr()), _vp(vals.data_ptr()), _vp(counts.data_ptr()), n, k,
                                  _vp(scores[q0].data_ptr()), ld, _vp(seed_ids[q0].data_ptr()), _vp(seed_sims[q0].data_ptr()),
                                  q1 - q0, kq, gamma, alpha, iters, tol, _vp(out[q0].data_ptr()), ld_out,
                                  _vp(residual[q0].data_ptr()) if return_residual else None,
                                  _vp(steps[q0].data_ptr()) if return_residual else None, _vp(ws.data_ptr()), ws.numel(),
                                  _stream()), "mdx_diffusion")
    return (out, residual, steps) if return_residual else out


def knn_graph_weights(ids, sims, gamma):
    """The unnormalised affinity W of the diffusion graph (``mdx_knn_graph_weights``): ``(cols int32 [N, k], w fp32 [N, k],
    counts int32 [N])``, cols and counts bit-identical to :func:`knn_graph`'s and ``w = max(s, 0) ** gamma`` before the
    symmetric normalisation.  What :func:`diffusion_truncated` renormalises on each query's subgraph."""
    gamma = _finite(gamma, "gamma")
    ip = _dev(ids, torch.int64, "ids")
    sp = _dev(sims, torch.float32, "sims")
    if ids.dim() != 2 or tuple(sims.shape) != tuple(ids.shape):
        raise ValueError("ids and sims must both be [N, k], got %s and %s" % (tuple(ids.shape), tuple(sims.shape)))
    n, k = ids.shape
    if n < 1 or k < 1:
        raise ValueError("ids must be a non-empty [N, k], got %s" % (tuple(ids.shape),))
    h = _lib.lib()
    cols = torch.empty((n, k), dtype=torch.int32, device=ids.device)
    w = torch.empty((n, k), dtype=torch.float32, device=ids.device)
    counts = torch.empty((n,), dtype=torch.int32, device=ids.device)
    nbytes = h.mdx_knn_graph_workspace(n)
    ws = _workspace(nbytes, ids.device)
    with _on(ids):
        check(h.mdx_knn_graph_weights(ip, sp, n, k, gamma, _vp(cols.data_ptr()), _vp(w.data_ptr()), _vp(counts.data_ptr()),
                                      _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_knn_graph_weights")
    return cols, w, counts


DIFFUSION_MAX_R = 4096            # include/mdx.h MDX_DIFFUSION_MAX_R: the subgraph of a truncated solve lives in LDS
DIFFUSION_TRUNCATED_WORKSPACE_CAP = 1 << 30     # bytes of per-query edge lists one truncated launch may hold


def diffusion_truncated(graph, scores, top_ids, top_sims, kq, gamma, alpha, iters, tol, out=None, return_residual=False):
    """Truncated diffusion scores ``[nq, N]`` (``mdx_diffusion_truncated``, the definition in ``include/mdx.h``): each query's
    CG on the subgraph of its top-R first-stage rows, renormalised there; ``f`` where positive, else ``scores - 3``.
    ``graph`` is ``(cols, w, counts)`` of :func:`knn_graph_weights` or an object with ``cols``, ``wvals`` and ``counts``;
    ``top_ids`` int64 / ``top_sims`` fp32 ``[nq, R]`` (:func:`topk` of the scores with ``k = R``, ``R <= 4096``); the seeds
    are their first ``min(kq, R)`` entries.  ``out`` may be ``scores`` (in place).  Queries run in groups whose workspace
    stays under 1 GiB, which gives the same bits.  With ``return_residual``: ``(out, residual fp32 [nq], steps int32 [nq])``."""
    cols, w, counts = graph if isinstance(graph, tuple) else (graph.cols, graph.wvals, graph.counts)
    gamma = _finite(gamma, "gamma")
    alpha = _finite(alpha, "alpha", 0.0, 1.0)
    tol = _finite(tol, "tol")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError("iters must be an integer >= 1, got %r" % (iters,))
    if isinstance(kq, bool) or not isinstance(kq, int) or kq < 1:
        raise ValueError("kq must be an integer >= 1, got %r" % (kq,))
    if w is None:
        raise ValueError("graph has no unnormalised weights (build it with weights=True)")
    _dev(cols, torch.int32, "cols")
    _dev(w, torch.float32, "w")
    _dev(counts, torch.int32, "counts")
    if cols.dim() != 2 or tuple(w.shape) != tuple(cols.shape) or tuple(counts.shape) != (cols.shape[0],):
        raise ValueError("graph: cols / w [N, k] and counts [N] expected, got %s, %s, %s"
                         % (tuple(cols.shape), tuple(w.shape), tuple(counts.shape)))
    n, k = cols.shape
    sp, ld = _rows(scores, "scores")
    nq = scores.shape[0]
    if scores.shape[1] != n:
        raise ValueError("scores must be [nq, %d], got %s" % (n, tuple(scores.shape)))
    _dev(top_ids, torch.int64, "top_ids")
    _dev(top_sims, torch.float32, "top_sims")
    if top_ids.dim() != 2 or tuple(top_sims.shape) != tuple(top_ids.shape) or top_ids.shape[0] != nq:
        raise ValueError("top_ids and top_sims must both be [%d, R], got %s and %s"
                         % (nq, tuple(top_ids.shape), tuple(top_sims.shape)))
    r = top_ids.shape[1]
    if not 1 <= r <= min(n, DIFFUSION_MAX_R):
        raise ValueError("R = %d must be in [1, min(N, %d)]" % (r, DIFFUSION_MAX_R))
    if out is None:
        out = torch.empty((nq, n), dtype=torch.float32, device=scores.device)
    elif tuple(out.shape) != (nq, n):
        raise ValueError("out must be [%d,%d]" % (nq, n))
    _, ld_out = _rows(out, "out")
    residual = torch.empty((nq,), dtype=torch.float32, device=scores.device) if return_residual else None
    steps = torch.empty((nq,), dtype=torch.int32, device=scores.device) if return_residual else None
    h = _lib.lib()
    group = max(1, min(nq, DIFFUSION_TRUNCATED_WORKSPACE_CAP // h.mdx_diffusion_truncated_workspace(n, k, 1, r)))
    nbytes = h.mdx_diffusion_truncated_workspace(n, k, group, r)
    ws = _workspace(nbytes, scores.device)
    with _on(scores):
        for q0 in range(0, nq, group):
            q1 = min(nq, q0 + group)
            check(h.mdx_diffusion_truncated(_vp(cols.data_ptr()), _vp(w.data_ptr()), _vp(counts.data_ptr()), n, k,
                                            _vp(scores[q0].data_ptr()), ld, _vp(top_ids[q0].data_ptr()),
                                            _vp(top_sims[q0].data_ptr()), q1 - q0, r, kq, gamma, alpha, iters, tol,
                                            _vp(out[q0].data_ptr()), ld_out,
                                            _vp(residual[q0].data_ptr()) if return_residual else None,
                                            _vp(steps[q0].data_ptr()) if return_residual else None, _vp(ws.data_ptr()),
                                            ws.numel(), _stream()), "mdx_diffusion_truncated")
    return (out, residual, steps) if return_residual else out


# ------------------------------------------------------------------ k-reciprocal re-ranking

KRECIP_MAX_K1 = 64                # include/mdx_krecip.h MDX_KRECIP_MAX_K1: one lane per list entry
KRECIP_MAX_NNZ = 4096             # MDX_KRECIP_MAX_NNZ: k2 * k1 * (1 + ceil(k1 / 2)) at most; a code lives in LDS
KRECIP_MAX_R = 4096               # MDX_KRECIP_MAX_R: the shortlist of one query


def _krecip_lists(ids, who):
    """(n, k) of the database lists ``ids`` int64 ``[N, k]``, ``k <= KRECIP_MAX_K1``."""
    _dev(ids, torch.int64, "ids")
    if ids.dim() != 2 or ids.shape[0] < 1 or not 1 <= ids.shape[1] <= KRECIP_MAX_K1:
        raise ValueError("%s: ids must be [N, k] with N >= 1 and 1 <= k <= %d, got %s" % (who, KRECIP_MAX_K1, tuple(ids.shape)))
    return ids.shape


def _krecip_k2(k, k2, who):
    if isinstance(k2, bool) or not isinstance(k2, int) or not 1 <= k2 <= k:
        raise ValueError("%s: k2 must be an integer in [1, k] = [1, %d], got %r" % (who, k, k2))
    if k2 * k * (1 + (k + 1) // 2) > KRECIP_MAX_NNZ:
        raise ValueError("%s: k2 * k * (1 + ceil(k / 2)) = %d > KRECIP_MAX_NNZ = %d (k=%d k2=%d)"
                         % (who, k2 * k * (1 + (k + 1) // 2), KRECIP_MAX_NNZ, k, k2))


def _krecip_sets(sets, n, k, who):
    rk, rk_counts, rh, rh_counts = sets
    h = (k + 1) // 2
    for t, name in ((rk, "rk"), (rk_counts, "rk_counts"), (rh, "rh"), (rh_counts, "rh_counts")):
        _dev(t, torch.int32, name)
    if tuple(rk.shape) != (n, k) or tuple(rh.shape) != (n, h) or tuple(rk_counts.shape) != (n,) or tuple(rh_counts.shape) != (n,):
        raise ValueError("%s: sets of krecip_sets expected (rk [%d, %d], rk_counts [%d], rh [%d, %d], rh_counts [%d]), got %s, %s, %s, %s"
                         % (who, n, k, n, n, h, n, tuple(rk.shape), tuple(rk_counts.shape), tuple(rh.shape), tuple(rh_counts.shape)))
    return [_vp(t.data_ptr()) for t in sets]


def _krecip_csr(csr, n, who, what, values=True):
    """(offsets, cols, vals pointers, nnz) of a CSR ``(offsets int64 [n + 1], cols int32 [nnz], vals fp32 [nnz])``."""
    offsets, cols, vals = csr
    _dev(offsets, torch.int64, what + " offsets")
    _dev(cols, torch.int32, what + " cols")
    if values:
        _dev(vals, torch.float32, what + " vals")
    if tuple(offsets.shape) != (n + 1,) or cols.dim() != 1 or (values and tuple(vals.shape) != tuple(cols.shape)):
        raise ValueError("%s: %s CSR expected (offsets [%d], cols [nnz], vals [nnz]), got %s, %s, %s"
                         % (who, what, n + 1, tuple(offsets.shape), tuple(cols.shape), tuple(vals.shape) if values else None))
    nnz = cols.shape[0]
    return (_vp(offsets.data_ptr()), _vp(cols.data_ptr()) if nnz else None, _vp(vals.data_ptr()) if nnz and values else None, nnz)


def krecip_sets(ids):
    """The reciprocal sets of the database lists ``ids`` int64 ``[N, k]`` (``mdx_krecip_sets``; the definition is in
    ``include/mdx_krecip.h``): ``(rk int32 [N, k], rk_counts int32 [N], rh int32 [N, ceil(k / 2)], rh_counts int32 [N])``, each
    row's members first in list order, then -1."""
    n, k = _krecip_lists(ids, "krecip_sets")
    h = (k + 1) // 2
    rk = torch.empty((n, k), dtype=torch.int32, device=ids.device)
    rk_counts = torch.empty((n,), dtype=torch.int32, device=ids.device)
    rh = torch.empty((n, h), dtype=torch.int32, device=ids.device)
    rh_counts = torch.empty((n,), dtype=torch.int32, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_krecip_sets(_vp(ids.data_ptr()), n, k, _vp(rk.data_ptr()), _vp(rk_counts.data_ptr()),
                                         _vp(rh.data_ptr()), _vp(rh_counts.data_ptr()), _stream()), "mdx_krecip_sets")
    return rk, rk_counts, rh, rh_counts


def krecip_raw_offsets(sets):
    """``offsets`` int64 ``[N + 1]`` of the raw codes (``mdx_krecip_raw_offsets``: count pass and scan on the device) from the
    ``sets`` of :func:`krecip_sets`.  ``offsets[N]`` is the nnz; nothing is read back here."""
    rk = sets[0]
    _dev(rk, torch.int32, "rk")
    if rk.dim() != 2 or rk.shape[0] < 1 or not 1 <= rk.shape[1] <= KRECIP_MAX_K1:
        raise ValueError("krecip_raw_offsets: rk must be [N, k] with N >= 1 and 1 <= k <= %d, got %s" % (KRECIP_MAX_K1, tuple(rk.shape)))
    n, k = rk.shape
    ptrs = _krecip_sets(sets, n, k, "krecip_raw_offsets")
    offsets = torch.empty((n + 1,), dtype=torch.int64, device=rk.device)
    with _on(rk):
        check(_lib.lib().mdx_krecip_raw_offsets(n, k, *ptrs, _vp(offsets.data_ptr()), _stream()), "mdx_krecip_raw_offsets")
    return offsets


def krecip_raw_fill(rows, ids, sims, sets, offsets, nnz):
    """``(cols int32 [nnz], vals fp32 [nnz])`` of the raw codes (``mdx_krecip_raw_fill``): ``rows`` fp32 ``[N, D]`` (contiguous
    rows; a column slice is fine), the lists ``ids`` / ``sims`` ``[N, k]``, the ``sets`` of :func:`krecip_sets`, ``offsets`` of
    :func:`krecip_raw_offsets` and ``nnz = offsets[N]``."""
    n, k = _krecip_lists(ids, "krecip_raw_fill")
    _dev(sims, torch.float32, "sims")
    if tuple(sims.shape) != (n, k):
        raise ValueError("krecip_raw_fill: sims must be [%d, %d] as ids, got %s" % (n, k, tuple(sims.shape)))
    rp, ld = _rows(rows, "rows")
    if rows.shape[0] != n:
        raise ValueError("krecip_raw_fill: rows must be [%d, D], got %s" % (n, tuple(rows.shape)))
    ptrs = _krecip_sets(sets, n, k, "krecip_raw_fill")
    _dev(offsets, torch.int64, "offsets")
    if tuple(offsets.shape) != (n + 1,) or isinstance(nnz, bool) or not isinstance(nnz, int) or nnz < 0:
        raise ValueError("krecip_raw_fill: offsets int64 [%d] and an integer nnz >= 0 expected, got %s and %r"
                         % (n + 1, tuple(offsets.shape), nnz))
    cols = torch.empty((nnz,), dtype=torch.int32, device=ids.device)
    vals = torch.empty((nnz,), dtype=torch.float32, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_krecip_raw_fill(rp, ld, rows.shape[1], _vp(ids.data_ptr()), _vp(sims.data_ptr()), n, k, *ptrs,
                                             _vp(offsets.data_ptr()), _vp(cols.data_ptr()) if nnz else None,
                                             _vp(vals.data_ptr()) if nnz else None, nnz, _stream()), "mdx_krecip_raw_fill")
    return cols, vals


def krecip_expand_offsets(ids, k2, raw):
    """``offsets`` int64 ``[N + 1]`` of the expanded codes (``mdx_krecip_expand_offsets``) from the raw CSR ``raw = (offsets,
    cols, vals)`` (``vals`` is not read and may be None)."""
    n, k = _krecip_lists(ids, "krecip_expand_offsets")
    _krecip_k2(k, k2, "krecip_expand_offsets")
    ro, rc, _, rnnz = _krecip_csr(raw, n, "krecip_expand_offsets", "raw", values=False)
    offsets = torch.empty((n + 1,), dtype=torch.int64, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_krecip_expand_offsets(_vp(ids.data_ptr()), n, k, k2, ro, rc, rnnz, _vp(offsets.data_ptr()), _stream()),
              "mdx_krecip_expand_offsets")
    return offsets


def krecip_expand_fill(ids, k2, raw, offsets, nnz):
    """``(cols int32 [nnz], vals fp32 [nnz])`` of the expanded codes (``mdx_krecip_expand_fill``), ``offsets`` of
    :func:`krecip_expand_offsets` and ``nnz = offsets[N]``."""
    n, k = _krecip_lists(ids, "krecip_expand_fill")
    _krecip_k2(k, k2, "krecip_expand_fill")
    ro, rc, rv, rnnz = _krecip_csr(raw, n, "krecip_expand_fill", "raw")
    _dev(offsets, torch.int64, "offsets")
    if tuple(offsets.shape) != (n + 1,) or isinstance(nnz, bool) or not isinstance(nnz, int) or nnz < 0:
        raise ValueError("krecip_expand_fill: offsets int64 [%d] and an integer nnz >= 0 expected, got %s and %r"
                         % (n + 1, tuple(offsets.shape), nnz))
    cols = torch.empty((nnz,), dtype=torch.int32, device=ids.device)
    vals = torch.empty((nnz,), dtype=torch.float32, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_krecip_expand_fill(_vp(ids.data_ptr()), n, k, k2, ro, rc, rv, rnnz, _vp(offsets.data_ptr()),
                                                _vp(cols.data_ptr()) if nnz else None, _vp(vals.data_ptr()) if nnz else None, nnz,
                                                _stream()), "mdx_krecip_expand_fill")
    return cols, vals


def krecip_rerank(half_sets, kth, k, k2, raw, expanded, scores, top_ids, lam, out=None):
    """k-reciprocal scores ``[nq, N]`` (``mdx_krecip_rerank``; the definition is in ``include/mdx_krecip.h``): for the rows of
    each query's shortlist ``top_ids`` int64 ``[nq, R]`` (:func:`topk` of ``scores``, ``R <= 4096``)
    ``(1 - lam) * m / (2 - m) + lam * (1 + s) / 2``, ``m`` the min-sum of the query's code and the row's; elsewhere
    ``scores - 3``.  ``half_sets = (rh, rh_counts)`` of :func:`krecip_sets`, ``kth`` fp32 ``[N]`` the k-th score of every
    database list, ``raw`` / ``expanded`` the two CSRs.  ``out`` may be ``scores`` (in place).  Reads nothing back."""
    rh, rh_counts = half_sets
    _dev(rh, torch.int32, "rh")
    _dev(rh_counts, torch.int32, "rh_counts")
    _dev(kth, torch.float32, "kth")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KRECIP_MAX_K1:
        raise ValueError("krecip_rerank: k must be an integer in [1, %d], got %r" % (KRECIP_MAX_K1, k))
    _krecip_k2(k, k2, "krecip_rerank")
    lam = _finite(lam, "lam", 0.0, None)
    if lam > 1.0:
        raise ValueError("lam must be in [0, 1], got %r" % (lam,))
    n, h = kth.shape[0], (k + 1) // 2
    if kth.dim() != 1 or n < 1 or tuple(rh.shape) != (n, h) or tuple(rh_counts.shape) != (n,):
        raise ValueError("krecip_rerank: rh [N, %d], rh_counts [N] and kth [N] expected, got %s, %s, %s"
                         % (h, tuple(rh.shape), tuple(rh_counts.shape), tuple(kth.shape)))
    ro, rc, rv, rnnz = _krecip_csr(raw, n, "krecip_rerank", "raw")
    eo, ec, ev, ennz = _krecip_csr(expanded, n, "krecip_rerank", "expanded")
    sp, ld = _rows(scores, "scores")
    nq = scores.shape[0]
    if scores.shape[1] != n:
        raise ValueError("scores must be [nq, %d], got %s" % (n, tuple(scores.shape)))
    _dev(top_ids, torch.int64, "top_ids")
    if top_ids.dim() != 2 or top_ids.shape[0] != nq:
        raise ValueError("top_ids must be [%d, R], got %s" % (nq, tuple(top_ids.shape)))
    r = top_ids.shape[1]
    if not 1 <= r <= min(n, KRECIP_MAX_R):
        raise ValueError("R = %d must be in [1, min(N, %d)]" % (r, KRECIP_MAX_R))
    if out is None:
        out = torch.empty((nq, n), dtype=torch.float32, device=scores.device)
    elif tuple(out.shape) != (nq, n):
        raise ValueError("out must be [%d,%d]" % (nq, n))
    op, ld_out = _rows(out, "out")
    h_ = _lib.lib()
    ws = _workspace(h_.mdx_krecip_rerank_workspace(nq, r), scores.device)
    with _on(scores):
        check(h_.mdx_krecip_rerank(_vp(rh.data_ptr()), _vp(rh_counts.data_ptr()), _vp(kth.data_ptr()), n, k, k2, ro, rc, rv, rnnz,
                                   eo, ec, ev, ennz, sp, ld, _vp(top_ids.data_ptr()), nq, r, lam, op, ld_out, _vp(ws.data_ptr()),
                                   ws.numel(), _stream()), "mdx_krecip_rerank")
    return out


# ------------------------------------------------------------------ trainable tail (include/mdx_train.h)

def pool_bwd(feat, pooled, grad_pooled, kind="gem", p=3.0, pool_eps=1e-6):
    """Backward of the global pooling (``mdx_pool_bwd``): ``feat`` [B,C,H,W], ``pooled`` [B,C] (:func:`pool_l2n` with
    ``l2n_eps=None``) and ``grad_pooled`` [B,C] -> ``(grad_feat [B,C,H,W], grad_p [1])``; ``grad_p`` is None for MAC / SPoC."""
    fp = _dev(feat, torch.float32, "feature map")
    if feat.dim() != 4:
        raise ValueError("feature map must be [B,C,H,W]")
    B, C, H, W = feat.shape
    pp, gp = _dev(pooled, torch.float32, "pooled"), _dev(grad_pooled, torch.float32, "grad_pooled")
    if pooled.numel() != B * C or grad_pooled.numel() != B * C:
        raise ValueError("pool_bwd: pooled and grad_pooled must be [%d,%d], got %s and %s" % (B, C, tuple(pooled.shape), tuple(grad_pooled.shape)))
    if kind not in POOL_KINDS:
        raise ValueError("pool_bwd: unknown pooling kind %r, one of %s" % (kind, sorted(POOL_KINDS)))
    grad_feat = torch.empty((B, C, H, W), dtype=torch.float32, device=feat.device)
    h = _lib.lib()
    grad_p = ws = None
    if kind == "gem":
        grad_p = torch.empty((1,), dtype=torch.float32, device=feat.device)
        ws = _workspace(h.mdx_pool_bwd_workspace(B, C), feat.device)
    with _on(feat):
        check(h.mdx_pool_bwd(fp, pp, gp, B, C, H, W, POOL_KINDS[kind], float(p), float(pool_eps), _vp(grad_feat.data_ptr()),
                             _vp(grad_p.data_ptr()) if grad_p is not None else None, _vp(ws.data_ptr()) if ws is not None else None,
                             ws.numel() if ws is not None else 0, _stream()), "mdx_pool_bwd")
    return grad_feat, grad_p


def l2n_rows_bwd(x, grad_out, eps=1e-6):
    """Backward of :func:`l2n_rows_` (``mdx_l2n_rows_bwd``): ``x`` [R,D] the rows BEFORE normalisation (bias added), ``grad_out``
    [R,D] -> ``grad_x`` [R,D].  The bias' gradient is ``grad_x.sum(0)``, the caller's."""
    xp, gp = _dev(x, torch.float32, "x"), _dev(grad_out, torch.float32, "grad_out")
    if x.dim() != 2 or tuple(grad_out.shape) != tuple(x.shape):
        raise ValueError("l2n_rows_bwd: x and grad_out must be [R,D], got %s and %s" % (tuple(x.shape), tuple(grad_out.shape)))
    grad_x = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    with _on(x):
        check(_lib.lib().mdx_l2n_rows_bwd(xp, gp, x.shape[0], x.shape[1], float(eps), _vp(grad_x.data_ptr()), _stream()), "mdx_l2n_rows_bwd")
    return grad_x


def _tuple_loss_args(x, label, nq, min_s, who):
    xp, lp = _dev(x, torch.float32, "x"), _dev(label, torch.float32, "label")
    if x.dim() != 2 or label.dim() != 1 or label.shape[0] != x.shape[1]:
        raise ValueError("%s: x must be [D,N] and label [N], got %s and %s" % (who, tuple(x.shape), tuple(label.shape)))
    d, n = x.shape
    if isinstance(nq, bool) or not isinstance(nq, int) or nq < 1 or n % nq or n // nq < min_s:
        raise ValueError("%s: N = %d columns are not nq = %r tuples of at least %d columns" % (who, n, nq, min_s))
    return xp, lp, d, n


def contrastive_loss(x, label, nq, margin=0.7, eps=1e-6):
    """``LF.contrastive_loss`` and its gradient in one call (``mdx_contrastive_loss``): ``x`` [D,N], ``label`` fp32 [N] in the
    layout of include/mdx_train.h (``nq`` tuples, the query first) -> ``(loss [1], grad_x [D,N])``.  The layout of ``label`` is the
    caller's to check (:func:`mdir_amd.criterion.tuple_layout`)."""
    xp, lp, d, n = _tuple_loss_args(x, label, nq, 2, "contrastive_loss")
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    grad_x = torch.empty((d, n), dtype=torch.float32, device=x.device)
    h = _lib.lib()
    ws = _workspace(h.mdx_tuple_loss_workspace(nq), x.device)
    with _on(x):
        check(h.mdx_contrastive_loss(xp, lp, d, n, nq, float(margin), float(eps), _vp(loss.data_ptr()), _vp(grad_x.data_ptr()),
                                     _vp(ws.data_ptr()), ws.numel(), _stream()), "mdx_contrastive_loss")
    return loss, grad_x


def triplet_loss(x, label, nq, margin=0.1):
    """``LF.triplet_loss`` and its gradient in one call (``mdx_triplet_loss``); arguments and results as :func:`contrastive_loss`,
    tuples of at least three columns with one positive each."""
    xp, lp, d, n = _tuple_loss_args(x, label, nq, 3, "triplet_loss")
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    grad_x = torch.empty((d, n), dtype=torch.float32, device=x.device)
    h = _lib.lib()
    ws = _workspace(h.mdx_tuple_loss_workspace(nq), x.device)
    with _on(x):
        check(h.mdx_triplet_loss(xp, lp, d, n, nq, float(margin), _vp(loss.data_ptr()), _vp(grad_x.data_ptr()), _vp(ws.data_ptr()),
                                 ws.numel(), _stream()), "mdx_triplet_loss")
    return loss, grad_x


# ------------------------------------------------------------------ spherical k-means (include/mdx_kmeans.h)

KMEANS_SEGMENT = 256              # include/mdx_kmeans.h MDX_KMEANS_SEGMENT: members per segment of the chain that defines a cluster's sum


def _kmeans_tensor(t, dtype, who, what, dims):
    """``t`` is a device tensor of ``dtype`` with ``dims`` dimensions, or a ValueError names it."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: %s must be a CUDA/ROCm tensor: the MI355X path has no CPU fallback" % (who, what))
    if t.dtype != dtype:
        raise ValueError("%s: %s must be %s, got %s" % (who, what, dtype, t.dtype))
    if t.dim() != dims or t.numel() < 1:
        raise ValueError("%s: %s must be a non-empty %d-d tensor, got %s" % (who, what, dims, tuple(t.shape)))


def _kmeans_matrix(t, who, what, strided=True):
    """(pointer, row stride) of an fp32 device matrix with contiguous rows (``strided``: at any row stride)."""
    _kmeans_tensor(t, torch.float32, who, what, 2)
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or not (strided or t.is_contiguous()):
        raise ValueError("%s: %s must be %s" % (who, what, "a matrix with contiguous rows" if strided else "contiguous"))
    return _vp(t.data_ptr()), (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def kmeans_argmax(scores, out_labels=None, out_best=None):
    """``(labels int64 [m], best fp32 [m])``: per row of ``scores`` (fp32 ``[m, K]`` on the device, rows contiguous at any stride)
    the first entry of :func:`topk` -- the larger score, equal scores by ascending id, ``-0 == +0``, NaN last -- in one pass
    (``mdx_kmeans_argmax``).  ``out_labels`` / ``out_best``: a tensor to fill, None to allocate one, or False to leave that output
    out (it comes back as None; not both)."""
    who = "kmeans_argmax"
    sp, ld = _kmeans_matrix(scores, who, "scores")
    m, k = scores.shape
    outs = []
    for out, dtype, what in ((out_labels, torch.int64, "out_labels"), (out_best, torch.float32, "out_best")):
        if out is False:
            outs.append(None)
            continue
        if out is None:
            out = torch.empty((m,), dtype=dtype, device=scores.device)
        _kmeans_tensor(out, dtype, who, what, 1)
        if out.shape[0] != m or not out.is_contiguous() or out.device != scores.device:
            raise ValueError("%s: %s must be a contiguous [%d] tensor on %s, got %s on %s" % (who, what, m, scores.device, tuple(out.shape), out.device))
        outs.append(out)
    if outs[0] is None and outs[1] is None:
        raise ValueError("%s: out_labels and out_best are both False: nothing to compute" % who)
    with _on(scores):
        check(_lib.lib().mdx_kmeans_argmax(sp, m, k, ld, _vp(outs[0].data_ptr()) if outs[0] is not None else None,
                                           _vp(outs[1].data_ptr()) if outs[1] is not None else None, _stream()), "mdx_kmeans_argmax")
    return outs[0], outs[1]


def kmeans_sums(rows, members, offsets, k):
    """fp32 ``[k, d]``: the sum of the rows of every cluster (``mdx_kmeans_sums``).  ``rows`` fp32 ``[n, d]`` on the device (rows
    contiguous at any stride), ``members`` int64: the row ids grouped by cluster, ascending inside a cluster (at most ``n`` of them;
    rows may be left out), ``offsets`` int64 ``[k + 1]``: cluster c owns ``members[offsets[c]:offsets[c + 1]]``.  Defined to the bit
    by the segment chain of include/mdx_kmeans.h (``KMEANS_SEGMENT`` members per segment, tests/kmeans_restatement.py); an empty
    cluster gets zeros, an id outside ``[0, n)`` is skipped."""
    who = "kmeans_sums"
    rp, ld = _kmeans_matrix(rows, who, "rows")
    n, d = rows.shape
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("%s: k must be an integer >= 1, got %r" % (who, k))
    _kmeans_tensor(members, torch.int64, who, "members", 1)
    _kmeans_tensor(offsets, torch.int64, who, "offsets", 1)
    if members.shape[0] > n or not members.is_contiguous() or members.device != rows.device:
        raise ValueError("%s: members must be a contiguous tensor of at most n = %d ids on %s, got %s on %s"
                         % (who, n, rows.device, tuple(members.shape), members.device))
    if offsets.shape[0] != k + 1 or not offsets.is_contiguous() or offsets.device != rows.device:
        raise ValueError("%s: offsets must be a contiguous [k + 1] = [%d] tensor on %s, got %s on %s"
                         % (who, k + 1, rows.device, tuple(offsets.shape), offsets.device))
    if members.shape[0] < n:                                   # the library clamps offsets to n: give it n entries to read
        padded = torch.full((n,), -1, dtype=torch.int64, device=rows.device)
        padded[:members.shape[0]] = members
        members = padded
    sums = torch.empty((k, d), dtype=torch.float32, device=rows.device)
    h = _lib.lib()
    ws = _workspace(h.mdx_kmeans_sums_workspace(n, k, d), rows.device)
    with _on(rows):
        check(h.mdx_kmeans_sums(rp, n, d, ld, _vp(members.data_ptr()), _vp(offsets.data_ptr()), k, _vp(sums.data_ptr()), _vp(ws.data_ptr()),
                                ws.numel(), _stream()), "mdx_kmeans_sums")
    return sums


def kmeans_finish(sums, eps=1e-6, previous=None):
    """fp32 ``[k, d]``: every row of ``sums`` divided by its norm plus ``eps`` (``mdx_kmeans_finish``; the L2N rule of
    :func:`l2n_rows_`); a row of zeros becomes the same row of ``previous`` (fp32 ``[k, d]``), or stays zero without one."""
    who = "kmeans_finish"
    sp, _ = _kmeans_matrix(sums, who, "sums", strided=False)
    k, d = sums.shape
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0 or math.isinf(eps):
        raise ValueError("%s: eps must be a finite number >= 0, got %r" % (who, eps))
    pp = None
    if previous is not None:
        pp, _ = _kmeans_matrix(previous, who, "previous", strided=False)
        if tuple(previous.shape) != (k, d) or previous.device != sums.device:
            raise ValueError("%s: previous must be [%d,%d] on %s, got %s on %s" % (who, k, d, sums.device, tuple(previous.shape), previous.device))
    out = torch.empty((k, d), dtype=torch.float32, device=sums.device)
    with _on(sums):
        check(_lib.lib().mdx_kmeans_finish(sp, k, d, float(eps), pp, _vp(out.data_ptr()), _stream()), "mdx_kmeans_finish")
    return out


# ------------------------------------------------------------------ inverted file (include/mdx_ivf.h)

IVF_QUERY_GROUP = 8               # include/mdx_ivf.h MDX_IVF_QUERY_GROUP: entries (query, probe) that share a tile in one workgroup
IVF_TILE = 64                     # include/mdx_ivf.h MDX_IVF_TILE: members of a list per workgroup of the scan


def _ivf_count(x, who, what, lo=1):
    if isinstance(x, bool) or not isinstance(x, int) or x < lo:
        raise ValueError("%s: %s must be an integer >= %d, got %r" % (who, what, lo, x))


def _ivf_vector(t, dtype, who, what, shape, device):
    """``t`` is a contiguous device tensor of ``dtype`` and ``shape`` on ``device``, or a ValueError names it."""
    _kmeans_tensor(t, dtype, who, what, len(shape))
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError("%s: %s must be a contiguous %s tensor on %s, got %s on %s" % (who, what, list(shape), device, tuple(t.shape), t.device))
    return _vp(t.data_ptr())


def _ivf_plan_arg(plan, who, nq, nprobe, k, device):
    _kmeans_tensor(plan, torch.uint8, who, "plan", 1)
    need = _lib.lib().mdx_ivf_plan_workspace(nq, nprobe, k)
    if need == 0:
        raise ValueError("%s: nq = %d, nprobe = %d, K = %d: nprobe must be in [1, K] and nq * nprobe below 2^31" % (who, nq, nprobe, k))
    if not plan.is_contiguous() or plan.device != device:
        raise ValueError("%s: plan must be a contiguous uint8 tensor on %s" % (who, device))
    return _vp(plan.data_ptr())


def _ivf_lists(who, members, offsets, m, device):
    """The lists of a scan, checked: ``members`` int64 ``[m]`` (``m=None``: as many as there are) and ``offsets`` int64 ``[K + 1]``,
    contiguous on ``device``; ``(members pointer, offsets pointer, m, K)``."""
    _kmeans_tensor(members, torch.int64, who, "members", 1)
    _kmeans_tensor(offsets, torch.int64, who, "offsets", 1)
    m, k = members.shape[0] if m is None else m, offsets.shape[0] - 1
    return (_ivf_vector(members, torch.int64, who, "members", (m,), device),
            _ivf_vector(offsets, torch.int64, who, "offsets", (k + 1,), device), m, k)


def _ivf_candidates(nq, cap, device):
    """The outputs of a scan, uninitialised: ``(cand_scores fp32 [nq, cap], cand_ids int64 [nq, cap])``."""
    return torch.empty((nq, cap), dtype=torch.float32, device=device), torch.empty((nq, cap), dtype=torch.int64, device=device)


def ivf_plan_views(plan, nq, nprobe, k):
    """The sections of a plan (include/mdx_ivf.h) as int64 views of it: ``{"base": [nq, nprobe], "count": [nq], "first": [k + 1],
    "item": [k + 1], "entry": [nq * nprobe]}``.  Of ``entry`` only the first ``first[k]`` are defined, and inside a list in no
    particular order."""
    up = lambda b: (b + 255) // 256 * 256
    words = plan[:plan.numel() // 8 * 8].view(torch.int64)
    views, at = {}, 0
    for name, shape in (("base", (nq, nprobe)), ("count", (nq,)), ("first", (k + 1,)), ("item", (k + 1,)), ("entry", (nq * nprobe,))):
        count = int(np.prod(shape))
        views[name] = words[at // 8:at // 8 + count].view(shape)
        at += up(8 * count)
    return views


def ivf_plan(probes, offsets, m, cap):
    """The plan (a uint8 device tensor of ``mdx_ivf_plan_workspace`` bytes; :func:`ivf_plan_views` names its sections) of a batch
    of probes (``mdx_ivf_plan``).  ``probes`` int64 ``[nq, nprobe]``: the lists every query probes, best first (a probe outside
    ``[0, K)`` is skipped); ``offsets`` int64 ``[K + 1]``: list l owns ``members[offsets[l]:offsets[l + 1]]`` of ``m`` members;
    ``cap``: the columns of a query's candidate row."""
    who = "ivf_plan"
    _kmeans_tensor(probes, torch.int64, who, "probes", 2)
    _kmeans_tensor(offsets, torch.int64, who, "offsets", 1)
    nq, nprobe = probes.shape
    k = offsets.shape[0] - 1
    _ivf_vector(probes, torch.int64, who, "probes", (nq, nprobe), probes.device)
    _ivf_vector(offsets, torch.int64, who, "offsets", (k + 1,), probes.device)
    _ivf_count(m, who, "m")
    _ivf_count(cap, who, "cap")
    if k < 1 or nprobe > k:
        raise ValueError("%s: nprobe = %d probes of K = %d lists: nprobe must be in [1, K]" % (who, nprobe, k))
    h = _lib.lib()
    plan = _workspace(h.mdx_ivf_plan_workspace(nq, nprobe, k), probes.device)
    with _on(probes):
        check(h.mdx_ivf_plan(_vp(probes.data_ptr()), nq, nprobe, _vp(offsets.data_ptr()), k, m, cap, _vp(plan.data_ptr()), plan.numel(),
                             _stream()), "mdx_ivf_plan")
    return plan


def ivf_scan(rows, members, offsets, queries, plan, nprobe, cap, items, qlayout="ND", center=None):
    """``(cand_scores fp32 [nq, cap], cand_ids int64 [nq, cap])``: the exact fp32 chain scores of every query against the members of
    the lists it probes (``mdx_ivf_scan``), list-major: a tile of a list is read once for up to ``IVF_QUERY_GROUP`` queries that probe
    it.  ``rows`` fp32 ``[n, d]`` on the device (rows contiguous at any stride); ``members`` int64 ``[m]`` and ``offsets`` int64
    ``[K + 1]``: the lists; ``plan``: :func:`ivf_plan` of the probes with the same ``offsets``, ``m = members.numel()`` and ``cap``;
    ``items``: the workgroups to launch, at least the plan's number of work items (``ivf.item_bound``).  A candidate's column is the
    base of its probe plus its index in the list; columns at or beyond a query's count hold NaN / -1; a member id outside ``[0, n)``
    scores NaN.  Every score is bit-identical to ``DescriptorIndex(rows, "ND").scores(queries, qlayout, center)`` at the same id."""
    who = "ivf_scan"
    rp, ld = _kmeans_matrix(rows, who, "rows")
    n, d = rows.shape
    _kmeans_tensor(queries, torch.float32, who, "queries", 2)
    nq, dq, lay = _layout(queries, qlayout, "queries")
    if dq != d:
        raise ValueError("%s: query dimension %d != rows dimension %d" % (who, dq, d))
    if not queries.is_contiguous() or queries.device != rows.device:
        raise ValueError("%s: queries must be contiguous on %s" % (who, rows.device))
    mp, op, m, k = _ivf_lists(who, members, offsets, None, rows.device)
    for x, what in ((nprobe, "nprobe"), (cap, "cap"), (items, "items")):
        _ivf_count(x, who, what)
    cp = None
    if center is not None:
        cp = _ivf_vector(center, torch.float32, who, "center", (d,), rows.device)
    pp = _ivf_plan_arg(plan, who, nq, nprobe, k, rows.device)
    cand_scores, cand_ids = _ivf_candidates(nq, cap, rows.device)
    with _on(rows):
        check(_lib.lib().mdx_ivf_scan(rp, n, d, ld, mp, m, op, k, _vp(queries.data_ptr()), nq, lay,
                                      cp, nprobe, pp, plan.numel(), cap, items, _vp(cand_scores.data_ptr()), _vp(cand_ids.data_ptr()),
                                      _stream()), "mdx_ivf_scan")
    return cand_scores, cand_ids


def ivf_select(cand_scores, cand_ids, plan, nprobe, lists, k):
    """``(ids int64 [nq, k], scores fp32 [nq, k])``: per query the first ``k`` of its candidates (the plan's count of them, the
    leading columns of ``cand_scores`` / ``cand_ids``, both ``[nq, cap]``) in :func:`rank_full`'s order -- larger score first,
    ``-0 == +0``, NaN last, equal keys by ascending id -- sorted (``mdx_ivf_select``); positions beyond the count hold -1 / NaN.
    ``lists``: the K of the plan."""
    who = "ivf_select"
    _kmeans_tensor(cand_scores, torch.float32, who, "cand_scores", 2)
    nq, cap = cand_scores.shape
    _ivf_vector(cand_scores, torch.float32, who, "cand_scores", (nq, cap), cand_scores.device)
    _kmeans_tensor(cand_ids, torch.int64, who, "cand_ids", 2)
    _ivf_vector(cand_ids, torch.int64, who, "cand_ids", (nq, cap), cand_scores.device)
    for x, what in ((nprobe, "nprobe"), (lists, "lists")):
        _ivf_count(x, who, what)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= RESCORE_MAX_K:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (who, RESCORE_MAX_K, k))
    pp = _ivf_plan_arg(plan, who, nq, nprobe, lists, cand_scores.device)
    out_ids = torch.empty((nq, k), dtype=torch.int64, device=cand_scores.device)
    out_scores = torch.empty((nq, k), dtype=torch.float32, device=cand_scores.device)
    with _on(cand_scores):
        check(_lib.lib().mdx_ivf_select(_vp(cand_scores.data_ptr()), _vp(cand_ids.data_ptr()), nq, cap, nprobe, lists, pp, plan.numel(), k,
                                        _vp(out_ids.data_ptr()), _vp(out_scores.data_ptr()), _stream()), "mdx_ivf_select")
    return out_ids, out_scores


# ------------------------------------------------------------------ inverted file, int8 lists (include/mdx_lists_i8.h)

LISTS_I8_MAX_D = 133120           # include/mdx.h MDX_I8: 127^2 * round_up(d, 64) stays below 2^31


def _lists_i8_storage(codes, scales, d, who):
    """``codes`` int8 ``[m, round_up(d, 64)]`` and ``scales`` fp32 ``[m]`` of :func:`lists_i8_encode`, checked; ``(pointers, m)``."""
    _kmeans_tensor(codes, torch.int8, who, "codes", 2)
    _ivf_count(d, who, "d")
    if d > LISTS_I8_MAX_D:
        raise ValueError("%s: d = %d > %d" % (who, d, LISTS_I8_MAX_D))
    m, d_pad = codes.shape[0], (d + 63) // 64 * 64
    _ivf_vector(codes, torch.int8, who, "codes", (m, d_pad), codes.device)
    _kmeans_tensor(scales, torch.float32, who, "scales", 1)
    _ivf_vector(scales, torch.float32, who, "scales", (m,), codes.device)
    return _vp(codes.data_ptr()), _vp(scales.data_ptr()), m


def lists_i8_encode(rows, members):
    """``(codes int8 [m, round_up(d, 64)], scales fp32 [m])``: the ``MDX_I8`` quantisation of the rows of the lists, in list order
    (``mdx_lists_i8_encode``).  Position ``p`` holds the bits ``quantize_i8`` gives for row ``members[p]`` and zeros in the padding
    columns; a member id outside ``[0, n)`` is never dereferenced and gets zero codes and a NaN scale.  ``rows`` fp32 ``[n, d]`` on the
    device (rows contiguous at any stride, read in place); ``members`` int64 ``[m]``."""
    who = "lists_i8_encode"
    rp, ld = _kmeans_matrix(rows, who, "rows")
    n, d = rows.shape
    if d > LISTS_I8_MAX_D:
        raise ValueError("%s: d = %d > %d" % (who, d, LISTS_I8_MAX_D))
    _kmeans_tensor(members, torch.int64, who, "members", 1)
    m = members.shape[0]
    _ivf_vector(members, torch.int64, who, "members", (m,), rows.device)
    codes = torch.empty((m, (d + 63) // 64 * 64), dtype=torch.int8, device=rows.device)
    scales = torch.empty((m,), dtype=torch.float32, device=rows.device)
    with _on(rows):
        check(_lib.lib().mdx_lists_i8_encode(rp, n, d, ld, _vp(members.data_ptr()), m, _vp(codes.data_ptr()), _vp(scales.data_ptr()),
                                             _stream()), "mdx_lists_i8_encode")
    return codes, scales


def lists_i8_bounds(codes, scales, d):
    """Device tensor (float64 ``[4]``, the bytes of ``mdx_i8_bounds``, as :meth:`DescriptorIndex.i8_bounds` returns) of the storage of
    :func:`lists_i8_encode` (``mdx_lists_i8_bounds``): for valid members the values of an int8 ``DescriptorIndex`` of the same rows,
    to the bit; a non-finite scale sets the flag.  ``d``: the dimension of the rows.  What :func:`rescore_certify` needs."""
    who = "lists_i8_bounds"
    cp, sp, m = _lists_i8_storage(codes, scales, d, who)
    b = torch.empty(4, dtype=torch.float64, device=codes.device)
    with _on(codes):
        check(_lib.lib().mdx_lists_i8_bounds(cp, sp, m, d, _vp(b.data_ptr()), _stream()), "mdx_lists_i8_bounds")
    return b


def lists_i8_scan(codes, scales, d, members, offsets, qcodes, qscales, plan, nprobe, cap, items):
    """``(cand_scores fp32 [nq, cap], cand_ids int64 [nq, cap])``: the ``MDX_I8`` scores of every query against the members of the
    lists it probes (``mdx_lists_i8_scan``), on the int8 MFMA over the contiguous codes of :func:`lists_i8_encode`.  ``members``,
    ``offsets``, ``plan``, ``nprobe``, ``cap``, ``items`` and the outputs are those of :func:`ivf_scan`; ``qcodes`` int8 ``[nq, d]`` and
    ``qscales`` fp32 ``[nq]`` are ``quantize_i8(center_rows(queries, qlayout, center))``.  Every score is bit-identical to
    ``DescriptorIndex(rows, "ND", storage="i8").scores(queries, qlayout, center)`` at the same id; a member whose scale is NaN (an id
    outside the rows) scores NaN."""
    who = "lists_i8_scan"
    cp, sp, m = _lists_i8_storage(codes, scales, d, who)
    _kmeans_tensor(qcodes, torch.int8, who, "qcodes", 2)
    nq, dq = qcodes.shape
    if dq != d:
        raise ValueError("%s: query dimension %d != rows dimension %d" % (who, dq, d))
    _ivf_vector(qcodes, torch.int8, who, "qcodes", (nq, d), codes.device)
    _kmeans_tensor(qscales, torch.float32, who, "qscales", 1)
    _ivf_vector(qscales, torch.float32, who, "qscales", (nq,), codes.device)
    mp, op, m, k = _ivf_lists(who, members, offsets, m, codes.device)
    for x, what in ((nprobe, "nprobe"), (cap, "cap"), (items, "items")):
        _ivf_count(x, who, what)
    pp = _ivf_plan_arg(plan, who, nq, nprobe, k, codes.device)
    cand_scores, cand_ids = _ivf_candidates(nq, cap, codes.device)
    with _on(codes):
        check(_lib.lib().mdx_lists_i8_scan(cp, sp, m, d, mp, op, k, _vp(qcodes.data_ptr()),
                                           _vp(qscales.data_ptr()), nq, nprobe, pp, plan.numel(), cap, items,
                                           _vp(cand_scores.data_ptr()), _vp(cand_ids.data_ptr()), _stream()), "mdx_lists_i8_scan")
    return cand_scores, cand_ids


# ------------------------------------------------------------------ inverted file, product-quantised lists (include/mdx_lists_pq.h)

PQ_MAX_M = 128                    # include/mdx_lists_pq.h MDX_PQ_MAX_M: sub-quantisers of a code; a query's table is M KiB of LDS
PQ_CODEWORDS = 256                # include/mdx_lists_pq.h MDX_PQ_CODEWORDS: a code is one byte


def _pq_codewords(codewords, who):
    """``codewords`` fp32 ``[M, 256, dsub]`` on the device, contiguous, checked; ``(M, dsub)``."""
    _kmeans_tensor(codewords, torch.float32, who, "codewords", 3)
    m, cw, dsub = codewords.shape
    if cw != PQ_CODEWORDS or not 1 <= m <= PQ_MAX_M or not codewords.is_contiguous():
        raise ValueError("%s: codewords must be a contiguous [M, %d, dsub] tensor with M in [1, %d], got %s"
                         % (who, PQ_CODEWORDS, PQ_MAX_M, tuple(codewords.shape)))
    return m, dsub


def pq_lut(codewords, queries, qlayout="ND", center=None):
    """fp32 ``[nq, M, 256]``: the look-up table of every query (``mdx_pq_lut``).  ``codewords`` fp32 ``[M, 256, dsub]`` on the device,
    contiguous; ``queries`` fp32 ``[nq, M * dsub]`` (``"ND"``) or ``[M * dsub, nq]`` (``"DN"``), contiguous; ``center`` fp32
    ``[M * dsub]`` or None (``x_q = q - center`` in one fp32 subtraction).  ``lut[q, m, j]`` is bit-identical to
    ``DescriptorIndex(codewords[m], "ND").scores`` of sub-vector ``m`` of ``x_q`` at codeword ``j``."""
    who = "pq_lut"
    m, dsub = _pq_codewords(codewords, who)
    _kmeans_tensor(queries, torch.float32, who, "queries", 2)
    nq, dq, lay = _layout(queries, qlayout, "queries")
    if dq != m * dsub:
        raise ValueError("%s: query dimension %d != M * dsub = %d" % (who, dq, m * dsub))
    if not queries.is_contiguous() or queries.device != codewords.device:
        raise ValueError("%s: queries must be contiguous on %s" % (who, codewords.device))
    cp = None
    if center is not None:
        cp = _ivf_vector(center, torch.float32, who, "center", (m * dsub,), codewords.device)
    lut = torch.empty((nq, m, PQ_CODEWORDS), dtype=torch.float32, device=codewords.device)
    with _on(codewords):
        check(_lib.lib().mdx_pq_lut(_vp(codewords.data_ptr()), m, dsub, _vp(queries.data_ptr()), nq, lay, cp, _vp(lut.data_ptr()), _stream()),
              "mdx_pq_lut")
    return lut


def lists_pq_scan(codes, members, n, offsets, lut, coarse, probes, plan, cap):
    """``(cand_scores fp32 [nq, cap], cand_ids int64 [nq, cap])``: the ADC scores of every query against the members of the lists it
    probes (``mdx_lists_pq_scan``), query-major, by look-ups in the query's table.  ``codes`` uint8 ``[m, M]`` on the device (rows
    contiguous at any row stride): row ``p`` holds the code of row ``members[p]``; ``members`` int64 ``[m]``, ``n``: the rows the ids
    refer to; ``offsets`` int64 ``[K + 1]``; ``lut`` fp32 ``[nq, M, 256]`` of :func:`pq_lut`; ``coarse`` fp32 and ``probes`` int64
    ``[nq, nprobe]``: the values and ids of :func:`topk` over the centroid scores; ``plan``: :func:`ivf_plan` of the probes with the same
    ``offsets``, ``m`` and ``cap``.  A candidate's column is the base of its probe plus its index in the list; its score is ``coarse``
    plus the ``M`` table entries of its code, added in subspace order in fp32; columns at or beyond a query's count hold NaN / -1; a
    member id outside ``[0, n)`` scores NaN."""
    who = "lists_pq_scan"
    _kmeans_tensor(codes, torch.uint8, who, "codes", 2)
    m, sub = codes.shape
    if not 1 <= sub <= PQ_MAX_M:
        raise ValueError("%s: codes are [m, %d]: M must be in [1, %d]" % (who, sub, PQ_MAX_M))
    if (sub > 1 and codes.stride(1) != 1) or (m > 1 and codes.stride(0) < sub):
        raise ValueError("%s: codes must be a matrix with contiguous rows" % who)
    ldc = codes.stride(0) if m > 1 else sub
    _kmeans_tensor(lut, torch.float32, who, "lut", 3)
    nq = lut.shape[0]
    _ivf_vector(lut, torch.float32, who, "lut", (nq, sub, PQ_CODEWORDS), codes.device)
    _kmeans_tensor(probes, torch.int64, who, "probes", 2)
    nprobe = probes.shape[1]
    _ivf_vector(probes, torch.int64, who, "probes", (nq, nprobe), codes.device)
    _kmeans_tensor(coarse, torch.float32, who, "coarse", 2)
    _ivf_vector(coarse, torch.float32, who, "coarse", (nq, nprobe), codes.device)
    mp, op, m, k = _ivf_lists(who, members, offsets, m, codes.device)
    for x, what in ((n, "n"), (cap, "cap")):
        _ivf_count(x, who, what)
    pp = _ivf_plan_arg(plan, who, nq, nprobe, k, codes.device)
    cand_scores, cand_ids = _ivf_candidates(nq, cap, codes.device)
    with _on(codes):
        check(_lib.lib().mdx_lists_pq_scan(_vp(codes.data_ptr()), m, sub, ldc, mp, n, op, k,
                                           _vp(lut.data_ptr()), _vp(coarse.data_ptr()), _vp(probes.data_ptr()), nq, nprobe, pp, plan.numel(),
                                           cap, _vp(cand_scores.data_ptr()), _vp(cand_ids.data_ptr()), _stream()), "mdx_lists_pq_scan")
    return cand_scores, cand_ids


# ------------------------------------------------------------------ inverted file, editing the lists (include/mdx_lists_edit.h)

def _lists_structure(rows, members, offsets, who, which, device=None, may_be_empty=False):
    """``(m, width, ld)`` of one list-ordered structure -- ``rows`` uint8 ``[m, width]`` with contiguous rows at any row stride,
    ``members`` int64 ``[m]``, ``offsets`` int64 ``[K + 1]``, all on one device --, checked; a ValueError names what is wrong."""
    for t, dtype, dims, what in ((rows, torch.uint8, 2, "rows"), (members, torch.int64, 1, "members"), (offsets, torch.int64, 1, "offsets")):
        what = which + what
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("%s: %s must be a CUDA/ROCm tensor: the MI355X path has no CPU fallback" % (who, what))
        if t.dtype != dtype or t.dim() != dims:
            raise ValueError("%s: %s must be a %d-d %s tensor, got %s %s" % (who, what, dims, dtype, t.dtype, tuple(t.shape)))
        if t.device != (device or rows.device):
            raise ValueError("%s: %s is on %s, not on %s as the rows before it" % (who, what, t.device, device or rows.device))
    m, width = rows.shape
    if width < 1 or (m < 1 and not may_be_empty):
        raise ValueError("%s: %srows must be a non-empty [m, width] tensor, got %s" % (who, which, tuple(rows.shape)))
    if m and ((width > 1 and rows.stride(1) != 1) or (m > 1 and rows.stride(0) < width)):
        raise ValueError("%s: %srows must be a matrix with contiguous rows" % (who, which))
    if tuple(members.shape) != (m,) or not members.is_contiguous():
        raise ValueError("%s: %smembers must be a contiguous [%d] tensor, got %s" % (who, which, m, tuple(members.shape)))
    if offsets.shape[0] < 2 or not offsets.is_contiguous():
        raise ValueError("%s: %soffsets must be a contiguous [K + 1] tensor with K >= 1, got %s" % (who, which, tuple(offsets.shape)))
    return m, width, rows.stride(0) if m > 1 else width


def _lists_outputs(who, out_rows, m, width, k, device):
    """``(rows, ld, members, offsets)`` a call writes: ``out_rows`` as given (uint8 ``[m, width]``, contiguous rows at any row stride)
    or a new contiguous block."""
    if out_rows is None:
        out_rows = torch.empty((m, width), dtype=torch.uint8, device=device)
    else:
        if not isinstance(out_rows, torch.Tensor) or not out_rows.is_cuda or out_rows.dtype != torch.uint8 or out_rows.device != device \
                or tuple(out_rows.shape) != (m, width):
            raise ValueError("%s: out_rows must be a uint8 [%d, %d] tensor on %s" % (who, m, width, device))
        if (width > 1 and out_rows.stride(1) != 1) or (m > 1 and out_rows.stride(0) < width):
            raise ValueError("%s: out_rows must be a matrix with contiguous rows" % who)
    members = torch.empty((m,), dtype=torch.int64, device=device)
    offsets = torch.empty((k + 1,), dtype=torch.int64, device=device)
    return out_rows, (out_rows.stride(0) if m > 1 else width), members, offsets


def lists_merge(a_rows, a_members, a_offsets, b_rows, b_members, b_offsets, out_rows=None):
    """``(rows, members, offsets)``: per list the rows of structure ``a`` followed by those of structure ``b`` (``mdx_lists_merge``).  A
    structure is ``rows`` uint8 ``[m, width]`` on the device (opaque payload; rows contiguous at any row stride), ``members`` int64
    ``[m]`` and ``offsets`` int64 ``[K + 1]``; ``a`` and ``b`` share ``K`` and ``width``, and one of them may have no rows.  The result
    has ``ma + mb`` rows, ``offsets = a_offsets + b_offsets`` (each clamped to its ``[0, m]``), rows and members moved together.
    ``out_rows``: a uint8 ``[ma + mb, width]`` tensor to write the rows to (any row stride; the bytes between its rows stay as they
    are) instead of a new one.  One pass, no temporary; nothing is read back."""
    who = "lists_merge"
    ma, width, a_ld = _lists_structure(a_rows, a_members, a_offsets, who, "a_", may_be_empty=True)
    mb, width_b, b_ld = _lists_structure(b_rows, b_members, b_offsets, who, "b_", a_rows.device, may_be_empty=True)
    if width_b != width or b_offsets.shape != a_offsets.shape:
        raise ValueError("%s: a is [%d, %d] over %d lists and b [%d, %d] over %d: width and K must agree"
                         % (who, ma, width, a_offsets.shape[0] - 1, mb, width_b, b_offsets.shape[0] - 1))
    if ma + mb < 1:
        raise ValueError("%s: neither structure has a row" % who)
    k = a_offsets.shape[0] - 1
    rows, out_ld, members, offsets = _lists_outputs(who, out_rows, ma + mb, width, k, a_rows.device)
    # a structure of no rows has no storage: the other one's pointers stand in, and are never dereferenced
    ar, am = (a_rows, a_members) if ma else (b_rows, b_members)
    br, bm = (b_rows, b_members) if mb else (a_rows, a_members)
    with _on(a_rows):
        check(_lib.lib().mdx_lists_merge(_vp(ar.data_ptr()), a_ld, _vp(am.data_ptr()), _vp(a_offsets.data_ptr()), ma, _vp(br.data_ptr()), b_ld,
                                         _vp(bm.data_ptr()), _vp(b_offsets.data_ptr()), mb, k, width, _vp(rows.data_ptr()), out_ld,
                                         _vp(members.data_ptr()), _vp(offsets.data_ptr()), _stream()), "mdx_lists_merge")
    return rows, members, offsets


def lists_compact(rows, members, offsets, kept, total=None, out_rows=None):
    """``(rows, members, offsets)``: the structure without the positions that are not kept (``mdx_lists_compact``).  ``rows``,
    ``members``, ``offsets`` as in :func:`lists_merge`; ``kept`` int64 ``[m + 1]`` is the exclusive prefix sum of the keep flags:
    position ``p`` is kept exactly when ``kept[p + 1] > kept[p]`` and goes to position ``kept[p]``; ``offsets`` becomes
    ``kept[offsets]``.  The order inside a list is unchanged.  ``total``: the rows of the result, ``kept[m]`` -- ``None`` reads it
    back (the one synchronisation; a caller that knows it passes it); it must be at least 1.  ``out_rows`` as in :func:`lists_merge`."""
    who = "lists_compact"
    m, width, ld = _lists_structure(rows, members, offsets, who, "")
    if not isinstance(kept, torch.Tensor) or not kept.is_cuda or kept.dtype != torch.int64 or tuple(kept.shape) != (m + 1,) \
            or not kept.is_contiguous() or kept.device != rows.device:
        raise ValueError("%s: kept must be a contiguous int64 [%d] tensor on %s" % (who, m + 1, rows.device))
    if total is None:
        total = int(kept[m])
    _ivf_count(total, who, "total")
    if total > m:
        raise ValueError("%s: total = %d > m = %d" % (who, total, m))
    k = offsets.shape[0] - 1
    out, out_ld, out_members, out_offsets = _lists_outputs(who, out_rows, total, width, k, rows.device)
    with _on(rows):
        check(_lib.lib().mdx_lists_compact(_vp(rows.data_ptr()), ld, _vp(members.data_ptr()), _vp(offsets.data_ptr()), m, k, width,
                                           _vp(kept.data_ptr()), total, _vp(out.data_ptr()), out_ld, _vp(out_members.data_ptr()),
                                           _vp(out_offsets.data_ptr()), _stream()), "mdx_lists_compact")
    return out, out_members, out_offsets


# ------------------------------------------------------------------ inverted file, int8 refinement of shortlists (include/mdx_refine.h)

def refine_i8(codes, scales, d, where, qcodes, qscales, ids):
    """``(ids int64 [nq, S], scores fp32 [nq, S])``: the ``MDX_I8`` scores of each query's shortlist ``ids`` (int64 ``[nq, S]``,
    ``S <= RESCORE_MAX_K``) against the storage of :func:`lists_i8_encode`, sorted as :func:`rescore` sorts (``mdx_refine_i8``).
    ``codes`` int8 ``[m, round_up(d, 64)]`` and ``scales`` fp32 ``[m]``; ``d``: the dimension of the rows; ``where`` int64 ``[n]``: the
    position in ``[0, m)`` that holds id ``i`` (any other value: the id is not stored); ``qcodes`` int8 ``[nq, d]`` and ``qscales`` fp32
    ``[nq]`` are ``quantize_i8(center_rows(queries, qlayout, center))``.  Every score is bit-identical to
    ``DescriptorIndex(rows, "ND", storage="i8").scores(queries, qlayout, center)`` at the same id; an id outside ``[0, n)`` or one that
    is not stored is never dereferenced, scores NaN and sorts last."""
    who = "refine_i8"
    cp, sp, m = _lists_i8_storage(codes, scales, d, who)
    _kmeans_tensor(where, torch.int64, who, "where", 1)
    n = where.shape[0]
    _ivf_vector(where, torch.int64, who, "where", (n,), codes.device)
    _kmeans_tensor(qcodes, torch.int8, who, "qcodes", 2)
    nq, dq = qcodes.shape
    if dq != d:
        raise ValueError("%s: query dimension %d != rows dimension %d" % (who, dq, d))
    _ivf_vector(qcodes, torch.int8, who, "qcodes", (nq, d), codes.device)
    _kmeans_tensor(qscales, torch.float32, who, "qscales", 1)
    _ivf_vector(qscales, torch.float32, who, "qscales", (nq,), codes.device)
    _kmeans_tensor(ids, torch.int64, who, "ids", 2)
    if ids.shape[0] != nq or not 1 <= ids.shape[1] <= RESCORE_MAX_K:
        raise ValueError("%s: ids must be [%d, S] with S in [1, %d], got %s" % (who, nq, RESCORE_MAX_K, tuple(ids.shape)))
    s = ids.shape[1]
    _ivf_vector(ids, torch.int64, who, "ids", (nq, s), codes.device)
    out_ids = torch.empty((nq, s), dtype=torch.int64, device=codes.device)
    out_scores = torch.empty((nq, s), dtype=torch.float32, device=codes.device)
    h = _lib.lib()
    ws = _workspace(h.mdx_refine_i8_workspace(nq, s), codes.device)
    with _on(codes):
        check(h.mdx_refine_i8(cp, sp, m, d, _vp(where.data_ptr()), n, _vp(qcodes.data_ptr()), _vp(qscales.data_ptr()), nq,
                              _vp(ids.data_ptr()), s, _vp(out_ids.data_ptr()), _vp(out_scores.data_ptr()), _vp(ws.data_ptr()), ws.numel(),
                              _stream()), "mdx_refine_i8")
    return out_ids, out_scores


# ------------------------------------------------------------------ kNN lists, reverse-edge merge (include/mdx_knn_reverse.h)

KNN_REVERSE_MAX_K = 128           # include/mdx_knn_reverse.h MDX_KNN_REVERSE_MAX_K: two list entries per lane


def _knn_reverse_lists(ids, scores, who):
    """(n, k) of the neighbour lists ``ids`` int64 / ``scores`` fp32 ``[n, k]``, contiguous, on one device."""
    _kmeans_tensor(ids, torch.int64, who, "ids", 2)
    n, k = ids.shape
    _ivf_vector(ids, torch.int64, who, "ids", (n, k), ids.device)
    _kmeans_tensor(scores, torch.float32, who, "scores", 2)
    _ivf_vector(scores, torch.float32, who, "scores", (n, k), ids.device)
    if k > KNN_REVERSE_MAX_K:
        raise ValueError("%s: k = %d > KNN_REVERSE_MAX_K = %d" % (who, k, KNN_REVERSE_MAX_K))
    if n * k >= 1 << 31:
        raise ValueError("%s: n * k = %d must be below 2^31" % (who, n * k))
    return n, k


def knn_reverse_count(ids, scores):
    """``counts`` int32 ``[n]``: per row the reverse-edge offers that can enter it (``mdx_knn_reverse_count``; the definition is in
    ``include/mdx_knn_reverse.h``)."""
    n, k = _knn_reverse_lists(ids, scores, "knn_reverse_count")
    counts = torch.empty((n,), dtype=torch.int32, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_knn_reverse_count(_vp(ids.data_ptr()), _vp(scores.data_ptr()), n, k, _vp(counts.data_ptr()), _stream()),
              "mdx_knn_reverse_count")
    return counts


def knn_reverse_offsets(counts):
    """``offsets`` int64 ``[n + 1]`` of the offer segments: 0, then the running sum of ``counts`` (one ``torch.cumsum`` on the
    device; nothing is read back)."""
    _kmeans_tensor(counts, torch.int32, "knn_reverse_offsets", "counts", 1)
    offsets = torch.zeros((counts.shape[0] + 1,), dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    return offsets


def knn_reverse_fill(ids, scores, offsets, capacity=None):
    """The offer buffer, int64 ``[capacity]`` (an offer is 8 bytes: the score's bits, then the source id as int32), filled along ``offsets`` of :func:`knn_reverse_offsets`
    (``mdx_knn_reverse_fill``).  ``capacity`` defaults to the bound ``n * k``, which no set of lists exceeds; the order of the offers
    inside a segment is that of their atomic tickets, and the merge does not depend on it."""
    who = "knn_reverse_fill"
    n, k = _knn_reverse_lists(ids, scores, who)
    capacity = n * k if capacity is None else capacity
    _ivf_count(capacity, who, "capacity")
    _kmeans_tensor(offsets, torch.int64, who, "offsets", 1)
    _ivf_vector(offsets, torch.int64, who, "offsets", (n + 1,), ids.device)
    cursor = torch.empty((n,), dtype=torch.int32, device=ids.device)
    offers = torch.empty((capacity,), dtype=torch.int64, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_knn_reverse_fill(_vp(ids.data_ptr()), _vp(scores.data_ptr()), n, k, _vp(offsets.data_ptr()),
                                              _vp(cursor.data_ptr()), _vp(offers.data_ptr()), capacity, _stream()), "mdx_knn_reverse_fill")
    return offers


def knn_reverse_apply(ids, scores, offsets, offers):
    """``(ids int64 [n, k], scores fp32 [n, k], gained int32 [n])``: every row's first ``k`` of its own valid entries and the offers
    of its segment (``mdx_knn_reverse_merge``)."""
    who = "knn_reverse_apply"
    n, k = _knn_reverse_lists(ids, scores, who)
    _kmeans_tensor(offsets, torch.int64, who, "offsets", 1)
    _ivf_vector(offsets, torch.int64, who, "offsets", (n + 1,), ids.device)
    _kmeans_tensor(offers, torch.int64, who, "offers", 1)
    capacity = offers.shape[0]
    _ivf_vector(offers, torch.int64, who, "offers", (capacity,), ids.device)
    out_ids = torch.empty((n, k), dtype=torch.int64, device=ids.device)
    out_scores = torch.empty((n, k), dtype=torch.float32, device=ids.device)
    gained = torch.empty((n,), dtype=torch.int32, device=ids.device)
    with _on(ids):
        check(_lib.lib().mdx_knn_reverse_merge(_vp(ids.data_ptr()), _vp(scores.data_ptr()), n, k, _vp(offsets.data_ptr()),
                                               _vp(offers.data_ptr()), capacity, _vp(out_ids.data_ptr()), _vp(out_scores.data_ptr()),
                                               _vp(gained.data_ptr()), _stream()), "mdx_knn_reverse_merge")
    return out_ids, out_scores, gained


def knn_reverse_merge(ids, scores):
    """The reverse-edge merge of the neighbour lists ``ids`` int64 / ``scores`` fp32 ``[n, k]`` (rows in ``rank_full``'s order, -1
    padding at the tail, ``k <= KNN_REVERSE_MAX_K``): ``(ids, scores, gained int32 [n])``.  Where row i lists j and j does not list
    i, ``(i, score)`` is offered to j; every row keeps the first ``k``, by (order key, id), of its own entries and its offers, and
    ``gained`` counts those that were offers.  The scores are taken to be symmetric (the exact chain is, to the bit); every output score
    is the bit pattern of an input entry.  :func:`knn_reverse_count`, :func:`knn_reverse_offsets`, :func:`knn_reverse_fill` with the
    offer buffer at its bound ``n * k``, :func:`knn_reverse_apply`: three launches and a prefix sum, nothing read back."""
    counts = knn_reverse_count(ids, scores)
    offsets = knn_reverse_offsets(counts)
    offers = knn_reverse_fill(ids, scores, offsets)
    return knn_reverse_apply(ids, scores, offsets, offers)


# ------------------------------------------------------------------ top-K lists, overlap (include/mdx_overlap.h)

OVERLAP_MAX_K = RESCORE_MAX_K     # include/mdx_overlap.h MDX_OVERLAP_MAX_K: the longest list of any search here
OVERLAP_MAX_DEPTHS = 8            # include/mdx_overlap.h MDX_OVERLAP_MAX_DEPTHS


def topk_overlap(a, b, depths):
    """``out`` int32 ``[nq, T]``: ``out[q, t]`` = the ids ``>= 0`` among the first ``min(depths[t], ka)`` entries of ``a[q]`` that also
    occur among the first ``min(depths[t], kb)`` entries of ``b[q]`` (``mdx_topk_overlap``; the definition is in
    ``include/mdx_overlap.h``).  ``a`` int64 ``[nq, ka]`` and ``b`` int64 ``[nq, kb]`` on one device, contiguous, ``1 <= ka, kb <=
    OVERLAP_MAX_K``; the ids ``>= 0`` of a row are distinct and negative ids are padding.  ``depths``: 1 to ``OVERLAP_MAX_DEPTHS``
    positive ascending integers.  An id at or above 2^31 is a ``ValueError`` -- the one read-back of this wrapper (the largest id of
    ``a`` and ``b``), left out while the current stream is capturing, where the kernel counts such an id as padding."""
    who = "topk_overlap"
    _kmeans_tensor(a, torch.int64, who, "a", 2)
    nq, ka = a.shape
    _ivf_vector(a, torch.int64, who, "a", (nq, ka), a.device)
    _kmeans_tensor(b, torch.int64, who, "b", 2)
    kb = b.shape[1]
    _ivf_vector(b, torch.int64, who, "b", (nq, kb), a.device)
    if max(ka, kb) > OVERLAP_MAX_K:
        raise ValueError("%s: ka = %d and kb = %d must be at most OVERLAP_MAX_K = %d" % (who, ka, kb, OVERLAP_MAX_K))
    depths = list(depths) if isinstance(depths, (list, tuple)) else [depths]
    if not 1 <= len(depths) <= OVERLAP_MAX_DEPTHS:
        raise ValueError("%s: between 1 and %d depths, got %d" % (who, OVERLAP_MAX_DEPTHS, len(depths)))
    for t, x in enumerate(depths):
        _ivf_count(x, who, "depths[%d]" % t)
        if x >= 1 << 31 or (t and x < depths[t - 1]):
            raise ValueError("%s: depths must be ascending and below 2^31, got %r" % (who, depths))
    if not torch.cuda.is_current_stream_capturing():
        top = max(int(a.max()), int(b.max()))
        if top >= 1 << 31:
            raise ValueError("%s: id %d is at or above 2^31" % (who, top))
    out = torch.empty((nq, len(depths)), dtype=torch.int32, device=a.device)
    with _on(a):
        check(_lib.lib().mdx_topk_overlap(_vp(a.data_ptr()), ka, _vp(b.data_ptr()), kb, nq, (ctypes.c_int32 * len(depths))(*depths),
                                          len(depths), _vp(out.data_ptr()), _stream()), "mdx_topk_overlap")
    return out


# ------------------------------------------------------------------ graph index (include/mdx_graph.h)

GRAPH_MAX_D = 8192                # include/mdx_graph.h MDX_GRAPH_MAX_D: the centred query stays in 32 KiB of LDS
GRAPH_MAX_DEGREE = 64             # MDX_GRAPH_MAX_DEGREE
GRAPH_MAX_SEEDS = 512             # MDX_GRAPH_MAX_SEEDS
GRAPH_MAX_BEAM = 512              # MDX_GRAPH_MAX_BEAM
GRAPH_MAX_WIDTH = 8               # MDX_GRAPH_MAX_WIDTH
GRAPH_MAX_CANDIDATES = 512        # MDX_GRAPH_MAX_CANDIDATES: width * degree of one step, = GRAPH_MAX_WIDTH * GRAPH_MAX_DEGREE
GRAPH_MAX_K0 = 128                # MDX_GRAPH_MAX_K0: the longest list of graph_detours


def graph_search(rows, graph, queries, seeds, k, beam, width=1, max_steps=None, qlayout="ND", center=None, table_bits=0):
    """``(ids int64 [nq, k], scores fp32 [nq, k], steps int32 [nq], scored int32 [nq])``: the beam search of every query over the
    neighbour graph ``graph`` (int32 ``[n, R]``, contiguous; entries outside ``[0, n)`` are padding) of ``rows`` (fp32 ``[n, d]`` on
    the device, rows contiguous at any stride), from ``seeds`` (int64 ``[nq, S]``) -- ``mdx_graph_search``; the sequential definition
    is in ``include/mdx_graph.h``.  ``beam`` is the beam length L (``k <= L <= GRAPH_MAX_BEAM``), ``width`` the parents per step,
    ``max_steps`` the step limit (default ``ceil(4 * beam / width)``).  Every score is bit-identical to
    ``DescriptorIndex(rows, "ND").scores(queries, qlayout, center)`` at the same id (a NaN score is the quiet NaN); the tail of a row
    is padded with -1 and NaN.  ``table_bits`` sizes the table of rows already scored and changes only ``scored``."""
    who = "graph_search"
    rp, ld = _kmeans_matrix(rows, who, "rows")
    n, d = rows.shape
    _kmeans_tensor(graph, torch.int32, who, "graph", 2)
    R = graph.shape[1]
    _ivf_vector(graph, torch.int32, who, "graph", (n, R), rows.device)
    _kmeans_tensor(queries, torch.float32, who, "queries", 2)
    nq, dq, lay = _layout(queries, qlayout, "queries")
    if dq != d or not queries.is_contiguous() or queries.device != rows.device:
        raise ValueError("%s: queries must be contiguous with dimension %d on %s, got %s (%s) on %s" % (
            who, d, rows.device, tuple(queries.shape), qlayout, queries.device))
    if center is not None:
        _ivf_vector(center, torch.float32, who, "center", (d,), rows.device)
    _kmeans_tensor(seeds, torch.int64, who, "seeds", 2)
    S = seeds.shape[1]
    _ivf_vector(seeds, torch.int64, who, "seeds", (nq, S), rows.device)
    for x, what in ((k, "k"), (beam, "beam"), (width, "width")):
        _ivf_count(x, who, what)
    if max_steps is None:
        max_steps = -(-4 * beam // width)
    _ivf_count(max_steps, who, "max_steps")
    _ivf_count(table_bits, who, "table_bits", 0)
    if d > GRAPH_MAX_D or R > GRAPH_MAX_DEGREE or S > GRAPH_MAX_SEEDS:
        raise ValueError("%s: d = %d, degree = %d and seeds = %d must be at most %d, %d and %d" % (
            who, d, R, S, GRAPH_MAX_D, GRAPH_MAX_DEGREE, GRAPH_MAX_SEEDS))
    if not k <= beam <= GRAPH_MAX_BEAM:
        raise ValueError("%s: beam = %d must be in [k = %d, GRAPH_MAX_BEAM = %d]" % (who, beam, k, GRAPH_MAX_BEAM))
    if width > GRAPH_MAX_WIDTH:                       # with it, width * degree <= GRAPH_MAX_CANDIDATES
        raise ValueError("%s: width = %d must be at most %d" % (who, width, GRAPH_MAX_WIDTH))
    if table_bits and not 8 <= table_bits <= 14:
        raise ValueError("%s: table_bits = %d must be 0 or in [8, 14]" % (who, table_bits))
    ids = torch.empty((nq, k), dtype=torch.int64, device=rows.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=rows.device)
    steps = torch.empty((nq,), dtype=torch.int32, device=rows.device)
    scored = torch.empty((nq,), dtype=torch.int32, device=rows.device)
    with _on(rows):
        check(_lib.lib().mdx_graph_search(rp, n, d, ld, _vp(graph.data_ptr()), R, _vp(queries.data_ptr()), nq, lay,
                                          None if center is None else _vp(center.data_ptr()), _vp(seeds.data_ptr()), S, k, beam, width,
                                          max_steps, table_bits, _vp(ids.data_ptr()), _vp(scores.data_ptr()), _vp(steps.data_ptr()),
                                          _vp(scored.data_ptr()), _stream()), "mdx_graph_search")
    return ids, scores, steps, scored


def graph_detours(lists):
    """``detours`` int32 ``[n, K0]`` of the neighbour lists ``lists`` (int64 ``[n, K0]`` on the device, contiguous, best first, own id
    removed, entries outside ``[0, n)`` padding, ``K0 <= GRAPH_MAX_K0``): for a valid ``b = lists[i, j]`` the ranks ``t < j`` whose
    ``a = lists[i, t]`` lists ``b`` before rank ``j``; ``K0`` for an invalid entry (``mdx_graph_detours``)."""
    who = "graph_detours"
    _kmeans_tensor(lists, torch.int64, who, "lists", 2)
    n, k0 = lists.shape
    _ivf_vector(lists, torch.int64, who, "lists", (n, k0), lists.device)
    if k0 > GRAPH_MAX_K0:
        raise ValueError("%s: K0 = %d > GRAPH_MAX_K0 = %d" % (who, k0, GRAPH_MAX_K0))
    out = torch.empty((n, k0), dtype=torch.int32, device=lists.device)
    with _on(lists):
        check(_lib.lib().mdx_graph_detours(_vp(lists.data_ptr()), n, k0, _vp(out.data_ptr()), _stream()), "mdx_graph_detours")
    return out


def _csr(id_lists, device):
    arrays =[np.asarray(ids, dtype=np.int64).reshape(-1) for ids in id_lists]
    offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
    if arrays:
        np.cumsum([len(a) for a in arrays], out=offsets[1:])
    flat = np.concatenate(arrays) if arrays else np.empty(0, dtype=np.int64)
    both = torch.from_numpy(np.concatenate([flat, offsets])).to(device)      # one copy
    return both[:len(flat)], both[len(flat):], [int(o) for o in offsets]


def rank_of(scores, id_lists):
    """Zero-based rank positions of the given ids, per query, without sorting.

    ``id_lists[q]`` = database ids of query q.  Returns (positions, id_scores) as
    flat device tensors plus the CSR offsets (python list)."""
    sp = _dev(scores, torch.float32, "scores")
    nq, n = scores.shape
    if len(id_lists) != nq:
        raise ValueError("need one id list per query")
    ids_t, off_t, offsets = _csr(id_lists, scores.device)
    total = ids_t.numel()
    pos = torch.zeros(total, dtype=torch.int64, device=scores.device)
    sc = torch.empty(total, dtype=torch.float32, device=scores.device)
    if total:
        flat = np.concatenate([np.asarray(ids, dtype=np.int64).reshape(-1) for ids in id_lists])
        if int(flat.min()) < 0 or int(flat.max()) >= n:
            raise IndexError("labelled id out of range [0,%d)" % n)
        with torch.cuda.device(scores.device):
            check(_lib.lib().mdx_rank_of(sp, n, nq, _vp(ids_t.data_ptr()), _vp(off_t.data_ptr()), total,
                                         _vp(sc.data_ptr()), _vp(pos.data_ptr()), _stream()), "mdx_rank_of")
    return pos, sc, offsets


def rank_positions(ranks, id_lists):
    """Positions of the given ids inside a ranking: ``ranks`` int64 ``[Q, N]`` on the device (rows contiguous; a row stride
    larger than N, e.g. the first columns of a wider matrix, is fine), ``id_lists[q]`` = non-negative ids, unique within a
    query.  Returns ``(pos, offsets)``: flat int64 device tensor aligned with the concatenated lists (-1 where the id does not
    occur in row q) and the CSR offsets.  ``np.arange(N)[np.in1d(ranks[:, q], ids)]`` of evaluate.py:80-81 in one pass."""
    if not (isinstance(ranks, torch.Tensor) and ranks.is_cuda and ranks.dtype == torch.int64 and ranks.dim() == 2):
        raise ValueError("ranks: a 2-d int64 CUDA tensor [Q, N]")
    if ranks.shape[1] != 1 and ranks.stride(1) != 1:        # (the stride of a one-element row means nothing)
        raise ValueError("ranks: every query's row must be contiguous (pass the [Q, N] matrix, not a copy of its transpose)")
    nq, n = ranks.shape
    if len(id_lists) != nq:
        raise ValueError("need one id list per query")
    ids_t, off_t, offsets = _csr(id_lists, ranks.device)
    total = ids_t.numel()
    pos = torch.empty(total, dtype=torch.int64, device=ranks.device)
    if total:
        with torch.cuda.device(ranks.device):
            check(_lib.lib().mdx_rank_positions(_vp(ranks.data_ptr()), n, nq, ranks.stride(0) if nq > 1 else n, _vp(ids_t.data_ptr()),
                                                _vp(off_t.data_ptr()), total, _vp(pos.data_ptr()), _stream()), "mdx_rank_positions")
    return pos, offsets


def gather_scores(scores, ids_t, off_t):
    sp = _dev(scores, torch.float32, "scores")
    nq, n = scores.shape
    out = torch.empty(ids_t.numel(), dtype=torch.float32, device=scores.device)
    if ids_t.numel():
        with torch.cuda.device(scores.device):
            check(_lib.lib().mdx_gather_scores(sp, n, nq, _dev(ids_t, torch.int64, "ids"),
                                               _dev(off_t, torch.int64, "offsets"), ids_t.numel(),
                                               _vp(out.data_ptr()), _stream()), "mdx_gather_scores")
    return out


def rank_count_(cnt, scores, id_offset, ref_scores, ref_ids, off_t):
    """cnt[t] += number of rows of this shard's ``scores`` that rank before
    (ref_scores[t], ref_ids[t]); the per-shard term of a global rank position."""
    sp = _dev(scores, torch.float32, "scores")
    nq, n = scores.shape
    if ref_ids.numel():
        with torch.cuda.device(scores.device):
            check(_lib.lib().mdx_rank_count(sp, n, nq, int(id_offset), _dev(ref_scores, torch.float32, "ref_scores"),
                                            _dev(ref_ids, torch.int64, "ref_ids"), _dev(off_t, torch.int64, "offsets"),
                                            ref_ids.numel(), _dev(cnt, torch.int64, "cnt"), _stream()),
                  "mdx_rank_count")
    return cnt


# ---------------------------------------------------------- whitening learning

def gram_f64(a, center=None):
    """``(a - center) @ (a - center).T`` for a float64 ``[d, n]`` device matrix -> ``[d, d]`` (exactly symmetric):
    the ``np.dot(df, df.T)`` / ``np.dot(Xc, Xc.T)`` of cirtorch/utils/whiten.py:22,42,46 on the f64 matrix cores."""
    ap = _dev(a, torch.float64, "a")
    if a.dim() != 2:
        raise ValueError("a must be [d, n]")
    d, n = a.shape
    cp = _center(center, d, torch.float64)
    out = torch.empty((d, d), dtype=torch.float64, device=a.device)
    need = _lib.lib().mdx_gram_f64_workspace(d, n)
    ws = _workspace(need, a.device)
    with _on(a):
        check(_lib.lib().mdx_gram_f64(ap, d, n, cp, _vp(out.data_ptr()), _vp(ws.data_ptr()), need, _stream()), "mdx_gram_f64")
    return out


def l2n_cols_f64_(x, eps=1e-6):
    """In place: every column of a float64 ``[d, n]`` matrix divided by (its L2 norm + eps) (``mdx_l2n_cols_f64``)."""
    xp = _dev(x, torch.float64, "x")
    if x.dim() != 2:
        raise ValueError("x must be [d, n]")
    with _on(x):
        check(_lib.lib().mdx_l2n_cols_f64(xp, x.shape[0], x.shape[1], float(eps), _stream()), "mdx_l2n_cols_f64")
    return x


def project_f64(p, x, center=None):
    """``p @ (x - center)`` for float64 ``p [dout, d]``, ``x [d, n]``, ``center [d]`` -> ``[dout, n]``
    (``np.dot(P, X-m)``, whiten.py:45)."""
    pp = _dev(p, torch.float64, "p")
    xp = _dev(x, torch.float64, "x")
    if p.dim() != 2 or x.dim() != 2 or p.shape[1] != x.shape[0]:
        raise ValueError("p [dout, d] and x [d, n] expected, got %s and %s" % (tuple(p.shape), tuple(x.shape)))
    cp = _center(center, x.shape[0], torch.float64)
    out = torch.empty((p.shape[0], x.shape[1]), dtype=torch.float64, device=x.device)
    need = _lib.lib().mdx_project_f64_workspace(p.shape[0], p.shape[1])
    ws = _workspace(need, x.device)
    with _on(x):
        check(_lib.lib().mdx_project_f64(pp, p.shape[0], p.shape[1], xp, x.shape[1], cp, _vp(out.data_ptr()), _vp(ws.data_ptr()), need,
                                         _stream()), "mdx_project_f64")
    return out


# ------------------------------------------------------------ multi-GPU exchange

def query_bounds(nq, nranks, rank):
    """Queries ``[lo, hi)`` of ``rank`` under the query split (``mdx_query_bounds``)."""
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    check(_lib.lib().mdx_query_bounds(int(nq), int(nranks), int(rank), ctypes.byref(lo), ctypes.byref(hi)), "mdx_query_bounds")
    return lo.value, hi.value


class Comm:
    """RCCL communicator of libmdx.so (``mdx_comm``): the exchange of per-shard partial scores through the C ABI.

    ``Comm.from_process_group(device)`` builds one over an initialised ``torch.distributed`` group (rank 0's unique id is
    broadcast through that group -- the only use made of it); ``Comm(id_bytes, nranks, rank)`` takes an id that
    travelled by other means (``Comm.unique_id()`` on one rank)."""

    def __init__(self, id_bytes, nranks, rank, device=None):
        self._h = None
        self.nranks, self.rank = int(nranks), int(rank)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if len(id_bytes) != 128:
            raise ValueError("a communicator id is 128 bytes")
        buf = (ctypes.c_char * 128).from_buffer_copy(bytes(id_bytes))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_comm_init(ctypes.byref(h), buf, self.nranks, self.rank), "mdx_comm_init")
        self._h = h

    @staticmethod
    def unique_id():
        buf = (ctypes.c_char * 128)()
        check(_lib.lib().mdx_comm_unique_id(buf), "mdx_comm_unique_id")
        return bytes(buf.raw)

    @classmethod
    def from_process_group(cls, device, group=None):
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        box = [cls.unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return cls(box[0], world, rank, device)

    def _widths(self, widths):
        if len(widths) != self.nranks:
            raise ValueError("need one width per rank")
        return (ctypes.c_int64 * self.nranks)(*[int(w) for w in widths])

    def allgather_scores(self, local, widths):
        """``local [nq, widths[rank]]`` -> list of the G blocks ``[nq, widths[g]]`` (views of one buffer, back to back)."""
        nq = local.shape[0]
        if local.shape[1] != widths[self.rank]:
            raise ValueError("local block is %s, widths[%d] = %d" % (tuple(local.shape), self.rank, widths[self.rank]))
        out = torch.empty(nq * int(sum(widths)), dtype=torch.float32, device=local.device)
        with torch.cuda.device(local.device):
            check(_lib.lib().mdx_allgather_scores(self._h, _dev(local, torch.float32, "local scores"), nq, self._widths(widths),
                                                  _vp(out.data_ptr()), _stream()), "mdx_allgather_scores")
        return self._blocks(out, nq, widths)

    def exchange_scores(self, local, widths):
        """``local [nq, widths[rank]]`` -> ``(blocks [nq_mine, widths[g]] of MY queries, (qlo, qhi))``."""
        nq = local.shape[0]
        if local.shape[1] != widths[self.rank]:
            raise ValueError("local block is %s, widths[%d] = %d" % (tuple(local.shape), self.rank, widths[self.rank]))
        qlo, qhi = query_bounds(nq, self.nranks, self.rank)
        out = torch.empty(max(1, (qhi - qlo) * int(sum(widths))), dtype=torch.float32, device=local.device)
        with torch.cuda.device(local.device):
            check(_lib.lib().mdx_exchange_scores(self._h, _dev(local, torch.float32, "local scores"), nq, self._widths(widths),
                                                 _vp(out.data_ptr()), _stream()), "mdx_exchange_scores")
        return self._blocks(out, qhi - qlo, widths), (qlo, qhi)

    @staticmethod
    def _blocks(buf, rows, widths):
        blocks, o = [], 0
        for w in widths:
            blocks.append(buf[o:o + rows * int(w)].view(rows, int(w)))
            o += rows * int(w)
        return blocks

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, None
            check(_lib.lib().mdx_comm_destroy(h), "mdx_comm_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceMemory:
    """Library-owned device memory as something ``torch.as_tensor`` accepts (the CUDA array interface)."""

    def __init__(self, ptr, shape, owner):
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner             # keeps the exchange (and with it the allocation) alive as long as the view is


class P2P:
    """The direct-store exchange of per-shard partial scores (``mdx_p2p_*``, include/mdx.h; round 6): every rank's
    similarity kernel writes its scores straight into the receive buffers of the ranks that own the queries, over xGMI
    (buffers shared with hipIpc); a step is closed by one flag per peer; the owner ranks a DENSE ``[nq_mine, n_total]`` matrix.

    ``P2P.from_process_group(nq, n_total, device)`` builds and connects one over an initialised ``torch.distributed`` group
    (the 64-byte handles are gathered through it -- the only use made of it); ``P2P(nranks, rank, nq, n_total)`` +
    ``connect(handles)`` / ``connect_local(peers)`` take handles that travelled by other means / ranks living in this
    process.  Every rank must run the same steps: ``index.scores_p2p(queries, p2p)`` for each of its shards or chunks, then
    ``close_step()``."""

    def __init__(self, nranks, rank, nq, n_total, device=None):
        self._h = None
        self.nranks, self.rank, self.nq, self.n_total = int(nranks), int(rank), int(nq), int(n_total)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.qlo, self.qhi = query_bounds(self.nq, self.nranks, self.rank)
        buf = (ctypes.c_char * 64)()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            status = _lib.lib().mdx_p2p_create(ctypes.byref(h), self.nranks, self.rank, self.nq, self.n_total, buf)
        self._h = h if h.value else None
        self.exportable = status == 0
        if status != 0 and self._h is None:
            check(status, "mdx_p2p_create")
        self.handle = bytes(buf.raw)
        self.connected = False

    @classmethod
    def from_process_group(cls, nq, n_total, device, group=None):
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        me = cls(world, rank, nq, n_total, device)
        handles = [None] * world
        if world > 1:
            dist.all_gather_object(handles, (me.handle, me.exportable), group=group)
            if not all(ok for _, ok in handles):
                me.close()
                raise _lib.MdxError("a rank could not export its receive buffer (hipIpcGetMemHandle): is HSA_ENABLE_IPC_MODE_LEGACY=0 set?")
            me.connect([h for h, _ in handles])
        else:
            me.connect([me.handle])
        return me

    def connect(self, handles):
        if len(handles) != self.nranks or any(len(h) != 64 for h in handles):
            raise ValueError("need one 64-byte handle per rank")
        blob = (ctypes.c_char * (64 * self.nranks)).from_buffer_copy(b"".join(bytes(h) for h in handles))
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_p2p_connect(self._h, blob), "mdx_p2p_connect")
        self.connected = True

    def connect_local(self, peers):
        """Ranks that live in ONE process: ``peers`` = the P2P objects of all ranks, in rank order."""
        bases = (ctypes.c_void_p * self.nranks)(*[_lib.lib().mdx_p2p_base(q._h) for q in peers])
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_p2p_connect_ptrs(self._h, bases), "mdx_p2p_connect_ptrs")
        self.connected = True

    def close_step(self):
        """Enqueue the end of a step (raise my flag at every peer, wait for theirs) on the current stream; returns the
        ``[nq_mine, n_total]`` similarities of MY queries against ALL rows -- a view of the receive buffer, valid until the
        step after next (clone it to keep it longer)."""
        mine = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_p2p_close_step(self._h, ctypes.byref(mine), _stream()), "mdx_p2p_close_step")
        rows = self.qhi - self.qlo
        if rows == 0:
            return torch.empty((0, self.n_total), dtype=torch.float32, device=self.device)
        return torch.as_tensor(_DeviceMemory(mine.value, (rows, self.n_total), self), device=self.device)

    def late_peers(self):
        """Synchronises the current stream; bit r set = a wait for peer r gave up (20 s): that step's result is undefined."""
        word = ctypes.c_uint32()
        with torch.cuda.device(self.device):
            check(_lib.lib().mdx_p2p_status(self._h, ctypes.byref(word), _stream()), "mdx_p2p_status")
        return int(word.value)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, None
            torch.cuda.synchronize(self.device)
            check(_lib.lib().mdx_p2p_destroy(h), "mdx_p2p_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

