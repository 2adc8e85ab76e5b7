"""Restatement of the datasets' image resizes (diner_amd/csrc/image_resize.hip, diner_amd/wire.py), in numpy: float64 for the float
resamplers, integers for PIL's.  Each resampler is defined by the library call it replaces:

  * :func:`nearest_index`     ``F.interpolate(mode="nearest")`` (torchvision's ``resize(.., InterpolationMode.NEAREST)`` on a tensor;
                              reference src/data/multiface.py:349-354): float32 scale and product, as ATen's
  * :func:`aa_table`          ``F.interpolate(mode="bilinear", align_corners=False, antialias=True)`` (current torchvision's ``resize`` on a
                              float tensor; multiface.py:347-348)
  * :func:`bilinear_table`    the same call with ``antialias=False`` (torchvision 0.12 on tensors)
  * :func:`pil_table`         PIL's ``Image.resize`` on 8-bit pixels, its default bicubic in fixed point (src/data/dtu.py:79-83)

A table is (xmin [out], n [out], weights [out, taps]); :func:`resize_float` and :func:`resize_pil_u8` apply one per axis.  The Multiface
composite (:func:`multiface_sample`) is the reference's order: decode, gamma and white fill at full size (tests/wire_images_ref.py, float32),
then the resize; its float64 filter runs on the float32 decoded image.

Bars of the float resamplers (:func:`float_bar`): twice the larger of ATen-fp32's own distance to ATen-float64 on the case (stored in the
fixture) and ``(n_w + n_h + 6) 2^-24 max|value|``, the rounding of two fp32 weighted sums with ``n`` the longest window per axis; the
factor 2 covers another summation order and nothing else.
"""
from __future__ import annotations

import numpy as np

from tests import wire_images_ref as W

F = np.float32
PRECISION_BITS = 22

# (in, out) pairs on which nearest_index was checked against ATen for every destination index
NEAREST_PAIRS = ((2048, 256), (1334, 160), (1334, 166), (667, 160), (1000, 333), (512, 160), (53, 17), (17, 53))
# resize cases (H, W) -> (h, w) of the fixture and of the GPU tests
SIZES = {"odd": ((37, 53), (18, 26)), "up": ((30, 40), (45, 60)), "mf": ((267, 167), (32, 20)), "one": ((5, 7), (1, 1)),
         "ident": ((33, 64), (33, 64))}
PIL_SIZES = {"odd": ((37, 53), (18, 26)), "up": ((30, 40), (45, 60)), "thirds": ((64, 48), (23, 17)), "rows": ((37, 53), (18, 53)),
             "cols": ((37, 53), (37, 26))}


def nearest_index(n_in, n_out):
    """source index of every destination index: min((int)floorf(dst * scale), in - 1), scale = float32(in) / float32(out)"""
    scale = F(n_in) / F(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F) * scale).astype(np.int64), n_in - 1)


def _windows(n_in, n_out, support):
    scale = n_in / n_out
    center = scale * (np.arange(n_out) + 0.5)
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)      # (int): truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    return scale, center, xmin, xmax - xmin


def aa_table(n_in, n_out):
    scale = n_in / n_out
    support, inv = (scale, 1.0 / scale) if scale >= 1 else (1.0, 1.0)
    _, center, xmin, n = _windows(n_in, n_out, support)
    j = np.arange(n.max())[None]
    w = np.maximum(0.0, 1.0 - np.abs((j + xmin[:, None] - center[:, None] + 0.5) * inv))
    w = np.where(j < n[:, None], w, 0.0)
    return xmin, n, w / w.sum(1, keepdims=True)


def bilinear_table(n_in, n_out):
    scale = n_in / n_out
    src = np.maximum(scale * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = src.astype(np.int64)
    two = i0 < n_in - 1
    lam = src - i0
    w = np.stack([np.where(two, 1.0 - lam, 1.0), np.where(two, lam, 0.0)], 1)
    return i0, 1 + two.astype(np.int64), w


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def pil_table(n_in, n_out):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc: int64 weights with 22 fractional bits"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    _, center, xmin, n = _windows(n_in, n_out, 2.0 * fs)
    j = np.arange(n.max())[None]
    k = _bicubic((j + xmin[:, None] - center[:, None] + 0.5) / fs)
    k = np.where(j < n[:, None], k, 0.0)
    k = k / k.sum(1, keepdims=True)
    return xmin, n, np.where(k < 0, (-0.5 + k * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + k * (1 << PRECISION_BITS)).astype(np.int64))


def _apply(x, table, axis):
    """x [..] -> the axis filtered by the table, in x's dtype family (float64 or int64); the sum runs over zero-padded windows"""
    xmin, n, w = table
    x = np.moveaxis(x, axis, -1)
    idx = np.minimum(xmin[:, None] + np.arange(w.shape[1])[None], x.shape[-1] - 1)       # padded taps carry weight 0
    out = (x[..., idx] * w).sum(-1)
    return np.moveaxis(out, -1, axis)


def resize_float(x, size, antialias=True):
    """x [..., H, W] (any float dtype; computed in float64) -> float64 [..., h, w]: horizontal pass, then vertical"""
    table = aa_table if antialias else bilinear_table
    x = np.asarray(x, np.float64)
    H, Wd = x.shape[-2:]
    return _apply(_apply(x, table(Wd, size[1]), -1), table(H, size[0]), -2)


def resize_pil_u8(px, size):
    """px uint8 [..., H, W, C] -> uint8 [..., h, w, C] as PIL's Image.resize((w, h)): horizontal pass into uint8, then vertical; a pass
    whose size does not change is skipped"""
    px = np.asarray(px)
    assert px.dtype == np.uint8
    H, Wd = px.shape[-3:-1]

    def one(x, table, axis):
        acc = _apply(x.astype(np.int64), table, axis) + (1 << (PRECISION_BITS - 1))
        return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)

    if size[1] != Wd:
        px = one(px, pil_table(Wd, size[1]), -2)
    if size[0] != H:
        px = one(px, pil_table(H, size[0]), -3)
    return px


def resize_nearest(x, size):
    """x [..., H, W] -> [..., h, w], the texels F.interpolate(mode="nearest") selects"""
    H, Wd = x.shape[-2:]
    return x[..., nearest_index(H, size[0])[:, None], nearest_index(Wd, size[1])[None]]


def decode_resized(pixels, alpha, fmt, symmetric_range, size, antialias=True):
    """the bytes decoded at full size (wire_images_ref.decode_image, float32), then resized -> rgb float64 [N,3,h,w], alpha float32
    [N,1,h,w] (None without any alpha)"""
    rule, bg, gamma = W.FORMATS[fmt]
    rgb, a = W.decode_image(pixels, alpha, rule, bg, gamma, symmetric_range)
    return resize_float(rgb, size, antialias), None if a is None else resize_nearest(a, size)


def multiface_size(H, Wd, downsample=8):
    return int((H / downsample) // 32 * 32), int((Wd / downsample) // 32 * 32)


def scale_intrinsics(K, full, size):
    """float32 [..., 3, 3]: rows 0 and 1 times float32(w / W) and float32(h / H)"""
    K = np.array(K, F)
    K[..., 0, :] *= F(size[1] / full[1])
    K[..., 1, :] *= F(size[0] / full[0])
    return K


def longest_windows(full, size, antialias=True):
    table = aa_table if antialias else bilinear_table
    return int(table(full[1], size[1])[1].max()), int(table(full[0], size[0])[1].max())


def float_bar(aten_distance, full, size, max_abs, antialias=True):
    n_w, n_h = longest_windows(full, size, antialias)
    return 2.0 * max(float(aten_distance), (n_w + n_h + 6) * 2.0 ** -24 * float(max_abs))
