"""Restatement of the datasets' image readers and of Multiface's depth planes (diner_amd/csrc/image_wire.hip, diner_amd/wire.py), in
numpy, float32, one rounding per reference operation.

What it restates (reference src/data/):
  * ``FacescapeDataSet.read_rgba``        facescape.py:59-66      bytes / 255, symmetric range, ``rgb[a < .5] = bg``
  * ``DTUDataSet.read_rgb``               dtu.py:83-88            bytes / 255, symmetric range (after its PIL resize)
  * ``MultiFaceDataset.read_img``         multiface.py:65-73      bytes / 255, ``gammaCorrect(..).clip(0, 1)``, symmetric range
  * ``MultiFaceDataset.read_alpha``       multiface.py:76-78      bytes / 255
  * ``MultiFaceDataset.gammaCorrect``     multiface.py:81-95      the torch branch
  * the white fill                        multiface.py:322-323    ``rgb[alpha < 1] = 1``
  * ``MultiFaceDataset.read_depth``       multiface.py:103-109    u16 * 1e-4
  * the depth std                         multiface.py:305-311    constant 1e-3 or ``clip(a conf + b, min=0)``, 0 where depth == 0

Every step is reproduced bit for bit by float32 numpy except the square root of ``gammaCorrect``: ``np.sqrt`` on float32 is the correctly
rounded root (and so is the kernel's), while a torch build's ``x ** 0.5`` may be one ulp below it for a few inputs; the fixture
(tests/golden/wire_images.npz, tools/gen_wire_images_golden.py) stores the mask of those entries, and :func:`compare` admits one ulp of
the root (2^-23 absolute, the root is below 2) inside the mask only.

``wrong``: the name of one deliberately wrong implementation (:data:`WRONG_IMAGE`, :data:`WRONG_DEPTH`) that the comparison has to
reject on the fixture's inputs (tests/test_wire_images_host.py); ``None`` is the restatement.
"""
from __future__ import annotations

import numpy as np

F = np.float32

BG_RULES = ("none", "below_half", "below_one")
GAMMA_SCALE = (1.4, 1.1, 1.6)                       # multiface.py:86 color_scale, as torch.tensor(..) float32
GAMMA_BLACK = 3.0 / 255.0                           # :86
GAMMA_GAIN = (1.0 / (1 - GAMMA_BLACK)) * 0.95       # :95, formed in double, rounded once when it meets the float32 tensor
GAMMA_OFFSET = 15.0 / 255.0                         # :95
MULTIFACE_CONF2STD = (-1.582e-2, 1.649e-2)          # multiface.py:310
MULTIFACE_CONST_STD = 1e-3                          # :307
SCALE_FACTOR = 1e-4                                 # :105
ROOT_ULP = 2.0 ** -23                               # one ulp of a root in [1, 2); the roots here stay below 1.18

# "alpha_le": `a <= threshold` in place of `a < threshold`.  For the threshold 0.5 this is the SAME function of a byte (no byte / 255 is
# 0.5: 127 / 255 < 0.5 < 128 / 255), so no input can tell `a <= 0.5` from `a < 0.5`; the variant is told apart at the threshold 1
# (byte 255), and the threshold 0.5 is pinned from both sides by its two one-byte neighbours instead.
WRONG_IMAGE = ("mul_recip_255", "alpha_le", "alpha_128_is_hole", "alpha_127_is_kept", "fill_before_symmetric", "bg_mapped_to_symmetric",
               "gamma_no_final_clip", "scale_after_division")
WRONG_DEPTH = ("std_not_zeroed", "no_clip")

# the formats of diner_amd.wire (bg_rule, bg, gamma), by the name the fixture's keys carry
FORMATS = {"facescape": ("below_half", 1.0, False), "dtu": ("none", 1.0, False), "multiface": ("below_one", 1.0, True)}


def gamma_pre_root(v):
    """v [N,3,H,W] float32 in [0, 1] -> the operand of gammaCorrect's root (steps 2.1 - 2.3)"""
    s = np.array(GAMMA_SCALE, F).reshape(1, 3, 1, 1)
    t = (v * s) / F(1.1)
    t = np.clip(t - F(GAMMA_BLACK), F(0), F(2))
    return F(GAMMA_GAIN) * t


def gamma_post_root(r, final_clip=True):
    t = np.clip(r - F(GAMMA_OFFSET), F(0), F(2))
    return np.clip(t, F(0), F(1)) if final_clip else t


def _four(pixels):
    px = np.asarray(pixels)
    assert px.dtype == np.uint8 and px.ndim in (3, 4) and px.shape[-1] in (3, 4)
    return px[None] if px.ndim == 3 else px


def decode_image(pixels, alpha=None, bg_rule="none", bg=1.0, gamma=False, symmetric_range=False, wrong=None):
    """pixels uint8 [N,H,W,C] or [H,W,C], C in {3, 4}; alpha uint8 [N,H,W] or [H,W] (optional; it wins over a fourth channel) ->
    rgb [N,3,H,W] float32, alpha [N,1,H,W] float32 (None without any alpha)"""
    assert bg_rule in BG_RULES and wrong in (None,) + WRONG_IMAGE
    px = _four(pixels)
    N, H, W, C = px.shape
    a8 = None
    if alpha is not None:
        a8 = np.asarray(alpha).reshape(N, H, W)
        assert a8.dtype == np.uint8
    elif C == 4:
        a8 = px[..., 3]
    if bg_rule != "none":
        assert a8 is not None, "a fill rule needs an alpha"

    def unit(b):
        return b.astype(F) * (F(1) / F(255)) if wrong == "mul_recip_255" else b.astype(F) / F(255)

    v = unit(np.ascontiguousarray(px[..., :3].transpose(0, 3, 1, 2)))
    a = None if a8 is None else unit(a8)[:, None]
    if gamma:
        if wrong == "scale_after_division":
            s = np.array(GAMMA_SCALE, F).reshape(1, 3, 1, 1)
            t = F(GAMMA_GAIN) * np.clip((v / F(1.1)) * s - F(GAMMA_BLACK), F(0), F(2))
        else:
            t = gamma_pre_root(v)
        v = gamma_post_root(np.sqrt(t), final_clip=wrong != "gamma_no_final_clip")
    fill = F(bg)
    if bg_rule != "none":
        thr = F(0.5 if bg_rule == "below_half" else 1.0)
        hole = (a <= thr) if wrong == "alpha_le" else (a < thr)
        if bg_rule == "below_half" and wrong == "alpha_128_is_hole":
            hole = a8[:, None] <= 128
        if bg_rule == "below_half" and wrong == "alpha_127_is_kept":
            hole = a8[:, None] < 127
        hole = np.broadcast_to(hole, v.shape)
    if bg_rule != "none" and wrong == "fill_before_symmetric":
        v = np.where(hole, fill, v)
    if symmetric_range:
        v = v * F(2) - F(1)
        if wrong == "bg_mapped_to_symmetric":
            fill = fill * F(2) - F(1)
    if bg_rule != "none" and wrong != "fill_before_symmetric":
        v = np.where(hole, fill, v)
    return v.astype(F), a


def decode_multiface_depth(depth, conf=None, const_std=MULTIFACE_CONST_STD, conf2std=MULTIFACE_CONF2STD, stride=1, wrong=None):
    """depth (, conf) uint16 [N,H,W] -> depth, std, mask [N,1,H/stride,W/stride] float32 (mask = depth > 0)"""
    assert wrong in (None,) + WRONG_DEPTH
    d16 = np.asarray(depth)
    assert d16.dtype == np.uint16 and d16.ndim == 3 and d16.shape[1] % stride == 0 and d16.shape[2] % stride == 0
    d = d16[:, ::stride, ::stride].astype(F) * F(SCALE_FACTOR)
    if conf is None:
        std = np.full_like(d, F(const_std))
    else:
        c = np.asarray(conf)[:, ::stride, ::stride].astype(F) * F(SCALE_FACTOR)
        std = F(conf2std[0]) * c + F(conf2std[1])
        if wrong != "no_clip":
            std = np.where(std < F(0), F(0), std)
    if wrong != "std_not_zeroed":
        std = np.where(d == F(0), F(0), std)
    return d[:, None], std.astype(F)[:, None], (d > F(0)).astype(F)[:, None]


def compare(got, want, mask=None):
    """'' when ``got`` meets the bars against ``want``: the same bits outside ``mask``, within one ulp of the root (2^-23 absolute)
    inside it, and a mask that holds at most 2 % of the entries; otherwise what is wrong."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return f"shape / dtype {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    same = got.view(np.uint32) == want.view(np.uint32)
    if mask is None:
        mask = np.zeros(got.shape, bool)
    mask = np.broadcast_to(mask, got.shape)
    if mask.mean() > 0.02:
        return f"the mask holds {mask.mean():.2%} of the entries (at most 2 %)"
    out = ~same & ~mask
    if out.any():
        i = np.argwhere(out)[0]
        return f"{int(out.sum())} of {out.size} entries differ outside the mask, first at {tuple(i)}: {got[tuple(i)]!r} against {want[tuple(i)]!r}"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))[mask]
    if err.size and not (err.max() <= ROOT_ULP):
        return f"inside the mask: max |difference| {err.max():.3e} above one ulp of the root ({ROOT_ULP:.3e})"
    return ""
