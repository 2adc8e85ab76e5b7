"""Numpy restatement, on the CPU, of the four functions of diner_amd/csrc/frame_out.hip, written from the stated arithmetic (DESIGN.md §7
"Frame output and scores") and not from the kernels: the depth range, the colour map of ``torch_cmap`` (reference
src/util/torch_helpers.py:43-76: numpy in float64 and matplotlib's ``Colormap._get_rgba_and_mask``), the two byte quantisations
(torchvision ``save_image``; ``save_torch_video``, torch_helpers.py:91) and the scores of ``evaluate_folder``
(src/evaluation/eval_suite.py:63-68) from exact integer sums.  ``variant`` selects a deliberately wrong form, which
tests/test_frame_out_host.py shows the comparisons to reject."""
import numpy as np

ROUNDINGS = ("save_image", "video")


def depth_range_ref(depth):
    """depth [N,1,H,W] -> [N,2] float64 (min, max); a NaN anywhere in an image makes both NaN (np.min / np.max)"""
    d = np.asarray(depth).reshape(len(depth), -1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([d.min(axis=1), d.max(axis=1)], axis=1)


def cmap_index_ref(depth, nc, vmin=None, vmax=None, variant=None):
    """depth [N,1,H,W] -> the table row per pixel [N,H,W] (int64).  vmin / vmax: a scalar, or None / 0 for the image's own range
    (the reference's ``vmin if vmin else ...``)."""
    x = np.asarray(depth).astype(np.float64)
    rng = depth_range_ref(x)
    lo = np.float64(vmin) if vmin else rng[:, 0].reshape(-1, 1, 1, 1)
    hi = np.float64(vmax) if vmax else rng[:, 1].reshape(-1, 1, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        xa = ((x - lo) / (hi - lo))[:, 0] * nc
        if variant != "no_eq_rule":
            xa[xa == nc] = nc - 1
        under, over, bad = xa < 0, xa >= nc, np.isnan(xa)
        safe = np.where(under | over | bad, 0.0, xa)
        idx = (np.rint(safe) if variant == "round_index" else np.trunc(safe)).astype(np.int64)
    if variant == "round_index":
        idx = np.minimum(idx, nc - 1)
    i_under, i_over = (nc + 1, nc) if variant == "swap_under_over" else (nc, nc + 1)
    idx[under], idx[over], idx[bad] = i_under, i_over, nc + 2
    return idx


def torch_cmap_ref(depth, table, vmin=None, vmax=None, variant=None):
    """depth [N,1,H,W], table [nc + 3, 3] float64 -> [N,3,H,W] float64"""
    table = np.asarray(table, dtype=np.float64)
    idx = cmap_index_ref(depth, len(table) - 3, vmin, vmax, variant)
    return np.ascontiguousarray(table[idx].transpose(0, 3, 1, 2))


def quantise_ref(x, rounding):
    """float32 (or float64: the colour table) -> uint8.  save_image: (uint8) clamp(x 255 + 0.5, 0, 255) in x's own precision, one rounding
    per operation; video: (uint8) ((double) x 255).  Saturating, NaN -> 0."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore", over="ignore"):
        if rounding == "save_image":
            assert x.dtype in (np.float32, np.float64)
            v = x * x.dtype.type(255)
            v = v + x.dtype.type(0.5)
        elif rounding == "video":
            v = x.astype(np.float64) * 255.0
        else:
            raise ValueError(rounding)
        v = np.where(v > 0, np.minimum(v, 255), 0)        # NaN and everything <= 0 -> 0
        return np.trunc(v).astype(np.uint8)


def frames_u8_ref(rgb, depth=None, rounding="save_image", stacked=False, table=None, vmin=None, vmax=None, variant=None):
    """rgb [N,3,H,W] fp32, depth [N,1,H,W] fp32 -> rgb bytes [N,H,W,3] (and depth bytes, or the stacked frames [N,2H,W,3])"""
    rule = {"save_image": "video", "video": "save_image"}[rounding] if variant == "other_rounding" else rounding
    c = quantise_ref(np.asarray(rgb, dtype=np.float32), rule).transpose(0, 2, 3, 1)
    if depth is None:
        return np.ascontiguousarray(c)
    tab8 = quantise_ref(np.asarray(table, dtype=np.float64), rule)
    d = tab8[cmap_index_ref(depth, len(tab8) - 3, vmin, vmax, variant)]
    if stacked:
        return np.concatenate([c, d], axis=1)
    return np.ascontiguousarray(c), np.ascontiguousarray(d)


def _window_sums(a, win):
    """sums over every whole win x win window: a [H,W,...] int64 -> [H-win+1, W-win+1, ...], exact"""
    c = np.cumsum(np.cumsum(a, axis=0), axis=1)
    c = np.pad(c, [(1, 0), (1, 0)] + [(0, 0)] * (a.ndim - 2))
    return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]


def ssim_windows_ref(x, y, win=7, variant=None):
    """S of every whole window of one image pair, x, y [H,W,3] uint8 -> [H-win+1, W-win+1, 3] float64, from the exact integer sums:
    mx = Sx / (n 255), vx = (n Sxx - Sx^2) / (n (n-1) 255^2) with n = win^2 (the sample variance: cov_norm = n / (n-1)), vxy alike,
    S = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)), C1 = 0.01^2, C2 = 0.03^2"""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    n = win * win
    sx, sy, sxx, syy, sxy = (_window_sums(a, win) for a in (x, y, x * x, y * y, x * y))
    mu = float(n) * 255.0
    var = float(n) * float(n if variant == "no_cov_norm" else n - 1) * 255.0 * 255.0
    mx, my = sx.astype(np.float64) / mu, sy.astype(np.float64) / mu
    vx, vy = (n * sxx - sx * sx).astype(np.float64) / var, (n * syy - sy * sy).astype(np.float64) / var
    vxy = (n * sxy - sx * sy).astype(np.float64) / var
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    a1, a2 = 2.0 * mx * my + c1, 2.0 * vxy + c2
    b1, b2 = mx * mx + my * my + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2)


def image_scores_ref(pred, gt, variant=None):
    """pred, gt [N,H,W,3] uint8 -> dict of float64 [N]: ssim, psnr, l2, l1 (exact integer sums, each window's S in float64, the mean over
    the (H-6)(W-6) whole windows per channel, then the mean of the three channel means)"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.dtype == gt.dtype == np.uint8 and pred.shape == gt.shape and pred.ndim == 4 and pred.shape[-1] == 3
    N, H, W, _ = pred.shape
    win = 11 if variant == "window_11" else 7
    if H < win or W < win:
        raise ValueError("an image side below the window")
    out = {k: np.zeros(N) for k in ("ssim", "psnr", "l2", "l1")}
    for i in range(N):
        d = pred[i].astype(np.int64) - gt[i].astype(np.int64)
        out["l1"][i] = float(np.abs(d).sum()) / (255.0 * (3.0 * H * W))
        out["l2"][i] = float((d * d).sum()) / (65025.0 * (3.0 * H * W))
        with np.errstate(divide="ignore"):
            out["psnr"][i] = 10.0 * np.log10(np.float64(1.0) / out["l2"][i])
        if variant == "no_crop":
            # the mean over the same-size filtered image (reflected borders) instead of the whole windows only
            p = win // 2
            S = ssim_windows_ref(np.pad(pred[i], [(p, p), (p, p), (0, 0)], mode="symmetric"),
                                 np.pad(gt[i], [(p, p), (p, p), (0, 0)], mode="symmetric"), win, variant)
        else:
            S = ssim_windows_ref(pred[i], gt[i], win, variant)
        m = S.reshape(-1, 3).mean(axis=0)
        out["ssim"][i] = (m[0] + m[1] + m[2]) / 3.0
    return out
