"""Golden vectors of the frame output and the image scores (diner_amd/csrc/frame_out.hip; glue.torch_cmap, glue.frames_u8,
glue.image_scores), and the viridis table the package ships (diner_amd/viridis_lut.py: matplotlib's 259-row table, CC0 data, as a literal).

Two kinds of record, and they are not the same kind of evidence:

* FROM REFERENCE CODE: the UNMODIFIED reference ``torch_cmap`` (src/util/torch_helpers.py:43-76, imported through
  ``oracle.ref_harness.install_stubs``) runs on the CPU for every colour-map case; inputs, the table and its float64 outputs are recorded.
* FROM STATED ARITHMETIC: torchvision (``save_image``), imageio and skimage are not installed here and are not part of the reference
  tree, so the quantisations of ``save_image`` / ``save_torch_video`` and the scores of ``evaluate_folder``
  (src/evaluation/eval_suite.py:63-68) are written below from their definitions (DESIGN.md §7 "Frame output and scores").  The scores
  are written twice: in the reference's form (float32 images, ``scipy.ndimage.uniform_filter`` as skimage's ``structural_similarity``
  calls it) and in the exact integer form; both values and their difference (the float32 form's own deviation) are recorded per case.
  These two parts are pinned by stated arithmetic, not by running reference code.

Runs only where the reference source tree, matplotlib and scipy exist; the tests read the committed ``tests/golden/frame_out.npz`` only
(data, no program text).

    python tools/gen_golden_frame_out.py            # (re)writes tests/golden/frame_out.npz and diner_amd/viridis_lut.py
"""
from __future__ import annotations

import json
import sys
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"
LUT = ROOT / "diner_amd" / "viridis_lut.py"
ROUNDINGS = ("save_image", "video")


# ---- colour-map cases: name -> (depth [N,1,H,W] fp32, vmin, vmax) ---------------------------------------------------------------------
def cmap_cases():
    rs = np.random.RandomState(41)
    rnd = lambda *s: (0.5 + 2.0 * rs.random_sample(s)).astype(np.float32)
    cases = {}
    cases["flat_1x1"] = (np.full((1, 1, 1, 1), 1.5, np.float32), None, None)                   # flat: 0 / 0 -> the bad colour, black
    cases["one_7x7"] = (rnd(1, 1, 7, 7), None, None)
    d = rnd(3, 1, 9, 13)
    d[1] = 0.75                                                                                # image 1 flat
    cases["three_9x13_flat1"] = (d, None, None)
    cases["two_33x70"] = (rnd(2, 1, 33, 70), None, None)                                       # W % 4 != 0
    cases["one_64x64"] = (rnd(1, 1, 64, 64), None, None)
    # t * 256 on the integers and just beside them: vmin + k (vmax - vmin) / 256 (exact in fp32) and the fp32 neighbours either side
    k = np.arange(257, dtype=np.float64)
    v = (0.5 + k * (2.0 / 256.0)).astype(np.float32)
    ramp = np.stack([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])
    cases["ramp"] = (ramp.reshape(1, 1, 3, 257), 0.5, 2.5)
    cases["under_over"] = (rnd(2, 1, 9, 13), 1.0, 2.0)                                         # values below vmin and above vmax
    cases["vmin0"] = (rnd(1, 1, 9, 13), 0, 1.5)                                                # vmin = 0 counts as absent
    cases["given_vmin_only"] = (rnd(2, 1, 9, 12), 0.25, None)
    d = rnd(2, 1, 9, 13)
    d[0, 0, 4, 5] = np.nan                                                                     # both limits NaN: the whole image bad
    d[1, 0, 2, 7] = np.inf                                                                     # vmax = inf: 0 everywhere, that pixel bad
    cases["nan_inf"] = (d, None, None)
    # a table whose under / over / bad rows differ from every colour (viridis' over row equals its last colour, which hides the
    # xa == N rule): the same ramp and limits through with_extremes
    cases["extremes_ramp"] = (ramp.reshape(1, 1, 3, 257).copy(), 0.5, 2.5)
    cases["extremes_under_over"] = (cases["under_over"][0].copy(), 1.0, 2.0)
    return cases


# ---- the byte rules, from their definitions ----------------------------------------------------------------------------------------------
def quantise(x, rounding):
    """save_image: torchvision's ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` in x's own precision; video: save_torch_video's
    ``(x.numpy() * 255).astype(np.uint8)`` on float64 frames.  Where the cast is undefined: saturate, NaN -> 0."""
    import torch
    if rounding == "save_image":
        v = torch.from_numpy(np.ascontiguousarray(x)).clone().mul(255).add_(0.5).clamp_(0, 255)
        return torch.nan_to_num(v, nan=0.0).to(torch.uint8).numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x).astype(np.float64) * 255
        v = np.clip(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0), 0, 255)
    return v.astype(np.uint8)


def byte_ramp():
    """k / 255 and (k + 0.5) / 255 with their fp32 neighbours, and the values outside the byte range"""
    k = np.arange(256, dtype=np.float64)
    vals = []
    for v in ((k / 255.0).astype(np.float32), ((k + 0.5) / 255.0).astype(np.float32)):
        vals += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    extra = np.array([-0.5, -1e-3, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -23, 256.0 / 255.0, np.nextafter(np.float32(256.0 / 255.0), np.float32(2)),
                      1.5, 300.0, 3e38, -3e38, np.nan, np.inf, -np.inf], dtype=np.float32)
    return np.concatenate(vals + [extra]).astype(np.float32)


# ---- the scores, twice -------------------------------------------------------------------------------------------------------------------
def scores_reference_form(pred_u8, gt_u8):
    """one image pair as evaluate_folder scores it (eval_suite.py:63-68): float32 images; skimage.metrics.structural_similarity(pred, gt,
    channel_axis=-1, data_range=1) written out (uniform 7 x 7 filter in float32, sample covariance, crop by 3, float64 mean per channel,
    mean of the channels); peak_signal_noise_ratio and mean_squared_error on the float64 copies; the float32 mean of |pred - gt|"""
    from scipy.ndimage import uniform_filter
    gt = gt_u8.astype(np.float32) / 255.0
    pred = pred_u8.astype(np.float32) / 255.0
    win, R, K1, K2 = 7, 1, 0.01, 0.03
    NP = win ** 2
    cov_norm = NP / (NP - 1)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    per_channel = []
    for ch in range(3):
        im1, im2 = pred[..., ch], gt[..., ch]
        ux, uy = uniform_filter(im1, size=win), uniform_filter(im2, size=win)
        uxx, uyy, uxy = uniform_filter(im1 * im1, size=win), uniform_filter(im2 * im2, size=win), uniform_filter(im1 * im2, size=win)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
        S = (A1 * A2) / (B1 * B2)
        assert S.dtype == np.float32
        pad = (win - 1) // 2
        per_channel.append(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64))
    ssim = np.asarray(per_channel).mean()
    a, b = pred.astype(np.float64), gt.astype(np.float64)
    mse = np.mean((a - b) ** 2, dtype=np.float64)
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10((R ** 2) / mse)
    return dict(ssim=float(ssim), psnr=float(psnr), l2=float(mse), l1=float(np.mean(np.abs(pred - gt))))


def scores_exact_form(pred_u8, gt_u8):
    """the same four numbers from exact integer sums, each window's value in float64 (window by window: no running sums here)"""
    x, y = pred_u8.astype(np.int64), gt_u8.astype(np.int64)
    H, W, _ = x.shape
    d = x - y
    l1 = float(np.abs(d).sum()) / (255.0 * (3.0 * H * W))
    l2 = float((d * d).sum()) / (65025.0 * (3.0 * H * W))
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(np.float64(1.0) / np.float64(l2))
    view = lambda a: np.lib.stride_tricks.sliding_window_view(a, (7, 7), axis=(0, 1)).sum(axis=(-1, -2))
    sx, sy, sxx, syy, sxy = view(x), view(y), view(x * x), view(y * y), view(x * y)
    mx, my = sx / (49.0 * 255.0), sy / (49.0 * 255.0)
    den = 49.0 * 48.0 * 255.0 * 255.0
    vx, vy, vxy = (49 * sxx - sx * sx) / den, (49 * syy - sy * sy) / den, (49 * sxy - sx * sy) / den
    C1, C2 = 0.01 * 0.01, 0.03 * 0.03
    S = ((2.0 * mx * my + C1) * (2.0 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    m = S.reshape(-1, 3).mean(axis=0)
    return dict(ssim=float((m[0] + m[1] + m[2]) / 3.0), psnr=float(psnr), l2=l2, l1=l1)


def score_cases():
    rs = np.random.RandomState(43)

    def pair(N, H, W, noise=12):
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([127 + 100 * np.sin(xx / (3.0 + c) + n) * np.cos(yy / (4.0 + n)) for n in range(N) for c in range(3)])
        gt = np.clip(base.reshape(N, 3, H, W).transpose(0, 2, 3, 1) + rs.randint(-20, 21, (N, H, W, 3)), 0, 255).astype(np.uint8)
        pred = np.clip(gt.astype(np.int64) + rs.randint(-noise, noise + 1, (N, H, W, 3)), 0, 255).astype(np.uint8)
        return pred, gt

    cases = {}
    cases["one_window_7x7"] = pair(1, 7, 7, noise=60)                  # few windows: strong noise, so that a wrong form shows
    cases["small_8x9"] = pair(1, 8, 9, noise=60)
    cases["three_33x70"] = pair(3, 33, 70)
    cases["tiles_75x141"] = pair(1, 75, 141, noise=30)                 # more than one tile of windows in both axes, no multiple of it
    p, _ = pair(1, 20, 24)
    cases["identical_20x24"] = (p, p.copy())
    cases["constant_12x15"] = (np.full((1, 12, 15, 3), 100, np.uint8), np.full((1, 12, 15, 3), 140, np.uint8))   # zero variance
    cases["extremes_9x10"] = (np.zeros((1, 9, 10, 3), np.uint8), np.full((1, 9, 10, 3), 255, np.uint8))          # the largest sums
    return cases


def generate():
    import matplotlib
    matplotlib.use("Agg")
    import torch

    from oracle import ref_harness
    ref_harness.install_stubs()
    from src.util.torch_helpers import torch_cmap
    torch.set_num_threads(1)

    cm = matplotlib.colormaps["viridis"]
    cm._init()
    table = np.ascontiguousarray(cm._lut[:, :3], dtype=np.float64)
    assert table.shape == (259, 3) and (table[256] == table[0]).all() and (table[257] == table[255]).all() and (table[258] == 0).all()
    # repr() of a double reads back to the same double: the literal is the table bit for bit
    rows = "\n".join("    (%s)," % ", ".join(repr(float(v)) for v in row) for row in table)
    LUT.write_text('"""matplotlib\'s viridis lookup table without alpha (Colormap._lut[:, :3]; CC0 data): 256 colours, then the under, over and bad\n'
                   'rows.  Written by tools/gen_golden_frame_out.py -- do not edit."""\n'
                   f"VIRIDIS_LUT = (\n{rows}\n)\n")

    extremes = cm.with_extremes(under=(1.0, 0.0, 0.0), over=(0.0, 0.0, 1.0), bad=(0.0, 1.0, 0.0))
    extremes._init()
    table_x = np.ascontiguousarray(extremes._lut[:, :3], dtype=np.float64)
    assert (table_x[:256] == table[:256]).all() and not (table_x[257] == table_x[255]).all()
    store, index = {"table": table, "table_extremes": table_x}, {"cmap": {}, "frames": {}, "scores": {}}
    rs = np.random.RandomState(42)
    for name, (depth, vmin, vmax) in cmap_cases().items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                         # the reference divides 0 by 0 and casts NaN, with numpy's warnings
            which = dict(cmap=extremes) if name.startswith("extremes_") else {}       # plt.get_cmap hands a Colormap through
            out = torch_cmap(torch.from_numpy(depth), vmin=vmin, vmax=vmax, **which).numpy()
        N, _, H, W = depth.shape
        assert out.shape == (N, 3, H, W) and out.dtype == np.float64
        index["cmap"][name] = dict(N=N, H=H, W=W, vmin=vmin, vmax=vmax, table="table_extremes" if which else "table")
        store[f"cmap.{name}.depth"], store[f"cmap.{name}.out"] = depth, out
        # the frames of the same case: a colour image around [0, 1], and the bytes of both rules (the depth's from the reference's own
        # float64 colours)
        rgb = (-0.1 + 1.2 * rs.random_sample((N, 3, H, W))).astype(np.float32)
        index["frames"][name] = index["cmap"][name]
        store[f"frames.{name}.rgb"] = rgb
        for r in ROUNDINGS:
            store[f"frames.{name}.rgb_u8.{r}"] = np.ascontiguousarray(quantise(rgb, r).transpose(0, 2, 3, 1))
            store[f"frames.{name}.depth_u8.{r}"] = np.ascontiguousarray(quantise(out, r).transpose(0, 2, 3, 1))
        print("cmap", name, depth.shape, "black pixels", int((out.sum(axis=1) == 0).sum()))

    ramp = byte_ramp()
    store["bytes.values"] = ramp
    for r in ROUNDINGS:
        store[f"bytes.u8.{r}"] = quantise(ramp, r)
    print("byte ramp", ramp.shape, "values; rules differ on", int((store["bytes.u8.save_image"] != store["bytes.u8.video"]).sum()))

    for name, (pred, gt) in score_cases().items():
        N, H, W, _ = pred.shape
        index["scores"][name] = dict(N=N, H=H, W=W)
        store[f"scores.{name}.pred"], store[f"scores.{name}.gt"] = pred, gt
        ref = [scores_reference_form(pred[i], gt[i]) for i in range(N)]
        exact = [scores_exact_form(pred[i], gt[i]) for i in range(N)]
        for k in ("ssim", "psnr", "l2", "l1"):
            a, b = np.array([r[k] for r in ref]), np.array([e[k] for e in exact])
            with np.errstate(invalid="ignore"):
                dev = np.where(a == b, 0.0, np.abs(a - b))          # inf == inf: no deviation
            store[f"scores.{name}.{k}_ref"], store[f"scores.{name}.{k}_exact"], store[f"scores.{name}.{k}_dev"] = a, b, dev
        print("scores", name, {k: (float(store[f"scores.{name}.{k}_exact"][0]), float(store[f"scores.{name}.{k}_dev"].max()))
                               for k in ("ssim", "psnr", "l2", "l1")})
    out = GOLDEN / "frame_out.npz"
    np.savez_compressed(out, index=json.dumps(index), **store)
    print(f"{out}: {out.stat().st_size} bytes; {LUT}: {LUT.stat().st_size} bytes")


if __name__ == "__main__":
    generate()
