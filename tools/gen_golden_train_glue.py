"""Golden vectors of a training step's ray selection and photometric losses (diner_gen_rays_at, diner_photo_loss): the UNMODIFIED
reference on the CPU runs the lines of ``DINER.calc_losses`` around the renderer (reference src/models/diner.py:224-227, :257-258,
:265-267, :280-282) -- ``gen_rays`` (src/util/cam_geometry.py:36-79), the two advanced-index lines, ``torch.nn.MSELoss`` and
``AntibiasLoss`` (loaded from src/losses/antibiasloss.py by path: src/losses/__init__.py does not import as shipped) -- with autograd, in
fp32 and again in float64 on the same (widened) inputs.  Per case the fixture holds the inputs, the fp32 losses, ``gt_colors``, ``d_pred``
for the recorded loss weights, the camera gradients for a random ``d_rays``, the float64 evaluation of all of them and the fp32 run's own
deviation from it.  Runs only where the reference source tree exists; the tests read the committed ``tests/golden/train_glue.npz`` only
(data, no program text).

    python tools/gen_golden_train_glue.py            # (re)writes tests/golden/train_glue.npz

Every non-degenerate pooled difference must be at least MIN_DIFF in magnitude (a last-ulp difference then cannot flip a sign): a case
whose draw misses that is redrawn with the next seed, and the seed used is recorded."""
from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"
MIN_DIFF = 1e-4

# name -> sizes; patch cases: s, n (the patch sits at (x0, y0) of the image); random cases: B.  equal: the cell (scene 0, cell row 1,
# cell column 0) of pred equals the ground truth in all three channels
CASES = {
    "patch_s8_n3": dict(H=24, W=40, SB=1, s=8, n=3, x0=5, y0=3, seed=11),                  # one cell
    "patch_s10_n2": dict(H=24, W=40, SB=2, s=10, n=2, x0=30, y0=14, seed=12),              # 2 x 2 cells, 2 trailing rows / columns dropped
    "patch_s12_n2": dict(H=24, W=40, SB=1, s=12, n=2, x0=0, y0=12, seed=13),
    "patch_s64_n3": dict(H=64, W=64, SB=1, s=64, n=3, x0=0, y0=0, seed=14),                # the shipped setting
    "patch_s12_n2_equal_cell": dict(H=24, W=40, SB=2, s=12, n=2, x0=17, y0=7, seed=15, equal=True),
    "random_b1": dict(H=24, W=40, SB=1, B=1, seed=16),
    "random_b130": dict(H=24, W=40, SB=2, B=130, seed=17),                                  # not a multiple of 64
    "random_b128": dict(H=24, W=40, SB=1, B=128, seed=18),
}


def case_inputs(cfg, seed):
    rs = np.random.RandomState(seed)
    H, W, SB = cfg["H"], cfg["W"], cfg["SB"]
    E = np.zeros((SB, 4, 4), dtype=np.float32)
    for b in range(SB):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        E[b, :3, :3] = q
        E[b, :3, 3] = rs.standard_normal(3)
    E[:, 3, 3] = 1
    K = np.zeros((SB, 3, 3), dtype=np.float32)
    K[:, 0, 0], K[:, 1, 1] = W * (0.8 + 0.4 * rs.random_sample(SB)), H * (0.8 + 0.4 * rs.random_sample(SB))
    K[:, 0, 2], K[:, 1, 2] = W * (0.4 + 0.2 * rs.random_sample(SB)), H * (0.4 + 0.2 * rs.random_sample(SB))
    K[:, 2, 2] = 1
    zn = (0.5 + rs.random_sample(SB)).astype(np.float32)
    zf = (zn + 2).astype(np.float32)
    target = rs.random_sample((SB, 3, H, W)).astype(np.float32)
    if "s" in cfg:
        s = cfg["s"]
        ys, xs = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        idx = np.broadcast_to(((cfg["x0"] + xs) + (cfg["y0"] + ys) * W).reshape(1, -1), (SB, s * s)).astype(np.int64).copy()
    else:
        B = cfg["B"]
        idx = rs.randint(0, H * W, size=(SB, B)).astype(np.int64)
        idx[:, 0] = H * W - 1                         # the last and the first pixel, and deliberate duplicates
        if B > 1:
            idx[:, -1] = 0
            idx[:, B // 2] = idx[:, B // 3]
            idx[:, 1] = idx[:, 0]
    B = idx.shape[1]
    pred = rs.random_sample((SB, B, 3)).astype(np.float32)
    if cfg.get("equal"):
        s, p = cfg["s"], 2 ** cfg["n"]
        gt = np.stack([target[b].reshape(3, -1).T[idx[b]] for b in range(SB)])
        pv, gv = pred.reshape(SB, s, s, 3), gt.reshape(SB, s, s, 3)
        pv[0, p:2 * p, 0:p] = gv[0, p:2 * p, 0:p]
    d_rays = rs.standard_normal((SB, B, 8)).astype(np.float32)
    g = (0.5 + rs.random_sample(2)).astype(np.float32)          # the loss weights d_pred is recorded for: g_mse mse + g_ab antibias
    return dict(E=E, K=K, zn=zn, zf=zf, target=target, idx=idx, pred=pred, d_rays=d_rays, g=g)


def reference_lines(gen_rays, AntibiasLoss, inp, cfg, dtype):
    """the reference's own lines on tensors of ``dtype``; returns numpy arrays"""
    import torch
    H, W, SB = cfg["H"], cfg["W"], cfg["SB"]
    t = lambda a: torch.from_numpy(inp[a]).to(dtype)
    cams = [t(k).requires_grad_(True) for k in ("E", "K", "zn", "zf")]
    pix_idcs = torch.from_numpy(inp["idx"])
    B = pix_idcs.shape[1]
    rays = gen_rays(extrinsics=cams[0], intrinsics=cams[1], W=W, H=H, z_near=cams[2], z_far=cams[3])                 # diner.py:224-227
    batch_idx_helper = torch.arange(SB).unsqueeze(-1).expand(-1, B)                                                  # :257
    rays = rays.view(SB, H * W, -1)[batch_idx_helper, pix_idcs]                                                      # :258
    d_cams = torch.autograd.grad(rays, cams, t("d_rays"))
    pred = t("pred").requires_grad_(True)
    gt_colors = t("target").view(SB, 3, -1).permute(0, 2, 1)[batch_idx_helper, pix_idcs]                             # :265
    mse = torch.nn.MSELoss(reduction="mean")(pred, gt_colors)                                                        # :267
    g = inp["g"]
    loss = float(g[0]) * mse
    out = dict(mse=mse, gt=gt_colors, rays=rays)
    if "s" in cfg:
        s = cfg["s"]
        crit = AntibiasLoss(cfg["n"])
        ab = crit(pred.view(SB, s, s, 3).permute(0, 3, 1, 2), gt_colors.view(SB, s, s, 3).permute(0, 3, 1, 2))       # :280-282
        pooled = crit.downsampling(pred.view(SB, s, s, 3).permute(0, 3, 1, 2)) - crit.downsampling(gt_colors.view(SB, s, s, 3).permute(0, 3, 1, 2))
        loss = loss + float(g[1]) * ab
        out.update(ab=ab, pooled=pooled)
    else:
        out.update(ab=torch.zeros((), dtype=dtype), pooled=torch.zeros((SB, 3, 0, 0), dtype=dtype))
    out["d_pred"], = torch.autograd.grad(loss, pred)
    out.update(dE=d_cams[0], dK=d_cams[1], dn=d_cams[2], df=d_cams[3])
    return {k: v.detach().numpy() for k, v in out.items()}


def generate():
    import torch

    from oracle import ref_harness
    ref_harness.install_stubs()
    from src.util.cam_geometry import gen_rays
    spec = importlib.util.spec_from_file_location("_ref_antibiasloss", Path(ref_harness.REFERENCE_ROOT) / "src" / "losses" / "antibiasloss.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(1)

    store, index = {}, {}
    for name, cfg in CASES.items():
        seed = cfg["seed"]
        while True:
            inp = case_inputs(cfg, seed)
            r32 = reference_lines(gen_rays, mod.AntibiasLoss, inp, cfg, torch.float32)
            r64 = reference_lines(gen_rays, mod.AntibiasLoss, inp, cfg, torch.float64)
            pooled = np.abs(r64["pooled"])
            degenerate = pooled == 0.0
            if cfg.get("equal"):
                assert degenerate[0, :, 1, 0].all() and degenerate.sum() == 3, "the equal cell must pool to an exact 0"
                assert (r32["pooled"][0, :, 1, 0] == 0).all()
            else:
                assert not degenerate.any()
            if pooled.size == 0 or pooled[~degenerate].min() >= MIN_DIFF:
                break
            seed += 1000
        assert np.array_equal(r32["gt"].astype(np.float64), r64["gt"])
        cfg = dict(cfg, seed=seed, B=int(inp["idx"].shape[1]))
        index[name] = cfg
        for k, v in inp.items():
            store[f"{name}.{k}"] = v
        store[f"{name}.gt"] = r32["gt"]
        store[f"{name}.min_abs_pooled_diff"] = np.float64(pooled[~degenerate].min() if (~degenerate).any() else np.inf)
        for k in ("mse", "ab", "d_pred", "dE", "dK", "dn", "df"):
            store[f"{name}.{k}32"] = r32[k]
            store[f"{name}.{k}64"] = r64[k]
            store[f"{name}.dev_{k}"] = np.float64(np.abs(r32[k].astype(np.float64) - r64[k]).max())
        store[f"{name}.dev_rays"] = np.float64(np.abs(r32["rays"].astype(np.float64) - r64["rays"]).max())
        print(name, {k: float(store[f"{name}.dev_{k}"]) for k in ("mse", "ab", "d_pred", "dE", "dK")}, "min |pooled diff|",
              float(store[f"{name}.min_abs_pooled_diff"]), "seed", seed)
    out = GOLDEN / "train_glue.npz"
    np.savez_compressed(out, index=json.dumps(index), min_diff=np.float64(MIN_DIFF), **store)
    print(f"{out}: {out.stat().st_size} bytes")


if __name__ == "__main__":
    generate()
