"""Float64 restatement, on the CPU, of the two training-step functions of diner_amd/csrc/train_glue.hip and of their gradients, written
from the formulas of include/diner_hip.h with explicit indices, not with the reference's operators:

* ``gen_rays_at_ref``: gen_rays (reference src/util/cam_geometry.py:36-79) at the selected pixels (src/models/diner.py:257-258),
  ``gen_rays_at_grads_ref``: its camera gradients for a given d_rays (autograd through the restatement);
* ``photo_loss_ref``: the ground-truth gather, the MSE and the antibias loss (diner.py:265-267, :280-282, src/losses/antibiasloss.py),
  ``photo_loss_dpred_ref``: d_pred in closed form, split into the MSE term and the antibias constant.

Inputs are the fp32 values widened to ``dtype`` (float64 by default: the oracle of the GPU tests).  ``variant`` builds a deliberately wrong
form; tests/test_train_glue_host.py shows that each comparison rejects the ones that touch it."""
import numpy as np
import torch

VARIANTS = ("swap_xy", "ceil_pool", "diff_pool_tiny_sign", "mean_div_channels")
TINY = 1e-30     # "diff_pool_tiny_sign": the residue a differently ordered sum leaves in a cell whose patches are equal


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a)).to(dtype) if not isinstance(a, torch.Tensor) else a.to(dtype)


def _xy(idx, H, W, variant=None):
    """pixel index -> (x, y): idx = x + y W (diner.py:246)"""
    idx = torch.as_tensor(np.asarray(idx)).long() if not isinstance(idx, torch.Tensor) else idx.long()
    if variant == "swap_xy":
        return idx // H, idx % H      # reads the index as y + x H
    return idx % W, idx // W


def gen_rays_at_ref(E, K, W, H, zn, zf, idx, dtype=torch.float64, variant=None):
    """E [SB,4,4], K [SB,3,3], zn / zf [SB], idx [SB,B] -> rays [SB,B,8] (origin, unit direction, near, far)"""
    E, K, zn, zf = _t(E, dtype), _t(K, dtype), _t(zn, dtype), _t(zf, dtype)
    SB, B = idx.shape
    x, y = _xy(idx, H, W, variant)
    px = (x.to(dtype) + 0.5 - K[:, 0, 2].view(SB, 1)) / K[:, 0, 0].view(SB, 1)
    py = (y.to(dtype) + 0.5 - K[:, 1, 2].view(SB, 1)) / K[:, 1, 1].view(SB, 1)
    n = (px * px + py * py + 1.0).sqrt()
    d = torch.stack((px / n, py / n, 1.0 / n), dim=-1)                     # [SB,B,3] camera space
    R, t = E[:, :3, :3], E[:, :3, 3]
    dirs = torch.stack([sum(R[:, k, r].view(SB, 1) * d[..., k] for k in range(3)) for r in range(3)], dim=-1)     # R^T d
    o = torch.stack([-sum(R[:, k, r] * t[:, k] for k in range(3)) for r in range(3)], dim=-1)                     # -R^T t
    return torch.cat((o.view(SB, 1, 3).expand(SB, B, 3), dirs, zn.view(SB, 1, 1).expand(SB, B, 1), zf.view(SB, 1, 1).expand(SB, B, 1)), dim=-1)


def gen_rays_at_grads_ref(E, K, W, H, zn, zf, idx, d_rays, dtype=torch.float64, variant=None):
    """-> (d_E [SB,4,4], d_K [SB,3,3], d_near [SB], d_far [SB]) of sum(rays * d_rays)"""
    leaves = [_t(a, dtype).clone().requires_grad_(True) for a in (E, K, zn, zf)]
    rays = gen_rays_at_ref(*leaves[:2], W, H, *leaves[2:], idx, dtype=dtype, variant=variant)
    return torch.autograd.grad(rays, leaves, _t(d_rays, dtype))


def gather_gt_ref(target, idx, variant=None):
    """target [SB,3,H,W], idx [SB,B] -> [SB,B,3] = target[b, :, y, x] (dtype kept)"""
    target = torch.as_tensor(np.asarray(target)) if not isinstance(target, torch.Tensor) else target
    SB, _, H, W = target.shape
    x, y = _xy(idx, H, W, variant)
    if variant == "swap_xy":
        x, y = x.clamp(max=W - 1), y.clamp(max=H - 1)
    b = torch.arange(SB).view(SB, 1).expand_as(x)
    return torch.stack([target[b, c, y, x] for c in range(3)], dim=-1)


def _cells(v, s, p, variant=None):
    """v [SB,B,3] as an s x s patch (row-major) -> the cell averages [SB,3,nc,nc] of p x p pixels; floor: trailing rows / columns dropped"""
    SB = v.shape[0]
    img = v.view(SB, s, s, 3)
    nc = -(-s // p) if variant == "ceil_pool" else s // p
    out = torch.zeros((SB, 3, nc, nc), dtype=v.dtype)
    for cy in range(nc):
        for cx in range(nc):
            win = img[:, cy * p:min((cy + 1) * p, s), cx * p:min((cx + 1) * p, s)]
            out[:, :, cy, cx] = win.sum(dim=(1, 2)) / (win.shape[1] * win.shape[2])
    return out


def pooled_diff_ref(pred, gt, s, n, variant=None):
    """avg_cell(pred) - avg_cell(gt) [SB,3,nc,nc]: pooled separately, then subtracted"""
    p = 2 ** n
    if variant == "diff_pool_tiny_sign":
        return _cells(pred - gt, s, p) + TINY
    return _cells(pred, s, p, variant) - _cells(gt, s, p, variant)


def photo_loss_ref(pred, target, idx, patch=None, n=3, dtype=torch.float64, variant=None):
    """-> (mse, antibias, gt_colors [SB,B,3] in the target's dtype): scalars in ``dtype``"""
    gt_raw = gather_gt_ref(target, idx, variant)
    pred, gt = _t(pred, dtype), gt_raw.to(dtype)
    SB, B, _ = pred.shape
    mse = ((pred - gt) ** 2).sum() / (SB * B * (1 if variant == "mean_div_channels" else 3))
    if patch is None:
        return mse, torch.zeros((), dtype=dtype), gt_raw
    diff = pooled_diff_ref(pred, gt, patch, n, variant)
    return mse, diff.abs().sum() / diff.numel(), gt_raw


def photo_loss_dpred_ref(pred, gt, patch=None, n=3, g_mse=1.0, g_ab=0.0, dtype=torch.float64, variant=None):
    """-> (d_pred, mse_term, ab_term) [SB,B,3]: d_pred = mse_term + ab_term,
    mse_term = g_mse 2 (pred - gt) / (SB B 3), ab_term = g_ab sign(cell diff) / (p^2 SB 3 nc^2) inside a cell, 0 outside every cell"""
    pred, gt = _t(pred, dtype), _t(gt, dtype)
    SB, B, _ = pred.shape
    mse_term = g_mse * 2.0 * (pred - gt) / (SB * B * (1 if variant == "mean_div_channels" else 3))
    ab_term = torch.zeros_like(mse_term)
    if patch is not None:
        s, p = patch, 2 ** n
        diff = pooled_diff_ref(pred, gt, s, n, variant)
        nc = diff.shape[-1]
        const = g_ab / (p * p * diff.numel())
        img = ab_term.view(SB, s, s, 3)
        for cy in range(nc):
            for cx in range(nc):
                win = img[:, cy * p:min((cy + 1) * p, s), cx * p:min((cx + 1) * p, s)]
                scale = 1.0 if variant != "ceil_pool" else (p * p) / (win.shape[1] * win.shape[2])
                win += (const * scale * torch.sign(diff[:, :, cy, cx])).view(SB, 1, 1, 3)
    return mse_term + ab_term, mse_term, ab_term
