"""Float64 restatements of the training step's point, scatter and reduction kernels, the case sets and the comparison functions that
tests/test_train_stage_refs_host.py (CPU) and tests/test_gpu_train_stage_kernels.py (GPU) share.

* ``point_inputs_ref``: ``o + z d -> R x + t -> uv -> nearest depth texel -> in55 -> grid_sample`` in differentiable torch
  (reference src/models/nerf_renderer.py:304-305, src/models/pixelnerf.py:91-121, 128, src/models/image_encoder.py:97-151,
  src/models/positional_encoding.py:33-53), for the six 4-tap lookup modes.  It returns the inputs, the latent lookup, and the footprint
  in the kernels' tap order (nw, ne, sw, se) with the kernels' convention for a tap that falls off the map: the index clamped into the
  map, the weight 0.  ``variant`` 0 / 1 are two float32 operation orders (multiply-then-add against a fused multiply-add emulated in
  float64, ``ey * ex`` against the expanded product, two association orders of the matrix products and the four-tap sum): the CPU float32
  side of every bound.
* ``backward_ref``: torch autograd of ``L = <d_in, in55> + <d_zlat, zlat>`` through that restatement.  Every leaf is expanded to one copy
  per (view, point) row, so that one backward pass gives each row's contribution: their sum is the gradient, the sum of their absolute
  values the magnitude the kernels' reductions are rounded at.
* ``scatter_runs``: the latent scatter as the kernel walks it (runs of SCATTER_RUN rows, merged while the view and the four indices
  agree); without a defect it is the plain scatter-add.
* float64 forms of amax, the column sums, the view mean, the head and the layout change.

Every restatement takes ``defect=<name>``: a deliberately wrong variant.  The CPU tests assert that the comparison functions below reject
each of them, so that a comparison which the GPU passes is known to be able to fail.

Tolerances.  A bound is ``MARGIN`` x the worse float32 CPU evaluation's error against float64 plus a floor, from CPU values only:
one float32 ulp of the family's magnitude for elementwise outputs (+ ``PE_SIN_BAR`` on the positional-code columns: the documented error
of the device's sine, diner_amd/csrc/common.hpp); for a summed output the error is taken relative to the sum of the absolute values of
each element's terms, with a floor of (summation depth) x 2^-24 of it (``reduce_depth``; a depth texel: the rows that reach it).  The
latent scatter's CPU-side part is the forward's tap-weight bound x sum |d_zlat| of the element's terms (``TrainStageCase.refs`` says
why), its floor (terms of the element) x 2^-24 of sum |d_zlat| |w|.  The cotangents of the positional codes are scaled by 1 / f^2
(``cotangent_in``): float32 cannot carry the top octave's derivative more finely than 6e-5, whatever evaluates it.
"""
from __future__ import annotations

import zlib
from types import SimpleNamespace

import numpy as np
import torch

F32 = np.float32
MARGIN = 4.0                    # tests/stage_refs.py
EPS32 = 2.0 ** -23
U32 = 2.0 ** -24
PE_SIN_BAR = 4.2e-7             # pe_sin (common.hpp, tools/sin_probe.hip)
DECISION_MARGIN = 1e-3          # texels
TINY = 1e-30
SCATTER_RUN = 16                # train_blocks.hpp
CAMG_BLOCKS = 256
MODES = [(i, p) for i in ("bilinear", "nearest") for p in ("border", "zeros", "reflection")]
MODE_IDS = [f"{i}-{p}" for i, p in MODES]
LEAVES = ("rays", "poses", "focal", "c", "image_shape", "depths")

FWD_DEFECTS = ("align_corners", "depth_floor", "no_feature_padding", "swap_ne_sw", "border_keeps_weight")     # point_inputs_ref(defect=)
GRAD_DEFECTS = ("border_grad_kept", "reflection_sign")                                                          # ... its gradient only
BWD_DEFECTS = ("dR_transposed", "dfocal_no_invz")                                                               # backward_ref(defect=)


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _fma(a, b, c, variant):
    """a * b + c: variant 0 rounds the product, variant 1 rounds once (the product and sum formed in float64)"""
    if variant == 0 or a.dtype == torch.float64:
        return a * b + c
    c = c if torch.is_tensor(c) else torch.tensor(c, dtype=torch.float64)
    return (a.double() * (b.double() if torch.is_tensor(b) else b) + c.double()).to(a.dtype)


def _pad_coord(x, size, padding, defect=None):
    """ATen's reflect_coordinates / clip_coordinates (align_corners=False) with their gradient conventions: the sign flips with every
    reflection, and the gradient is 0 where the coordinate is clipped (x <= 0 or x >= size - 1)"""
    if padding == "reflection":
        a = x + 0.5
        span = float(size)
        flips = torch.floor(a.abs() / span)
        extra = a.abs() - flips * span
        r = torch.where(flips % 2 == 0, extra - 0.5, span - extra - 0.5)
        x = r.detach() + (x - x.detach()) if defect == "reflection_sign" else r
    if padding != "zeros":
        clipped = x.detach().clamp(0.0, float(size - 1))
        if defect == "border_grad_kept":
            x = clipped + (x - x.detach())
        else:
            x = torch.where((x > 0) & (x < size - 1), x, clipped)
    return x


def expand_rows(scene, rays, z, dtype, grad=False):
    """one copy of every leaf per (view, point) row: dict of tensors [NV, P, ...]"""
    NV = scene.poses.shape[0]
    NR, K = z.shape
    P = NR * K
    rays_p = np.repeat(np.asarray(rays, F32), K, 0)                                     # [P, 8]
    rows = dict(o=np.broadcast_to(rays_p[None, :, 0:3], (NV, P, 3)), d=np.broadcast_to(rays_p[None, :, 3:6], (NV, P, 3)),
                R=np.broadcast_to(scene.poses[:, None, :3, :3], (NV, P, 3, 3)), t=np.broadcast_to(scene.poses[:, None, :3, 3], (NV, P, 3)),
                focal=np.broadcast_to(scene.focal[:, None], (NV, P, 2)), c=np.broadcast_to(scene.c[:, None], (NV, P, 2)),
                ishape=np.broadcast_to(np.asarray(scene.image_shape, F32)[None, None], (NV, P, 2)))
    rows = {k: _t(v.copy(), dtype).requires_grad_(grad) for k, v in rows.items()}
    rows["z"] = _t(np.broadcast_to(np.asarray(z, F32).reshape(1, P, 1), (NV, P, 1)).copy(), dtype)
    return rows


def point_inputs_ref(scene, rays, z, mode=("bilinear", "border"), dtype=torch.float64, variant=0, defect=None, grad=False, coords_only=False):
    """scene: poses [NV,4,4], focal [NV,2], c [NV,2], image_shape [2] = (w, h), depths [NV,H,W], latent [NV,C,h,w], feature_padding,
    freq_factor, num_freqs (float32 data); rays [NR,8]; z [NR,K].  Rows are view-major: [NV, P = NR K, ...].
    -> namespace: in55 [NV,P,7+8F], zlat [NV,P,C], idx [NV,P,4] (y w + x), wt [NV,P,4], dd [NV,P,2] = (ddy, ddx), uv, the unpadded
    coordinates ix, iy (latent) and dx, dy (depth map), pz, and the leaves (rows, depth_row, latent)."""
    interp, padding = mode
    V = variant
    NV, Cc, h, w = scene.latent.shape
    H, W = scene.depths.shape[1:]
    F = int(scene.num_freqs)
    r = expand_rows(scene, rays, z, dtype, grad)
    o, d, R, t, zz = r["o"], r["d"], r["R"], r["t"], r["z"]
    pts = _fma(zz, d, o, V)                                                             # nerf_renderer.py:304
    if V == 0:
        xc = ((R[..., 0] * pts[..., None, 0] + R[..., 1] * pts[..., None, 1]) + R[..., 2] * pts[..., None, 2]) + t   # pixelnerf.py:91-93
        dc = (R[..., 0] * d[..., None, 0] + R[..., 1] * d[..., None, 1]) + R[..., 2] * d[..., None, 2]               # :99-101
    else:
        xc = R[..., 2] * pts[..., None, 2] + (R[..., 1] * pts[..., None, 1] + (R[..., 0] * pts[..., None, 0] + t))
        dc = R[..., 2] * d[..., None, 2] + (R[..., 1] * d[..., None, 1] + R[..., 0] * d[..., None, 0])
    pz = xc[..., 2:3]
    if V == 0:
        uv = xc[..., :2] / pz * r["focal"] + r["c"]                                     # :105-106
        uv = uv / r["ishape"] * 2.0 - 1.0                                               # :107-108
    else:
        uv = (xc[..., :2] * r["focal"]) / pz + r["c"]
        uv = uv * (2.0 / r["ishape"]) - 1.0
    u, vv = uv[..., 0], uv[..., 1]
    # nearest depth texel, border padding (image_encoder.py:129-151, pixelnerf.py:114-117)
    dx = _fma(u + 1.0, W / 2.0, -0.5, V)
    dy = _fma(vv + 1.0, H / 2.0, -0.5, V)
    if coords_only:     # the unpadded coordinates alone (what the case generator's margin loop needs)
        fp = float(F32(scene.feature_padding))
        return SimpleNamespace(dx=dx, dy=dy, ix=_fma(u * ((w - fp * 2.0) / w) + 1.0, w / 2.0, -0.5, V),
                               iy=_fma(vv * ((h - fp * 2.0) / h) + 1.0, h / 2.0, -0.5, V))
    rnd = torch.floor if defect == "depth_floor" else torch.round
    ddx = rnd(dx.detach().clamp(0.0, W - 1.0)).long()
    ddy = rnd(dy.detach().clamp(0.0, H - 1.0)).long()
    vid = torch.arange(NV)[:, None].expand(NV, u.shape[1])
    depth_row = _t(scene.depths, dtype)[vid, ddy, ddx].clone().requires_grad_(grad)
    delta = depth_row[..., None] - pz
    # positional codes (positional_encoding.py:45-49): column 3 j + i = sin(f_(j>>1) x_i + (j & 1) pi / 2)
    half_pi = float(F32(1.5707963267948966))
    freqs = [float(F32(F32(scene.freq_factor) * F32(2.0 ** (j >> 1)))) for j in range(2 * F)]

    def code(x):
        return torch.cat([torch.sin(_fma(x, freqs[j], half_pi if j & 1 else 0.0, V)) for j in range(2 * F)], -1)

    in55 = torch.cat([xc, code(xc), dc, delta, code(delta)], -1)
    # the latent footprint (image_encoder.py:97-127)
    fp = float(F32(scene.feature_padding))
    one = torch.ones((), dtype=dtype)
    sxl = (one * w - one * fp * 2.0) / w
    syl = (one * h - one * fp * 2.0) / h
    if defect == "no_feature_padding":
        sxl, syl = one, one
    if defect == "align_corners":
        ix, iy = (u * sxl + 1.0) / 2.0 * (w - 1), (vv * syl + 1.0) / 2.0 * (h - 1)
    else:
        ix, iy = _fma(u * sxl + 1.0, w / 2.0, -0.5, V), _fma(vv * syl + 1.0, h / 2.0, -0.5, V)
    px_, py_ = _pad_coord(ix, w, padding, defect), _pad_coord(iy, h, padding, defect)
    if interp == "nearest":
        xa, ya = torch.round(px_.detach()), torch.round(py_.detach())
        xb, yb = xa, ya
        wt = [torch.ones_like(px_), torch.zeros_like(px_), torch.zeros_like(px_), torch.zeros_like(px_)]
    else:
        xa, ya = torch.floor(px_.detach()), torch.floor(py_.detach())
        xb, yb = xa + 1.0, ya + 1.0
        fx, fy = px_ - xa, py_ - ya
        if V == 0:
            ex, ey = 1.0 - fx, 1.0 - fy
            wt = [ey * ex, ey * fx, fy * ex, fy * fx]
        else:
            wt = [1.0 - fy - fx + fy * fx, fx - fy * fx, fy - fy * fx, fy * fx]
    if defect == "swap_ne_sw":
        wt[1], wt[2] = wt[2], wt[1]
    inx = lambda p, n: (p >= 0) & (p <= n - 1)
    ok = [inx(xa, w) & inx(ya, h), inx(xb, w) & inx(ya, h), inx(xa, w) & inx(yb, h), inx(xb, w) & inx(yb, h)]
    if defect != "border_keeps_weight":
        wt = [torch.where(m, x, torch.zeros_like(x)) for m, x in zip(ok, wt)]
    cl = lambda p, n: p.clamp(0.0, n - 1.0).long()
    x0, x1, y0, y1 = cl(xa, w), cl(xb, w), cl(ya, h), cl(yb, h)
    idx = torch.stack([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1], -1)
    wt = torch.stack(wt, -1)
    latent = _t(scene.latent, dtype).clone().requires_grad_(grad)
    flat = latent.permute(0, 2, 3, 1).reshape(NV, h * w, Cc)
    tx = [flat[vid, idx[..., i]] * wt[..., i:i + 1] for i in range(4)]
    zlat = ((tx[0] + tx[1]) + tx[2]) + tx[3] if V == 0 else (tx[3] + tx[2]) + (tx[1] + tx[0])
    return SimpleNamespace(in55=in55, zlat=zlat, idx=idx, wt=wt, dd=torch.stack([ddy, ddx], -1), u=u, v=vv, ix=ix, iy=iy, dx=dx, dy=dy, pz=pz[..., 0],
                           rows=r, depth_row=depth_row, latent=latent, ok=torch.stack(ok, -1))


def decision_margin(f):
    """the smallest distance (texels) of a float64 run's latent and depth-map coordinates to a multiple of 0.5: the integers decide the
    footprint's floor, the border clip (0, size - 1) and its zeroed gradient; the half-integers the depth texel's and the nearest lookup's
    rint and the reflection seams (x + 0.5 a multiple of the size)"""
    m = np.inf
    for x in (f.ix, f.iy, f.dx, f.dy):
        x = x.detach().double().numpy() * 2.0
        m = min(m, float(np.abs(x - np.round(x)).min()) / 2.0)
    return m


def backward_ref(f, d_in, d_zlat, d_far, NR, K, depths_shape, defect=None):
    """autograd of <d_in, in55> + <d_zlat, zlat> through a ``point_inputs_ref(..., grad=True)`` run -> (grads, scales): dicts over LEAVES +
    'latent' of the gradient and of the sum of the absolute values of its per-row terms (float64 numpy; in the run's dtype summed in
    numpy float64 from the per-row values, so a float32 run's error is its rows' error)."""
    NV, P = f.in55.shape[:2]
    L = (f.in55 * _t(d_in, f.in55.dtype).view(NV, P, -1)).sum() + (f.zlat * _t(d_zlat, f.zlat.dtype).view(NV, P, -1)).sum()
    r = f.rows
    leaves = [r["o"], r["d"], r["R"], r["t"], r["focal"], r["c"], r["ishape"], f.depth_row, f.latent]
    g = [x.double().numpy() for x in torch.autograd.grad(L, leaves, allow_unused=True, materialize_grads=True)]
    go, gd, gR, gt, gf, gc, gi, gdep, glat = g
    if defect == "dfocal_no_invz":
        gf = gf * f.pz.detach().double().numpy()[..., None]
    if defect == "dR_transposed":
        gR = gR.transpose(0, 1, 3, 2)
    out, scale = {}, {}
    for red, store in ((lambda a: a, out), (np.abs, scale)):
        rays = np.zeros((NR, 8))
        rays[:, 0:3] = red(go).reshape(NV, NR, K, 3).sum((0, 2))
        rays[:, 3:6] = red(gd).reshape(NV, NR, K, 3).sum((0, 2))
        rays[:, 7] = red(np.asarray(d_far, np.float64)) if d_far is not None else 0.0
        poses = np.zeros((NV, 4, 4))
        poses[:, :3, :3], poses[:, :3, 3] = red(gR).sum(1), red(gt).sum(1)
        dep = np.zeros(depths_shape)
        dd = f.dd.numpy()
        np.add.at(dep, (np.arange(NV)[:, None].repeat(P, 1), dd[..., 0], dd[..., 1]), red(gdep))
        store.update(rays=rays, poses=poses, focal=red(gf).sum(1), c=red(gc).sum(1), image_shape=red(gi).sum((0, 1)), depths=dep)
    out["latent"] = glat
    cnt = np.zeros(depths_shape)
    np.add.at(cnt, (np.arange(NV)[:, None].repeat(P, 1), dd[..., 0], dd[..., 1]), 1.0)
    scale["depth_rows"] = cnt                                  # rows per depth texel
    return out, scale


def reduce_depth(name, NR, K, NV):
    """the number of float32 additions behind one element of a reduced leaf, from the reductions' documented shape: rays sum NV K records
    in sequence; the per-view leaves sum ceil(P / (nblk 256)) rows per thread, a 256-wide tree (8 levels) and nblk <= CAMG_BLOCKS partials;
    image_shape adds the NV views.  (A depth texel: the number of rows that map to it, see refs.)"""
    P = NR * K
    nblk = min((P + 255) // 256, CAMG_BLOCKS)
    per_view = -(-P // (nblk * 256)) + 8 + nblk
    return {"rays": NV * K, "image_shape": per_view + NV}.get(name, per_view)


def scatter_runs(idx, wt, dz, P, NV, hw, start=None, defect=None):
    """dlatent [NV, hw, C] += dz[row] * wt[row, i] at idx[row, i], walked as bilinear_scatter_kernel walks it; float64.
    defect 'no_view_flush': a run is not flushed where the view changes (its sums land in the previous view)."""
    R, Cc = dz.shape
    out = np.zeros((NV, hw, Cc)) if start is None else np.array(start, np.float64)
    idx, wt, dz = np.asarray(idx).reshape(R, 4), np.asarray(wt, np.float64).reshape(R, 4), np.asarray(dz, np.float64)
    for row0 in range(0, R, SCATTER_RUN):
        cur, cur_v, acc, used = None, -1, None, None
        for row in range(row0, min(row0 + SCATTER_RUN, R)):
            v = row // P
            new_v = v != cur_v and defect != "no_view_flush"
            if cur is None or new_v or not np.array_equal(idx[row], cur):
                if cur is not None:
                    for i in range(4):
                        if used[i]:
                            out[cur_v, cur[i]] += acc[i]
                cur, cur_v, acc, used = idx[row].copy(), v, np.zeros((4, Cc)), [False] * 4
            for i in range(4):
                if wt[row, i] != 0.0:
                    acc[i] += dz[row] * wt[row, i]
                    used[i] = True
        if cur is not None:
            for i in range(4):
                if used[i]:
                    out[cur_v, cur[i]] += acc[i]
    return out


def scatter_plain(idx, wt, dz, P, NV, hw, absolute=False):
    """the same sums without the walk (np.add.at) -> (sum [NV,hw,C], number of non-zero terms per texel [NV,hw]); absolute: of
    |dz| |w|; absolute = 'dz': of |dz| over the taps of non-zero weight"""
    R, Cc = dz.shape
    idx, wt, dz = np.asarray(idx).reshape(R, 4), np.asarray(wt, np.float64).reshape(R, 4), np.asarray(dz, np.float64)
    if absolute:
        wt, dz = np.abs(wt), np.abs(dz)
    out, cnt = np.zeros((NV, hw, Cc)), np.zeros((NV, hw))
    v = np.arange(R) // P
    for i in range(4):
        np.add.at(out, (v, idx[:, i]), dz * (wt[:, i:i + 1] if absolute != "dz" else (wt[:, i:i + 1] != 0)))
        np.add.at(cnt, (v, idx[:, i]), (wt[:, i] != 0).astype(np.float64))
    return out, cnt


# ------------------------------------------------------------------------------------------------
# reductions, view mean, head, layout
# ------------------------------------------------------------------------------------------------
def amax_ref(x, defect=None):
    x = np.asarray(x, F32).reshape(-1)
    if defect == "no_tail":
        x = x[: x.size // 4 * 4]
    return F32(np.abs(x).max(initial=0.0))


def colsum_ref(dY, db0, defect=None, absolute=False):
    """db0 + column sums of dY [M,N] in float64 (absolute: of |dY|, without db0)"""
    dY = np.asarray(dY, np.float64)
    if defect == "first_sweep":          # rows past one sweep of a 2048-block grid of 4-row blocks are never visited
        dY = dY[: 2048 * 4]
    return np.abs(dY).sum(0) if absolute else np.asarray(db0, np.float64) + dY.sum(0)


def view_mean_ref(x, NV, backward=False, defect=None):
    """forward: x [NV,PC] -> [PC]; backward: d_mean [PC] -> [NV,PC] (resnetfc.py:146-149)"""
    x = np.asarray(x, np.float64)
    div = NV - 1 if defect == "nv_minus_1" else NV
    return np.broadcast_to(x / div, (NV,) + x.shape).copy() if backward else x.sum(0) / div


def head_ref(out, dtype=np.float64):
    """pixelnerf.py:139-143: sigmoid on the colour slots, relu on the sigma slot of out [n4] (n4 = 4 points' worth of slots)"""
    v = np.asarray(out, dtype)
    sig = (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(dtype) if dtype == np.float64 else (F32(1) / (F32(1) + np.exp(-v)))
    sigma = (np.arange(v.size) & 3) == 3
    return np.where(sigma, np.maximum(v, 0), sig).astype(dtype)


def head_bwd_ref(out, y, g, defect=None):
    """d_out from the saved output y: colour g y (1 - y); sigma g [out > 0] (threshold_backward)"""
    out, y, g = (np.asarray(a, np.float64) for a in (out, y, g))
    sigma = (np.arange(out.size) & 3) == 3
    gate = out >= 0 if defect == "relu_ge" else out > 0
    return np.where(sigma, np.where(gate, g, 0.0), g * y * (1.0 - y))


def nhwc_to_nchw_ref(x, N, Cc, hw):
    return np.ascontiguousarray(np.asarray(x).reshape(N, hw, Cc).transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------
# comparison functions: each returns a list of findings ([] = equal within the bound); NaN fails
# ------------------------------------------------------------------------------------------------
def _within(d, tol):
    return bool(np.all(d <= tol))


def compare_taps(idx, wt, ref_idx, ref_wt, wt_bound, hw):
    bad = []
    idx, ref_idx = np.asarray(idx), np.asarray(ref_idx)
    if idx.min() < 0 or idx.max() > hw - 1:
        bad.append(f"tap index outside the map: [{idx.min()}, {idx.max()}] of {hw}")
    if not np.array_equal(idx, ref_idx):
        rows = np.nonzero((idx != ref_idx).any(-1))[0]
        bad.append(f"tap indices differ on {rows.size} rows (first {rows[:5].tolist()})")
    d = np.abs(np.asarray(wt, np.float64) - ref_wt)
    if not _within(d, wt_bound):
        bad.append(f"tap weights: max error {np.nanmax(d):.3e} > {wt_bound:.3e}")
    z = ref_wt == 0
    if not np.all(np.asarray(wt)[z] == 0):
        bad.append(f"{int((np.asarray(wt)[z] != 0).sum())} taps off the map keep a weight")
    return bad


def in_families(F):
    """column families of the 7 + 8F inputs: name -> column slice / list"""
    fam = {"position": list(range(0, 3)), "direction": list(range(3 + 6 * F, 6 + 6 * F)), "depth_dist": [6 + 6 * F]}
    for k in range(F):
        fam[f"code_xyz_f{k}"] = list(range(3 + 6 * k, 9 + 6 * k))
        fam[f"code_dist_f{k}"] = [7 + 6 * F + 2 * k, 8 + 6 * F + 2 * k]
    return fam


def compare_inputs(inp, ref_in, bounds, F):
    """inp [R, ld] (ld >= 7 + 8F; the columns past the inputs must be 0) against ref_in [R, 7 + 8F], bounds: family -> tolerance"""
    bad = []
    inp = np.asarray(inp, np.float64)
    n = 7 + 8 * F
    if not np.all(inp[:, n:] == 0):
        bad.append("padding columns are not 0")
    for name, cols in in_families(F).items():
        d = np.abs(inp[:, cols] - ref_in[:, cols])
        if not _within(d, bounds[name]):
            bad.append(f"{name}: max error {np.nanmax(d):.3e} > {bounds[name]:.3e}")
    return bad


def compare_abs(name, got, ref, tol):
    d = np.abs(np.asarray(got, np.float64) - ref)
    return [] if _within(d, tol) else [f"{name}: max error {np.nanmax(d):.3e} > {np.max(tol):.3e}"]


def compare_scaled(name, got, ref, scale, rel):
    """|got - ref| <= rel * scale + TINY elementwise (scale: the sum of the absolute values of the element's terms)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    tol = rel * scale + TINY
    if _within(d, tol):
        return []
    return [f"{name}: max error / scale {np.nanmax(d / (scale + TINY)):.3e} > {np.max(rel):.3e}" if np.isfinite(d).all() else f"{name}: not finite"]


def scaled_error(got, ref, scale):
    s = np.asarray(scale) > 0
    if not s.any():
        return 0.0
    return float((np.abs(np.asarray(got, np.float64) - ref)[s] / np.asarray(scale)[s]).max())


def compare_bits(name, got, ref):
    a, b = np.ascontiguousarray(got, F32).view(np.uint32), np.ascontiguousarray(ref, F32).view(np.uint32)
    if a.shape == b.shape and np.array_equal(a, b):
        return []
    if a.shape != b.shape:
        return [f"{name}: shape {a.shape} against {b.shape}"]
    i = np.flatnonzero(a != b)[0]
    return [f"{name}: {int((a != b).sum())} elements differ in their bits (first: {a.view(F32).flat[i]!r} against {b.view(F32).flat[i]!r} at {i})"]


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr_ = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr_, 0], [sr_, cr, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cotangent_in(rs, shape, F, freq_factor):
    """N(0,1) cotangents of the inputs, those of the positional codes of frequency f divided by f^2.  d sin(f x) / dx = f cos(f x): a
    rounding dx of x_cam changes that term by f^2 dx per unit of cotangent, so with unit cotangents the top octave (f = 201) alone would
    put a relative 6e-5 -- float32's ulp of x_cam times f -- on every geometric gradient, in any float32 evaluation, and nothing finer
    could be seen.  Divided by f^2 every octave's rounding weighs the same, and every column still carries a share of the gradient
    (the top octave's 1.5 % of the codes' part) that is thousands of times the bound."""
    g = rs.standard_normal(shape)
    for name, cols in in_families(F).items():
        if name.startswith("code"):
            g[..., cols] /= (float(freq_factor) * 2.0 ** int(name.rsplit("f", 1)[1])) ** 2
    return g.astype(F32)


class TrainStageCase:
    """A seeded scene of rotated, translated cameras with unequal focal lengths and off-centre principal points (identity cameras hide
    row-major against column-major and fx against fy), rays whose consecutive samples move by a fraction of a texel, about a third of
    the points outside the image / the map, and every point at least DECISION_MARGIN texels from every decision boundary (build nudges
    the offenders' depths; refs() asserts it for every row).  SB scenes with their own cameras and latents."""
    exact = False
    H, W = 5, 6
    image_shape = (12.0, 10.0)

    def __init__(self, hw, fpad, NV, NR, K, C=512, F=6, SB=1):
        self.h, self.w = hw
        self.fpad, self.NV, self.NR, self.K, self.C, self.F, self.SB = float(fpad), NV, NR, K, C, F, SB
        self.P = NR * K
        self.id = f"{self.h}x{self.w}-fp{fpad}-NV{NV}-NR{NR}-K{K}-C{C}-F{F}" + (f"-SB{SB}" if SB > 1 else "")
        self.seed = zlib.crc32(self.id.encode()) % 100000
        self._refs = {}

    # -- generation ---------------------------------------------------------------------------
    def _scene(self, rs):
        NV, h, w = self.NV, self.h, self.w
        iw, ih = self.image_shape
        sxl, syl = (w - 2 * self.fpad) / w, (h - 2 * self.fpad) / h
        ext = 1.0 if self.fpad == 0 else 0.8 / min(sxl, syl)      # NDC half-extent of the box the points are drawn from
        poses = np.tile(np.eye(4), (NV, 1, 1))
        for v in range(NV):
            poses[v, :3, :3] = _rot(*rs.uniform(-0.35, 0.35, 3))
            poses[v, :3, 3] = [rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2), 2.2 + rs.uniform(-0.2, 0.2)]
        focal = np.stack([ext * iw / 2 * 2.2 * rs.uniform(0.9, 1.1, NV), 0.8 * ext * ih / 2 * 2.2 * rs.uniform(0.9, 1.1, NV)], -1)
        c = np.stack([iw / 2 + rs.uniform(-1, 1, NV), ih / 2 + rs.uniform(-1, 1, NV)], -1)
        return SimpleNamespace(poses=poses.astype(F32), focal=focal.astype(F32), c=c.astype(F32), image_shape=np.array([iw, ih], F32),
                               depths=(2.2 + rs.uniform(-0.5, 0.5, (NV, self.H, self.W))).astype(F32),
                               latent=rs.uniform(-1, 1, (NV, self.C, h, w)).astype(F32), feature_padding=F32(self.fpad),
                               freq_factor=F32(6.28), num_freqs=self.F)

    def _rays(self, rs, scene):
        NR, K = self.NR, self.K
        ctr = rs.uniform(-1, 1, (NR, 3)) * [1, 1, 0.3]
        d = rs.standard_normal((NR, 3)) * [0.3, 0.3, 1.0]
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        rays = np.concatenate([ctr - 1.5 * d, d, np.full((NR, 1), 1.0), np.full((NR, 1), 3.0)], -1).astype(F32)
        z = (1.5 + (np.arange(K) - (K - 1) / 2) * 0.05 + rs.uniform(0, 0.01, (NR, K))).astype(F32)
        for it in range(400):                                 # nudge the points that sit within the margin of a decision
            f = point_inputs_ref(scene, rays, z, coords_only=True)
            viol = np.zeros(NR * K, bool)
            for x in (f.ix, f.iy, f.dx, f.dy):
                x2 = x.numpy() * 2.0
                viol |= (np.abs(x2 - np.round(x2)) < 2.5 * DECISION_MARGIN * 2.0).any(0)
            if not viol.any():
                break
            viol = viol.reshape(NR, K)
            z[viol] += rs.uniform(0.002, 0.02, int(viol.sum())).astype(F32)
            if it % 25 == 24:
                rays[viol.any(1), :3] += (rs.standard_normal((int(viol.any(1).sum()), 3)) * 0.01).astype(F32)
        return rays, z

    def build(self):
        if hasattr(self, "scenes"):
            return self
        for attempt in range(200):       # the first seed whose scenes reach what coverage() asks of this shape
            rs = np.random.RandomState(self.seed + 1000 * attempt)
            self.scenes, self.rays, self.z = [], [], []
            for s in range(self.SB):
                sc = self._scene(rs)
                rays, z = self._rays(rs, sc)
                self.scenes.append(sc), self.rays.append(rays), self.z.append(z)
            self.rays, self.z = np.stack(self.rays), np.stack(self.z)          # [SB,NR,8], [SB,NR,K]
            if all(self.coverage_missing(sb=s) == [] for s in range(self.SB)):
                break
        else:
            raise AssertionError(f"{self.id}: no seed reaches the coverage")
        R, n = self.NV * self.P, 7 + 8 * self.F
        self.ld_in = (n + 3) // 4 * 4
        self.d_in = cotangent_in(rs, (self.SB, R, self.ld_in), self.F, 6.28)
        self.d_zlat = rs.standard_normal((self.SB, R, self.C)).astype(F32)
        self.d_far = rs.standard_normal((self.SB, self.NR)).astype(F32)
        return self

    # -- expectations ---------------------------------------------------------------------------
    def forward64(self, mode, sb=0, defect=None, grad=False):
        self.build()
        return point_inputs_ref(self.scenes[sb], self.rays[sb], self.z[sb], mode, torch.float64, 0, defect, grad)

    def refs(self, mode, sb=0, backward=True):
        """float64 expectations and the bounds of one lookup mode, computed once: namespace with in55, zlat, idx, wt, dd (numpy),
        bounds (family -> tolerance; 'zlat', 'wt'), cpu_err (the float32 side), and with backward: grads, scales, rel (leaf -> relative
        bound), cpu_rel."""
        key = (mode, sb, backward)
        if key in self._refs:
            return self._refs[key]
        self.build()
        sc, rays, z = self.scenes[sb], self.rays[sb], self.z[sb]
        NV, P, n = self.NV, self.P, 7 + 8 * self.F
        f64 = point_inputs_ref(sc, rays, z, mode, torch.float64, 0, None, backward)
        margin = decision_margin(f64)
        assert self.exact or margin >= DECISION_MARGIN, f"{self.id}: a point sits {margin:.2e} texels from a decision boundary"
        flat = lambda a: a.detach().double().numpy().reshape(NV * P, -1)
        out = SimpleNamespace(in55=flat(f64.in55), zlat=flat(f64.zlat), idx=f64.idx.numpy().reshape(NV * P, 4), wt=flat(f64.wt),
                              dd=f64.dd.numpy().reshape(NV * P, 2), margin=margin, f64=f64)
        runs = [point_inputs_ref(sc, rays, z, mode, torch.float32, V, None, backward) for V in (0, 1)]
        for f in runs:       # the float32 evaluations take the float64 decisions (the margin's purpose)
            assert torch.equal(f.idx, f64.idx) and torch.equal(f.dd, f64.dd), self.id
        cpu, bounds = {}, {}
        for name, cols in in_families(self.F).items():
            cpu[name] = max(float(np.abs(flat(f.in55)[:, cols] - out.in55[:, cols]).max()) for f in runs)
            bounds[name] = MARGIN * cpu[name] + EPS32 * float(np.abs(out.in55[:, cols]).max()) + (PE_SIN_BAR if name.startswith("code") else 0.0)
        for name, a in (("zlat", "zlat"), ("wt", "wt")):
            cpu[name] = max(float(np.abs(flat(getattr(f, a)) - getattr(out, a)).max()) for f in runs)
            bounds[name] = MARGIN * cpu[name] + EPS32 * float(np.abs(getattr(out, a)).max())
        out.cpu_err, out.bounds = cpu, bounds
        if backward:
            args = (self.d_in[sb][:, :n], self.d_zlat[sb], self.d_far[sb], self.NR, self.K, sc.depths.shape)
            out.grads, out.scales = backward_ref(f64, *args)
            g32 = [backward_ref(f, *args)[0] for f in runs]
            out.cpu_rel, out.rel = {}, {}
            for name in LEAVES:
                out.cpu_rel[name] = max(scaled_error(g[name], out.grads[name], out.scales[name]) for g in g32)
                depth = np.maximum(out.scales["depth_rows"], 1.0) if name == "depths" else reduce_depth(name, self.NR, self.K, NV)
                out.rel[name] = MARGIN * out.cpu_rel[name] + depth * U32
            # the scatter: terms |d_zlat| |w| of each latent element, float64 (the same scatter on the absolute values)
            hw = self.h * self.w
            out.lat_scale, out.lat_terms = scatter_plain(out.idx, out.wt, self.d_zlat[sb], P, NV, hw, absolute=True)
            lat32 = [scatter_plain(out.idx, flat(f.wt), self.d_zlat[sb], P, NV, hw)[0] for f in runs]
            ref_nhwc = out.grads["latent"].transpose(0, 2, 3, 1).reshape(NV, hw, self.C)
            out.lat_ref = ref_nhwc
            # The scatter runs on the kernel's own taps, whose weights the forward test holds within bounds["wt"] of the float64 ones (4 x
            # the float32 CPU side's weight error + an ulp): an ABSOLUTE error, the coordinate's, whatever the weight's size.  So the
            # CPU-side part of an element's bound is bounds["wt"] x sum |d_zlat| over its terms -- relative to sum |d_zlat| |w| a single
            # figure per family would be set by the one texel that only weights of 1e-3 reach and be 100 times too wide for the others --
            # and the floor is the summation's: n_terms x 2^-24 of sum |d_zlat| |w|.
            out.lat_absdz = scatter_plain(out.idx, out.wt, self.d_zlat[sb], P, NV, hw, absolute="dz")[0]
            out.cpu_rel["latent"] = max(scaled_error(g, ref_nhwc, out.lat_absdz) for g in lat32)            # in units of a weight
            out.lat_bound = out.bounds["wt"] * out.lat_absdz + out.lat_terms[..., None] * U32 * out.lat_scale
        self._refs[key] = out
        return out

    # -- coverage -------------------------------------------------------------------------------
    def coverage_missing(self, sb=0):
        """what this shape can reach and does not (the list the host test asserts empty): with 8 (view, ray) pairs or more a row outside every side
        of the latent map and between 0.2 and 0.7 of the rows outside map or image; with K > 1 a row that repeats the previous
        row's footprint; with NV > 1 and P no multiple of SCATTER_RUN a scatter run across a view boundary -- on the 2 x 3 map one whose
        rows on both sides share their footprint, where a missing flush would show"""
        cov, miss = self.coverage(sb=sb), []
        if self.exact:
            return miss
        if self.NR * self.NV >= 8:      # (a ray's K samples lie within a texel or two: fewer (view, ray) pairs cannot surround the map)
            miss += [s for s in ("left", "right", "above", "below") if getattr(cov, s) == 0]
            miss += ["outside share"] if not 0.2 <= cov.outside <= 0.7 else []
        if self.K > 1 and cov.repeats == 0:
            miss.append("repeats")
        if self.NV > 1 and self.P % SCATTER_RUN:
            miss += ["crossings"] if cov.crossings == 0 else []
            miss += ["merge_at_view"] if (self.h, self.w) == (2, 3) and self.P >= 15 and cov.merge_at_view == 0 else []
        return miss

    def coverage(self, mode=("bilinear", "border"), sb=0):
        """what the rows of a scene reach: sides of the latent map left / right / above / below with a row outside, rows repeating the
        previous row's four indices (in the same view), scatter runs that cross a view boundary (merge_at_view: with the same four
        indices on both sides), share of rows outside map or image"""
        f = point_inputs_ref(self.scenes[sb], self.rays[sb], self.z[sb], mode)
        ix, iy, dx, dy = (a.numpy() for a in (f.ix, f.iy, f.dx, f.dy))
        idx = f.idx.numpy()
        rep = int((idx[:, 1:] == idx[:, :-1]).all(-1).sum())
        cross = sum(1 for v in range(1, self.NV) if (v * self.P) % SCATTER_RUN)
        merge = sum(1 for v in range(1, self.NV) if (v * self.P) % SCATTER_RUN and np.array_equal(idx[v, 0], idx[v - 1, -1]))
        outside = (ix < 0) | (ix > self.w - 1) | (iy < 0) | (iy > self.h - 1) | (dx < 0) | (dx > self.W - 1) | (dy < 0) | (dy > self.H - 1)
        return SimpleNamespace(left=int((ix < 0).sum()), right=int((ix > self.w - 1).sum()), above=int((iy < 0).sum()),
                               below=int((iy > self.h - 1).sum()), repeats=rep, crossings=cross, merge_at_view=merge,
                               outside=float(outside.mean()))


# the grid: every value of every quantity, each pair of map size and feature_padding, both NV with every (NR, K).  A 2 x 3 map with
# feature_padding 1 is degenerate (its y scale (h - 2) / h is 0: every row sits at iy = 0.5 exactly, a tie of the nearest lookup's rint),
# so the small map takes 0.5 where the large one takes 1.
TRAIN_STAGE_CASES = [
    TrainStageCase((2, 3), 0, 1, 1, 1), TrainStageCase((2, 3), 0.5, 3, 3, 5), TrainStageCase((2, 3), 0, 3, 13, 5),
    TrainStageCase((2, 3), 0.5, 1, 4, 16), TrainStageCase((5, 7), 1, 1, 3, 5), TrainStageCase((5, 7), 0, 3, 1, 1),
    TrainStageCase((5, 7), 1, 3, 13, 5), TrainStageCase((5, 7), 0, 3, 4, 16),
]
GEN_SHAPES = [(1, 8), (6, 72), (6, 512)]                                                     # (num_freqs, C) of the _gen entries
GEN_CASES = [TrainStageCase((2, 3), 0.5, 3, 13, 5, C=8, F=1), TrainStageCase((5, 7), 1, 3, 13, 5, C=72, F=6),
             TRAIN_STAGE_CASES[7]]
SB2_CASE = TrainStageCase((5, 7), 1, 3, 13, 5, SB=2)
SCATTER_CONTENTION = TrainStageCase((2, 3), 0, 3, 257, 16, C=72)                             # thousands of rows on six texels
SCATTER_ONE = TrainStageCase((2, 3), 0, 1, 1, 1, C=8)
# the three sizes of the fixed-order camera reduction: one partial, a ragged last chunk, the CAMG_BLOCKS cap
REDUCE_CASES = [TrainStageCase((5, 7), 0, 2, 9, 13, C=8, F=1), TrainStageCase((5, 7), 0, 2, 99, 13, C=8, F=1),
                TrainStageCase((5, 7), 0, 2, 16459, 4, C=8, F=1)]


class BoundaryCase(TrainStageCase):
    """Rows exactly ON the decision boundaries, built like ``Stage`` of tests/test_gpu_bicubic.py: identity cameras, depth 1, focal 1,
    image_shape 2, dyadic ray origins and principal points, a 4 x 8 latent map and an 8 x 16 depth map (powers of two: every step of the
    chain is exact in float32 and in float64, so the restatement starts from the kernel's own coordinate and no margin is needed).
    Latent ix in {-1, -0.5, 0, 0.5, 1, 2.5, 3, w - 1, w - 0.5, w + 1} and the same in y, shifted by whole texels in views 1 and 2; there
    the depth-map coordinate 2 ix + 0.5 is a half-integer wherever ix is an integer (round half to even)."""
    exact = True
    H, W = 8, 16
    image_shape = (2.0, 2.0)

    def __init__(self, NV=3, C=8, F=1):
        super().__init__((4, 8), 0, NV, 100, 1, C=C, F=F)
        self.id = "boundary-" + self.id

    def build(self):
        if hasattr(self, "scenes"):
            return self
        NV, h, w = self.NV, self.h, self.w
        xs = np.array([-1.0, 0.0, 0.5, 1.0, 2.5, w - 1.0, w - 0.5, w + 1.0, -0.5, 3.0])
        ys = np.array([-1.0, 0.0, 0.5, 1.0, 1.5, h - 1.0, h - 0.5, h + 1.0, -0.5, 2.0])
        gx, gy = np.meshgrid(xs, ys)
        ix, iy = gx.reshape(-1), gy.reshape(-1)
        rs = np.random.RandomState(self.seed)
        rays = np.zeros((self.NR, 8), F32)
        rays[:, 0], rays[:, 1] = (2 * ix + 1) / w - 1.0, (2 * iy + 1) / h - 1.0              # u = (x + c) / 2 * 2 - 1 with c = 1
        rays[:, 5], rays[:, 7] = 1.0, 2.0
        c = np.array([[1.0, 1.0], [1.25, 0.5], [0.75, 1.5]], F32)[:NV]                        # views 1, 2: one texel right / up, left / down
        sc = SimpleNamespace(poses=np.tile(np.eye(4, dtype=F32), (NV, 1, 1)), focal=np.ones((NV, 2), F32), c=c,
                             image_shape=np.array(self.image_shape, F32), depths=np.ones((NV, self.H, self.W), F32),
                             latent=rs.uniform(-1, 1, (NV, self.C, h, w)).astype(F32), feature_padding=F32(0.0), freq_factor=F32(1.0),
                             num_freqs=self.F)
        self.scenes, self.rays, self.z = [sc], rays[None], np.ones((1, self.NR, 1), F32)
        R = NV * self.P
        self.ld_in = (7 + 8 * self.F + 3) // 4 * 4
        self.d_in = cotangent_in(rs, (1, R, self.ld_in), self.F, 1.0)
        self.d_zlat = rs.standard_normal((1, R, self.C)).astype(F32)
        self.d_far = rs.standard_normal((1, self.NR)).astype(F32)
        return self


BOUNDARY_CASES = [BoundaryCase(3, 8, 1), BoundaryCase(2, 512, 6)]
