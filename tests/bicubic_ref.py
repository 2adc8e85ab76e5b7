"""Torch restatement of the bicubic latent lookup (grid_sample(mode="bicubic", align_corners=False) as ATen evaluates it; the semantics of
include/diner_hip.h, "the bicubic latent lookup") and of both its gradients, written out tap by tap so that the HIP kernels can be checked
stage by stage against it.  tests/test_bicubic_host.py proves it against torch's own F.grid_sample forward and autograd.

Coordinates are normalised (grid_sample's grid, after the feature_padding rescale).  ``coord_dtype=torch.float32`` evaluates the centre
coordinate in the kernels' fp32 operation order (one fma: (u + 1) * size / 2 - 0.5) and the weights in ATen's own float32 operations
(one rounding per operation of get_cubic_upsample_coefficients), then the sums in float64.  That is what a float32 grid_sample
defines and what the kernels follow operation for operation: the Horner form of the outer weight adds terms of magnitude up to 12 to a
result near 0, so its float32 value is up to 1.1e-6 away from the exact polynomial (measured over 2e5 fractions; 1.4e-6 summed over an
axis), and a coordinate of magnitude ~10 rounds by 1e-6 texel.  Neither rounding belongs to a kernel's error."""
import torch

A = -0.75
PADDINGS = ("border", "zeros", "reflection")


def centre(u, size, coord_dtype=torch.float64):
    """ix = ((u + 1) * size - 1) / 2, not clipped, not reflected"""
    if coord_dtype == torch.float32:
        up1 = (u.to(torch.float32) + 1.0).to(torch.float64)
        return (up1 * (size / 2.0) - 0.5).to(torch.float32).to(torch.float64)    # the product of two floats is exact in double: an fma
    return (u.to(torch.float64) + 1.0) * (size / 2.0) - 0.5


def clamped_centre(u, size, coord_dtype=torch.float64):
    """the deliberately WRONG variant: the centre clipped to [0, size - 1] as the bilinear / border lookup does"""
    return centre(u, size, coord_dtype).clamp(0, size - 1)


def weights(t, dtype=torch.float64):
    """cubic-convolution weights at distances t + 1, t, 1 - t, 2 - t and their derivatives in t: [..., 4] each (float64).  ``dtype``
    float32: the weights (not the derivatives) evaluated in float32, operation by operation as ATen does"""
    inner = lambda d: ((A + 2) * d - (A + 3)) * d * d + 1
    outer = lambda d: ((A * d - 5 * A) * d + 8 * A) * d - 4 * A
    if dtype == torch.float32:
        tf = t.to(torch.float32)
        c32 = torch.stack([outer(tf + 1), inner(tf), inner(1 - tf), outer((1 - tf) + 1)], -1)
        assert c32.dtype == torch.float32
        return c32.to(torch.float64), weights(t)[1]
    d_inner = lambda d: (3 * (A + 2) * d - 2 * (A + 3)) * d
    d_outer = lambda d: (3 * A * d - 10 * A) * d + 8 * A
    c = torch.stack([outer(t + 1), inner(t), inner(1 - t), outer(2 - t)], -1)
    dc = torch.stack([d_outer(t + 1), d_inner(t), -d_inner(1 - t), -d_outer(2 - t)], -1)
    return c, dc


def reflect(p, size):
    """ATen's reflect_coordinates over [-0.5, size - 0.5]"""
    a = (p + 0.5).abs()
    extra = torch.fmod(a, float(size))
    flips = torch.floor(a / size)
    return torch.where(flips % 2 == 0, extra - 0.5, size - extra - 0.5)


def axis(ic, size, padding, dtype=torch.float64):
    """taps of one axis for centre coordinates ``ic``: indices [..., 4] (long, inside the map), weights and derivatives [..., 4]; each
    integer tap position goes through the padding on its own; zeros: weight and derivative 0 outside the map"""
    c0 = torch.floor(ic)
    c, dc = weights(ic - c0, dtype)
    p = c0.unsqueeze(-1) + torch.arange(-1, 3, dtype=ic.dtype)
    inside = (p >= 0) & (p <= size - 1)
    if padding == "reflection":
        p = reflect(p, size)
    idx = p.clamp(0, size - 1).long()
    if padding == "zeros":
        c, dc = c * inside, dc * inside
    return idx, c, dc, inside


def footprint(u, v, h, w, padding, coord_dtype=torch.float64, centre_fn=centre):
    xi, cx, dcx, inx = axis(centre_fn(u, w, coord_dtype), w, padding, coord_dtype)
    yi, cy, dcy, iny = axis(centre_fn(v, h, coord_dtype), h, padding, coord_dtype)
    return xi, yi, cx, cy, dcx, dcy, inx, iny


def lookup(latent, u, v, padding, coord_dtype=torch.float64, centre_fn=centre):
    """latent [C, h, w], u / v [N] -> [N, C] = sum_j cy_j (sum_i cx_i texel_ij) in float64"""
    C, h, w = latent.shape
    xi, yi, cx, cy, *_ = footprint(u, v, h, w, padding, coord_dtype, centre_fn)
    lat = latent.to(torch.float64)
    tex = lat[:, yi[:, :, None], xi[:, None, :]]                       # [C, N, 4 (j), 4 (i)]
    return torch.einsum("cnji,ni,nj->nc", tex, cx, cy)


def lookup_grads(latent, u, v, g, padding, coord_dtype=torch.float64, centre_fn=centre):
    """gradients of <g, lookup>: (d_latent [C, h, w], d_u [N], d_v [N]).  The grid gradient is the weights' derivative times size / 2;
    the padding puts no factor on it."""
    C, h, w = latent.shape
    xi, yi, cx, cy, dcx, dcy, *_ = footprint(u, v, h, w, padding, coord_dtype, centre_fn)
    lat, g = latent.to(torch.float64), g.to(torch.float64)
    tex = lat[:, yi[:, :, None], xi[:, None, :]]
    gt = torch.einsum("nc,cnji->nji", g, tex)
    d_u = torch.einsum("nji,ni,nj->n", gt, dcx, cy) * (w / 2.0)
    d_v = torch.einsum("nji,ni,nj->n", gt, cx, dcy) * (h / 2.0)
    wt = cy[:, :, None] * cx[:, None, :]                                # [N, 4, 4]
    flat = (yi[:, :, None] * w + xi[:, None, :]).reshape(-1)
    d_lat = torch.zeros(C, h * w, dtype=torch.float64)
    d_lat.index_add_(1, flat, (g.t()[:, :, None, None] * wt[None]).reshape(C, -1))
    return d_lat.view(C, h, w), d_u, d_v


def footprint_stats(u, v, h, w):
    """(straddle_frac, inside_frac) of lookups at normalised coordinates u, v: the share whose 4 x 4 footprint has some but not all taps
    in the map, and the share with all 16 inside"""
    *_, inx, iny = footprint(u.reshape(-1), v.reshape(-1), h, w, "zeros")
    n_in = inx.sum(-1) * iny.sum(-1)
    return float(((n_in > 0) & (n_in < 16)).double().mean()), float((n_in == 16).double().mean())
