"""Plain restatements of the stages around the point/MLP kernel, the case sets and the comparison functions that
tests/test_stage_refs_host.py (CPU) and tests/test_gpu_stage_kernels.py (GPU) share.

* ``select_from_likelihood``: the decisions of sample_depthguided given a likelihood array (oracle/diner_oracle.c:206-246).
* ``fill_up_f32``: fill_up_uniform_samples (oracle/diner_oracle.c:258-280), numpy float32.
* ``composite_ref``: the reference's compositing formula in torch (float64 or float32), differentiable by autograd.
* ``composite_f32`` / ``composite_backward_f32``: the same formula hand-written in float32 with a sequential sweep and a correctly
  rounded exp (another summation order and another exp than torch's), the second independent float32 evaluation of the tolerances.
* ``gen_rays64`` / ``depth2normal64``: float64 forms of synthetic/synth.py's restatements (which cast to float32 throughout).

Every float32 restatement takes ``defect=<name>``: a deliberately wrong variant.  The CPU tests assert that the comparison functions
below reject each of them, so that a comparison which the GPU passes is known to be able to fail.

Tolerances.  A bound is ``MARGIN`` x the error an independent float32 CPU evaluation makes on the same inputs (against float64) plus a
floor equal to the existing stage bars; it is computed from CPU values only.
"""
from __future__ import annotations

import copy
import zlib

import numpy as np
import torch

from synthetic import synth

F32 = np.float32
MARGIN = 4.0
FLOOR_W, FLOOR_RGB, FLOOR_DEPTH = 1e-6, 2e-6, 2e-6     # tests/test_gpu_parity.py::test_composite
FLOOR_GAUSS = 2e-6                                     # a gaussian sample is a depth
FLOOR_GRAD = 2e-6                                      # of the element's own scale (see grad_scale)
TINY = 1e-30   # absolute floor of a gradient's scale: below ~1e-31 float32 products are denormal and carry no relative precision
LIK_ATOL, LIK_FLIP_SHARE = 1.2e-7, 2e-3                # tests/test_gpu_parity.py::test_likelihood_and_shortlist

SAMPLER_DEFECTS = ("tie_high", "keep_zero", "ignore_hit")
FILL_DEFECTS = ("no_neg_offset",)
FWD_DEFECTS = ("no_carry", "last_delta_z", "no_eps")
BWD_DEFECTS = ("no_carry", "last_delta_z", "no_eps", "no_white_grad", "s_before", "relu_ge")


# ------------------------------------------------------------------------------------------------
# sampler decisions
# ------------------------------------------------------------------------------------------------
def select_from_likelihood(L, z_cand, K, G, n_gauss, defect=None):
    """One ray: likelihood L [NC] (float32), candidates z_cand [NC], n_gauss [G] -> (z_dg [K] float64, hit).
    Slots 0..K-G-1: the K-G most likely candidates (ties to the lower index, a zero likelihood never kept, empty = 0);
    slots K-G..K-1: n * std + mean of the occlusion-aware likelihood O_j = L_j prod_{i<j}(1 - L_i), moments in float64; 0 if no hit."""
    L = np.asarray(L, F32)
    z = np.asarray(z_cand, F32)
    NC, keep = L.size, K - G
    # hit as float32 decides it (an underflow of the running product is a decision, not a rounding)
    cp32 = np.cumprod(np.concatenate([[1.0], 1.0 - L[:-1]]).astype(F32), dtype=F32)
    hit = bool(((L * cp32) != 0).any())
    out = np.zeros(K, np.float64)
    idx = np.arange(NC)
    order = np.lexsort((-idx if defect == "tie_high" else idx, -L.astype(np.float64)))[:keep]
    sel = order if defect == "keep_zero" else order[L[order] > 0]
    out[:sel.size] = z[sel]
    if G > 0 and (hit or defect == "ignore_hit"):
        L64, z64 = L.astype(np.float64), z.astype(np.float64)
        O = L64 * np.cumprod(np.concatenate([[1.0], 1.0 - L64[:-1]]))
        wsum = O.sum()
        if wsum > 0:
            mean = (z64 * O).sum() / wsum
            std = np.sqrt((((z64 - mean) ** 2) * O).sum() / wsum)
        else:
            mean, std = z64.mean(), z64.std()
        out[keep:] = np.asarray(n_gauss, np.float64)[:G] * std + mean
    return out, hit


def select_rows(L, z_cand, K, G, n_gauss, defect=None):
    """select_from_likelihood on every ray: -> (z_dg [NR,K] float64, hit [NR])"""
    NR = L.shape[0]
    ng = n_gauss if G > 0 else np.zeros((NR, 0))
    rows = [select_from_likelihood(L[r], z_cand[r], K, G, ng[r], defect) for r in range(NR)]
    return np.stack([z for z, _ in rows]), np.array([h for _, h in rows])


def gauss_bound(oracle_z_dg, ref_z_dg, K, G):
    """MARGIN x the float32 oracle's error on the gaussian slots (against the float64 moments on the oracle's own likelihood) + floor"""
    err = float(np.abs(oracle_z_dg[:, K - G:] - ref_z_dg[:, K - G:]).max(initial=0.0))
    return MARGIN * err + FLOOR_GAUSS, err


def compare_decisions(z_dg, ref_z_dg, ref_hit, K, G, gauss_tol):
    """z_dg [NR,K] of the code under test against select_rows of ITS OWN likelihood.  Every ray, no filter.  -> list of findings."""
    bad = []
    keep = K - G
    a = np.sort(np.asarray(z_dg, F32)[:, :keep], -1)
    b = np.sort(ref_z_dg[:, :keep].astype(F32), -1)
    rows = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(-1))[0]
    if rows.size:
        bad.append(f"short-list differs on {rows.size} rays (first {rows[:5].tolist()})")
    hit = (np.asarray(z_dg) != 0).any(-1)
    if not np.array_equal(hit, ref_hit):
        bad.append(f"hit / no-hit differs on {(hit != ref_hit).sum()} rays")
    if G > 0:
        d = np.abs(np.asarray(z_dg, np.float64)[:, keep:] - ref_z_dg[:, keep:])
        if not (d <= gauss_tol).all():      # (NaN fails)
            bad.append(f"gaussian slots: max error {np.nanmax(d):.3e} > {gauss_tol:.3e}")
    return bad


def gauss_error(z_dg, ref_z_dg, K, G):
    return float(np.abs(np.asarray(z_dg, np.float64)[:, K - G:] - ref_z_dg[:, K - G:]).max(initial=0.0))


def compare_likelihood(L, ref):
    """the bar of test_likelihood_and_shortlist: atol 1.2e-7; zero / non-zero flips only where both are <= 1.2e-7, share <= 2e-3"""
    bad = []
    d = np.abs(L.astype(np.float64) - ref)
    if not (d <= LIK_ATOL).all():
        bad.append(f"likelihood: max error {np.nanmax(d):.3e}")
    flips = (L == 0) != (ref == 0)
    if flips.mean() > LIK_FLIP_SHARE:
        bad.append(f"likelihood: {flips.mean():.2e} of the values flip between zero and non-zero")
    if flips.any() and max(L[flips].max(), ref[flips].max()) > LIK_ATOL:
        bad.append("likelihood: a value above 1.2e-7 flips to zero")
    return bad


def fill_up_f32(z_dg, rays, u_fill, defect=None):
    """fill_up_uniform_samples: sort, the i-th of the m zeros (sorted column k = n_neg + i) becomes near + k step + u_i step, sort."""
    z = np.sort(np.asarray(z_dg, F32), -1)
    out = z.copy()
    for r in range(z.shape[0]):
        near, far = F32(rays[r, 6]), F32(rays[r, 7])
        cols = np.nonzero(z[r] == 0)[0]
        if cols.size == 0:
            continue
        step = F32(far - near) / F32(cols.size)
        pos = np.arange(cols.size) if defect == "no_neg_offset" else cols
        zm = near + pos.astype(F32) * step
        out[r, cols] = zm + np.asarray(u_fill[r, :cols.size], F32) * step
    return np.sort(out, -1)


# ------------------------------------------------------------------------------------------------
# sampler cases
# ------------------------------------------------------------------------------------------------
class SamplerCase:
    """A seeded scene + rays + noise.  ``special``: one of the dedicated cases (see build)."""

    def __init__(self, NC, K, G, NV=2, HW=(24, 24), SB=1, special=None):
        self.NC, self.K, self.G, self.NV, self.HW, self.SB, self.special = NC, K, G, NV, HW, SB, special
        self.id = f"NC{NC}-K{K}-G{G}-NV{NV}-{HW[1]}x{HW[0]}" + (f"-SB{SB}" if SB > 1 else "") + (f"-{special}" if special else "")
        self.seed = zlib.crc32(self.id.encode()) % 100000

    def build(self):
        if hasattr(self, "rays"):
            return self
        H, W = self.HW
        NC, K, G = self.NC, self.K, self.G
        self.scenes = [synth.make_scene(H, W, self.NV, seed=self.seed + 7 * s, with_latent=False, bg_sigma_zero=(s == 1)) for s in range(self.SB)]
        sc = self.scenes[0]
        stride = 2 if H * W <= 800 else 3
        rays = np.concatenate([s.target_rays()[:, (i % stride)::stride] for i, s in enumerate(self.scenes)], 0)   # [SB,NR,8]
        NR = rays.shape[1]
        rs = np.random.RandomState(self.seed)
        if NC <= 2:
            # one or two candidates per ray: [near, far] narrowed to the front of the sphere so that enough of them land within
            # depth_diff_max of the surface
            rays[..., 6], rays[..., 7] = 1.27, 1.45
        if self.special == "near_eq_far":
            rays[:, ::4, 7] = rays[:, ::4, 6]
        if self.special == "miss_all":                       # a wide field of view: most rays leave the source images
            rays = np.concatenate([s.target_rays(focal_scale=0.6)[:, (i % stride)::stride] for i, s in enumerate(self.scenes)], 0)
        self.rays = np.ascontiguousarray(rays, F32)
        assert NR <= 400
        noise = [synth.make_noise(NR, NC, G, K, seed=self.seed + 1 + s) for s in range(self.SB)]
        self.u_coarse, self.n_gauss, self.u_fill = [np.stack([n[i] for n in noise]) for i in range(3)]
        if self.special == "gauss_negative":                 # the n_neg path of the fill-up: samples in front of the camera
            self.n_gauss = (-300.0 - 3000.0 * np.abs(self.n_gauss)).astype(F32)
            self.n_gauss[:, 1::2, : max(1, G // 2)] *= F32(-1e-5)   # ... mixed with ordinary ones
        if self.special == "gauss_beyond_far":
            self.n_gauss = (300.0 + 3000.0 * np.abs(self.n_gauss)).astype(F32)
        self.z_cand_inject = None
        if self.special == "ties":
            # [near, far] so wide that erf saturates: every candidate within the depth mask has likelihood exactly 1.0f; candidates
            # 0.011 apart in front of the surface, so ~9 distinct z tie at the cut (K - G = 4); every fifth value repeated
            self.rays[..., 6], self.rays[..., 7] = 0.5, 12.5
            base = np.linspace(1.2, 1.9, NC).astype(F32)
            base[4::5] = base[3::5][: base[4::5].size]
            self.z_cand_inject = np.ascontiguousarray(np.broadcast_to(base, (self.SB, NR, NC)))
        return self

    def oracle(self):
        """CPU expectations, computed once: z_cand, likelihood, z_dg of the oracle, its hit flags"""
        if hasattr(self, "orc_L"):
            return self
        from oracle.oracle import Oracle
        self.build()
        self.z_cand, self.orc_L, self.orc_z_dg = [], [], []
        for s, sc in enumerate(self.scenes):
            one = copy.copy(sc)
            orc = Oracle(one, None)
            zc = orc.sample_coarse(self.rays[s], self.NC, self.u_coarse[s]) if self.z_cand_inject is None else self.z_cand_inject[s]
            z, L = orc.sample_depthguided(self.rays[s], zc, self.K, self.G, self.n_gauss[s], want_L=True)
            self.z_cand.append(zc), self.orc_L.append(L), self.orc_z_dg.append(z)
        self.z_cand, self.orc_L, self.orc_z_dg = np.stack(self.z_cand), np.stack(self.orc_L), np.stack(self.orc_z_dg)
        self.surface = (self.orc_L > 0).any(-1)
        return self

    def batched_scene(self):
        sc = copy.copy(self.scenes[0])
        for name in ("poses", "focal", "c", "depths", "depths_std", "normals"):
            setattr(sc, name, np.concatenate([getattr(s, name) for s in self.scenes], 0))
        return sc


# NC x K x G x NV paired, not the full product: every CPL variant (NC <= 256 / 1024 / 2048 / 4096) on both sides of its boundary,
# with a small K, K = 64 +- 1 and a large K; G in {0, 1, middle, K}; K <= NC (the reference's topk needs it)
SAMPLER_GRID = [SamplerCase(*a, **k) for a, k in [
    ((1, 1, 0), dict(NV=1)), ((1, 1, 1), dict(NV=2)), ((2, 1, 0), dict(NV=2)), ((2, 2, 1), dict(NV=1)),
    ((63, 8, 0), {}), ((63, 40, 15), dict(NV=8)), ((64, 63, 1), {}), ((64, 64, 64), dict(NV=1)),
    ((65, 65, 20), {}), ((65, 8, 8), {}), ((256, 100, 30), dict(HW=(28, 40))), ((256, 256, 1), dict(NV=8)), ((256, 129, 0), {}),
    ((257, 8, 1), {}), ((257, 64, 20), dict(NV=1)), ((257, 128, 48), {}),
    ((1024, 63, 0), {}), ((1024, 65, 65), {}), ((1024, 300, 100), dict(NV=1)), ((1024, 128, 48), dict(SB=2, NV=3)),
    ((1025, 1, 0), {}), ((1025, 64, 1), {}), ((1025, 256, 80), dict(NV=1)),
    ((2048, 40, 15), {}), ((2048, 63, 63), {}), ((2048, 300, 0), dict(NV=1)), ((2048, 1500, 500), dict(NV=1)),
    ((2049, 8, 3), {}), ((2049, 65, 1), {}), ((2049, 129, 40), dict(NV=1)),
    ((4096, 100, 100), dict(NV=1)), ((4096, 64, 20), {}), ((4096, 128, 48), dict(NV=8, HW=(28, 40))), ((4096, 2000, 700), dict(NV=1)),
]]
SAMPLER_SPECIAL = [
    SamplerCase(256, 40, 15, special="gauss_negative"), SamplerCase(1024, 256, 30, special="gauss_negative"),
    SamplerCase(256, 40, 15, special="gauss_beyond_far"), SamplerCase(64, 8, 4, special="ties"),
    SamplerCase(256, 40, 15, HW=(28, 40), special="miss_all"), SamplerCase(257, 64, 20, special="near_eq_far"),
]
SAMPLER_CASES = SAMPLER_GRID + SAMPLER_SPECIAL
PHILOX_NC = (64, 1024, 2048, 4096)     # one per CPL variant


# ------------------------------------------------------------------------------------------------
# compositing
# ------------------------------------------------------------------------------------------------
def composite_ref(rays, z, rgbsigma, white, dtype=torch.float64):
    """The reference's compositing (src/models/nerf_renderer.py:299-301, 341-360) on torch tensors [N,8], [N,K], [N,K,4]
    -> (weights, rgb, depth).  ``rays`` / ``rgbsigma`` may require grad (far = rays[:, 7])."""
    rays, z, c = rays.to(dtype), z.to(dtype), rgbsigma.to(dtype)
    deltas = torch.cat([z[..., 1:] - z[..., :-1], rays[..., -1:] - z[..., -1:]], -1)
    alphas = 1 - torch.exp(-deltas * torch.relu(c[..., 3]))
    shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-10], -1)
    T = torch.cumprod(shifted, -1)
    weights = alphas * T[..., :-1]
    rgb = torch.sum(weights.unsqueeze(-1) * c[..., :3], -2)
    depth = torch.sum(weights * z, -1)
    if white:
        rgb = rgb + 1 - weights.sum(-1).unsqueeze(-1)
    return weights, rgb, depth


def composite_ref_grads(rays, z, rgbsigma, white, d_rgb, d_depth, d_weights, dtype):
    """autograd of composite_ref: -> (weights, rgb, depth, d_rgbsigma [N,K,4], d_far [N]) as float64 numpy"""
    r = torch.from_numpy(rays).to(dtype).requires_grad_(True)
    c = torch.from_numpy(rgbsigma).to(dtype).requires_grad_(True)
    w, rgb, depth = composite_ref(r, torch.from_numpy(z), c, white, dtype)
    loss = (rgb * torch.from_numpy(d_rgb).to(dtype)).sum()
    if d_depth is not None:
        loss = loss + (depth * torch.from_numpy(d_depth).to(dtype)).sum()
    if d_weights is not None:
        loss = loss + (w * torch.from_numpy(d_weights).to(dtype)).sum()
    gc, gr = torch.autograd.grad(loss, [c, r])
    n = lambda t: t.detach().to(torch.float64).numpy()
    return n(w), n(rgb), n(depth), n(gc), n(gr[:, 7])


def _exp32(x):
    with np.errstate(over="ignore"):
        return np.exp(x.astype(np.float64)).astype(F32)     # correctly rounded: not the exp of torch or of the kernels


def _alpha_keep(rays, z, rgbsigma, defect, ge=False):
    far = rays[:, 7:8].astype(F32)
    last = z[:, -1:] if defect == "last_delta_z" else far
    delta = np.concatenate([z[:, 1:] - z[:, :-1], last - z[:, -1:]], -1).astype(F32)
    sraw = rgbsigma[..., 3].astype(F32)
    sg = np.where(sraw > 0, sraw, F32(0))
    e = _exp32(-delta * sg)
    alpha = F32(1) - e
    keep = (F32(1) - alpha) + (F32(0) if defect == "no_eps" else F32(1e-10))
    return delta, sraw, sg, e, alpha, keep


def composite_f32(rays, z, rgbsigma, white, defect=None):
    """float32, sample after sample (numpy arrays [N,8], [N,K], [N,K,4]) -> (weights, rgb, depth, T)"""
    rays, z, c = np.asarray(rays, F32), np.asarray(z, F32), np.asarray(rgbsigma, F32)
    N, K = z.shape
    _, _, _, _, alpha, keep = _alpha_keep(rays, z, c, defect)
    T = np.empty((N, K), F32)
    t = np.ones(N, F32)
    for k in range(K):
        if defect == "no_carry" and k % 64 == 0:
            t = np.ones(N, F32)
        T[:, k] = t
        t = t * keep[:, k]
    w = alpha * T
    rgb, depth, acc = np.zeros((N, 3), F32), np.zeros(N, F32), np.zeros(N, F32)
    for k in range(K):
        rgb += w[:, k, None] * c[:, k, :3]
        depth += w[:, k] * z[:, k]
        acc += w[:, k]
    if white:
        rgb = rgb + F32(1) - acc[:, None]
    return w, rgb, depth, T


def composite_backward_f32(rays, z, rgbsigma, white, d_rgb, d_depth, d_weights, defect=None):
    """the hand-written reverse sweep in float32 -> (d_rgbsigma [N,K,4], d_far [N])"""
    rays, z, c = np.asarray(rays, F32), np.asarray(z, F32), np.asarray(rgbsigma, F32)
    N, K = z.shape
    delta, sraw, sg, e, alpha, keep = _alpha_keep(rays, z, c, defect)
    w, _, _, T = composite_f32(rays, z, c, white, defect)
    g = np.asarray(d_rgb, F32)
    gd = np.zeros(N, F32) if d_depth is None else np.asarray(d_depth, F32)
    gwhite = g.sum(-1).astype(F32) if (white and defect != "no_white_grad") else np.zeros(N, F32)
    out, d_far = np.zeros((N, K, 4), F32), np.zeros(N, F32)
    S = np.zeros(N, F32)
    gate = (sraw >= 0) if defect == "relu_ge" else (sraw > 0)
    with np.errstate(all="ignore"):
        for k in range(K - 1, -1, -1):
            dLdw = (c[:, k, :3] * g).sum(-1).astype(F32) + gd * z[:, k] - gwhite + (F32(0) if d_weights is None else np.asarray(d_weights, F32)[:, k])
            if defect == "s_before":
                S = S + dLdw * w[:, k]
            dLda = dLdw * T[:, k] - S / keep[:, k]
            out[:, k, :3] = g * w[:, k, None]
            out[:, k, 3] = np.where(gate[:, k], dLda * delta[:, k] * e[:, k], F32(0))
            if k == K - 1:
                d_far = np.where(gate[:, k], dLda * sg[:, k] * e[:, k], F32(0)).astype(F32)
            if defect != "s_before":
                S = S + dLdw * w[:, k]
    return out, d_far


def grad_scale(rays, z, rgbsigma, white, d_rgb, d_depth, d_weights):
    """Per-element scale of the sigma gradient and of d_far, in float64: (|dL/dw| T + |S| / keep) delta e with S_k = sum_{j>k} |dL/dw_j| w_j
    and the sum of absolute values in dL/dw (what the terms of the gradient add up from before they cancel): every float32 evaluation
    order errs by a few ulp of this, wherever the gradient itself happens to cancel.  -> (scale_sigma [N,K], scale_far [N])"""
    rays, z, c = [np.asarray(a, np.float64) for a in (rays, z, rgbsigma)]
    delta = np.concatenate([z[:, 1:] - z[:, :-1], rays[:, 7:8] - z[:, -1:]], -1)
    sg = np.maximum(c[..., 3], 0)
    e = np.exp(-delta * sg)
    alpha = 1 - e
    keep = 1 - alpha + 1e-10
    T = np.cumprod(np.concatenate([np.ones_like(keep[:, :1]), keep[:, :-1]], -1), -1)
    g = np.abs(np.asarray(d_rgb, np.float64))
    a = (c[..., :3] * g[:, None]).sum(-1) + (0 if d_depth is None else np.abs(d_depth)[:, None] * np.abs(z))
    a = a + (g.sum(-1)[:, None] if white else 0) + (0 if d_weights is None else np.abs(d_weights))
    aw = a * np.abs(alpha) * T
    S = np.concatenate([np.cumsum(aw[:, ::-1], -1)[:, ::-1][:, 1:], np.zeros_like(aw[:, :1])], -1)
    base = a * T + S / keep
    return base * np.abs(delta) * e, base[:, -1] * sg[:, -1] * e[:, -1]


class CompositeCase:
    """Seeded inputs of one compositing case.  sigma families: moderate, zero, negative (mixed in, exact zeros among them), opaque_one
    (one sample with delta sigma >= 40 per ray: early, middle, last in turn), opaque_all.  z families: uniform, repeated, last_eq_far,
    last_beyond_far.  cot: which cotangents the backward gets (rgb | rgb+depth | rgb+depth+weights)."""

    def __init__(self, K, N, white, sigma, zfam, cot, want_weights=True):
        self.K, self.N, self.white, self.sigma, self.zfam, self.cot, self.want_weights = K, N, white, sigma, zfam, cot, want_weights
        self.id = f"K{K}-N{N}-{'white' if white else 'black'}-{sigma}-{zfam}-{cot}" + ("" if want_weights else "-noweights")

    def build(self):
        if hasattr(self, "z"):
            return self
        K, N = self.K, self.N
        rs = np.random.RandomState(zlib.crc32(self.id.encode()) % 100000)
        near, far = 1.0, 2.5
        z = np.sort(near + (far - near) * 0.98 * rs.random_sample((N, K)), -1).astype(F32)
        if self.zfam == "repeated" and K > 1:
            z[:, 1::3] = z[:, 0::3][:, : z[:, 1::3].shape[1]]
        rays = np.zeros((N, 8), F32)
        rays[:, :3], rays[:, 5], rays[:, 6], rays[:, 7] = rs.standard_normal((N, 3)), 1.0, near, far
        if self.zfam == "last_eq_far":
            z[:, -1] = rays[:, 7]
        if self.zfam == "last_beyond_far":
            rays[:, 7] = z[:, -1] - F32(0.03) * rs.random_sample(N).astype(F32) - F32(1e-3)
        c = rs.random_sample((N, K, 4)).astype(F32)
        delta = np.concatenate([z[:, 1:] - z[:, :-1], rays[:, 7:8] - z[:, -1:]], -1).astype(np.float64)
        sig = rs.random_sample((N, K)) * 6.0 / (far - near)          # optical depth ~3 along the ray: the transmittance is still there at the last sample
        sig = np.minimum(sig, 4.0 / np.maximum(np.abs(delta), 1e-30))   # and <= 4 everywhere: well inside the regular regime
        if self.sigma == "zero":
            sig[:] = 0
        if self.sigma == "negative":
            m = (np.arange(N)[:, None] * (K + 1) + np.arange(K)[None]) % 5
            sig = np.where(m == 0, -sig - 0.5, np.where(m == 1, 0.0, sig))
        if self.sigma.startswith("opaque"):
            # opaque = delta sigma in [40, 200]: 1 - exp(-x) is exactly 1.0f under every exp, so float32 keep is exactly 1e-10; nothing lies
            # between 4 and 40, where the rounding of alpha to 2^-24 would decide keep's leading digits
            x = 40.0 + 160.0 * rs.random_sample((N, K))
            pos = delta > 1e-4
            if self.sigma == "opaque_all":
                sig = np.where(pos, x / np.where(pos, delta, 1), sig)
            else:
                for r in range(N):
                    cand = np.nonzero(pos[r])[0]
                    want = [min(2, K - 1), K // 2, K - 1][r % 3]
                    k = cand[np.argmin(np.abs(cand - want))]
                    sig[r, k] = x[r, k] / delta[r, k]
        c[..., 3] = sig.astype(F32)
        self.rays, self.z, self.rgbsigma = rays, z, c
        x32 = (np.concatenate([z[:, 1:] - z[:, :-1], rays[:, 7:8] - z[:, -1:]], -1).astype(F32) * np.maximum(c[..., 3], 0)).astype(F32)
        self.opaque = bool((x32 > 9).any())                  # the regime, from the inputs
        self.d_rgb = rs.standard_normal((N, 3)).astype(F32)
        self.d_depth = rs.standard_normal(N).astype(F32) if self.cot in ("rgbd", "rgbdw") else None
        self.d_weights = rs.standard_normal((N, K)).astype(F32) if self.cot == "rgbdw" else None
        return self

    def cotangents(self):
        return self.d_rgb, self.d_depth, self.d_weights

    def keep_is_eps(self):
        """[N,K] where float32 keep == 1e-10 exactly"""
        return _alpha_keep(self.rays, self.z, self.rgbsigma, None)[5] == F32(1e-10)

    def opaque_followed(self, n=8):
        """number of samples with float32 keep == 1e-10 that at least n more samples follow"""
        return int(self.keep_is_eps()[:, : max(0, self.K - n)].sum())

    def refs(self):
        """CPU values, computed once and shared: float64 and float32 autograd, the hand-written float32 sweep, the bounds"""
        if hasattr(self, "r64"):
            return self
        self.build()
        a = (self.rays, self.z, self.rgbsigma, self.white)
        self.r64 = composite_ref_grads(*a, *self.cotangents(), torch.float64)
        self.r32 = composite_ref_grads(*a, *self.cotangents(), torch.float32)
        self.s32 = composite_f32(*a)[:3] + composite_backward_f32(*a, *self.cotangents())
        self.scale_sigma, self.scale_far = grad_scale(*a, *self.cotangents())
        # forward: both float32 evaluations against float64 (bounded weights: absolute)
        e = lambda i: max(float(np.abs(self.r32[i] - self.r64[i]).max()), float(np.abs(self.s32[i] - self.r64[i]).max()))
        self.cpu_err = dict(weights=e(0), rgb=e(1), depth=e(2))
        self.bound = dict(weights=MARGIN * e(0) + FLOOR_W, rgb=MARGIN * e(1) + FLOOR_RGB, depth=MARGIN * e(2) + FLOOR_DEPTH)
        # backward: regular regime against float64; opaque regime against float32 autograd, the CPU-side error being the disagreement
        # of the two float32 evaluations
        self.grad_ref = self.r32 if self.opaque else self.r64
        other = self.s32
        ge = [grad_errors(self.r32[3], self.r32[4], self), grad_errors(other[3], other[4], self)]
        self.cpu_gerr = {k: max(g[k] for g in ge) for k in ge[0]}
        self.gbound = {k: MARGIN * v + FLOOR_GRAD for k, v in self.cpu_gerr.items()}
        self.gbound["rgb"] = self.bound["weights"]          # d c_k = d_rgb w_k: the weights' bound per unit of cotangent
        return self


def grad_errors(d_rgbsigma, d_far, case):
    """errors of a backward against case.grad_ref, normalised: sigma and far by grad_scale (+ TINY), the colour gradients by |d_rgb|"""
    ref_c, ref_far = case.grad_ref[3], case.grad_ref[4]
    with np.errstate(all="ignore"):
        es = np.abs(np.asarray(d_rgbsigma, np.float64)[..., 3] - ref_c[..., 3]) / (case.scale_sigma + TINY)
        ef = np.abs(np.asarray(d_far, np.float64) - ref_far) / (case.scale_far + TINY)
        ec = np.abs(np.asarray(d_rgbsigma, np.float64)[..., :3] - ref_c[..., :3]) / (np.abs(case.d_rgb.astype(np.float64))[:, None, :] + TINY)
    worst = lambda a: float("inf") if not np.isfinite(a).all() else float(a.max(initial=0.0))
    return dict(sigma=worst(es), far=worst(ef), rgb=worst(ec))


def compare_composite(weights, rgb, depth, case):
    """forward outputs against float64 composite_ref within case.bound; the properties.  weights may be None.  -> findings"""
    bad = []
    for name, got, i in (("weights", weights, 0), ("rgb", rgb, 1), ("depth", depth, 2)):
        if got is None:
            continue
        d = np.abs(np.asarray(got, np.float64) - case.r64[i])
        if not (d <= case.bound[name]).all():
            bad.append(f"{name}: max error {np.nanmax(d):.3e} > {case.bound[name]:.3e}")
    if weights is not None:
        delta = np.concatenate([case.z[:, 1:] - case.z[:, :-1], case.rays[:, 7:8] - case.z[:, -1:]], -1)
        if (np.asarray(weights)[delta >= 0] < 0).any():
            bad.append("a weight is negative where delta >= 0")
        if not (np.asarray(weights, np.float64).sum(-1) <= 1 + 1e-5).all():
            bad.append("a weight sum exceeds 1 + 1e-5")
    return bad


def compare_composite_grads(d_rgbsigma, d_far, case):
    """backward outputs against case.grad_ref within case.gbound; exact zeros for sigma <= 0.  d_far may be None.  -> findings"""
    bad = []
    errs = grad_errors(d_rgbsigma, case.grad_ref[4] if d_far is None else d_far, case)
    for k, v in errs.items():
        if not v <= case.gbound[k]:
            bad.append(f"d_{k}: normalised error {v:.3e} > {case.gbound[k]:.3e}")
    off = case.rgbsigma[..., 3] <= 0
    if (np.asarray(d_rgbsigma)[..., 3][off] != 0).any():
        bad.append("a sigma gradient is non-zero where sigma <= 0")
    if d_far is not None and (np.asarray(d_far)[off[:, -1]] != 0).any():
        bad.append("d_far is non-zero where the last sigma <= 0")
    return bad


def _composite_cases():
    Ks = [1, 2, 40, 63, 64, 65, 127, 128, 129, 256, 300]
    Ns = [1, 3, 5, 64, 1001]
    sigmas = ["moderate", "zero", "negative", "opaque_one", "opaque_all"]
    zfams = ["uniform", "repeated", "last_eq_far", "last_beyond_far"]
    cots = ["rgb", "rgbd", "rgbdw"]
    cases, i = [], 0
    # every K with every sigma family; N, the background, the z family, the cotangents and the weights output cycle with coprime
    # strides so that each value meets many of the others.  K < 10 cannot hold an opaque sample that 8 more follow: regular only.
    for K in Ks:
        for sigma in sigmas:
            if sigma.startswith("opaque") and K < 10:
                continue
            cases.append(CompositeCase(K, Ns[i % 5], bool(i % 2), sigma, zfams[(i // 2) % 4], cots[i % 3], want_weights=(i % 7 != 3)))
            i += 1
    return cases


COMPOSITE_CASES = _composite_cases()


# ------------------------------------------------------------------------------------------------
# gen_rays / depth2normal in float64
# ------------------------------------------------------------------------------------------------
def gen_rays64(extrinsics, K, W, H, near, far):
    """synthetic.synth.gen_rays (reference src/util/cam_geometry.py:36-79) in float64: one camera -> [H,W,8]"""
    E, K = np.asarray(extrinsics, np.float64), np.asarray(K, np.float64)
    ys, xs = np.meshgrid(np.arange(0.5, H, 1), np.arange(0.5, W, 1), indexing="ij")
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    r_c2w = E[:3, :3].T
    rays = np.empty((H, W, 8))
    rays[..., :3] = -r_c2w @ E[:3, 3]
    rays[..., 3:6] = d @ r_c2w.T
    rays[..., 6], rays[..., 7] = near, far
    return rays


def depth2normal64(dmap, K):
    """synthetic.synth.depth2normal (reference src/util/depth2normal.py:7-87) in float64: [N,1,H,W], [N,3,3] -> [N,3,H,W]"""
    dmap, K = np.asarray(dmap, np.float64), np.asarray(K, np.float64)
    N, _, H, W = dmap.shape
    out = np.zeros((N, 3, H, W))
    ys, xs = np.meshgrid(np.arange(0.5, H, 1), np.arange(0.5, W, 1), indexing="ij")
    for n in range(N):
        k = K[n]
        pts = np.stack([(xs - k[0, 2]) / k[0, 0], (ys - k[1, 2]) / k[1, 1], np.ones_like(xs)], -1) * dmap[n, 0][..., None]
        pts = np.pad(pts, ((1, 1), (1, 1), (0, 0)), mode="edge")
        down, up, right, left = pts[2:, 1:-1], pts[:-2, 1:-1], pts[1:-1, 2:], pts[1:-1, :-2]
        nrm = np.cross(down - up, right - left)
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True))
        off_y = -1 * (down[..., 0] == 0) + 1 * (up[..., 0] == 0)
        off_x = -1 * (right[..., 0] == 0) + 1 * (left[..., 0] == 0)
        iy, ix = np.nonzero((off_y != 0) | (off_x != 0))
        src = nrm[np.clip(iy + off_y[iy, ix], 0, H - 1), np.clip(ix + off_x[iy, ix], 0, W - 1)].copy()
        nrm[iy, ix] = src
        nrm[dmap[n, 0] == 0] = 0
        out[n] = nrm.transpose(2, 0, 1)
    return out


def glue_case(W, H, B=3, seed=0):
    """B cameras with different intrinsics and a depth map each: a smooth surface, background zeros on the border, isolated foreground
    pixels and a one-pixel-wide foreground strip in the background"""
    rs = np.random.RandomState(1000 + seed)
    ext = np.stack([synth.look_at_origin_w2c(0.3 - 0.35 * b, 1.75 - 0.1 * b) for b in range(B)]).astype(F32)
    k = np.stack([synth.intrinsics(W, H) for _ in range(B)])
    for b in range(B):
        k[b, 0, 0] *= F32(1 - 0.07 * b)
        k[b, 1, 1] *= F32(1 + 0.05 * b)
        k[b, 0, 2] += F32(0.75 * b)
        k[b, 1, 2] -= F32(0.5 * b)
    near, far = (1.0 - 0.1 * np.arange(B)).astype(F32), (2.5 + 0.2 * np.arange(B)).astype(F32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([1.4 + 0.1 * b + 0.25 * np.sin(0.9 * xs / max(W, 8) * 6 + b) + 0.2 * np.cos(0.7 * ys / max(H, 8) * 6) for b in range(B)])
    d = d[:, None].astype(F32)
    if W >= 8 and H >= 8:
        d[:, :, 0, :] = 0
        d[:, :, -1, :] = 0
        d[:, :, :, 0] = 0
        d[:, :, :, -2:] = 0
        d[:, :, H // 2 - 2: H // 2 + 3, 2: W // 2] = 0       # a background block ...
        d[:, :, H // 2, 4] = 1.3                               # ... with an isolated foreground pixel
        d[:, :, H // 2, 8: W // 2 - 2] = 1.5                   # ... and a one-pixel-wide strip
        d[:, :, 3, W - 1] = 1.2                                # a foreground pixel on the image border
    elif W * H > 1:
        d[:, :, 0, 0] = 0
    return dict(extrinsics=ext, intrinsics=k.astype(F32), z_near=near, z_far=far, W=W, H=H, dmap=d, seed=rs.randint(1 << 30))


GLUE_SIZES = [(1, 1), (3, 5), (17, 33), (640, 480)]      # W x H
