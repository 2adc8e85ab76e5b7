"""Host restatement of the NOVEL renderers' depth-guided sampler (diner_amd/novel.py, csrc/sampler_points.hip), with no arithmetic of
its own: every stage is an existing restatement.

* deformed candidates -- ``knn_ref.ray_points`` -> ``knn_ref.nearest_batch`` (the fp32 contract search) -> ``knn_ref.deform``: the bits
  ``glue.deform_ray_points`` is pinned to (tests/test_gpu_nearest_vertex.py)
* likelihood          -- the C oracle (oracle/diner_oracle.c, built without contraction) on PSEUDO-RAYS, one per candidate: origin = the
  deformed point, the ray's direction, near = 0, far = fp32((far - near) / fp32(NC)), one candidate at z = 0.  The oracle then evaluates
  exactly that point (o + 0 d) with exactly the ray's half step (((far' - 0) / 1) / 2).  With zero offsets this is ``Oracle.likelihood``
  on the true rays bit for bit (tests/test_novel_sampler_host.py).
* decisions, fill-up  -- ``stage_refs.select_rows`` and ``stage_refs.fill_up_f32``

and the cases the host and the GPU tests share.
"""
from __future__ import annotations

import copy

import numpy as np

from synthetic import synth
from tests import knn_ref
from tests import stage_refs as sr

F32 = np.float32
MAX_POINTS = 150_000       # SB * NR * NC of a case


def mesh(V, SB=1):
    """vertices [SB,V,3] on the scenes' sphere (radius 0.45 about the origin) and offsets [SB,V,3] ~ 0.03 N(0,1); scene s > 0: other
    vertices and other offsets"""
    verts = np.stack([knn_ref.sphere_mesh(V, 11 + 100 * s, radius=0.45, centre=(0, 0, 0)) for s in range(SB)])
    offs = np.stack([(0.03 * np.random.default_rng(1 + s).normal(size=(V, 3))).astype(F32) for s in range(SB)])
    return verts, offs


def deformed_candidates(rays, z_cand, vertices, offsets):
    """rays [SB,NR,8], z_cand [SB,NR,NC] -> (xyz [SB,NR,NC,3] float32, idx [SB,NR*NC])"""
    SB, NR, NC = z_cand.shape
    pts = knn_ref.ray_points(rays, z_cand)
    idx, _ = knn_ref.nearest_batch(pts, np.asarray(vertices, F32))
    return knn_ref.deform(pts, idx, offsets).reshape(SB, NR, NC, 3), idx


def pseudo_rays(rays, xyz):
    """rays [NR,8], xyz [NR,NC,3] -> [NR*NC,8]: the ray of the module docstring for every candidate"""
    NR, NC = xyz.shape[:2]
    r = np.asarray(rays, F32)
    out = np.zeros((NR, NC, 8), F32)
    out[..., :3] = xyz
    out[..., 3:6] = r[:, None, 3:6]
    out[..., 7] = (F32(1) * (r[:, 7] - r[:, 6]) / F32(NC))[:, None]
    return out.reshape(NR * NC, 8)


def likelihood(scene, rays, xyz):
    """one scene (synth.Scene with SB = 1 arrays), rays [NR,8], xyz [NR,NC,3] -> the oracle's likelihood of the points [NR,NC]"""
    from oracle.oracle import Oracle
    NR, NC = xyz.shape[:2]
    pr = pseudo_rays(rays, xyz)
    return Oracle(scene, None).likelihood(pr, np.zeros((NR * NC, 1), F32)).reshape(NR, NC)


def standin_model_np(in_pts, gen_pts, dirs):
    """the analytic stand-in point model of tools/gen_novel_sampler_golden.py, restated (float64 numpy): a smooth function of the two
    deformed points and the view direction -> [..,4] = rgb in (0,1), sigma of order 10"""
    a, b, d = [np.asarray(t, np.float64) for t in (in_pts, gen_pts, dirs)]
    rgb = 0.5 + 0.5 * np.sin(3.0 * a + 2.0 * b[..., [1, 2, 0]] + d)
    r2 = (a * a).sum(-1) + 0.5 * (b * b).sum(-1)
    sigma = 12.0 * np.exp(-4.0 * r2) * (1.2 + np.cos(5.0 * b[..., 0] + d[..., 2])) - 1.0
    return np.concatenate([rgb, sigma[..., None]], -1)


class NovelCase:
    """The scene of the fixture (synth.make_scene(24, 24, NV, seed=3)), its target rays thinned to SB * NR * NC <= MAX_POINTS, dense noise,
    a mesh of V vertices and offsets; scene s > 0 of a batch: another seed, other rays, vertices and offsets."""

    def __init__(self, NC, K, G, NV, V=331, SB=1):
        self.NC, self.K, self.G, self.NV, self.V, self.SB = NC, K, G, NV, V, SB
        self.id = f"NC{NC}-K{K}-G{G}-NV{NV}-V{V}" + (f"-SB{SB}" if SB > 1 else "")

    def build(self):
        if hasattr(self, "rays"):
            return self
        NC, K, G = self.NC, self.K, self.G
        self.scenes = [synth.make_scene(24, 24, self.NV, seed=3 + 7 * s, with_latent=False, bg_sigma_zero=(s == 1)) for s in range(self.SB)]
        stride = 2
        while (576 // stride) * NC * self.SB > MAX_POINTS:
            stride *= 2
        rays = np.concatenate([sc.target_rays()[:, (i % stride)::stride] for i, sc in enumerate(self.scenes)], 0)
        if NC <= 2:
            # one or two candidates per ray: [near, far] = 0.02 either side of where the ray meets the scene's sphere, so that the
            # candidate lies within depth_diff_max of the surface and its half step (0.02 / NC) does not saturate the erf difference
            # (sigma is 0.004 .. 0.008): the likelihood then depends on where the point is, as it does for large NC
            for s, sc in enumerate(self.scenes):
                o, d = rays[s, :, :3].astype(np.float64), rays[s, :, 3:6].astype(np.float64)
                b, cc = (o * d).sum(-1), (o * o).sum(-1) - sc.meta["sphere_radius"] ** 2
                hit = b * b - cc > 0
                t = -b - np.sqrt(np.where(hit, b * b - cc, 0.0))
                rays[s, hit, 6], rays[s, hit, 7] = (t - 0.02)[hit], (t + 0.02)[hit]
        self.rays = np.ascontiguousarray(rays, F32)
        NR = self.NR = rays.shape[1]
        noise = [synth.make_noise(NR, NC, G, K, seed=5 + s) for s in range(self.SB)]
        self.u_coarse, self.n_gauss, self.u_fill = [np.stack([n[i] for n in noise]) for i in range(3)]
        self.vertices, self.offsets = mesh(self.V, self.SB)
        return self

    def refs(self):
        """CPU expectations, computed once: z_cand, xyz, the restated likelihood with and without the offsets"""
        if hasattr(self, "L"):
            return self
        from oracle.oracle import Oracle
        self.build()
        self.z_cand = np.stack([Oracle(sc, None).sample_coarse(self.rays[s], self.NC, self.u_coarse[s]) for s, sc in enumerate(self.scenes)])
        self.xyz, self.idx = deformed_candidates(self.rays, self.z_cand, self.vertices, self.offsets)
        self.L = np.stack([likelihood(sc, self.rays[s], self.xyz[s]) for s, sc in enumerate(self.scenes)])
        self.L_plain = np.stack([Oracle(sc, None).likelihood(self.rays[s], self.z_cand[s]) for s, sc in enumerate(self.scenes)])
        return self

    def batched_scene(self):
        sc = copy.copy(self.scenes[0])
        for name in ("poses", "focal", "c", "depths", "depths_std", "normals"):
            setattr(sc, name, np.concatenate([getattr(s, name) for s in self.scenes], 0))
        return sc


# (NC, K, G, NV, V[, SB]): every sampler_points_kernel<CPL> (NC <= 256 / 1024 / 2048 / 4096) on both sides of its boundary; K in
# {1, 8, 63, 64, 65, 128} with G in {0, 1, middle, K}, K <= NC, paired; NV 1 and 3; V 1, 331 and 1031 (1031: the pruned search); one batch
# of two scenes.  (64, 8, 4, NV 3) and (1024, 40, 15, NV 2) are the two cases of tests/golden/novel_sampler.npz.
GOLDEN_CASES = {"nc64": NovelCase(64, 8, 4, 3), "nc1024": NovelCase(1024, 40, 15, 2)}
GRID = [NovelCase(1, 1, 0, 1), NovelCase(1, 1, 1, 3, V=1), GOLDEN_CASES["nc64"], NovelCase(64, 64, 64, 1), NovelCase(256, 63, 1, 3, V=1031),
        NovelCase(257, 65, 20, 1), GOLDEN_CASES["nc1024"], NovelCase(1024, 128, 48, 3, SB=2), NovelCase(1025, 64, 0, 1, V=1031),
        NovelCase(2048, 128, 128, 3), NovelCase(2049, 8, 1, 1, V=1), NovelCase(4096, 64, 20, 3), NovelCase(4096, 128, 0, 1, V=1031)]
PHILOX_CASES = [NovelCase(64, 8, 4, 3), NovelCase(1024, 40, 15, 3), NovelCase(2048, 128, 48, 1), NovelCase(4096, 64, 20, 1)]   # one per CPL
