"""Times of the NOVEL renderer's sampler of deformed candidates (diner_amd/novel.py) on one GPU, one process, device events, median
after warm-ups -- the settings of tools/bench_deform.py's table: 4096 rays, NC = 1000, K = 40, G = 15, a mesh of 26 317 vertices.

* the scene: ``synth.make_scene(256, 256, 4, seed=0)`` (the maps of four source views), its 64 x 64 target rays; the mesh:
  ``--vertices`` vertices on the scene's sphere (radius 0.45), offsets 0.01 N(0,1);
* the three launches of a deformed ``sample_depthguided``: ``diner_sample_coarse``, ``diner_deform_ray_points`` (one offset set, the
  cached cluster structure) and ``diner_sample_depthguided_points``; their sum; the whole Python call;
* beside them the plain renderer's ``sample_depthguided`` (undeformed, candidates drawn in the kernel), and the existing sampler kernel
  on the SAME injected candidate depths: the figure to hold the new kernel against -- it reads 12 B more per candidate.

A record, not a gate: writes --out (profiles/novel_sampler.json).

    python tools/bench_novel_sampler.py [--vertices 26317] [--steps 7] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NR_SIDE, NC, K, G, NV, HW = 64, 1000, 40, 15, 4, 256


def stats(v, **kw):
    v = sorted(v)
    return dict(median_ms=float(v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])), min_ms=float(v[0]),
                max_ms=float(v[-1]), n=len(v), clock="device events", **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=26317)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "novel_sampler.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import diner_amd
    from diner_amd import _lib, deform
    from diner_amd.novel import NeRFRendererDGS, _MapsModel
    from diner_amd.renderer import _ptr, _stream, check
    from synthetic import synth
    from tests import knn_ref as R
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

    def device_ms(fn, **kw):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return stats(ms, **kw)

    sc = synth.make_scene(HW, HW, NV, seed=0, with_latent=False)
    model = SimpleNamespace(poses=t(sc.poses), focal=t(sc.focal), c=t(sc.c), image_shape=t(sc.image_shape),
                            encoder=SimpleNamespace(depths=t(sc.depths), depths_std=t(sc.depths_std), normals=t(sc.normals)))
    rays = t(sc.target_rays(Ht=NR_SIDE, Wt=NR_SIDE))
    NR = rays.shape[1]
    verts = t(R.sphere_mesh(a.vertices, seed=a.vertices, radius=0.45, centre=(0.0, 0.0, 0.0)))[None]
    offs = 0.01 * torch.randn_like(verts)

    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G)
    plain = diner_amd.NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G)
    scene, _keep = r._scene(_MapsModel(model), need_latent=False)
    cfg = r._cfg(K, NC, G)
    L, st = _lib.lib(), _stream(dev)
    z_cand = torch.empty((1, NR, NC), device=dev)
    z, z_dg = torch.empty((1, NR, K), device=dev), torch.empty((1, NR, K), device=dev)

    def coarse():
        check(L.diner_sample_coarse(_ptr(rays), NR, NC, None, 11, _ptr(z_cand), st), "diner_sample_coarse")

    coarse()
    xyz = deform.deform_ray_points(rays, z_cand, verts, offs)          # (builds and caches the cluster structure)

    def points_kernel():
        check(L.diner_sample_depthguided_points(C.byref(scene), _ptr(rays), _ptr(z_cand), _ptr(xyz), NR, C.byref(cfg), None, None, 11,
                                                _ptr(z), _ptr(z_dg), None, st), "diner_sample_depthguided_points")

    def rays_kernel(zc):
        check(L.diner_sample_depthguided(C.byref(scene), _ptr(rays), NR, C.byref(cfg), None, None, None, _ptr(zc), 11, _ptr(z), _ptr(z_dg),
                                         None, st), "diner_sample_depthguided")

    res = {"device": torch.cuda.get_device_name(0), "rays": NR, "n_candidates": NC, "n_samples": K, "n_gaussian": G, "source_views": NV,
           "maps": [HW, HW], "vertices": a.vertices, "steps": a.steps, "warmup": a.warmup,
           "xyz_cand_bytes": int(xyz.numel() * 4)}
    res["sample_coarse"] = device_ms(coarse)
    res["deform_ray_points_1set_auto"] = device_ms(lambda: deform.deform_ray_points(rays, z_cand, verts, offs))
    res["sampler_points_kernel"] = device_ms(points_kernel)
    res["three_launches_sum_ms"] = sum(res[k]["median_ms"] for k in ("sample_coarse", "deform_ray_points_1set_auto", "sampler_points_kernel"))
    res["novel_sample_depthguided_call"] = device_ms(lambda: r.sample_depthguided(rays, model, K, NC, verts, offs))
    res["sampler_kernel_same_candidates"] = device_ms(lambda: rays_kernel(z_cand), what="diner_sample_depthguided, z_cand injected")
    res["sampler_kernel_philox_candidates"] = device_ms(lambda: rays_kernel(None), what="diner_sample_depthguided, candidates in the kernel")
    stub = SimpleNamespace(poses=model.poses, focal=model.focal, c=model.c, image_shape=model.image_shape,
                           encoder=SimpleNamespace(depths=model.encoder.depths, depths_std=model.encoder.depths_std,
                                                   normals=model.encoder.normals, feature_padding=0.0),
                           poscode=SimpleNamespace(num_freqs=0, freqs=[1.0]))
    res["plain_sample_depthguided_call"] = device_ms(lambda: plain.sample_depthguided(rays, stub, K, NC), what="the undeformed renderer")
    res["points_over_rays_kernel"] = res["sampler_points_kernel"]["median_ms"] / res["sampler_kernel_same_candidates"]["median_ms"]
    # the same decisions where nothing is deformed: both kernels on o + z d
    plain_xyz = (rays[..., None, :3] + z_cand[..., None] * rays[..., None, 3:6]).reshape(1, -1, 3).contiguous()
    za = torch.empty_like(z)
    check(L.diner_sample_depthguided_points(C.byref(scene), _ptr(rays), _ptr(z_cand), _ptr(plain_xyz), NR, C.byref(cfg), None, None, 11,
                                            _ptr(za), None, None, st), "diner_sample_depthguided_points")
    rays_kernel(z_cand)
    res["undeformed_points_equal_rays_kernel"] = bool(torch.equal(za, z))
    res["rays_with_samples"] = int((z_dg != 0).any(-1).sum())
    print(json.dumps(res), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
