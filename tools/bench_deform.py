"""Times of the nearest-vertex search and the fused deformation (diner_amd/csrc/nearest_vertex.hip; glue.nearest_vertex,
glue.deform_points, glue.deform_ray_points) on one GPU, one process, device events, median after warm-ups.

* the mesh: ``--vertices`` (26 317, the vertex count quoted for FaceScape's topologically uniform mesh) vertices on a bumpy sphere of
  radius 0.15; the rays: 4096 rays from 1.75 away through the mesh, near / far 1.0 / 2.5;
* ``candidates``: N = 4096 x 1000, the candidates of one forward, stratified along the rays; ``samples``: N = 4096 x 40;
* per size: the brute-force kernel, the pruned kernel excluding and including the cluster build (keys, stable sort, boxes), the fused
  forms (``deform_points`` with one and two offset sets, ``deform_ray_points`` on the samples), and the baseline a ROCm user can write
  today: a chunked ``torch.cdist`` + ``argmin``;
* ``threshold_sweep``: both kernels on both workloads at smaller V, the numbers ``deform.AUTO_CLUSTERS_MIN_V`` is set from.

Both kernels' results are compared bit for bit at every timed size, and the share of points on which cdist + argmin (another
arithmetic) picks the same vertex is recorded.  A record, not a gate: writes --out (profiles/deform_points.json).

    python tools/bench_deform.py [--vertices 26317] [--steps 7] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NR, NC, K = 4096, 1000, 40
NEAR, FAR = 1.0, 2.5


def stats(v, **kw):
    v = sorted(v)
    return dict(median_ms=float(v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])), min_ms=float(v[0]),
                max_ms=float(v[-1]), n=len(v), clock="device events", **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=26317)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deform_points.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from diner_amd import deform, glue
    from tests import knn_ref as R
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")

    def device_ms(fn, calls=1, **kw):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1) / calls)
        return stats(ms, calls_per_window=calls, **kw)

    def mesh(V):
        return torch.from_numpy(R.sphere_mesh(V, seed=V, centre=(0.0, 0.0, 0.0)))[None].to(dev)

    g = torch.Generator(device=dev).manual_seed(7)
    o = torch.randn((1, NR, 3), generator=g, device=dev)
    o = 1.75 * o / o.norm(dim=-1, keepdim=True)
    target = 0.12 * torch.randn((1, NR, 3), generator=g, device=dev)
    d = target - o
    d = d / d.norm(dim=-1, keepdim=True)
    rays = torch.cat([o, d, torch.full((1, NR, 1), NEAR, device=dev), torch.full((1, NR, 1), FAR, device=dev)], -1).contiguous()

    def depths(n):
        step = (torch.arange(n, device=dev) + torch.rand((1, NR, n), generator=g, device=dev)) / n
        return (NEAR * (1 - step) + FAR * step).contiguous()

    def points(z):
        return (rays[..., None, :3] + z[..., None] * rays[..., None, 3:6]).reshape(1, -1, 3).contiguous()

    def cdist_argmin(p, v, chunk=8192):
        out = torch.empty(p.shape[1], dtype=torch.int64, device=dev)
        for s in range(0, p.shape[1], chunk):
            out[s:s + chunk] = torch.cdist(p[0, s:s + chunk], v[0]).argmin(1)
        return out

    def build_only(v):
        deform.clear_cache()
        deform._clusters(v, v)

    V = a.vertices
    verts = mesh(V)
    off1, off2 = 0.02 * torch.randn_like(verts), 0.02 * torch.randn_like(verts)
    results = {"device": torch.cuda.get_device_name(0), "vertices": V, "rays": NR, "near_far": [NEAR, FAR], "steps": a.steps,
               "warmup": a.warmup, "auto_clusters_min_v": deform.AUTO_CLUSTERS_MIN_V, "sizes": {}}
    results["build_ms"] = device_ms(lambda: build_only(verts), what="keys + stable sort + cluster boxes")
    z_samples = depths(K)
    for name, z in (("samples", z_samples), ("candidates", depths(NC))):
        p = points(z)
        N = p.shape[1]
        rec = {"N": N, "pairs": N * V}
        ib, db = glue.nearest_vertex(p, verts, method="brute")
        ic, dc = glue.nearest_vertex(p, verts, method="clusters")
        rec["kernels_bit_equal"] = bool(torch.equal(ib, ic) and torch.equal(db.view(torch.int32), dc.view(torch.int32)))
        rec["brute"] = device_ms(lambda: glue.nearest_vertex(p, verts, method="brute"))
        rec["clusters_excluding_build"] = device_ms(lambda: glue.nearest_vertex(p, verts, method="clusters"))

        def with_build():
            deform.clear_cache()
            glue.nearest_vertex(p, verts, method="clusters")
        rec["clusters_including_build"] = device_ms(with_build)
        rec["deform_points_1set_auto"] = device_ms(lambda: glue.deform_points(p, verts, off1))
        rec["deform_points_2sets_auto"] = device_ms(lambda: glue.deform_points(p, verts, off1, off2))
        if name == "samples":
            rec["deform_ray_points_2sets_auto"] = device_ms(lambda: glue.deform_ray_points(rays, z, verts, off1, off2))
            rec["deform_ray_points_2sets_points_auto"] = device_ms(lambda: glue.deform_ray_points(rays, z, verts, off1, off2, return_points=True))
        rec["baseline_cdist_argmin_same_vertex_share"] = float((cdist_argmin(p, verts) == ib[0].long()).float().mean())
        rec["baseline_cdist_argmin"] = device_ms(lambda: cdist_argmin(p, verts), chunk=8192)
        results["sizes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
        del p

    # ---- where the pruned kernel starts to pay: both kernels on both workloads at smaller V -------------------------------------------------
    # (a wave of samples spans one or two whole rays, a wave of candidates a short stretch of one: the union of the clusters its lanes
    # need, which is what the wave scans, differs accordingly)
    sweep = {}
    for wname, z in (("samples", z_samples), ("candidates", depths(NC))):
        p = points(z)
        calls = 20 if wname == "samples" else 1
        for Vs in (256, 1024, 4096, 8192, 16384):
            vs = mesh(Vs)
            rec = sweep.setdefault(str(Vs), {})
            rec[wname] = {"brute": device_ms(lambda: glue.nearest_vertex(p, vs, method="brute"), calls=calls),
                          "clusters_excluding_build": device_ms(lambda: glue.nearest_vertex(p, vs, method="clusters"), calls=calls)}
            rec["build"] = device_ms(lambda: build_only(vs))
        del p
    for Vs, rec in sweep.items():
        rec["forward_ms"] = {m: rec["samples"][m]["median_ms"] + rec["candidates"][m]["median_ms"] for m in ("brute", "clusters_excluding_build")}
    results["threshold_sweep"] = {"N": {"samples": NR * K, "candidates": NR * NC}, "by_vertices": sweep,
                                  "forward_ms": "one search of the candidates + one of the samples, medians added"}
    print(json.dumps({"threshold_sweep": {k: v["forward_ms"] for k, v in sweep.items()}}), flush=True)
    print(json.dumps({"threshold_sweep_detail": sweep}), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
