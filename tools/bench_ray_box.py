"""Frame time of ``render_image(bounds=)`` against the share of rays that meet the box (diner_amd/csrc/ray_box.hip; glue.box_rays,
glue.frame_from_hits) on one GPU, on bench.py's cfg3 scene (512 x 512 target, 4 source views, K = 128, G = 48, NC = 1000, f16x3).

* ``full_frame``: ``render_image`` without ``bounds``, in fresh child processes, alternating between this tree and -- with
  ``--parent DIR``, a built checkout of the parent commit -- the parent's.  The code path is unchanged, so the two must agree within
  their run-to-run spread; both medians and spreads are recorded.
* ``boxes``: cubes around the origin whose half side is bisected (``glue.ray_box``'s mask) until about 25 % and 50 % of the rays hit,
  and a box that contains the camera (100 %: every ray, over [z_near, z_far]).  Per box: hit share, frame ms (host clock around a
  synchronise: the route reads its counts on the host), and the ms of the three new pieces with device events over windows of
  ``--calls`` calls: ``select`` (diner_ray_box_select: three launches), ``gen_rays_box`` and ``frame_from_hits``.
* ``model``: hit share x the full frame + the new kernels, next to the measured frame; the difference is what the synchronisation, the
  compact-ray round trip and the smaller launches' tails cost.

A record, not a gate: writes --out (profiles/ray_box.json).

    python tools/bench_ray_box.py [--parent DIR] [--steps 10] [--warmup 3] [--rounds 2] [--calls 50] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CFG3 = dict(H=512, W=512, NV=4, K=128, G=48, NC=1000)         # bench.py CONFIGS["cfg3"]


def setup(root):
    """cfg3's scene, model, renderer and target camera as bench.py builds them, from the tree at ``root``"""
    if str(root) not in sys.path:
        sys.path.insert(0, str(root))
    import torch

    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    H, W, NV = CFG3["H"], CFG3["W"], CFG3["NV"]
    scene = synth.make_scene(H, W, NV, seed=0, dataset="facescape", with_latent=False)
    h, w = scene.latent_hw
    gen = torch.Generator(device=dev).manual_seed(1234)
    latent = torch.randn((1, NV, 512, h, w), generator=gen, device=dev, dtype=torch.float32)
    model = model_from_scene(scene, synth.make_mlp_weights(7, bias_scale=0.1), device=dev, latent=latent)
    rend = NeRFRendererDGS(n_samples=CFG3["K"], n_depth_candidates=CFG3["NC"], n_gaussian=CFG3["G"], white_bkgd=scene.white_bkgd)
    E = torch.from_numpy(scene.target_extrinsics.astype("float32"))[None].to(dev)
    Kt = torch.from_numpy(scene.target_intrinsics.astype("float32"))[None].to(dev)
    return torch, dev, scene, model, rend, E, Kt


def frame_ms(torch, fn, steps, warmup):
    """ms per call of ``fn``: the host clock around a call that ends in a device synchronise"""
    ms = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def worker(a):
    torch, dev, scene, model, rend, E, Kt = setup(Path(a.worker))
    H, W = CFG3["H"], CFG3["W"]
    ms = frame_ms(torch, lambda: rend.render_image(model, E, Kt, H, W, float(scene.near), float(scene.far), return_depth=True), a.steps, a.warmup)
    print("FULL_FRAME_MS " + json.dumps(ms), flush=True)


def stats(v, **kw):
    v = sorted(v)
    return dict(median=float(v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])), min=float(v[0]), max=float(v[-1]),
                n=len(v), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its full frame is timed next to this tree's)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="child processes per tree for the full frame, alternating")
    ap.add_argument("--calls", type=int, default=50, help="calls per device-event window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ray_box.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    # ---- the full frame, fresh processes, this tree and the parent's alternating ----------------------------------------------------------
    trees = {"this": ROOT}
    if a.parent:
        trees = {"parent": Path(a.parent).resolve(), "this": ROOT}
    full = {k: [] for k in trees}
    for _ in range(a.rounds):
        for name, root in trees.items():
            out = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--worker", str(root), "--steps", str(a.steps), "--warmup",
                                  str(a.warmup)], check=True, capture_output=True, text=True, timeout=600, cwd=str(root)).stdout
            full[name] += json.loads([l for l in out.splitlines() if l.startswith("FULL_FRAME_MS ")][-1].split(" ", 1)[1])
    results = {"config": dict(CFG3, precision="f16x3"), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
               "full_frame_ms": {k: stats(v, clock="host, synchronised", processes=a.rounds) for k, v in full.items()}}
    if not a.parent:
        results["full_frame_ms"]["parent"] = "not measured (no --parent checkout given)"
    print(json.dumps({"full_frame_ms": results["full_frame_ms"]}), flush=True)

    # ---- the boxes ---------------------------------------------------------------------------------------------------------------------
    import ctypes as C

    import numpy as np

    torch, dev, scene, model, rend, E, Kt = setup(ROOT)
    from diner_amd import _lib, glue
    results["device"] = torch.cuda.get_device_name(0)
    H, W = CFG3["H"], CFG3["W"]
    zn, zf = float(scene.near), float(scene.far)

    def cube(s):
        return np.array([[-s, -s, -s], [s, s, s]], np.float32)

    def share(b):
        return float(glue.ray_box(E, Kt, W, H, zn, zf, b)[2].float().mean())

    def cube_for(target):
        lo, hi = 0.0, 2.0
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if share(cube(mid)) < target else (lo, mid)
        return cube(hi)

    def device_ms(fn):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1) / a.calls)
        return stats(ms, clock="device events", calls_per_window=a.calls)

    full_here = frame_ms(torch, lambda: rend.render_image(model, E, Kt, H, W, zn, zf, return_depth=True), a.steps, a.warmup)
    results["full_frame_ms"]["this_same_process"] = stats(full_here, clock="host, synchronised")
    full_med = results["full_frame_ms"]["this_same_process"]["median"]
    boxes = {"hit_25": cube_for(0.25), "hit_50": cube_for(0.50), "hit_100": cube(float(scene.meta["cam_radius"]) + 1.0)}
    results["boxes"] = {}
    for name, b in boxes.items():
        ms = frame_ms(torch, lambda: rend.render_image(model, E, Kt, H, W, zn, zf, return_depth=True, bounds=b), a.steps, a.warmup)
        hits = rend.last_box_hits[0]
        cam, bt, lo, hi, _keep = glue._box_args(E, Kt, W, H, zn, zf, b, glue.BOX_OFFSET, "bench_ray_box")
        _, idx, slot, count = glue._ray_box_select(cam, 1, bt, lo, hi, dev, False)
        rays = torch.empty((1, hits, 8), dtype=torch.float32, device=dev)
        rgb_c, depth_c = torch.rand((1, hits, 3), device=dev), torch.rand((1, hits), device=dev)
        L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        kernels = {"select": device_ms(lambda: glue._ray_box_select(cam, 1, bt, lo, hi, dev, False)),
                   "gen_rays_box": device_ms(lambda: _lib.check(L.diner_gen_rays_box(C.byref(cam), 1, bt.data_ptr(), lo, hi, idx.data_ptr(),
                                                                                      count.data_ptr(), None, hits, rays.data_ptr(), st),
                                                                "diner_gen_rays_box")),
                   "frame_from_hits": device_ms(lambda: glue.frame_from_hits(rgb_c, depth_c, slot, H, W, scene.white_bkgd))}
        frame = stats(ms, clock="host, synchronised")
        new_ms = sum(k["median"] for k in kernels.values())
        model_ms = hits / (H * W) * full_med + new_ms
        rec = {"bounds": b.tolist(), "hits": hits, "hit_share": hits / (H * W), "route": rend.last_route, "frame_ms": frame,
               "new_kernels_ms": kernels, "model_ms": model_ms, "frame_minus_model_ms": frame["median"] - model_ms,
               "frame_over_full": frame["median"] / full_med}
        results["boxes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
