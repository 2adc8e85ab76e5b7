"""Throughput of the shape-general inference path (points_mlp_gen.hip; --precision f16x3: points_mlp_gen_f16.hip) on one GPU: rays/s of a whole 512 x 512 frame through
NeRFRendererDGS.forward for a non-standard model, with the event time of each stage (sampler | generic point kernel | compositing).
A record, not a gate.  Default: case (a) of tools/gen_shape_golden.py (d_hidden 128, 5 blocks, combine_layer 3) at K = 40,
NV = 2, the reference's renderer defaults otherwise.  --num_freqs other than 6 keeps a model with the standard ResnetFC (d_hidden 512,
5 blocks, combine_layer 3) on the shape-general route.

    python tools/bench_mlp_shapes.py [--res 512] [--K 40] [--NV 2] [--d_hidden 128] [--num_freqs 6] [--precision fp32|f16x3]
                                     [--steps 5] [--warmup 2]

--linz-maps: the lin_z maps of the shape-general routes (renderer.linz_maps_any_shape) on and off, in one process on one box: cases (a)
(d_hidden 128, NV 2, K 40) and (b) (d_hidden 512, num_freqs 10, NV 4, K 128) of DESIGN.md §4's table in both precisions, the point
kernel's HIP-event time as the median of --steps frames after --warmup, the builder's time per encode() and the maps' bytes; writes
--out (default profiles/linz_maps_gen.json).  A record, not a gate: no ratio is asserted.

    python tools/bench_mlp_shapes.py --linz-maps [--res 512] [--steps 5] [--warmup 2] [--out profiles/linz_maps_gen.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


LINZ_CASES = {   # DESIGN.md §4, the rows of the shape-general kernels
    "a": dict(d_hidden=128, n_blocks=5, combine_layer=3, num_freqs=6, NV=2, K=40),
    "b": dict(d_hidden=512, n_blocks=5, combine_layer=3, num_freqs=10, NV=4, K=128),
}


def linz_maps(a):
    import numpy as np
    import torch
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene

    dev = torch.device("cuda:0")
    results = []
    for cname, cfg in LINZ_CASES.items():
        dims = dict(d_hidden=cfg["d_hidden"], n_blocks=cfg["n_blocks"], combine_layer=cfg["combine_layer"])
        sc = synth.make_scene(a.res, a.res, cfg["NV"], seed=0, feature_padding=32, with_latent=False)
        h, w = sc.latent_hw
        latent = torch.randn((1, cfg["NV"], 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1, d_in=7 + 8 * cfg["num_freqs"], **dims), device=dev, latent=latent,
                             num_freqs=cfg["num_freqs"], **dims)
        rays = torch.from_numpy(np.ascontiguousarray(sc.target_rays())).to(dev)
        for precision in ("fp32", "f16x3"):
            rec = dict(case=cname, precision=precision, rays=int(rays.shape[1]), latent_bytes=latent.numel() * 4, **cfg)
            for on in (False, True):
                r = NeRFRendererDGS(n_samples=cfg["K"], n_gaussian=a.G, white_bkgd=sc.white_bkgd, f16x3_any_shape=precision == "f16x3",
                                    linz_maps_any_shape=on)
                r.precision = precision
                with torch.no_grad():
                    for _ in range(a.warmup):
                        r(m, rays)
                    torch.cuda.synchronize()
                    r.stage_events = []
                    for _ in range(a.steps):
                        r(m, rays)
                    torch.cuda.synchronize()
                    route = ("points_mlp_gen_f16" if precision == "f16x3" else "points_mlp_gen") + ("_lz" if on else "")
                    assert r.last_route == route and r.effective_precision == precision, (r.last_route, r.effective_precision)
                    st = np.array([[ev[i].elapsed_time(ev[i + 1]) for i in range(3)] for ev in r.stage_events])
                    key = "maps_on" if on else "maps_off"
                    rec[key] = dict(route=route, point_kernel_ms=float(np.median(st[:, 1])), point_kernel_min_ms=float(st[:, 1].min()),
                                    point_kernel_max_ms=float(st[:, 1].max()), frame_ms=float(np.median(st.sum(1))))
                    if on:   # the builder alone: every other pack is cached, so _scene builds the maps and nothing else
                        shape = r._validate(m)
                        times = []
                        for i in range(a.warmup + a.steps):
                            r._linz_gen_key = None
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            r._scene(m, need_latent=True, gen_shape=shape)
                            e1.record()
                            torch.cuda.synchronize()
                            if i >= a.warmup:
                                times.append(e0.elapsed_time(e1))
                        rec["builder_ms_per_encode"] = float(np.median(times))
                        rec["linz_maps_gen_bytes"] = int(r.memory_report()["cached"]["linz_maps_gen"])
                del r
                torch.cuda.empty_cache()
            results.append(rec)
            print(json.dumps(rec), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(tool="tools/bench_mlp_shapes.py --linz-maps", res=a.res, steps=a.steps, warmup=a.warmup,
                                   device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--K", type=int, default=40)
    ap.add_argument("--G", type=int, default=15)
    ap.add_argument("--NV", type=int, default=2)
    ap.add_argument("--d_hidden", type=int, default=128)
    ap.add_argument("--n_blocks", type=int, default=5)
    ap.add_argument("--combine_layer", type=int, default=3)
    ap.add_argument("--num_freqs", type=int, default=6)
    ap.add_argument("--precision", choices=["fp32", "f16x3"], default="fp32",
                    help="fp32: points_mlp_gen (exact fp32 MFMA); f16x3: points_mlp_gen_f16 (renderer.f16x3_any_shape)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--linz-maps", action="store_true", help="time the lin_z maps of the shape-general routes on and off (see above)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "linz_maps_gen.json"), help="--linz-maps: the JSON record to write")
    a = ap.parse_args()
    if a.linz_maps:
        return linz_maps(a)

    import numpy as np
    import torch
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene

    dev = torch.device("cuda:0")
    dims = dict(d_hidden=a.d_hidden, n_blocks=a.n_blocks, combine_layer=a.combine_layer)
    sc = synth.make_scene(a.res, a.res, a.NV, seed=0, feature_padding=32, with_latent=False)
    h, w = sc.latent_hw
    g = torch.Generator(device=dev).manual_seed(1)
    latent = torch.randn((1, a.NV, 512, h, w), device=dev, generator=g)
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1, d_in=7 + 8 * a.num_freqs, **dims), device=dev, latent=latent,
                         num_freqs=a.num_freqs, **dims)
    rays = torch.from_numpy(np.ascontiguousarray(sc.target_rays())).to(dev)
    NR = rays.shape[1]
    r = NeRFRendererDGS(n_samples=a.K, n_gaussian=a.G, white_bkgd=sc.white_bkgd, f16x3_any_shape=a.precision == "f16x3")
    r.precision = a.precision
    route = "points_mlp_gen_f16" if a.precision == "f16x3" else "points_mlp_gen"
    with torch.no_grad():
        for _ in range(a.warmup):
            r(m, rays)
        torch.cuda.synchronize()
        r.stage_events = []
        for _ in range(a.steps):
            r(m, rays)
        torch.cuda.synchronize()
    assert r.last_route == route and r.effective_precision == a.precision, (r.last_route, r.effective_precision)
    st = np.array([[ev[i].elapsed_time(ev[i + 1]) for i in range(3)] for ev in r.stage_events])   # ms
    frame = float(np.median(st.sum(1)))
    print(json.dumps(dict(path=route, precision=a.precision, num_freqs=a.num_freqs, d_hidden=a.d_hidden, n_blocks=a.n_blocks, combine_layer=a.combine_layer, NV=a.NV, K=a.K,
                          rays=NR, steps=a.steps, rays_per_s=NR / (frame / 1e3), frame_ms=frame,
                          sampler_ms=float(np.median(st[:, 0])), points_mlp_gen_ms=float(np.median(st[:, 1])),
                          composite_ms=float(np.median(st[:, 2])),
                          points_mlp_gen_min_ms=float(st[:, 1].min()), points_mlp_gen_max_ms=float(st[:, 1].max()))))


if __name__ == "__main__":
    main()
