"""Cost of the bicubic latent lookup (index_interp="bicubic", renderer.bicubic_index) next to bilinear on the SAME kernels, on one GPU:
(a) a cfg3-like frame (512 x 512 target, 4 source views, K = 128, G = 48, NC = 1000) of the standard model through
    NeRFRendererDGS.forward on the two shape-general kernels (points_mlp_gen in fp32, points_mlp_gen_f16 in f16x3): bicubic/border
    against bilinear/border (the default compilation) and bilinear/zeros (the _ix compilation), with the event time of each stage;
(b) a 4096-ray training step (forward + backward of diner_amd/training_gen.py, K = 40, 4 views) in both precisions.
The standard model is sent to the shape-general routes for the bilinear baselines as well (the routing predicate is overridden here,
as the tests' _force_gen does for fp32), so that a ratio compares gathers, not kernels.  A record, not a gate: writes
profiles/bicubic.json.

    python tools/bench_bicubic.py [--steps 5] [--warmup 2] [--out profiles/bicubic.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

MODES = ["bilinear/border", "bilinear/zeros", "bicubic/border"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--G", type=int, default=48)
    ap.add_argument("--NC", type=int, default=1000)
    ap.add_argument("--NV", type=int, default=4)
    ap.add_argument("--train-rays", type=int, default=4096)
    ap.add_argument("--train-K", type=int, default=40)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bicubic.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene

    dev = torch.device("cuda:0")
    sc = synth.make_scene(a.res, a.res, a.NV, seed=0, feature_padding=32, with_latent=False)
    h, w = sc.latent_hw
    g = torch.Generator(device=dev).manual_seed(1)
    latent = torch.randn((1, a.NV, 512, h, w), device=dev, generator=g)
    weights = synth.make_mlp_weights(1, bias_scale=0.1)
    rays = torch.from_numpy(np.ascontiguousarray(sc.target_rays())).to(dev)
    NR = rays.shape[1]

    def renderer(precision, K, G):
        r = NeRFRendererDGS(n_samples=K, n_gaussian=G, n_depth_candidates=a.NC, white_bkgd=sc.white_bkgd, bicubic_index=True,
                            f16x3_any_shape=True, train_any_shape=True, train_f16x3_any_shape=True)
        r.precision = precision
        r._needs_gen = lambda shape, model=None: True          # the bilinear baselines on the shape-general routes too
        return r

    rec = dict(device=torch.cuda.get_device_name(0), frame=dict(res=a.res, NV=a.NV, K=a.K, G=a.G, NC=a.NC, rays=NR, steps=a.steps, rows=[]),
               train=dict(rays=a.train_rays, K=a.train_K, NV=a.NV, steps=a.steps, rows=[]))
    for precision in ("fp32", "f16x3"):
        for mode in MODES:
            interp, padding = mode.split("/")
            m = model_from_scene(sc, weights, device=dev, latent=latent, index_interp=interp, index_padding=padding)
            r = renderer(precision, a.K, a.G)
            with torch.no_grad():
                for _ in range(a.warmup):
                    r(m, rays)
                torch.cuda.synchronize()
                r.stage_events = []
                for _ in range(a.steps):
                    r(m, rays)
                torch.cuda.synchronize()
            st = np.array([[ev[i].elapsed_time(ev[i + 1]) for i in range(3)] for ev in r.stage_events])   # ms
            row = dict(mode=mode, precision=precision, route=r.last_route, frame_ms=float(np.median(st.sum(1))),
                       sampler_ms=float(np.median(st[:, 0])), points_ms=float(np.median(st[:, 1])),
                       points_ms_min=float(st[:, 1].min()), points_ms_max=float(st[:, 1].max()), composite_ms=float(np.median(st[:, 2])))
            rec["frame"]["rows"].append(row)
            print(json.dumps(row), flush=True)
    tr = rays[:, torch.randperm(NR, generator=torch.Generator().manual_seed(2))[:a.train_rays].to(dev)].contiguous()
    for precision in ("fp32", "f16x3"):
        for mode in ("bilinear/border", "bicubic/border"):
            interp, padding = mode.split("/")
            m = model_from_scene(sc, weights, device=dev, latent=latent.clone(), index_interp=interp, index_padding=padding)
            for p in m.mlp_fine.parameters():
                p.requires_grad_(True)
            m.encoder.latent.requires_grad_(True)
            r = renderer(precision, a.train_K, 15)
            with torch.no_grad():
                z = r._sample(tr, m, a.train_K, a.NC, 15, 0.05, None, None)["z"]
            times = []
            for i in range(a.warmup + a.steps):
                for t in list(m.mlp_fine.parameters()) + [m.encoder.latent]:
                    t.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = r(m, tr, z_samples=z).fine
                (out.rgb.sum() + out.depth.sum()).backward()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times.append(e0.elapsed_time(e1))
            row = dict(mode=mode, precision=precision, route=r.last_route, step_ms=float(np.median(times)), step_ms_min=float(min(times)),
                       step_ms_max=float(max(times)))
            rec["train"]["rows"].append(row)
            print(json.dumps(row), flush=True)
            del out, m, r
            torch.cuda.empty_cache()

    def ratio(rows, key, precision, base):
        f = {x["mode"]: x[key] for x in rows if x["precision"] == precision}
        return f["bicubic/border"] / f[base]

    rec["ratios"] = {}
    for precision in ("fp32", "f16x3"):
        rec["ratios"][precision] = dict(
            frame_vs_bilinear_border=ratio(rec["frame"]["rows"], "frame_ms", precision, "bilinear/border"),
            points_vs_bilinear_border=ratio(rec["frame"]["rows"], "points_ms", precision, "bilinear/border"),
            points_vs_bilinear_zeros_ix=ratio(rec["frame"]["rows"], "points_ms", precision, "bilinear/zeros"),
            train_step_vs_bilinear_border=ratio(rec["train"]["rows"], "step_ms", precision, "bilinear/border"))
    print(json.dumps(rec["ratios"]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
