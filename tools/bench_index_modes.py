"""Frame time of the latent lookup modes (SpatialEncoder index_interp / index_padding) on one GPU: a cfg3-like frame (512 x 512
target, 4 source views, K = 128, G = 48, NC = 1000) through NeRFRendererDGS.forward for the standard model, once per mode, with the
event time of each stage (sampler | point kernel | compositing).  A record, not a gate.

    python tools/bench_index_modes.py [--precision f16x3] [--steps 5] [--warmup 2] [--modes bilinear/border,bilinear/zeros,...]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--G", type=int, default=48)
    ap.add_argument("--NC", type=int, default=1000)
    ap.add_argument("--NV", type=int, default=4)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "fp32"])
    ap.add_argument("--modes", default="bilinear/border,bilinear/zeros,nearest/border,bilinear/reflection,nearest/zeros")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
    for mode in a.modes.split(","):
        interp, padding = mode.split("/")
        m = model_from_scene(sc, weights, device=dev, latent=latent, index_interp=interp, index_padding=padding)
        r = NeRFRendererDGS(n_samples=a.K, n_gaussian=a.G, n_depth_candidates=a.NC, white_bkgd=sc.white_bkgd)
        r.precision = a.precision
        with torch.no_grad():
            for _ in range(a.warmup):
                r(m, rays)
            torch.cuda.synchronize()
            r.stage_events = []
            for _ in range(a.steps):
                r(m, rays)
            torch.cuda.synchronize()
        st = np.array([[ev[i].elapsed_time(ev[i + 1]) for i in range(3)] for ev in r.stage_events])   # ms
        frame = float(np.median(st.sum(1)))
        print(json.dumps(dict(mode=mode, precision=a.precision, route=r.last_route, NV=a.NV, K=a.K, rays=NR, steps=a.steps,
                              frame_ms=frame, rays_per_s=NR / (frame / 1e3), sampler_ms=float(np.median(st[:, 0])),
                              points_ms=float(np.median(st[:, 1])), composite_ms=float(np.median(st[:, 2])))), flush=True)


if __name__ == "__main__":
    main()
