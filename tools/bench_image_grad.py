#!/usr/bin/env python3
"""Forward + backward time of ONE whole 512 x 512 frame through ``render_image`` under autograd (the inference frame, then the chunked
recomputation of the training path and the gen_rays backward to the target camera), and the peak allocated memory, at the reference's
shipped configuration (K = 40, G = 15, NC = 1000, NV = 2) and at cfg3 (K = 128, G = 48, NC = 1000, NV = 4), in both precisions.
Every MLP parameter, encoder.latent and the target extrinsics require grad.  One warm-up frame per configuration, then ``--reps``
timed frames (host clock around work that ends in a device synchronise); prints one JSON line with min / median / max.

    python tools/bench_image_grad.py [--reps 3] [--configs shipped,cfg3] [--precisions f16x3,fp32] [--chunk 4096]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from diner_amd import NeRFRendererDGS  # noqa: E402
from synthetic import synth  # noqa: E402
from synthetic.model_stub import model_from_scene  # noqa: E402

CONFIGS = {"shipped": dict(K=40, G=15, NC=1000, NV=2), "cfg3": dict(K=128, G=48, NC=1000, NV=4)}


def run(name, precision, reps, chunk, H=512, W=512):
    c = CONFIGS[name]
    dev = torch.device("cuda:0")
    sc = synth.make_scene(H, W, c["NV"], seed=0, with_latent=False)
    h, w = sc.latent_hw
    latent = torch.randn((1, c["NV"], 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    m = model_from_scene(sc, synth.make_mlp_weights(7, bias_scale=0.1), device=dev, latent=latent)
    params = list(m.mlp_fine.parameters())
    for p in params:
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=c["K"], n_depth_candidates=c["NC"], n_gaussian=c["G"], white_bkgd=sc.white_bkgd)
    r.precision, r.grad_chunk_rays = precision, chunk
    E = torch.from_numpy(sc.target_extrinsics)[None].to(dev).requires_grad_(True)
    Kt = torch.from_numpy(sc.target_intrinsics)[None].to(dev)
    zn, zf = torch.tensor([sc.near], device=dev), torch.tensor([sc.far], device=dev)
    tgt = torch.rand((1, 3, H, W), device=dev)
    times = []
    for i in range(reps + 1):
        for t in params + [m.encoder.latent, E]:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        ((r.render_image(m, E, Kt, H, W, zn, zf) - tgt) ** 2).mean().backward()
        torch.cuda.synchronize()
        if i:
            times.append(time.perf_counter() - t0)
    assert E.grad is not None and torch.isfinite(E.grad).all()
    return {"config": name, "precision": precision, **c, "H": H, "W": W, "grad_chunk_rays": chunk,
            "s_per_frame": {"min": min(times), "median": statistics.median(times), "max": max(times)},
            "peak_alloc_GB": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="shipped,cfg3")
    ap.add_argument("--precisions", default="f16x3,fp32")
    ap.add_argument("--chunk", type=int, default=4096)
    a = ap.parse_args()
    res = [run(n, p, a.reps, a.chunk) for n in a.configs.split(",") for p in a.precisions.split(",")]
    print(json.dumps({"what": "render_image forward + backward of one 512x512 frame (MLP, latent and target extrinsics require grad)",
                      "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
