#!/usr/bin/env python3
"""Cost of the camera / ray / depth-map gradients on the training step of tools/bench_train.py (4096 rays, K = 40, NV = 4: 655,360
(view, sample) rows): one step with the MLP and the latent requiring grad ("off"), and the same with rays, poses, focal, c,
image_shape and encoder.depths requiring grad as well ("on").  Prints one JSON line: ms per step of both, the overhead, and the
device times of the new kernels in one "on" step (torch.profiler).  lin_in's input-gradient GEMM runs on the existing GEMM kernel:
it is inside the step delta but not in the per-kernel list."""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from diner_amd import NeRFRendererDGS  # noqa: E402
from synthetic import synth  # noqa: E402
from synthetic.model_stub import model_from_scene  # noqa: E402

NEW_KERNELS = ("point_inputs_bwd_kernel", "camg_ray_reduce_kernel", "camg_view_partial_kernel", "camg_view_final_kernel",
               "composite_bwd_far_kernel")


def main(NV=4, H=256, W=256, NR=4096, K=40, G=15, NC=1000, steps=5):
    dev = torch.device("cuda:0")
    sc = synth.make_scene(H, W, NV, seed=0, with_latent=False)
    h, w = sc.latent_hw
    latent = torch.randn((1, NV, 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1), device=dev, latent=latent)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G)
    rays = torch.from_numpy(sc.target_rays(crop=(H // 2 - 32, W // 2 - 32, 64, 64))).to(dev)
    assert rays.shape[1] == NR
    tgt = torch.rand((1, NR, 3), device=dev)
    cams = [m.poses, m.focal, m.c, m.image_shape, m.encoder.depths]

    def step(on):
        for t in list(m.mlp_fine.parameters()) + [m.encoder.latent, rays] + cams:
            t.grad = None
        rays.requires_grad_(on)
        for t in cams:
            t.requires_grad_(on)
        out = r(m, rays)
        ((out.fine.rgb - tgt) ** 2).mean().backward()

    res = {}
    for on in (False, True, False, True):      # interleaved: both sides see the same clocks
        times = []
        for i in range(steps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(on)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        key = "on" if on else "off"
        res[key] = min(res.get(key, 1e9), min(times[1:]))
    assert m.poses.grad is not None and rays.grad is not None
    kern = {}
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(True)
        torch.cuda.synchronize()
    for e in prof.key_averages():
        for k in NEW_KERNELS:
            if k in e.key:
                kern[k] = kern.get(k, 0.0) + e.device_time_total / 1e3    # ms (one step)
    print(json.dumps({"what": "training step (sampler + forward + backward), 4096 rays x 40 samples x %d views; camera gradients off / on" % NV,
                      "ms_per_step_off": res["off"] * 1e3, "ms_per_step_on": res["on"] * 1e3,
                      "overhead_pct": (res["on"] / res["off"] - 1) * 100, "new_kernels_ms": kern,
                      "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}))


if __name__ == "__main__":
    main()
