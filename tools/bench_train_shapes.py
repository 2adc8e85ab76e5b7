#!/usr/bin/env python3
"""Training-step timing of the shape-general training path (diner_amd/training_gen.py), on tools/bench_train.py's batch (4096 rays
x 40 samples, n_gaussian 15, 1000 candidates, 4 views): forward with saved activations + backward, sampler included.  Three runs:
  case_a             d_hidden 128, 5 blocks, combine_layer 3, ReLU (tools/gen_trainshape_golden.py case (a)) through train_any_shape;
  standard_gen       the standard shape forced through the new path (renderer._force_gen_train);
  standard_fp32      the standard shape on the existing training path with precision "fp32" (the same fp32 MFMA rate).
Prints one JSON line.  Not a gate: a figure to record."""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from diner_amd import NeRFRendererDGS  # noqa: E402
from synthetic import synth  # noqa: E402
from synthetic.model_stub import model_from_scene  # noqa: E402


def mlp_flop(NR, K, NV, d_in=55, C=512, H=512, n_blocks=5, combine_layer=3):
    """forward + 2x backward FLOP of the fusion MLP's GEMMs for one batch"""
    nlz = min(combine_layer, n_blocks)
    per_view = d_in * H + nlz * C * H + min(combine_layer, n_blocks) * 2 * H * H
    per_point = (n_blocks - min(combine_layer, n_blocks)) * 2 * H * H + 4 * H
    return 3 * 2 * NR * K * (NV * per_view + per_point)


def run(dims, mode, NV=4, H=256, W=256, NR=4096, K=40, G=15, NC=1000, steps=3):
    dev = torch.device("cuda:0")
    sc = synth.make_scene(H, W, NV, seed=0, with_latent=False)
    h, w = sc.latent_hw
    latent = torch.randn((1, NV, 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1, **{k: v for k, v in dims.items() if k != "beta"}), device=dev,
                         latent=latent, **dims)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, train_any_shape=True)
    r.precision = "fp32"
    r._force_gen_train = mode == "gen"
    rays = torch.from_numpy(sc.target_rays(crop=(H // 2 - 32, W // 2 - 32, 64, 64))).to(dev)
    assert rays.shape[1] == NR
    tgt = torch.rand((1, NR, 3), device=dev)
    times = []
    for i in range(steps + 1):
        for p in m.mlp_fine.parameters():
            p.grad = None
        m.encoder.latent.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = r(m, rays)
        loss = ((out.fine.rgb - tgt) ** 2).mean()
        loss.backward()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = min(times[1:])
    full = dict(d_hidden=512, n_blocks=5, combine_layer=3)
    full.update(dims)
    flop = mlp_flop(NR, K, NV, C=512, H=full["d_hidden"], n_blocks=full["n_blocks"], combine_layer=full["combine_layer"])
    res = {"ms_per_step": round(t * 1e3, 2), "mlp_tflop_per_step": round(flop / 1e12, 3), "mlp_tflops": round(flop / t / 1e12, 2),
           "route": r.last_route or "standard", "mlp_grad_norm": float(sum(float(p.grad.norm()) ** 2 for p in m.mlp_fine.parameters()) ** 0.5),
           "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    del out, loss, m, r
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def main():
    out = {"what": "training step (sampler + forward + backward), 4096 rays x 40 samples x 4 views, fp32"}
    out["case_a"] = run(dict(d_hidden=128, n_blocks=5, combine_layer=3), "any_shape")
    out["standard_gen"] = run({}, "gen")
    out["standard_fp32"] = run({}, "standard")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
