"""Time of a NOVEL training step's ``composite()`` + backward with the point model on the HIP training path
(diner_amd/novel.py ``train_hip_point_model``; diner_amd/training_novel.py, csrc/train_novel.hip) against the point model and its autograd
on PyTorch, one GPU, one process, one run, device events.

* the model: the NOVEL config's shape (d_hidden 512, 5 blocks, combine_layer 3, 6 frequencies, d_latent 512) as the stand-in of
  tests/novel_train_ref.py (the restated model with its graph kept), ``--views`` source views of ``--size`` x ``--size`` pixels,
  feature_padding 32, a ``gen_latent`` of [512, --gen-size, --gen-size] and one general camera; every fusion-MLP parameter,
  ``encoder.latent`` and ``gen_latent`` require grad;
* the work: 4096 rays x 40 samples, deformed by ``--vertices`` mesh vertices with both offset sets (part of every window: the same
  launches in all three), ``composite()``, the loss ``rgb c1 + depth c2 + weights c3`` with fixed cotangents, ``backward()``;
* three windows, alternated step by step so that what else runs on the host weighs on all alike: the HIP route in fp32, the HIP route
  in f16x3 (``train_f16x3_any_shape``), and the ``"torch"`` route, where the restated model runs in the reference's chunks of
  ``eval_batch_size`` points under torch's autograd.  Each HIP window carries the device-event split of the two new kernels
  (``diner_train_point_inputs_novel``, ``diner_train_novel_gen_scatter``; taken in steps of their own, outside the timed ones) and the
  bytes the autograd function keeps between forward and backward; the torch window the bytes its graph keeps.

The gradients of the three routes are compared with one another before anything is timed.  A record, not a gate: writes --out
(profiles/novel_train.json).

    python tools/bench_novel_train.py [--steps 7] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NR, K = 4096, 40
DIMS = dict(d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3, beta=0.0)


def stats(v, **kw):
    v = sorted(v)
    return dict(median_ms=float(v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])), min_ms=float(v[0]),
                max_ms=float(v[-1]), n=len(v), clock="device events", **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--gen-size", type=int, default=192)
    ap.add_argument("--vertices", type=int, default=26317)
    ap.add_argument("--rays", type=int, default=NR, help="a square number (the target image's pixels)")
    ap.add_argument("--eval-batch-size", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "novel_train.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from diner_amd.novel import NeRFRendererDGS
    from synthetic import synth
    from tests import knn_ref
    from tests import novel_point_ref as R
    from tests import novel_train_ref as TR
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")

    fp = 32
    side = int(round(a.rays ** 0.5))
    assert side * side == a.rays
    sc = synth.make_scene(a.size, a.size, a.views, seed=5, feature_padding=fp, with_latent=False)
    g = torch.Generator(device=dev).manual_seed(11)
    h = a.size // 2 + 2 * fp
    inp = {k: getattr(sc, k) for k in ("poses", "focal", "c", "image_shape", "depths", "depths_std", "normals")}
    inp["latent"] = np.zeros((1, a.views, 8, 1, 1), np.float32)           # replaced by a device tensor below
    inp["weights"] = synth.make_mlp_weights(6, bias_scale=0.1, d_in=55, **{k: v for k, v in DIMS.items() if k != "beta"})
    inp["gen_latent"] = np.zeros((8, 1, 1), np.float32)
    gW = gH = 2 * a.gen_size
    inp["gen_poses"] = synth.look_at_origin_w2c(0.3, 1.75)[None, None]
    inp["gen_focal"], inp["gen_c"] = np.array([[[1.2 * gW, 1.2 * gW]]], np.float32), np.array([[[gW / 2, gH / 2]]], np.float32)
    inp["gen_image_shape"] = np.array([gW, gH], np.float32)
    inp["cfg"] = dict(scene=dict(feature_padding=fp), num_freqs=6, index_interp="bilinear", index_padding="border")
    inp["dims"] = DIMS
    m = R.model_from_inputs(inp, device=dev)
    # the restated model with its graph kept; its cameras and maps as device tensors, so that the torch route copies nothing per call
    on_dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items() if isinstance(v, np.ndarray)}
    m.__class__, m.case_inputs = TR.TrainableNovelModel, dict(inp, **on_dev)
    m.encoder.latent = torch.randn((1, a.views, 512, h, h), generator=g, device=dev).requires_grad_(True)
    m.gen_latent = torch.nn.Parameter(torch.randn((512, a.gen_size, a.gen_size), generator=g, device=dev))
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    leaves = list(m.mlp_fine.parameters()) + [m.encoder.latent, m.gen_latent]

    rays = torch.from_numpy(np.ascontiguousarray(sc.target_rays(side, side))).to(dev)
    assert rays.shape[1] == a.rays
    z = (1.0 + 1.5 * (torch.arange(K, device=dev) + torch.rand((1, a.rays, K), generator=g, device=dev)) / K).contiguous()
    verts = torch.from_numpy(knn_ref.sphere_mesh(a.vertices, seed=3, radius=0.45, centre=(0.0, 0.0, 0.0)))[None].to(dev)
    o_in, o_gen = 0.03 * torch.randn(verts.shape, generator=g, device=dev), 0.03 * torch.randn(verts.shape, generator=g, device=dev)
    c_rgb, c_depth = torch.randn((1, a.rays, 3), generator=g, device=dev), torch.randn((1, a.rays), generator=g, device=dev)
    c_w = torch.randn((1, a.rays, K), generator=g, device=dev)

    def renderer(precision, on):
        r = NeRFRendererDGS(n_samples=K, eval_batch_size=a.eval_batch_size, hip_point_model=on, train_hip_point_model=on,
                            train_f16x3_any_shape=precision == "f16x3")
        r.precision = precision
        return r

    def forward(r):
        w, rgb, depth = r.composite(m, rays, z, verts, o_in, o_gen)
        return (rgb * c_rgb).sum() + (depth * c_depth).sum() + (w * c_w).sum()

    def step(r):
        for t in leaves:
            t.grad = None
        forward(r).backward()

    def timed(r):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(r)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def kept_bytes(r):
        """bytes allocated between the start of the forward and the start of the backward: what the route keeps for its backward"""
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        loss = forward(r)
        torch.cuda.synchronize()
        kept = torch.cuda.memory_allocated(dev) - before
        loss.backward()
        return int(kept)

    def kernel_split(r):
        """device-event times of the two new kernels in steps of their own (the events sit between launches of one stream)"""
        per = {}
        for _ in range(3):
            r.novel_train_events = []
            step(r)
            torch.cuda.synchronize()
            for name, e0, e1 in r.novel_train_events:
                per.setdefault(name, []).append(e0.elapsed_time(e1))
        r.novel_train_events = None
        return {name: stats(v, what="one launch") for name, v in per.items()}

    variants = {"hip_fp32": renderer("fp32", True), "hip_f16x3": renderer("f16x3", True), "torch_chunked": renderer("fp32", False)}
    results = {"device": torch.cuda.get_device_name(0), "rays": a.rays, "samples": K, "views": a.views, "image": a.size, "latent": [512, h, h],
               "gen_latent": [512, a.gen_size, a.gen_size], "vertices": a.vertices, "mlp": DIMS, "eval_batch_size": a.eval_batch_size,
               "steps": a.steps, "warmup": a.warmup, "what": "composite() + loss + backward(), every MLP parameter, encoder.latent and gen_latent "
               "requiring grad", "windows": {}}
    grads = {}
    for k, r in variants.items():        # results first: the three routes' gradients against one another
        step(r)
        results.setdefault("routes", {})[k] = r.last_route
        grads[k] = [t.grad.detach().clone() for t in leaves]
    rel = lambda x, y: float((x - y).norm() / y.norm())
    for k in ("hip_fp32", "hip_f16x3"):
        results[f"grad_rel_l2_{k}_vs_torch"] = dict(mlp_max=max(rel(x, y) for x, y in zip(grads[k][:-2], grads["torch_chunked"][:-2])),
                                                    latent=rel(grads[k][-2], grads["torch_chunked"][-2]),
                                                    gen_latent=rel(grads[k][-1], grads["torch_chunked"][-1]))
    del grads
    times = {k: [] for k in variants}
    for i in range(a.warmup + a.steps):  # alternating: one step of each route per round
        for k, r in variants.items():
            ms = timed(r)
            if i >= a.warmup:
                times[k].append(ms)
    for k, r in variants.items():
        rec = stats(times[k], route=r.last_route)
        rec["rays_per_s"] = a.rays / (rec["median_ms"] * 1e-3)
        rec["kept_for_backward_bytes"] = kept_bytes(r)
        if k != "torch_chunked":
            rec["new_kernels"] = kernel_split(r)
        results["windows"][k] = rec
        print(json.dumps({k: rec}), flush=True)
    t = results["windows"]["torch_chunked"]["median_ms"]
    results["torch_over_hip"] = {k: t / results["windows"][k]["median_ms"] for k in ("hip_fp32", "hip_f16x3")}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")
    print(json.dumps({kk: vv for kk, vv in results.items() if kk != "windows"}), flush=True)


if __name__ == "__main__":
    main()
