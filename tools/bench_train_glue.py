"""Time of a training step's glue around the renderer -- ray selection before it, the photometric losses after it (reference
DINER.calc_losses, src/models/diner.py:217-290) -- forward + backward on one GPU, on two routes:

(a) ``parent``: glue.gen_rays for the whole image + the advanced index (diner.py:258), then the ATen loss sequence: view / permute /
                advanced index of the target (:265), MSELoss (:267), two view / permute pairs, AvgPool2d x 2 and L1Loss (:280-282);
(b) ``kernel``: glue.gen_rays_at + glue.photo_loss.

Sizes: SB = 1 and SB = 4 target images of 512 x 512, a 64 x 64 patch (4096 rays per scene), antibias_downsampling = 3.  ``pred`` always
requires grad (it is the renderer's output); the target camera requires grad only in the ``cams_learned`` rows (then the parent's backward
scatters into a zero-filled [SB, H*W, 8] gradient and reduces all of it).  (c) one whole step in the manner of tools/bench_train.py (its
scene: 4 views of 256 x 256, 4096 rays x 40 samples) on each route: rays -> renderer.forward -> losses -> backward.
Device-event times: a window is --calls back-to-back calls of one route between two events (per-call time = window / calls), the two
routes alternate window by window in one process, median / min / max over --steps windows after --warmup windows each.  Launch counts
come from torch.profiler and slow the host: they are taken with --launches only, in a run of their own (no times then).  A record, not a
gate: writes --out (profiles/train_glue.json, or profiles/train_glue_launches.json with --launches).

    python tools/bench_train_glue.py [--steps 20] [--warmup 3] [--calls 200] [--out FILE]
    python tools/bench_train_glue.py --launches
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

RES, PATCH, N_DOWN, W_AB = 512, 64, 3, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--launches", action="store_true", help="count device launches with torch.profiler instead of timing")
    ap.add_argument("--no-step", action="store_true", help="skip (c), the whole training step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("train_glue_launches.json" if a.launches else "train_glue.json"))

    import numpy as np
    import torch
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    from synthetic.model_stub import model_from_scene

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    pool = torch.nn.AvgPool2d(kernel_size=2 ** N_DOWN, stride=2 ** N_DOWN)

    def patch_indices(SB, H, W, s):
        ys, xs = torch.meshgrid(torch.arange(s, device=dev), torch.arange(s, device=dev), indexing="ij")
        return ((W // 2 - s // 2 + xs) + (H // 2 - s // 2 + ys) * W).reshape(1, -1).expand(SB, -1).contiguous()

    def parent_rays(E, K, W, H, zn, zf, idx):
        SB, B = idx.shape
        helper = torch.arange(SB, device=dev).unsqueeze(-1).expand(-1, B)
        return glue.gen_rays(E, K, W, H, zn, zf).view(SB, H * W, -1)[helper, idx]

    def parent_losses(pred, target, idx, s):
        SB, B = idx.shape
        helper = torch.arange(SB, device=dev).unsqueeze(-1).expand(-1, B)
        gt = target.view(SB, 3, -1).permute(0, 2, 1)[helper, idx]
        mse = torch.nn.functional.mse_loss(pred, gt)
        ab = torch.nn.functional.l1_loss(pool(pred.view(SB, s, s, 3).permute(0, 3, 1, 2)), pool(gt.view(SB, s, s, 3).permute(0, 3, 1, 2)))
        return mse, ab, gt

    def kernel_losses(pred, target, idx, s):
        return glue.photo_loss(pred, target, idx, patch=s, antibias_downsampling=N_DOWN)

    def timed_pair(fns, calls):
        """{name: ms per call}: windows of `calls` calls, the routes alternating window by window"""
        ms = {k: [] for k in fns}
        for i in range(a.warmup + a.steps):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1) / calls)
        return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "calls_per_window": calls} for k, v in ms.items()}

    def launches(fn):
        """device kernels of one call (raises when the profiler records no device events: a count of 0 is not a result)"""
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower())
        if n == 0:
            raise RuntimeError("torch.profiler recorded no device events")
        return n

    results = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "calls": a.calls, "H": RES, "W": RES,
               "patch": PATCH, "antibias_downsampling": N_DOWN, "sizes": {}}
    g = torch.Generator(device=dev).manual_seed(1)
    for SB in (1, 4):
        H = W = RES
        E = torch.eye(4, device=dev).expand(SB, 4, 4).contiguous()
        E[:, :3, 3] = torch.randn((SB, 3), device=dev, generator=g)
        K = torch.tensor([[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]], device=dev).expand(SB, 3, 3).contiguous()
        zn, zf = torch.full((SB,), 0.5, device=dev), torch.full((SB,), 2.5, device=dev)
        idx = patch_indices(SB, H, W, PATCH)
        target = torch.rand((SB, 3, H, W), device=dev, generator=g)
        pred = torch.rand((SB, PATCH * PATCH, 3), device=dev, generator=g).requires_grad_(True)
        cot = torch.randn((SB, PATCH * PATCH, 8), device=dev, generator=g)
        E_learned = E.clone().requires_grad_(True)

        def glue_step(rays_fn, loss_fn, Ecam):
            def run():
                rays = rays_fn(Ecam, K, W, H, zn, zf, idx)
                if rays.requires_grad:
                    rays.backward(cot)
                    Ecam.grad = None
                mse, ab, _ = loss_fn(pred, target, idx, PATCH)
                (mse + W_AB * ab).backward()
                pred.grad = None
            return run

        with torch.no_grad():
            rp, rk = parent_rays(E, K, W, H, zn, zf, idx), glue.gen_rays_at(E, K, W, H, zn, zf, idx)
            lp, lk = parent_losses(pred, target, idx, PATCH), kernel_losses(pred, target, idx, PATCH)
        rec = {"SB": SB, "rays": SB * PATCH * PATCH,
               "agreement": {"rays_bit_identical": bool(torch.equal(rp, rk)), "gt_colors_bit_identical": bool(torch.equal(lp[2], lk[2])),
                             "mse_abs_diff": abs(float(lp[0]) - float(lk[0])), "antibias_abs_diff": abs(float(lp[1]) - float(lk[1]))}}
        routes = {"cams_fixed": {"parent": glue_step(parent_rays, parent_losses, E), "kernel": glue_step(glue.gen_rays_at, kernel_losses, E)},
                  "cams_learned": {"parent": glue_step(parent_rays, parent_losses, E_learned),
                                   "kernel": glue_step(glue.gen_rays_at, kernel_losses, E_learned)}}
        for row, fns in routes.items():
            if a.launches:
                rec.setdefault("launches", {})[row] = {k: launches(fn) for k, fn in fns.items()}
            else:
                rec.setdefault("glue_fwd_bwd_ms", {})[row] = timed_pair(fns, a.calls)
        results["sizes"][f"SB{SB}"] = rec
        print(json.dumps({f"SB{SB}": rec}), flush=True)

    # ---- (c) one whole training step on tools/bench_train.py's scene, each route ------------------------------------------------------
    if not a.launches and not a.no_step:
        NV, H, W, K_s, G, NC = 4, 256, 256, 40, 15, 1000
        sc = synth.make_scene(H, W, NV, seed=0, with_latent=False)
        h, w = sc.latent_hw
        latent = torch.randn((1, NV, 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1), device=dev, latent=latent)
        for p in m.mlp_fine.parameters():
            p.requires_grad_(True)
        m.encoder.latent.requires_grad_(True)
        r = NeRFRendererDGS(n_samples=K_s, n_depth_candidates=NC, n_gaussian=G)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        E, K = t(sc.target_extrinsics)[None], t(sc.target_intrinsics)[None]
        zn, zf = torch.tensor([sc.near], device=dev), torch.tensor([sc.far], device=dev)
        idx = patch_indices(1, H, W, PATCH)
        target = torch.rand((1, 3, H, W), device=dev, generator=g)

        def step(rays_fn, loss_fn):
            def run():
                for p in m.mlp_fine.parameters():
                    p.grad = None
                m.encoder.latent.grad = None
                pred = r(m, rays_fn(E, K, W, H, zn, zf, idx)).fine.rgb
                mse, ab, _ = loss_fn(pred, target, idx, PATCH)
                (mse + W_AB * ab).backward()
            return run

        results["train_step_ms"] = timed_pair({"parent": step(parent_rays, parent_losses), "kernel": step(glue.gen_rays_at, kernel_losses)},
                                              max(a.calls // 40, 1))
        results["train_step"] = {"NV": NV, "H": H, "W": W, "rays": PATCH * PATCH, "n_samples": K_s, "n_gaussian": G, "n_depth_candidates": NC}
        print(json.dumps({"train_step_ms": results["train_step_ms"]}), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
