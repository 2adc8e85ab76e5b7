"""Time of the encoder's tail -- the latent assembled from the ResNet's feature pyramid -- on one GPU, on the route the renderer had
before glue.assemble_latent and on the new kernels, at two sizes:

* ``cfg3``:  N = 4 views, levels of 64 / 64 / 128 / 256 channels at 320^2, 160^2, 80^2, 40^2 (a 512 x 512 source image, 0.84 GB latent);
* ``train``: the 4096-ray training scene of tools/bench_train.py (256 x 256 source images, 4 views: levels at 192^2 ... 24^2).

(a) ``nchw``:   forward = F.interpolate x L + torch.cat + diner_pack_latent; backward = diner_train_nhwc_to_nchw + autograd through cat
                and the interpolates, from the NHWC gradient buffer the training path's scatter fills;
(b) ``packed``: diner_assemble_latent; diner_assemble_latent_backward from the same buffer;
(c) one whole training step (assembly with grad + sampler + forward + backward down to the pyramid levels and the MLP parameters) on
    each route, the two alternating in one process.
Device-event times, median over --steps after --warmup.  A record, not a gate: writes --out (profiles/latent_assemble.json).

    python tools/bench_latent_assemble.py [--steps 10] [--warmup 3] [--train-steps 3] [--sizes cfg3,train] [--out FILE]

``--mode bicubic``: the tail of an encoder with upsample_interp="bicubic" at cfg3's pyramid, forward and backward, in one process, median
of 5 runs after 2 warm-ups (device events), with the number of device launches of each (torch.profiler's device events, taken after the
times):
``aten`` = the sequence the reference runs on the same GPU, F.interpolate(mode="bicubic", align_corners=True) per level + cat +
diner_pack_latent, and for the backward torch autograd of that sequence (the gradient arrives NCHW-strided: the transposed view of the
NHWC buffer goes through cat's backward as it is); ``packed`` = diner_assemble_latent_bicubic / _backward.  There is no earlier bicubic
path of this project to compare with.  Writes profiles/latent_assemble_bicubic.json.

    python tools/bench_latent_assemble.py --mode bicubic [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SIZES = {"cfg3": dict(res=512, NV=4), "train": dict(res=256, NV=4)}
PYRAMID = [(64, 1), (64, 2), (128, 4), (256, 8)]      # (channels, stride)


def bicubic(out_path):
    """--mode bicubic (see the module's docstring)"""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from diner_amd import _lib, glue
    from diner_amd._lib import check
    from synthetic import synth

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    STEPS, WARMUP = 5, 2

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        ms = []
        for _ in range(STEPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}

    def launches(fn):
        """device events (kernels and copies) of one call, as tools/bench_encoder_input.py counts them; raises when the profiler records
        none: a count of 0 is not a result"""
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower())
        if n == 0:
            raise RuntimeError("torch.profiler recorded no device events")
        return n

    res, NV = SIZES["cfg3"]["res"], SIZES["cfg3"]["NV"]
    sc = synth.make_scene(res, res, NV, seed=0, with_latent=False)
    h, w = sc.latent_hw
    g = torch.Generator(device=dev).manual_seed(1)
    levels = [torch.randn((NV, c, -(-h // s), -(-w // s)), device=dev, generator=g) for c, s in PYRAMID]
    Cc = sum(c for c, _ in PYRAMID)
    d_nhwc = torch.randn((1, NV, h, w, Cc), device=dev, generator=g)
    lat_bytes = d_nhwc.numel() * 4
    rec = {"device": torch.cuda.get_device_name(0), "steps": STEPS, "warmup": WARMUP, "size": "cfg3", "N": NV, "C": Cc, "h": h, "w": w,
           "latent_GB": lat_bytes / 1e9, "levels": [list(t.shape) for t in levels]}

    def upcat(lv):
        return torch.cat([F.interpolate(t, size=(h, w), mode="bicubic", align_corners=True) for t in lv], 1)

    def fwd_aten():
        with torch.no_grad():
            lat = upcat(levels)
            out = torch.empty((1, NV, h, w, Cc), dtype=torch.float32, device=dev)
            check(L.diner_pack_latent(p(lat), NV, Cc, h, w, p(out), st()), "diner_pack_latent")
        return out

    def fwd_packed():
        return glue.assemble_latent_bicubic(levels, 1, NV)

    lv_g = [t.clone().requires_grad_(True) for t in levels]
    lat_g = upcat(lv_g)               # the autograd graph of the ATen sequence, built once: its backward is what is timed
    d_view = d_nhwc[0].permute(0, 3, 1, 2)

    def bwd_aten():
        return torch.autograd.grad(lat_g, lv_g, d_view, retain_graph=True)

    shapes = [tuple(t.shape) for t in levels]

    def bwd_packed():
        return glue.assemble_latent_bicubic_backward(d_nhwc.permute(0, 1, 4, 2, 3), shapes)

    a, b = fwd_packed().permute(0, 1, 3, 4, 2), fwd_aten()
    rec["agreement"] = {"same_size_level_bit_identical": bool(torch.equal(a[..., :64], b[..., :64])),
                        "forward_max_abs_diff": float((a - b).abs().max()),
                        "backward_max_rel_diff": max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(bwd_packed(), bwd_aten()))}
    del a, b
    fns = (("forward_aten", fwd_aten), ("forward_packed", fwd_packed), ("backward_aten", bwd_aten), ("backward_packed", bwd_packed))
    for key, fn in fns:
        rec[key + "_ms"] = timed(fn)
    for key, fn in fns:               # after every time is taken: the profiler slows the host
        rec[key + "_launches"] = launches(fn)
    need = lat_bytes + sum(t.numel() * 4 for t in levels)     # every level read once + the latent written once (forward); the reverse
    rec["packed_GBps"] = {"forward": need / rec["forward_packed_ms"]["median"] / 1e6, "backward": need / rec["backward_packed_ms"]["median"] / 1e6}
    print(json.dumps(rec), flush=True)
    out = Path(out_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("bilinear", "bicubic"), default="bilinear")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=3)
    ap.add_argument("--sizes", default="cfg3,train")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "bicubic":
        return bicubic(a.out or str(ROOT / "profiles" / "latent_assemble_bicubic.json"))
    a.out = a.out or str(ROOT / "profiles" / "latent_assemble.json")

    import numpy as np
    import torch
    import torch.nn.functional as F
    from diner_amd import NeRFRendererDGS, _lib, glue
    from diner_amd._lib import check
    from synthetic import synth
    from synthetic.model_stub import model_from_scene

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    results = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "train_steps": a.train_steps, "sizes": {}}
    for name in a.sizes.split(","):
        res, NV = SIZES[name]["res"], SIZES[name]["NV"]
        sc = synth.make_scene(res, res, NV, seed=0, with_latent=False)
        h, w = sc.latent_hw
        g = torch.Generator(device=dev).manual_seed(1)
        levels = [torch.randn((NV, c, -(-h // s), -(-w // s)), device=dev, generator=g) for c, s in PYRAMID]
        Cc = sum(c for c, _ in PYRAMID)
        d_nhwc = torch.randn((1, NV, h, w, Cc), device=dev, generator=g)
        lat_bytes = d_nhwc.numel() * 4
        rec = {"N": NV, "C": Cc, "h": h, "w": w, "latent_GB": lat_bytes / 1e9, "levels": [list(t.shape) for t in levels]}

        def upcat(lv):
            return torch.cat([F.interpolate(t, size=(h, w), mode="bilinear", align_corners=True) for t in lv], 1)

        # ---- (a) / (b): the assembly alone, forward and backward ------------------------------------------------------------------
        def fwd_nchw():
            with torch.no_grad():
                lat = upcat(levels)
                out = torch.empty((1, NV, h, w, Cc), dtype=torch.float32, device=dev)
                check(L.diner_pack_latent(p(lat), NV, Cc, h, w, p(out), st()), "diner_pack_latent")
            return out

        def fwd_packed():
            return glue.assemble_latent(levels, 1, NV)

        lv_g = [t.clone().requires_grad_(True) for t in levels]
        lat_g = upcat(lv_g)               # the autograd graph of the parent route, built once: its backward is what is timed

        def bwd_nchw():
            d_lat = torch.empty((NV, Cc, h, w), dtype=torch.float32, device=dev)
            check(L.diner_train_nhwc_to_nchw(p(d_nhwc), NV, Cc, h, w, p(d_lat), st()), "diner_train_nhwc_to_nchw")
            return torch.autograd.grad(lat_g, lv_g, d_lat, retain_graph=True)

        shapes = [tuple(t.shape) for t in levels]

        def bwd_packed():
            return glue.assemble_latent_backward(d_nhwc.permute(0, 1, 4, 2, 3), shapes)

        same = torch.equal(fwd_packed().permute(0, 1, 3, 4, 2)[..., :64], fwd_nchw()[..., :64])     # the same-size level, bit for bit
        err = float((fwd_packed().permute(0, 1, 3, 4, 2) - fwd_nchw()).abs().max())
        gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(bwd_packed(), bwd_nchw()))
        rec["agreement"] = {"same_size_level_bit_identical": bool(same), "forward_max_abs_diff": err, "backward_max_rel_diff": gerr}
        for key, fn in (("forward_nchw_ms", fwd_nchw), ("forward_packed_ms", fwd_packed), ("backward_nchw_ms", bwd_nchw),
                        ("backward_packed_ms", bwd_packed)):
            med, lo, hi = timed(fn, a.steps, a.warmup)
            rec[key] = {"median": med, "min": lo, "max": hi}
        # bytes the algorithm needs: every level read once + the latent written once (forward); the reverse (backward)
        need = lat_bytes + sum(t.numel() * 4 for t in levels)
        rec["packed_GBps"] = {"forward": need / rec["forward_packed_ms"]["median"] / 1e6, "backward": need / rec["backward_packed_ms"]["median"] / 1e6}
        del lat_g, lv_g
        torch.cuda.empty_cache()

        # ---- (c): one whole training step on each route ----------------------------------------------------------------------------
        m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1), device=dev, latent=None)
        for q in m.mlp_fine.parameters():
            q.requires_grad_(True)
        lv_t = [t.clone().requires_grad_(True) for t in levels]
        rays = torch.from_numpy(sc.target_rays(crop=(res // 2 - 32, res // 2 - 32, 64, 64))).to(dev)
        tgt = torch.rand((1, rays.shape[1], 3), device=dev)
        r = NeRFRendererDGS(n_samples=40, n_depth_candidates=1000, n_gaussian=15)

        def step(route):
            for q in list(m.mlp_fine.parameters()) + lv_t:
                q.grad = None
            m.encoder.latent = glue.assemble_latent(lv_t, 1, NV) if route == "packed" else upcat(lv_t).reshape(1, NV, Cc, h, w)
            out = r(m, rays)
            ((out.fine.rgb - tgt) ** 2).mean().backward()
            m.encoder.latent = None

        ms = {"nchw": [], "packed": []}
        peak = {}
        for i in range(a.train_steps + 1):
            for route in ("nchw", "packed"):          # alternating, in one process
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(route)
                e1.record()
                e1.synchronize()
                if i:                                  # (the first round is the warm-up)
                    ms[route].append(e0.elapsed_time(e1))
                    peak[route] = torch.cuda.max_memory_allocated() / 1e9
        rec["train_step_ms"] = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}
        rec["train_step_peak_GB"] = peak
        rec["train_step"] = "assembly + sampler + forward + backward, %d rays x 40 samples x %d views, f16x3" % (rays.shape[1], NV)
        results["sizes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
        del m, lv_t, r, levels, d_nhwc
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
