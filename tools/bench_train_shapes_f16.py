#!/usr/bin/env python3
"""Training-step timing of the shape-general training path with renderer.train_f16x3_any_shape off (exact fp32, diner_train_gemm_act)
and on (f16x3, csrc/train_gen_f16.hip), on tools/bench_train.py's batch (4096 rays x 40 samples, n_gaussian 15, 1000 candidates,
4 views): sampler + forward with saved activations + backward, 2 warm-up steps, median and min / max of 5 timed steps (thin for a
median: the figures resolve gaps of tens of percent, not of a few).  Cases:
  case_a          d_hidden 128, 5 blocks, combine_layer 3, ReLU;
  wide_f4         d_hidden 512 with num_freqs 4 (a wide non-standard shape);
  standard_gen    the standard shape forced through the path (renderer._force_gen_train), next to
  standard_f16x3  the standard path's own f16x3 step.
Then the per-GEMM rate of 655,360 x 512 x 512 forward / dX / dW (algorithmic TFLOP/s) for the fp32 and the f16x3 kernels.
Prints one JSON line.  Not a gate: figures to record (profiles/train_shapes_f16.json)."""
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from diner_amd import NeRFRendererDGS, _lib  # noqa: E402
from diner_amd.training import EXP_ACT, EXP_W  # noqa: E402
from diner_amd.training_gen import SplitWeight  # noqa: E402
from synthetic import synth  # noqa: E402
from synthetic.model_stub import model_from_scene  # noqa: E402


def step_ms(dims, mode, f16, NV=4, H=256, W=256, NR=4096, K=40, G=15, NC=1000, warmup=2, steps=5):
    dev = torch.device("cuda:0")
    sc = synth.make_scene(H, W, NV, seed=0, with_latent=False)
    h, w = sc.latent_hw
    latent = torch.randn((1, NV, 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    wdims = {k: v for k, v in dims.items() if k not in ("beta", "num_freqs")}
    if "num_freqs" in dims:
        wdims["d_in"] = 7 + 8 * dims["num_freqs"]
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1, **wdims), device=dev, latent=latent, **dims)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, train_any_shape=True, train_f16x3_any_shape=f16)
    r.precision = "f16x3" if (f16 or mode == "standard") else "fp32"
    r._force_gen_train = mode == "gen"
    rays = torch.from_numpy(sc.target_rays(crop=(H // 2 - 32, W // 2 - 32, 64, 64))).to(dev)
    tgt = torch.rand((1, NR, 3), device=dev)
    times = []
    for i in range(warmup + steps):
        for p in m.mlp_fine.parameters():
            p.grad = None
        m.encoder.latent.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = r(m, rays)
        ((out.fine.rgb - tgt) ** 2).mean().backward()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    t = times[warmup:]
    res = {"ms_median": round(statistics.median(t), 2), "ms_min": round(min(t), 2), "ms_max": round(max(t), 2),
           "route": r.last_route or "standard", "precision": r.effective_precision or r.precision,
           "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
    del out, m, r
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def gemm_rates(M=655360, N=512, K=512, reps=5):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    X, dY, W = torch.randn(M, K, device=dev), torch.randn(M, N, device=dev), torch.randn(N, K, device=dev) / 22.0
    Y, dX, dW = torch.empty(M, N, device=dev), torch.empty(M, K, device=dev), torch.zeros(N, K, device=dev)
    amax = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(L.diner_train_amax(p(dY), dY.numel(), p(amax), st), "amax")
    sw, swt = SplitWeight(W, False), SplitWeight(W, True)
    R, SP = _lib.ACT_RELU, _lib.ACT_NONE
    calls = {
        "fp32_fwd": lambda: L.diner_train_gemm_act(p(X), p(W), None, None, p(Y), M, N, K, K, 1, 1, K, N, 0, R, 0, 0, 1.0, 0, 0, 0, st),
        "fp32_dx": lambda: L.diner_train_gemm_act(p(dY), p(W), None, p(X), p(dX), M, K, N, N, 1, K, 1, K, K, 0, 0, R, 1.0, 0, 0, 0, st),
        "fp32_dw": lambda: L.diner_train_gemm_act(p(dY), p(X), None, None, p(dW), N, K, M, 1, N, K, 1, K, 0, 0, R, 0, 1.0, 0, 1, 4096, st),
        "f16x3_fwd": lambda: L.diner_train_gemm_act_f16x3_w(p(X), K, p(sw.hi), p(sw.lo), None, None, 0, p(Y), N, M, N, K, R, 0, 1.0, 0, None,
                                                            EXP_ACT, EXP_W, st),
        "f16x3_dx": lambda: L.diner_train_gemm_act_f16x3_w(p(dY), N, p(swt.hi), p(swt.lo), None, p(X), K, p(dX), K, M, K, N, 0, R, 1.0, 0,
                                                           p(amax), 0, EXP_W, st),
        "f16x3_dw": lambda: L.diner_train_gemm_act_f16x3(p(dY), p(X), None, None, p(dW), N, K, M, 1, N, K, 1, K, 0, 0, R, 0, 1.0, 0, 1, 4096,
                                                         p(amax), None, 0, EXP_ACT, st),
        "f16x3_fwd_streamed_weight": lambda: L.diner_train_gemm_act_f16x3(p(X), p(W), None, None, p(Y), M, N, K, K, 1, 1, K, N, 0, R, 0, 0, 1.0,
                                                                          0, 0, 0, None, None, EXP_ACT, EXP_W, st),
    }
    out = {}
    for name, fn in calls.items():
        _lib.check(fn(), name)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn(), name)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = statistics.median(ts)
        out[name] = {"ms": round(ms, 3), "tflops": round(2.0 * M * N * K / ms / 1e9, 1)}
    return out


def main():
    out = {"what": "training step (sampler + forward + backward), 4096 rays x 40 samples x 4 views; train_f16x3_any_shape off / on"}
    for name, dims, mode in (("case_a", dict(d_hidden=128, n_blocks=5, combine_layer=3), "any_shape"), ("wide_f4", dict(num_freqs=4), "any_shape"),
                             ("standard_gen", {}, "gen")):
        out[name] = {"off_fp32": step_ms(dims, mode, False), "on_f16x3": step_ms(dims, mode, True)}
    out["standard_f16x3"] = step_ms({}, "standard", False)
    out["gemm_655360x512x512"] = gemm_rates()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
