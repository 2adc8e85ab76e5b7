"""From a sample's image bytes on the host to the resized float images on the GPU, at the sizes the datasets ship with, on three routes
timed in the same run, alternating:

(i)   ``fused``:       the upload of the bytes and the resize kernels -- Multiface: wire.decode_multiface_image(.., size=) (decode +
                       horizontal pass, vertical pass + nearest alpha); DTU: wire.decode_dtu_rgb(.., downsample=.5) (the fixed-point
                       bicubic passes, then the decode of the small image);
(ii)  ``interpolate``: the upload of the bytes, wire.decode_image_u8 at full size, then F.interpolate on the device (bilinear with
                       antialias for Multiface and nearest for its alpha; for DTU bicubic with antialias on the decoded floats, which
                       is NOT PIL's fixed-point result: it stands for the cost of a float resize there);
(iii) ``host``:        what the dataset's reader does: float decode + resize on the CPU, then the upload of the small float images --
                       Multiface: the float32 steps of tests/wire_images_ref.py in torch, F.interpolate(antialias=True) and nearest; DTU:
                       PIL's Image.resize on the bytes, / 255.  PNG decoding is outside all three.

Shapes: ``multiface`` 5 images (four sources and the target) of 2048 x 1334 RGB + alpha plane -> 256 x 160 (downsample 8, multiples of
32); ``dtu`` 4 images of 512 x 640 RGB -> 256 x 320 (downsample .5).  Route times: the host clock around one whole route that ends in a
device synchronise, median / min / max of --steps after --warmup.  Kernel times alone: device events around --calls back-to-back calls
of (i) and (ii) on bytes already on the device.  Bytes each route moves on the device, from the shapes.  How far (i) is from (ii) and
(iii) is recorded before anything is timed.  A record, not a gate: writes --out (profiles/wire_resize.json).

    python tools/bench_wire_resize.py [--steps 20] [--warmup 3] [--calls 50] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SIZES = {"multiface": dict(N=5, H=2048, W=1334, h=256, w=160, plane=True), "dtu": dict(N=4, H=512, W=640, h=256, w=320, plane=False)}


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50, help="calls per device-event window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wire_resize.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as TF
    from diner_amd import wire
    from tests import wire_images_ref as R

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    F32 = torch.float32
    c = lambda v: torch.tensor(v, dtype=F32)

    def host_multiface(px, alpha, size):
        v = px.permute(0, 3, 1, 2).to(F32).div(c(255.0))
        t = v.mul(torch.tensor(R.GAMMA_SCALE, dtype=F32).view(1, 3, 1, 1)).div(c(1.1))
        t = t.sub(c(R.GAMMA_BLACK)).clamp(0, 2).mul(c(R.GAMMA_GAIN)).sqrt()
        v = t.sub(c(R.GAMMA_OFFSET)).clamp(0, 2).clamp(0, 1)
        al = alpha.to(F32).div(c(255.0)).unsqueeze(1)
        v = torch.where(al < 1.0, c(1.0), v)
        return (TF.interpolate(v, size=size, mode="bilinear", align_corners=False, antialias=True), TF.interpolate(al, size=size, mode="nearest"))

    def host_dtu(px, size):
        from PIL import Image
        small = np.stack([np.asarray(Image.fromarray(im).resize((size[1], size[0]))) for im in px.numpy()])
        return torch.from_numpy(small).permute(0, 3, 1, 2).to(F32).div(c(255.0))

    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, steps=a.steps, calls=a.calls, sizes={})
    for name, sz in SIZES.items():
        N, H, W, size = sz["N"], sz["H"], sz["W"], (sz["h"], sz["w"])
        rs = np.random.RandomState(7)
        px = torch.from_numpy(rs.randint(0, 256, (N, H, W, 3)).astype(np.uint8)).pin_memory()
        alpha = torch.from_numpy(rs.choice(np.array([0, 254, 255, 255], np.uint8), (N, H, W))).pin_memory() if sz["plane"] else None

        if name == "multiface":
            fused = lambda p, al: wire.decode_multiface_image(p, al, device=dev, size=size)

            def interp(p, al):
                rgb, al_f = wire.decode_multiface_image(p, al, device=dev)
                return (TF.interpolate(rgb, size=size, mode="bilinear", align_corners=False, antialias=True),
                        TF.interpolate(al_f, size=size, mode="nearest"))

            host = lambda: tuple(t.to(dev) for t in host_multiface(px, alpha, size))
        else:
            fused = lambda p, al: (wire.decode_dtu_rgb(p, downsample=.5, device=dev),)
            interp = lambda p, al: (TF.interpolate(wire.decode_dtu_rgb(p, device=dev), size=size, mode="bicubic", align_corners=False,
                                                   antialias=True),)
            host = lambda: (host_dtu(px, size).to(dev),)

        def timed(fn):
            def run():
                out = fn()
                torch.cuda.synchronize()
                return out
            return run

        up = lambda: (px.to(dev), None if alpha is None else alpha.to(dev))
        routes = {"fused": timed(lambda: fused(*up())), "interpolate": timed(lambda: interp(*up())), "host": timed(host)}
        first = {k: fn() for k, fn in routes.items()}
        agree = {k: float((first["fused"][0] - first[k][0]).abs().max()) for k in ("interpolate", "host")}
        if alpha is not None:
            agree["alpha_equal"] = bool(torch.equal(first["fused"][1], first["interpolate"][1]) and torch.equal(first["fused"][1], first["host"][1]))
        times = {k: [] for k in routes}
        for i in range(a.warmup + a.steps):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if i >= a.warmup:
                    times[k].append(dt * 1e3)

        dpx, dal = up()
        kernels = {"fused": lambda: fused(dpx, dal), "interpolate": lambda: interp(dpx, dal)}
        ktimes = {k: [] for k in kernels}
        for i in range(a.warmup + a.steps):
            for k, fn in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    ktimes[k].append(e0.elapsed_time(e1) / a.calls * 1e3)
        src = N * H * W * (3 + (1 if sz["plane"] else 0))
        small = N * size[0] * size[1]
        if name == "multiface":
            moved = dict(fused=src + 2 * N * 3 * H * size[1] * 4 + small * 4 * 4,                     # bytes in; tmp out and in; rgb + alpha out
                         interpolate=src + 2 * N * 4 * H * W * 4 + small * 4 * 4)                     # full-size floats out and in
        else:
            moved = dict(fused=src + 2 * N * H * size[1] * 3 + 2 * small * 3 + small * 3 * 4,         # u8 tmp and small image out and in; floats out
                         interpolate=src + 2 * N * 3 * H * W * 4 + small * 3 * 4)
        rec["sizes"][name] = dict(**sz, max_abs_difference_to_fused=agree, route_ms={k: stats(v) for k, v in times.items()},
                                  device_us={k: stats(v) for k, v in ktimes.items()}, device_bytes_moved=moved,
                                  uploaded=dict(fused=src, interpolate=src, host=small * (4 if sz["plane"] else 3) * 4))
        r = rec["sizes"][name]
        print(f"{name}: routes " + ", ".join(f"{k} {v['median']:.3f} ms" for k, v in r["route_ms"].items()) + "; on the device "
              + ", ".join(f"{k} {v['median']:.1f} us" for k, v in r["device_us"].items()) + f"; differences {agree}", flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
