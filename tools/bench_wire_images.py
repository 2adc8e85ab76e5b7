"""From a sample's image bytes on the host to conv1's input on the GPU, per dataset at the size of its configuration, on two routes:

(a) ``reference``: a host reader's arithmetic in torch on the CPU (bytes / 255, the gamma steps, the background fill: the float32 steps of
                   tests/wire_images_ref.py, one torch operation each; PNG decoding is outside both routes), the upload of the float32
                   images, glue.encoder_input;
(b) ``bytes``:     the upload of the bytes, glue.encoder_input(bytes, image_format=..) -- one launch of diner_encoder_input_u8.

Sizes (N source views of H x W, image_padding 64, padding_pe 4 as configs/train_diner_facescape.yaml and train_dtu.yaml have them):
``facescape`` 2 x 256 x 256 RGBA; ``dtu`` 4 x 256 x 320 RGB (512 x 640 at downsample 0.5); ``multiface`` 4 x 256 x 160 RGB + an alpha plane
(2048 x 1334 at downsample 8, cut to a multiple of 32).

Route times: the host clock around one whole route that ends in a device synchronise, the two routes alternating, median / min / max of
--steps after --warmup.  Kernel times alone, with device events around --calls back-to-back launches: diner_decode_image_u8,
diner_encoder_input_u8 and diner_encoder_input (on the decoded floats), alternating window by window.  Bytes each needs, from the shapes:
the kernel reads N H W (C + plane) bytes where the float route uploads and reads N 3 H W 4.  A record, not a gate: writes --out
(profiles/wire_images.json).

    python tools/bench_wire_images.py [--steps 20] [--warmup 3] [--calls 200] [--out FILE]
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

SIZES = {"facescape": dict(N=2, H=256, W=256, C=4, plane=False), "dtu": dict(N=4, H=256, W=320, C=3, plane=False),
         "multiface": dict(N=4, H=256, W=160, C=3, plane=True)}
PAD, FREQS = 64, 4


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200, help="launches per device-event window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wire_images.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from diner_amd import glue, wire
    from tests import wire_images_ref as R

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    formats = dict(facescape=wire.FACESCAPE_RGBA, dtu=wire.DTU_RGB, multiface=wire.MULTIFACE_RGB)
    F32 = torch.float32
    c = lambda v: torch.tensor(v, dtype=F32)          # a python double rounded once to float32, as it is when it meets a float32 tensor

    def unit(b):
        return b.to(F32).div(c(255.0))

    def gamma(v):
        """tests/wire_images_ref.py's steps 2.1 - 2.6 in torch, one float32 operation each: v [N,3,H,W]"""
        t = v.mul(torch.tensor(R.GAMMA_SCALE, dtype=F32).view(1, 3, 1, 1)).div(c(1.1))
        t = t.sub(c(R.GAMMA_BLACK)).clamp(0, 2)
        t = t.mul(c(R.GAMMA_GAIN)).sqrt()
        return t.sub(c(R.GAMMA_OFFSET)).clamp(0, 2).clamp(0, 1)

    def readers(name, px, alpha):
        """what a host reader computes from the decoded PNG's bytes, in torch on the CPU: [N,H,W,C] uint8 (, [N,H,W]) -> [N,3,H,W] float32"""
        rule, bg, with_gamma = R.FORMATS[name]
        v = unit(px[..., :3].permute(0, 3, 1, 2))
        if with_gamma:
            v = gamma(v)
        if rule == "none":
            return v.contiguous()
        a = unit(alpha if alpha is not None else px[..., 3]).unsqueeze(1)
        return torch.where(a < (0.5 if rule == "below_half" else 1.0), c(bg), v)

    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, pad=PAD, padding_pe=FREQS, steps=a.steps, calls=a.calls, sizes={})
    for name, sz in SIZES.items():
        N, H, W, Cc = sz["N"], sz["H"], sz["W"], sz["C"]
        rs = np.random.RandomState(7)
        px = torch.from_numpy(rs.randint(0, 256, (N, H, W, Cc)).astype(np.uint8)).pin_memory()
        alpha = torch.from_numpy(rs.choice(np.array([0, 128, 255], np.uint8), (N, H, W))).pin_memory() if sz["plane"] else None
        fmt = formats[name]

        def route_reference():
            x = glue.encoder_input(readers(name, px, alpha).to(dev), PAD, FREQS)
            torch.cuda.synchronize()
            return x

        def route_bytes():
            x = glue.encoder_input(px.to(dev), PAD, FREQS, alpha=None if alpha is None else alpha.to(dev), image_format=fmt)
            torch.cuda.synchronize()
            return x

        # how far the two routes agree, recorded before either is timed (expected: bit-equal, unless the CPU's float32 root is not the
        # correctly rounded one: then one ulp of the root carried through Normalize)
        ra, rb = route_reference(), route_bytes()
        differ = float((ra != rb).float().mean())
        maxdiff = float((ra - rb).abs().max())
        routes = {"reference": route_reference, "bytes": route_bytes}
        times = {k: [] for k in routes}
        for i in range(a.warmup + a.steps):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if i >= a.warmup:
                    times[k].append(dt * 1e3)

        dpx, dal = px.to(dev), None if alpha is None else alpha.to(dev)
        rgb = wire.decode_image_u8(dpx, dal, fmt, device=dev)[0]
        kernels = {"decode_image_u8": lambda: wire.decode_image_u8(dpx, dal, fmt, device=dev),
                   "encoder_input_u8": lambda: glue.encoder_input(dpx, PAD, FREQS, alpha=dal, image_format=fmt),
                   "encoder_input_f32": lambda: glue.encoder_input(rgb, PAD, FREQS)}
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
        src_bytes = N * H * W * (Cc + (1 if sz["plane"] else 0))
        out_bytes = N * (3 + 2 * (1 + 2 * FREQS)) * (H + 2 * PAD) * (W + 2 * PAD) * 4
        rec["sizes"][name] = dict(
            **sz, routes_agree=dict(share_of_entries_that_differ=differ, max_abs_difference=maxdiff),
            route_ms={k: stats(v) for k, v in times.items()}, kernel_us={k: stats(v) for k, v in ktimes.items()},
            bytes=dict(uploaded_bytes_route=src_bytes, uploaded_reference_route=N * 3 * H * W * 4, encoder_input_written=out_bytes,
                       decode_read=src_bytes, decode_written=N * (3 + (1 if Cc == 4 or sz["plane"] else 0)) * H * W * 4))
        r = rec["sizes"][name]
        print(f"{name}: route reference {r['route_ms']['reference']['median']:.3f} ms, bytes {r['route_ms']['bytes']['median']:.3f} ms; kernels "
              + ", ".join(f"{k} {v['median']:.1f} us" for k, v in r["kernel_us"].items()), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
