"""Time from a rendered frame to its bytes and its scores (glue.frames_u8, glue.image_scores; diner_amd/csrc/frame_out.hip) on one GPU,
next to the route the reference takes on the same machine:

* ``prediction`` (create_prediction_folder, reference src/models/diner.py:120-133): ``torch_cmap`` -- ``.cpu()``, numpy in float64, the
  table lookup, the copy back (src/util/torch_helpers.py:63-74; the lookup is written with numpy here, matplotlib is not needed) -- then
  torchvision ``save_image``'s chain per image, ``mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)``, for the
  colour and the depth image.  Ours: one ``frames_u8(rgb, depth)`` and one device-to-host copy of the bytes each.
* ``sweep`` (create_cam_sweep, diner.py:194-214): per frame ``.cpu()`` and ``torch_cmap``, then stack, ``cat(dim=-2)``, and
  ``save_torch_video``'s ``(frames.permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)``.  Ours: ``frames_u8(.., rounding="video",
  stacked=True)`` and one copy.
* ``scores`` (evaluate_folder, src/evaluation/eval_suite.py:63-68): ours on the device; next to it the float64 restatement of
  tests/frame_out_ref.py on the CPU (numpy: l1, l2, psnr, ssim from integer sums -- a stand-in for skimage's CPU evaluation, which is
  not installed here), per image.

Sizes: 512 x 512 with N = 1 (a prediction) and N = 30 (a sweep), and 1024 x 1024 once.  Routes that end on the host are timed with the
host clock around a synchronise; the device-only calls (frames_u8, image_scores) with device events over windows of --calls back-to-back
calls; median / min / max over --steps windows after --warmup, one process.  The baseline is the reference's route, never our own code.
A record, not a gate: writes --out (profiles/frame_out.json).

    python tools/bench_frame_out.py [--steps 20] [--warmup 3] [--calls 50] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50, help="calls per device-event window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_out.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from diner_amd import glue
    from tests import frame_out_ref as R

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    table = glue._cmap_table("viridis")[1].numpy()

    def stats(v, **kw):
        return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), **kw)

    def device_ms(fn):
        """ms per call: windows of --calls back-to-back calls between two device events"""
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1) / a.calls)
        return stats(ms, clock="device events", calls_per_window=a.calls)

    def host_ms(fns, steps):
        """{name: ms per call}: the host clock around one call that ends on the host; the routes alternate call by call"""
        ms = {k: [] for k in fns}
        for i in range(a.warmup + steps):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        return {k: stats(v, clock="host, synchronised") for k, v in ms.items()}

    def reference_cmap(x):
        """torch_cmap's route: to the host, float64, min / max, normalise, the table lookup, back to the device"""
        dev_, shape = x.device, x.shape
        x = x.view(*[1 for i in range(4 - len(x.shape))], *x.shape)
        v = x.detach().cpu().numpy().astype(float)
        vmin = np.min(v.reshape(v.shape[0], -1), axis=-1).reshape((-1, 1, 1, 1))
        vmax = np.max(v.reshape(v.shape[0], -1), axis=-1).reshape((-1, 1, 1, 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            xa = ((v - vmin) / (vmax - vmin))[:, 0] * 256
            xa[xa == 256] = 255
            under, over, bad = xa < 0, xa >= 256, np.isnan(xa)
            idx = np.where(bad, 0, xa).astype(int)
        idx[under], idx[over], idx[bad] = 256, 257, 258
        return torch.from_numpy(table[idx]).permute(0, 3, 1, 2).reshape(list(shape[:-3]) + [3] + list(shape[-2:])).to(dev_)

    def save_image_bytes(img):
        return img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)

    results = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "sizes": {}}
    g = torch.Generator(device=dev).manual_seed(1)
    for N, S in ((1, 512), (30, 512), (1, 1024)):
        rgb = torch.rand((N, 3, S, S), device=dev, generator=g)
        depth = 0.5 + 2.0 * torch.rand((N, 1, S, S), device=dev, generator=g)
        gt = (rgb + 0.05 * torch.randn(rgb.shape, device=dev, generator=g)).clamp(0, 1)

        def ref_prediction():
            d = reference_cmap(depth)
            return [(save_image_bytes(rgb[i]), save_image_bytes(d[i])) for i in range(N)]

        def our_prediction():
            c, d = glue.frames_u8(rgb, depth)
            return c.cpu(), d.cpu()

        def ref_sweep():
            rgbs = torch.stack([rgb[i].cpu() for i in range(N)])
            depths = torch.stack([reference_cmap(depth[i].cpu()) for i in range(N)])
            frames = torch.cat((rgbs, depths), dim=-2)
            return (frames.permute(0, 2, 3, 1).detach().cpu().numpy() * 255).astype(np.uint8)

        def our_sweep():
            return glue.frames_u8(rgb, depth, rounding="video", stacked=True).cpu()

        # the routes agree before they are timed
        rp, op = ref_prediction(), our_prediction()
        same = all(torch.equal(rp[i][0], op[0][i]) and torch.equal(rp[i][1], op[1][i]) for i in range(N))
        same_sweep = bool(np.array_equal(ref_sweep(), our_sweep().numpy()))
        pred_u8, gt_u8 = glue.frames_u8(rgb), glue.frames_u8(gt)
        host_steps = a.steps if N * S * S <= 1 << 20 else max(a.steps // 4, 3)
        rec = {"N": N, "H": S, "W": S, "bytes_agree": {"prediction": bool(same), "sweep": same_sweep},
               "to_host_ms": {"prediction": host_ms({"reference": ref_prediction, "ours": our_prediction}, host_steps),
                              "sweep": host_ms({"reference": ref_sweep, "ours": our_sweep}, host_steps)},
               "device_ms": {"frames_u8_save_image": device_ms(lambda: glue.frames_u8(rgb, depth)),
                             "frames_u8_video_stacked": device_ms(lambda: glue.frames_u8(rgb, depth, rounding="video", stacked=True)),
                             "torch_cmap": device_ms(lambda: glue.torch_cmap(depth)),
                             "image_scores": device_ms(lambda: glue.image_scores(pred_u8, gt_u8))},
               # what the kernels must move: frames_u8 reads 4 floats and writes 6 bytes per pixel, image_scores reads 6 bytes per pixel
               "bytes_moved": {"frames_u8": N * S * S * (4 * 4 + 6), "image_scores": N * S * S * 6}}
        p1, g1 = pred_u8[:1].cpu().numpy(), gt_u8[:1].cpu().numpy()
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref_scores = R.image_scores_ref(p1, g1)
            cpu.append((time.perf_counter() - t0) * 1e3)
        ours = glue.image_scores(pred_u8[:1], gt_u8[:1])
        rec["scores_cpu_restatement_ms_per_image"] = stats(cpu, clock="host", threads=torch.get_num_threads())
        rec["scores_abs_diff_to_restatement"] = {k: float(abs(float(ours[k][0]) - float(ref_scores[k][0]))) for k in ref_scores}
        results["sizes"][f"N{N}_{S}x{S}"] = rec
        print(json.dumps({f"N{N}_{S}x{S}": rec}), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
