"""Time of the encoder's head -- conv1's input: normalise, replicate pad, the padding's positional encoding -- on one GPU, on the ATen
sequence of the reference (src/models/pixelnerf.py:44, src/models/image_encoder.py:222-232) and on glue.encoder_input, at two sizes:

* ``cfg3``:  N = 4 views of 512 x 512, image_padding 64, padding_pe 4 -> [4, 21, 640, 640] (138 MB);
* ``train``: the training scene of tools/bench_train.py (N = 4 views of 256 x 256) -> [4, 21, 384, 384].

(a) ``aten``:   Normalize, ReplicationPad2d, linspace x 2, meshgrid, stack, PositionalEncoding (repeat, addcmul, sin, cat), the interior's
                zero fill, expand, cat -- restated here in torch on the same inputs;
(b) ``kernel``: diner_encoder_input;
(c) one whole encode on synthetic/encoder_stub.py's small trunk: glue.encode against the hand-subclassed route INTEGRATION.md described
    before it (the ATen head, the trunk, glue.assemble_latent; glue.depth2normal on both).
Device-event times: a window is --calls back-to-back calls of one variant between two events (per-call time = window / calls), the two
variants of a pair alternate window by window in one process, median / min / max over --steps windows after --warmup windows each.
Bytes the kernel needs: N (3 + Cpe) Hp Wp 4 written + N 3 H W 4 read.  Launch counts come from torch.profiler and slow the host: they are
taken only with --launches, in a run of their own (no times are recorded then).  A record, not a gate: writes --out
(profiles/encoder_input.json, or profiles/encoder_input_launches.json with --launches).

    python tools/bench_encoder_input.py [--steps 20] [--warmup 3] [--calls 200] [--sizes cfg3,train] [--out FILE]
    python tools/bench_encoder_input.py --launches
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SIZES = {"cfg3": dict(res=512, NV=4), "train": dict(res=256, NV=4)}
PAD, FREQS = 64, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--sizes", default="cfg3,train")
    ap.add_argument("--launches", action="store_true", help="count device launches with torch.profiler instead of timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("encoder_input_launches.json" if a.launches else "encoder_input.json"))

    import numpy as np
    import torch
    import torch.nn.functional as F
    from diner_amd import glue
    from synthetic.encoder_stub import encoder_model

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    mean, std = torch.tensor(glue.IMAGENET_MEAN, device=dev).view(-1, 1, 1), torch.tensor(glue.IMAGENET_STD, device=dev).view(-1, 1, 1)
    freqs = torch.repeat_interleave(math.pi * 2.0 ** torch.arange(0, FREQS), 2).view(1, -1, 1).to(dev)
    phases = torch.zeros(2 * FREQS)
    phases[1::2] = math.pi * 0.5
    phases = phases.view(1, -1, 1).to(dev)

    def aten_head(images):
        """the reference's operator sequence on [N,3,H,W]"""
        x = F.pad((images - mean) / std, [PAD] * 4, mode="replicate")
        N, _, Hp, Wp = x.shape
        pe = torch.stack(torch.meshgrid(torch.linspace(-1, 1, Hp, device=dev), torch.linspace(-1, 1, Wp, device=dev), indexing="ij")[::-1], dim=-1)
        flat = pe.reshape(-1, 2)
        emb = torch.sin(torch.addcmul(phases, flat.unsqueeze(1).repeat(1, 2 * FREQS, 1), freqs)).view(flat.shape[0], -1)
        pe = torch.cat((flat, emb), dim=-1).reshape(Hp, Wp, -1)
        pe[PAD:-PAD, PAD:-PAD] = 0
        return torch.cat((x, pe.permute(2, 0, 1).unsqueeze(0).expand(N, -1, -1, -1)), dim=1)

    def timed_pair(fns, calls):
        """{name: ms per call}: windows of `calls` calls, the variants alternating window by window"""
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

    results = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "calls": a.calls, "image_padding": PAD, "padding_pe": FREQS,
               "sizes": {}}
    for name in a.sizes.split(","):
        res, NV = SIZES[name]["res"], SIZES[name]["NV"]
        g = torch.Generator(device=dev).manual_seed(1)
        images = torch.rand((1, NV, 3, res, res), device=dev, generator=g)
        flat = images.flatten(0, 1)
        with torch.no_grad():
            ref, got = aten_head(flat), glue.encoder_input(images, PAD, FREQS)
            rec = {"N": NV, "H": res, "W": res, "out": list(got.shape),
                   "agreement": {"image_channels_bit_identical": bool(torch.equal(ref[:, :3], got[:, :3])),
                                 "encoding_max_abs_diff": float((ref[:, 3:] - got[:, 3:]).abs().max())}}
            need = got.numel() * 4 + flat.numel() * 4
            rec["bytes_needed"] = need
            head = {"aten": lambda: aten_head(flat), "kernel": lambda: glue.encoder_input(images, PAD, FREQS)}
            if a.launches:
                rec["launches"] = {k: launches(fn) for k, fn in head.items()}
                results["sizes"][name] = rec
                print(json.dumps({name: rec}), flush=True)
                continue
            rec["head_ms"] = timed_pair(head, a.calls)
            rec["kernel_GBps"] = need / rec["head_ms"]["kernel"]["median"] / 1e6
            rec["aten_GBps_of_needed_bytes"] = need / rec["head_ms"]["aten"]["median"] / 1e6

            # ---- (c) one whole encode on the stub trunk ------------------------------------------------------------------------------
            m = encoder_model(device=dev, image_padding=PAD, padding_pe=FREQS).eval()
            enc = m.encoder
            depths = 1.0 + torch.rand((1, NV, 1, res, res), device=dev, generator=g)
            dstd = 0.004 + 0.004 * torch.rand((1, NV, 1, res, res), device=dev, generator=g)
            E = torch.eye(4, device=dev).expand(1, NV, 4, 4).contiguous()
            Kc = torch.tensor([[1.2 * res, 0, res / 2], [0, 1.2 * res, res / 2], [0, 0, 1]], device=dev).expand(1, NV, 3, 3).contiguous()

            def by_hand():
                t = enc.model
                x = t.relu(t.bn1(t.conv1(aten_head(flat))))
                lv = [x]
                x = t.layer1(t.maxpool(x))
                lv.append(x)
                for i in (2, 3):
                    x = getattr(t, f"layer{i}")(x)
                    lv.append(x)
                enc.normals = glue.depth2normal(depths.flatten(0, 1), Kc.flatten(0, 1)).reshape(1, NV, 3, res, res)
                enc.latent = glue.assemble_latent(lv, 1, NV)

            rec["encode_ms"] = timed_pair({"by_hand": by_hand, "glue_encode": lambda: glue.encode(m, images, depths, dstd, E, Kc)},
                                          max(a.calls // 5, 1))
            del m
        results["sizes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
        del ref, got
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
