"""Time of the NOVEL renderer's ``composite()`` for the NOVEL_PE model (``pass_points``) with the point model on the HIP kernels
against the point model on PyTorch (diner_amd/novel.py ``hip_point_model``; csrc/points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip,
novel_pe_map.hip), one GPU, one process, device events, median after warm-ups.  The sibling of tools/bench_novel_point_model.py, at
the same sizes:

* the model: the NOVEL_PE config's shape (d_hidden 512, 5 blocks, combine_layer 3, 6 frequencies, C = 512, d_latent 518) as
  tests/novel_pe_point_ref.py's stand-in, ``--views`` source views of ``--size`` x ``--size`` pixels, feature_padding 32, a
  ``gen_latent`` of [512, --gen-size, --gen-size], pos-encoding maps of the image size, one general and one target camera;
* the work: 4096 rays x 40 samples, deformed by ``--vertices`` mesh vertices with both offset sets (that search is part of every
  window: the same launch in all of them);
* windows: ``composite()`` with the switch on in fp32, with the switch on in f16x3 (``f16x3_any_shape``), and with the switch off,
  where the restated torch model runs on the same GPU in the reference's chunks of ``eval_batch_size`` points; for the ratio to the
  NOVEL kernel, the NOVEL stand-in (tests/novel_point_ref.py, d_latent 512) with the switch on in both precisions;
* the one-off build of the deformation map (``diner_pack_novel_pe_map``), which the windows do not contain: it is cached per encode.

The results are compared with one another before they are timed (max |d rgb|).  A record, not a gate: writes --out
(profiles/novel_pe_point_model.json).

    python tools/bench_novel_pe_point_model.py [--steps 7] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools.bench_novel_point_model import stats  # noqa: E402

NR, K, CH = 4096, 40, 512
MLP = dict(d_hidden=512, n_blocks=5, combine_layer=3, beta=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--gen-size", type=int, default=192)
    ap.add_argument("--vertices", type=int, default=26317)
    ap.add_argument("--eval-batch-size", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "novel_pe_point_model.json"))
    a = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    from diner_amd import _lib
    from diner_amd.novel import NeRFRendererDGS
    from diner_amd.renderer import _ptr, _stream
    from synthetic import synth
    from tests import knn_ref
    from tests import novel_pe_point_ref as R
    from tests import novel_point_ref as RN
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")

    fp = 32
    sc = synth.make_scene(a.size, a.size, a.views, seed=5, feature_padding=fp, with_latent=False)
    g = torch.Generator(device=dev).manual_seed(11)
    h = a.size // 2 + 2 * fp
    rs = np.random.RandomState(12)
    inp = {k: getattr(sc, k) for k in ("poses", "focal", "c", "image_shape", "depths", "depths_std", "normals")}
    inp["latent"] = np.zeros((1, a.views, 8, 1, 1), np.float32)           # replaced by a device tensor below
    inp["gen_latent"] = np.zeros((8, 1, 1), np.float32)
    gW = gH = 2 * a.gen_size
    inp["gen_poses"] = synth.look_at_origin_w2c(0.3, 1.75)[None, None]
    inp["gen_focal"], inp["gen_c"] = np.array([[[1.2 * gW, 1.2 * gW]]], np.float32), np.array([[[gW / 2, gH / 2]]], np.float32)
    inp["gen_image_shape"] = np.array([gW, gH], np.float32)
    inp["tgt_poses"] = synth.look_at_origin_w2c(-0.2, 1.75)[None, None]
    inp["tgt_focal"], inp["tgt_c"] = np.array([[[1.2 * a.size, 1.2 * a.size]]], np.float32), np.array([[[a.size / 2, a.size / 2]]], np.float32)
    inp["tgt_image_shape"] = np.array([a.size, a.size], np.float32)
    inp["pos_encodings"] = rs.uniform(-1, 1, (1, a.views, 3, a.size, a.size)).astype(np.float32)
    inp["tgt_pos_encoding"] = rs.uniform(-1, 1, (1, 1, 3, a.size, a.size)).astype(np.float32)
    inp["deform_w"] = np.concatenate([rs.uniform(-1, 1, (CH, CH)) / np.sqrt(CH + 6), rs.uniform(-1, 1, (CH, 6))], 1).astype(np.float32)
    inp["deform_b"] = rs.uniform(-0.1, 0.1, CH).astype(np.float32)
    inp["cfg"] = dict(scene=dict(feature_padding=fp, C=CH), num_freqs=6, index_interp="bilinear", index_padding="border")
    latent = torch.randn((1, a.views, CH, h, h), generator=g, device=dev)
    gen_latent = torch.randn((CH, a.gen_size, a.gen_size), generator=g, device=dev)

    def model(pe):
        dims = dict(MLP, d_latent=CH + 6 if pe else CH)
        i = dict(inp, dims=dims, weights=synth.make_mlp_weights(6, bias_scale=0.1, d_in=55, **{k: v for k, v in dims.items() if k != "beta"}))
        m = (R if pe else RN).model_from_inputs(i, device=dev)
        m.encoder.latent = latent
        m.gen_latent = torch.nn.Parameter(gen_latent, requires_grad=False)
        return m

    m_pe, m_nv = model(True), model(False)
    rays = torch.from_numpy(np.ascontiguousarray(sc.target_rays(64, 64))).to(dev)
    assert rays.shape[1] == NR
    z = (1.0 + 1.5 * (torch.arange(K, device=dev) + torch.rand((1, NR, K), generator=g, device=dev)) / K).contiguous()
    verts = torch.from_numpy(knn_ref.sphere_mesh(a.vertices, seed=3, radius=0.45, centre=(0.0, 0.0, 0.0)))[None].to(dev)
    o_in, o_gen = 0.03 * torch.randn(verts.shape, generator=g, device=dev), 0.03 * torch.randn(verts.shape, generator=g, device=dev)

    def renderer(precision, on, pe=True):
        r = NeRFRendererDGS(n_samples=K, eval_batch_size=a.eval_batch_size, hip_point_model=on, pass_points=pe)
        r.precision, r.f16x3_any_shape = precision, precision == "f16x3"
        return r

    def device_ms(fn, **kw):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return stats(ms, **kw)

    variants = {"hip_fp32": (renderer("fp32", True), m_pe), "hip_f16x3": (renderer("f16x3", True), m_pe),
                "torch_chunked": (renderer("fp32", False), m_pe),
                "novel_hip_fp32": (renderer("fp32", True, pe=False), m_nv), "novel_hip_f16x3": (renderer("f16x3", True, pe=False), m_nv)}
    results = {"device": torch.cuda.get_device_name(0), "rays": NR, "samples": K, "views": a.views, "image": a.size, "latent": [CH, h, h],
               "gen_latent": [CH, a.gen_size, a.gen_size], "pos_encodings": [3, a.size, a.size], "vertices": a.vertices,
               "mlp": dict(MLP, d_latent=CH + 6, d_latent_padded=CH + 8), "eval_batch_size": a.eval_batch_size, "steps": a.steps,
               "warmup": a.warmup, "windows": {}}
    with torch.no_grad():
        outs = {k: r.composite(m, rays, z, verts, o_in, o_gen) for k, (r, m) in variants.items()}
        results["routes"] = {k: r.last_route for k, (r, _) in variants.items()}
        for k in ("hip_fp32", "hip_f16x3"):
            results[f"max_abs_rgb_{k}_vs_torch"] = float((outs[k][1] - outs["torch_chunked"][1]).abs().max())
        for k, (r, m) in variants.items():
            rec = device_ms(lambda: r.composite(m, rays, z, verts, o_in, o_gen), route=r.last_route)
            rec["rays_per_s"] = NR / (rec["median_ms"] * 1e-3)
            results["windows"][k] = rec
            print(json.dumps({k: rec}), flush=True)
        w = results["windows"]
        results["ratio_to_novel_kernel"] = {p: w[f"hip_{p}"]["median_ms"] / w[f"novel_hip_{p}"]["median_ms"] for p in ("fp32", "f16x3")}
        results["speedup_vs_torch"] = {p: w["torch_chunked"]["median_ms"] / w[f"hip_{p}"]["median_ms"] for p in ("fp32", "f16x3")}
        # the one-off map build: the entry point alone, on the scene and the packed latent the renderer holds
        r = variants["hip_fp32"][0]
        scn, keep = r._scene(m_pe, need_latent=True)
        wl = m_pe.deformation_layer.weight[:, :CH].contiguous()
        dmap = torch.empty_like(keep[4])
        results["map_build"] = device_ms(lambda: _lib.check(_lib.lib().diner_pack_novel_pe_map(C.byref(scn), _ptr(wl), _ptr(dmap), _stream(dev)),
                                                            "diner_pack_novel_pe_map"), texels=a.views * h * h, bytes=dmap.numel() * 4,
                                         what="once per encode, cached; not part of the windows")
        assert torch.equal(dmap, r._pe_map_pack)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")
    print(json.dumps({kk: vv for kk, vv in results.items() if kk != "windows"}), flush=True)


if __name__ == "__main__":
    main()
