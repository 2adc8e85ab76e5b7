"""Golden vectors of the NOVEL_PE point model on the shape-general kernels (diner_amd.novel.NeRFRendererDGS.render_points_novel_pe):
the UNMODIFIED reference ``src.models.novel_pe.pe_novel_pixelnerf.PixelNeRF`` evaluated on the CPU at given points.  Runs only where
the reference source tree exists (``oracle.ref_harness``); the tests read the committed ``tests/golden/novel_pe_point_*.npz`` only.

    python tools/gen_novel_pe_point_golden.py            # (re)writes tests/golden/novel_pe_point_*.npz
    python tools/gen_novel_pe_point_golden.py --case=novel_pe_point_b

Same scheme as tools/gen_novel_point_golden.py: every input is rebuilt from seeds (``case_inputs``, shared with the tests) and a
fixture holds the sha256 digests of those inputs and the reference's rgb-sigma [SB,P,4], nothing else.  Points only, no sampler.  In
every case xyz_tgt, xyz_in and xyz_gen all differ, the viewdirs are drawn on their own, every scene has a general and a target camera
of its own, the general latent and both pos-encoding maps have (non-square) sizes of their own, and about a tenth of the target
projections (and of the general ones) leave their map.  ``case_inputs`` asserts, after re-drawing the points that fail by a seeded
rule, that every point has camera depth > 0.1 in every source, general and target camera and that no nearest-type lookup coordinate
(the depth lookup always; the four map lookups when index_interp is "nearest") lies within 1e-3 texel of a rounding boundary: the
tests compare every point.
"""
from __future__ import annotations

import hashlib
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from synthetic import synth  # noqa: E402
from tools.gen_novel_point_golden import ENCODER_LAYERS, MIN_DEPTH, STANDARD, _cam_uv, _near_boundary  # noqa: E402

F32 = np.float32
_SCENE = dict(H=32, W=32, dataset="facescape", feature_padding=4)     # latent 24 x 24
# general latent [C, 28, 20], general image 40 x 56 pixels; source pos-encodings [3, 36, 30]; target pos-encoding [3, 26, 34], target
# image 48 x 60 pixels
_MAPS = dict(gen_h=28, gen_w=20, gen_H=56, gen_W=40, src_h=36, src_w=30, tgt_h=26, tgt_w=34, tgt_H=60, tgt_W=48)

# name: scene (NV, C = encoder.latent_size; the fusion MLP's d_latent is C + 6), SB scenes (seed + 10 sb), model, lookup, P, seeds
CASES = {
    # (a) the NOVEL_PE config's shape: two gather pieces, 512 + 8, the second one the pe tail; a tail tile; two target cameras
    "novel_pe_point_a": dict(scene=dict(_SCENE, NV=4, seed=170, C=512), SB=2, num_freqs=6, mlp=STANDARD, P=200,
                             index_interp="bilinear", index_padding="border", wseed=171, pseed=172, **_MAPS),
    # (b) <1,1>; one piece of 264 columns; the nearest lookup with zeros padding, one point past a tile
    "novel_pe_point_b": dict(scene=dict(_SCENE, NV=2, seed=173, C=256), SB=1, num_freqs=6, mlp=dict(d_hidden=128, n_blocks=3, combine_layer=2),
                             P=65, index_interp="nearest", index_padding="zeros", wseed=174, pseed=175, **_MAPS),
    # (c) <2,1>; Softplus; reflection padding; exactly one tile; 72 columns
    "novel_pe_point_c": dict(scene=dict(_SCENE, NV=3, seed=176, C=64), SB=1, num_freqs=6,
                             mlp=dict(d_hidden=256, n_blocks=4, combine_layer=2, beta=100.0), P=64,
                             index_interp="bilinear", index_padding="reflection", wseed=177, pseed=178, **_MAPS),
    # (d) combine_layer >= n_blocks (no mean over views, NV = 1)
    "novel_pe_point_d": dict(scene=dict(_SCENE, NV=1, seed=179, C=512), SB=1, num_freqs=6, mlp=dict(d_hidden=64, n_blocks=2, combine_layer=1000),
                             P=130, index_interp="bilinear", index_padding="border", wseed=180, pseed=181, **_MAPS),
    # (e) combine_layer 0: no latent, map or pe is read; a single point (pseed: one whose reference sigma is above 0, so that relu hides nothing)
    "novel_pe_point_e": dict(scene=dict(_SCENE, NV=3, seed=182, C=256), SB=1, num_freqs=6, mlp=dict(d_hidden=96, n_blocks=2, combine_layer=0),
                             P=1, index_interp="bilinear", index_padding="border", wseed=183, pseed=190, **_MAPS),
}
MARGIN = 1e-3


def mlp_dims(cfg):
    d = dict(dict(d_hidden=128, n_blocks=5, combine_layer=1000, beta=0.0), **cfg["mlp"])      # resnetfc.py:72-82
    d["d_in"] = 7 + 8 * cfg["num_freqs"]
    d["d_latent"] = cfg["scene"]["C"] + 6                                                      # pe_novel_pixelnerf.py:21
    return d


def _scale(w, h, fp):
    return np.array([(w - 2.0 * fp) / w, (h - 2.0 * fp) / h])


def case_inputs(cfg):
    """Rebuild every input of a case from its seeds (shared by the generator and the tests): a dict of float32 arrays + cfg, dims."""
    SB, P, NV, C, fp = cfg["SB"], cfg["P"], cfg["scene"]["NV"], cfg["scene"]["C"], cfg["scene"]["feature_padding"]
    scenes = [synth.make_scene(**dict(cfg["scene"], seed=cfg["scene"]["seed"] + 10 * sb)) for sb in range(SB)]
    cat = lambda k: np.concatenate([getattr(s, k) for s in scenes], 0)
    inp = {k: np.ascontiguousarray(cat(k), dtype=F32) for k in ("poses", "focal", "c", "depths", "depths_std", "normals", "latent")}
    inp["image_shape"] = scenes[0].image_shape.astype(F32)
    d = mlp_dims(cfg)
    inp["weights"] = synth.make_mlp_weights(cfg["wseed"], bias_scale=0.1, d_in=d["d_in"], d_latent=d["d_latent"], d_hidden=d["d_hidden"],
                                            n_blocks=d["n_blocks"], combine_layer=d["combine_layer"])
    rs = np.random.RandomState(cfg["pseed"])
    inp["gen_latent"] = rs.standard_normal((C, cfg["gen_h"], cfg["gen_w"])).astype(F32)
    # deformation_layer Linear(C + 6 -> C): torch's default scale for the latent part, the six pe columns of order 1 so that they matter
    inp["deform_w"] = np.concatenate([rs.uniform(-1, 1, (C, C)) / np.sqrt(C + 6), rs.uniform(-1, 1, (C, 6))], 1).astype(F32)
    inp["deform_b"] = rs.uniform(-0.1, 0.1, C).astype(F32)
    inp["pos_encodings"] = rs.uniform(-1, 1, (SB, NV, 3, cfg["src_h"], cfg["src_w"])).astype(F32)
    inp["tgt_pos_encoding"] = rs.uniform(-1, 1, (SB, 1, 3, cfg["tgt_h"], cfg["tgt_w"])).astype(F32)
    # one general and one target camera per scene: their own yaw and distance, principal points off the centre
    gW, gH, tW, tH = cfg["gen_W"], cfg["gen_H"], cfg["tgt_W"], cfg["tgt_H"]
    inp["gen_poses"] = np.stack([synth.look_at_origin_w2c(0.8 - 1.3 * sb, 1.6 + 0.2 * sb) for sb in range(SB)])[:, None].astype(F32)
    inp["gen_c"] = np.stack([[gW / 2 + 1.5 - sb, gH / 2 - 2.25 + sb] for sb in range(SB)])[:, None].astype(F32)
    inp["gen_image_shape"] = np.array([gW, gH], F32)
    inp["tgt_poses"] = np.stack([synth.look_at_origin_w2c(-0.5 + 0.9 * sb, 1.8 - 0.15 * sb) for sb in range(SB)])[:, None].astype(F32)
    inp["tgt_c"] = np.stack([[tW / 2 - 1.25 + sb, tH / 2 + 2.5 - sb] for sb in range(SB)])[:, None].astype(F32)
    inp["tgt_image_shape"] = np.array([tW, tH], F32)
    scale_g, scale_t = _scale(cfg["gen_w"], cfg["gen_h"], fp), _scale(cfg["tgt_w"], cfg["tgt_h"], fp)
    scale_s = _scale(cfg["src_w"], cfg["src_h"], fp)
    scale_l = _scale(inp["latent"].shape[-1], inp["latent"].shape[-2], fp)
    Hs, Ws = inp["depths"].shape[-2:]
    nearest = cfg["index_interp"] == "nearest"

    def draw(r, n):
        xyz = r.uniform(-0.5, 0.5, (n, 3)).astype(F32)
        gen = (xyz + r.uniform(-0.08, 0.08, (n, 3)).astype(F32) + F32(0.01)).astype(F32)
        tgt = (xyz + r.uniform(-0.08, 0.08, (n, 3)).astype(F32) - F32(0.01)).astype(F32)
        return xyz, gen, tgt

    def edge_focal(x, pose, scale, W, H):
        """the focal length that puts the 0.9 quantile of the (feature-padding scaled) uv on the map's edge"""
        cam, _ = _cam_uv(x, pose, np.ones(2), np.zeros(2), np.ones(2))
        r = np.maximum(np.abs(cam[:, 0] / cam[:, 2]) * 2 * scale[0] / W, np.abs(cam[:, 1] / cam[:, 2]) * 2 * scale[1] / H)
        f = F32(1.0 / np.quantile(r, 0.9)) if P > 1 else F32(1.2 * W)
        return (f, f * F32(1.05))

    xyz_in, xyz_gen, xyz_tgt = (np.empty((SB, P, 3), F32) for _ in range(3))
    gen_focal, tgt_focal = np.empty((SB, 1, 2), F32), np.empty((SB, 1, 2), F32)
    for sb in range(SB):
        xyz_in[sb], xyz_gen[sb], xyz_tgt[sb] = draw(rs, P)
        gen_focal[sb, 0] = edge_focal(xyz_gen[sb], inp["gen_poses"][sb, 0], scale_g, gW, gH)
        tgt_focal[sb, 0] = edge_focal(xyz_tgt[sb], inp["tgt_poses"][sb, 0], scale_t, tW, tH)

        def bad(xi, xg, xt):
            b = np.zeros(len(xi), bool)
            for v in range(NV):
                cam, uv = _cam_uv(xi, inp["poses"][sb, v], inp["focal"][sb, v], inp["c"][sb, v], inp["image_shape"])
                b |= (cam[:, 2] <= MIN_DEPTH) | _near_boundary(uv, np.array([Ws, Hs], np.float64))
                if nearest:
                    b |= _near_boundary(uv, np.array(inp["latent"].shape[:-3:-1], np.float64), scale_l)
                    b |= _near_boundary(uv, np.array([cfg["src_w"], cfg["src_h"]], np.float64), scale_s)
            cam, uv = _cam_uv(xg, inp["gen_poses"][sb, 0], gen_focal[sb, 0], inp["gen_c"][sb, 0], inp["gen_image_shape"])
            b |= cam[:, 2] <= MIN_DEPTH
            if nearest:
                b |= _near_boundary(uv, np.array([cfg["gen_w"], cfg["gen_h"]], np.float64), scale_g)
            cam, uv = _cam_uv(xt, inp["tgt_poses"][sb, 0], tgt_focal[sb, 0], inp["tgt_c"][sb, 0], inp["tgt_image_shape"])
            b |= cam[:, 2] <= MIN_DEPTH
            if nearest:
                b |= _near_boundary(uv, np.array([cfg["tgt_w"], cfg["tgt_h"]], np.float64), scale_t)
            return b

        for attempt in range(1, 50):     # the seeded re-draw: the points that fail, from RandomState(pseed + 1000 attempt + sb)
            b = bad(xyz_in[sb], xyz_gen[sb], xyz_tgt[sb])
            if not b.any():
                break
            xyz_in[sb, b], xyz_gen[sb, b], xyz_tgt[sb, b] = draw(np.random.RandomState(cfg["pseed"] + 1000 * attempt + sb), int(b.sum()))
        assert not bad(xyz_in[sb], xyz_gen[sb], xyz_tgt[sb]).any(), "re-draw did not converge"
    inp["gen_focal"], inp["tgt_focal"] = gen_focal, tgt_focal
    inp["xyz_in"], inp["xyz_gen"], inp["xyz_tgt"] = xyz_in, xyz_gen, xyz_tgt
    v = np.random.RandomState(cfg["pseed"] + 7).standard_normal((SB, P, 3))
    inp["viewdirs"] = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)
    assert not np.array_equal(xyz_in, xyz_gen) and not np.array_equal(xyz_in, xyz_tgt) and not np.array_equal(xyz_gen, xyz_tgt)
    inp["cfg"], inp["dims"] = cfg, d
    return inp


def outside_fraction(inp, which="tgt"):
    """fraction of the target (``which="gen"``: general) projections whose (feature-padding scaled) uv leaves [-1, 1]: outside the map"""
    cfg = inp["cfg"]
    scale = _scale(cfg[which + "_w"], cfg[which + "_h"], cfg["scene"]["feature_padding"])
    out = []
    for sb in range(cfg["SB"]):
        _, uv = _cam_uv(inp["xyz_" + which][sb], inp[which + "_poses"][sb, 0], inp[which + "_focal"][sb, 0], inp[which + "_c"][sb, 0],
                        inp[which + "_image_shape"])
        out.append((np.abs(uv * scale) > 1).any(-1))
    return float(np.concatenate(out).mean())


def input_digests(inp):
    h = lambda *arrs: hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrs)).hexdigest()
    w = inp["weights"]
    return dict(maps=h(*[inp[k] for k in ("poses", "focal", "c", "image_shape", "depths", "depths_std", "normals")]), latent=h(inp["latent"]),
                weights=h(*[w[k] for k in sorted(w)]), gen=h(*[inp[k] for k in ("gen_latent", "gen_poses", "gen_focal", "gen_c", "gen_image_shape")]),
                pe=h(*[inp[k] for k in ("deform_w", "deform_b", "pos_encodings", "tgt_pos_encoding", "tgt_poses", "tgt_focal", "tgt_c",
                                        "tgt_image_shape")]),
                points=h(inp["xyz_in"], inp["xyz_gen"], inp["xyz_tgt"], inp["viewdirs"]))


def _intrinsics(torch, focal, c):
    K = torch.zeros(focal.shape[0], 3, 3)
    K[:, 0, 0], K[:, 1, 1] = torch.from_numpy(focal[:, 0, 0]), torch.from_numpy(focal[:, 0, 1])
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = torch.from_numpy(c[:, 0, 0]), torch.from_numpy(c[:, 0, 1]), 1.0
    return K


def build_reference_model(inp):
    """The reference's NOVEL_PE PixelNeRF with this case's configuration; gen_latent re-assigned after construction (index() reads its
    shape), the general and target state through encode_gen / encode_tgt"""
    import torch
    from oracle import ref_harness as rh
    rh.install_stubs()
    from src.models.novel_pe.pe_novel_pixelnerf import PixelNeRF
    cfg, d = inp["cfg"], inp["dims"]
    fp, C = cfg["scene"]["feature_padding"], cfg["scene"]["C"]
    nerf = PixelNeRF(
        poscode_conf=NS(kwargs=dict(num_freqs=cfg["num_freqs"], freq_factor=6.28, include_input=True)),
        encoder_conf=NS(module="src.models.image_encoder.SpatialEncoder",
                        kwargs=dict(image_padding=2 * fp, padding_pe=4, pretrained=False, num_layers=ENCODER_LAYERS[C],
                                    index_interp=cfg["index_interp"], index_padding=cfg["index_padding"])),
        mlp_fine_conf=NS(module="src.models.resnetfc.ResnetFC", kwargs=dict(cfg["mlp"], combine_type="average")))
    assert nerf.d_latent == d["d_latent"] and nerf.deformation_layer.weight.shape == inp["deform_w"].shape
    res = nerf.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    nerf.deformation_layer.load_state_dict(dict(weight=torch.from_numpy(inp["deform_w"]), bias=torch.from_numpy(inp["deform_b"])), strict=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    enc = nerf.encoder
    enc.depths, enc.depths_std, enc.normals = t(inp["depths"]), t(inp["depths_std"]), t(inp["normals"])
    enc.nviews, enc.nobjects = inp["poses"].shape[1], inp["poses"].shape[0]
    enc.latent = t(inp["latent"])
    nerf.poses, nerf.focal, nerf.c, nerf.image_shape = t(inp["poses"]), t(inp["focal"]), t(inp["c"]), t(inp["image_shape"])
    nerf.pos_encodings = t(inp["pos_encodings"])
    assert enc.feature_padding == fp and enc.latent_size == C
    nerf.gen_latent = torch.nn.Parameter(t(inp["gen_latent"]))
    nerf.encode_gen(torch.zeros(inp["poses"].shape[0], 3, 2, 2), t(inp["gen_poses"][:, 0]), _intrinsics(torch, inp["gen_focal"], inp["gen_c"]),
                    (cfg["gen_H"], cfg["gen_W"]))
    nerf.encode_tgt(t(inp["tgt_pos_encoding"][:, 0]), t(inp["tgt_poses"][:, 0]), _intrinsics(torch, inp["tgt_focal"], inp["tgt_c"]),
                    (cfg["tgt_H"], cfg["tgt_W"]))
    for k in ("gen_poses", "gen_focal", "gen_c", "gen_image_shape", "tgt_poses", "tgt_focal", "tgt_c", "tgt_image_shape", "tgt_pos_encoding"):
        assert np.array_equal(getattr(nerf, k).numpy(), inp[k]), k
    return nerf.eval()


def main():
    import torch
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        inp = case_inputs(cfg)
        nerf = build_reference_model(inp)
        t = lambda a: torch.from_numpy(a)
        with torch.no_grad():
            ref = nerf(t(inp["xyz_in"]), t(inp["xyz_gen"]), t(inp["xyz_tgt"]), viewdirs=t(inp["viewdirs"])).numpy()
        assert ref.shape == (cfg["SB"], cfg["P"], 4) and np.isfinite(ref).all()
        path = out_dir / f"{name}.npz"
        np.savez_compressed(path, config=json.dumps(cfg), digests=json.dumps(input_digests(inp)), rgbsigma=ref.astype(F32))
        print(f"{name}: dims={inp['dims']} outside tgt={outside_fraction(inp):.2f} gen={outside_fraction(inp, 'gen'):.2f} "
              f"sigma_max={ref[..., 3].max():.2f} sigma>0: {(ref[..., 3] > 0).mean():.2f} -> {path.name} "
              f"{path.stat().st_size / 1e3:.1f} kB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
