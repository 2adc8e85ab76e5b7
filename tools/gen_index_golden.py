"""Golden vectors of the encoder's other latent lookup modes (SpatialEncoder index_interp / index_padding, reference
src/models/image_encoder.py:24-25,119-125): the UNMODIFIED reference PixelNeRF built with each non-default mode, rendered on the
CPU, plus two training cases with the reference's autograd gradients.  Runs only where the reference source tree exists
(``oracle.ref_harness.import_reference``); the GPU tests read the committed ``tests/golden/index_*.npz`` only.

    python tools/gen_index_golden.py            # (re)writes tests/golden/index_*.npz
    python tools/gen_index_golden.py --case=index_zeros

Same scheme as tools/gen_shape_golden.py: every input is rebuilt from seeds (``case_inputs``, shared with the tests), the fixture
stores sha256 digests of the seeded inputs next to the reference's outputs, and the tests inject the reference's samples
(``z_samples``).  Most scenes use feature_padding 0, two use 4 (as the shipped configs use a non-zero one: the mode then applies to the
rescaled coordinate); all use a wide target field of view (focal_scale < 1), so that many sample points project outside the source views
and the padding mode decides their latent: the fixture records ``out_frac``, the fraction of
(view, sample) lookups whose footprint leaves the latent map.  For nearest lookups it stores ``firm`` [NR,K]: samples whose lookup is
further than 1e-4 texel from a rounding boundary in every view (elsewhere a last-ulp difference of the projection may pick the other
texel); the tests compare firm samples only.  Names start with ``index_``: tests/conftest.py parametrises over ``g[0-9]*.npz``.
"""
from __future__ import annotations

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
from tools.gen_shape_golden import ENCODER_LAYERS, RESNETFC_DEFAULTS  # noqa: E402

_SCENE = dict(H=32, W=32, dataset="facescape", feature_padding=0)
_RENDER = dict(K=24, NC=200, G=8, ray_stride=3, focal_scale=0.5, bias_scale=0.1)
STANDARD_MLP = dict(d_hidden=512, n_blocks=5, combine_layer=3)
FIRM_TEXELS = 1e-4

# name: lookup mode, scene (NV, seed, C = d_latent), model (ResnetFC kwargs + num_freqs), seeds
CASES = {
    "index_zeros": dict(interp="bilinear", padding="zeros", scene=dict(_SCENE, NV=4, seed=60, C=512), num_freqs=6, mlp=STANDARD_MLP,
                        wseed=61, nseed=62, **_RENDER),
    "index_reflection": dict(interp="bilinear", padding="reflection", scene=dict(_SCENE, NV=4, seed=63, C=512), num_freqs=6,
                             mlp=STANDARD_MLP, wseed=64, nseed=65, **_RENDER),
    "index_nearest_border": dict(interp="nearest", padding="border", scene=dict(_SCENE, NV=4, seed=66, C=512), num_freqs=6,
                                 mlp=STANDARD_MLP, wseed=67, nseed=68, **_RENDER),
    "index_nearest_zeros": dict(interp="nearest", padding="zeros", scene=dict(_SCENE, NV=3, seed=69, C=512), num_freqs=6,
                                mlp=STANDARD_MLP, wseed=70, nseed=71, **_RENDER),
    "index_nearest_reflection": dict(interp="nearest", padding="reflection", scene=dict(_SCENE, NV=4, seed=72, C=512), num_freqs=6,
                                     mlp=STANDARD_MLP, wseed=73, nseed=74, **_RENDER),
    # the shipped configs' situation: a non-zero feature_padding, so the mode applies to the rescaled coordinate (image_encoder.py:113-114)
    "index_zeros_fpad4": dict(interp="bilinear", padding="zeros", scene=dict(_SCENE, NV=4, seed=90, C=512, feature_padding=4), num_freqs=6,
                              mlp=STANDARD_MLP, wseed=91, nseed=92, **dict(_RENDER, focal_scale=0.35)),
    "index_reflection_fpad4": dict(interp="bilinear", padding="reflection", scene=dict(_SCENE, NV=3, seed=93, C=512, feature_padding=4),
                                   num_freqs=6, mlp=STANDARD_MLP, wseed=94, nseed=95, **dict(_RENDER, focal_scale=0.35)),
    # a non-standard shape (the shape-general kernel) with zeros padding
    "index_gen_zeros_h128": dict(interp="bilinear", padding="zeros", scene=dict(_SCENE, NV=2, seed=75, C=256), num_freqs=6,
                                 mlp=dict(d_hidden=128, n_blocks=4, combine_layer=2), wseed=76, nseed=77, **_RENDER),
}
# training: gradients of L = <c_rgb, rgb> + <c_depth, depth> (oracle/gen_golden.py gen_train) for the standard model
TRAIN_CASES = {
    "index_train_zeros": dict(interp="bilinear", padding="zeros", scene=dict(_SCENE, H=16, W=16, NV=2, seed=80, C=512), num_freqs=6,
                              mlp=STANDARD_MLP, K=8, NC=64, G=3, ray_stride=4, focal_scale=0.5, wseed=81, bias_scale=0.1, nseed=82,
                              cseed=83),
    "index_train_nearest": dict(interp="nearest", padding="border", scene=dict(_SCENE, H=16, W=16, NV=2, seed=84, C=512), num_freqs=6,
                                mlp=STANDARD_MLP, K=8, NC=64, G=3, ray_stride=4, focal_scale=0.5, wseed=85, bias_scale=0.1, nseed=86,
                                cseed=87),
}


def mlp_dims(cfg):
    d = dict(RESNETFC_DEFAULTS, **cfg["mlp"])
    d["d_in"] = 7 + 8 * cfg["num_freqs"]
    d["d_latent"] = cfg["scene"]["C"]
    return d


def case_inputs(cfg):
    """Rebuild every input of a case from its seeds (shared by the generator and the tests)."""
    sc = synth.make_scene(**cfg["scene"])
    d = mlp_dims(cfg)
    w = synth.make_mlp_weights(cfg["wseed"], bias_scale=cfg["bias_scale"], d_in=d["d_in"], d_latent=d["d_latent"],
                               d_hidden=d["d_hidden"], n_blocks=d["n_blocks"], combine_layer=d["combine_layer"])
    rays = sc.target_rays(focal_scale=cfg["focal_scale"])[:, ::cfg["ray_stride"]]
    noise = synth.make_noise(rays.shape[1], cfg["NC"], cfg["G"], cfg["K"], seed=cfg["nseed"])
    return sc, w, np.ascontiguousarray(rays), noise


def input_digests(sc, w, rays, noise):
    from oracle.gen_golden import input_digests as _digests
    return _digests(sc, w, rays, noise)


def build_reference_model(cfg, sc, w):
    """The reference PixelNeRF with this case's configuration; index_interp / index_padding go in through encoder_conf.kwargs, the
    way a config sets them"""
    import torch
    from oracle import ref_harness as rh
    ref = rh.import_reference()
    nerf = ref.PixelNeRF(
        poscode_conf=NS(kwargs=dict(num_freqs=cfg["num_freqs"], freq_factor=6.28, include_input=True)),
        encoder_conf=NS(module="src.models.image_encoder.SpatialEncoder",
                        kwargs=dict(image_padding=2 * sc.feature_padding, padding_pe=4, pretrained=False,
                                    num_layers=ENCODER_LAYERS[sc.C], index_interp=cfg["interp"], index_padding=cfg["padding"])),
        mlp_fine_conf=NS(module="src.models.resnetfc.ResnetFC", kwargs=dict(cfg["mlp"], combine_type="average")))
    res = nerf.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    enc = nerf.encoder
    assert enc.index_interp == cfg["interp"] and enc.index_padding == cfg["padding"]
    enc.depths, enc.depths_std, enc.normals = t(sc.depths), t(sc.depths_std), t(sc.normals)
    enc.nviews, enc.nobjects = sc.NV, sc.poses.shape[0]
    enc.latent = t(sc.latent)
    nerf.poses, nerf.focal, nerf.c, nerf.image_shape = t(sc.poses), t(sc.focal), t(sc.c), t(sc.image_shape)
    assert enc.feature_padding == sc.feature_padding and enc.latent_size == sc.C
    return nerf.eval()


def _reflect(x, size):
    """ATen's reflect_coordinates(x, -1, 2 size - 1) in float64"""
    span = float(size)
    a = np.abs(x + 0.5)
    extra = np.fmod(a, span)
    flips = np.floor(a / span)
    return np.where(flips % 2 == 0, extra - 0.5, span - extra - 0.5)


def lookup_stats(nerf, cfg, rays, z):
    """(out_frac, firm [NR,K]) of the latent lookups of the sample points: the uv SpatialEncoder.index receives, in float64"""
    import torch
    cap = []
    enc = nerf.encoder
    orig = enc.index
    enc.index = lambda uv: (cap.append(uv.detach().clone()), orig(uv))[1]
    try:
        rays_t, z_t = torch.from_numpy(rays), torch.from_numpy(z)
        SB, NR, K = z_t.shape
        pts = rays_t[..., None, :3] + z_t.unsqueeze(-1) * rays_t[..., None, 3:6]
        vd = rays_t[..., None, 3:6].expand(-1, -1, K, -1)
        with torch.no_grad():
            nerf(pts.reshape(SB, NR * K, 3), viewdirs=vd.reshape(SB, NR * K, 3))
    finally:
        enc.index = orig
    uv = cap[0].double().numpy()[0]                          # [NV, P, 2]
    h, w = enc.latent.shape[-2:]
    fp = float(enc.feature_padding)
    u = uv[..., 0] * ((w - 2 * fp) / w)
    v = uv[..., 1] * ((h - 2 * fp) / h)
    ix, iy = ((u + 1) * w - 1) / 2, ((v + 1) * h - 1) / 2
    out = (ix < 0) | (ix > w - 1) | (iy < 0) | (iy > h - 1)
    if cfg["padding"] == "reflection":
        ix, iy = _reflect(ix, w), _reflect(iy, h)
    if cfg["padding"] != "zeros":
        ix, iy = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
    dist = np.minimum(np.abs(np.abs(ix - np.floor(ix)) - 0.5), np.abs(np.abs(iy - np.floor(iy)) - 0.5))
    firm = (dist > FIRM_TEXELS).all(axis=0).reshape(z.shape[1:])
    return float(out.mean()), firm


def gen_render(name, cfg, out_dir):
    from oracle import ref_harness as rh
    sc, w, rays, noise = case_inputs(cfg)
    nerf = build_reference_model(cfg, sc, w)
    ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    out_frac, firm = lookup_stats(nerf, cfg, rays, ref["z_fill"])
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), rays=rays,
                   z_fill=ref["z_fill"][0], rgbsigma=ref["rgbsigma"][0], weights=ref["weights"][0], rgb=ref["rgb"][0],
                   depth=ref["depth"][0], out_frac=np.float64(out_frac), firm=firm)
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return f"NR={rays.shape[1]} out_frac={out_frac:.3f} firm={firm.mean():.4f}"


def gen_train(name, cfg, out_dir):
    import torch
    from oracle import ref_harness as rh
    from oracle.gen_golden import grad_probe_indices, train_cotangents
    sc, w, rays, noise = case_inputs(cfg)
    nerf = build_reference_model(cfg, sc, w)
    ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    out_frac, firm = lookup_stats(nerf, cfg, rays, ref["z_fill"])
    z = torch.from_numpy(ref["z_fill"])
    nerf.encoder.latent = nerf.encoder.latent.clone().requires_grad_(True)
    for p in nerf.mlp_fine.parameters():
        p.requires_grad_(True)
    rend = rh.import_reference().NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"],
                                                 white_bkgd=sc.white_bkgd)
    weights, rgb, depth = rend.composite(nerf, torch.from_numpy(rays), z)
    c_rgb, c_depth = train_cotangents(rays.shape[1], cfg["cseed"])
    loss = (rgb * torch.from_numpy(c_rgb)).sum() + (depth * torch.from_numpy(c_depth)).sum()
    loss.backward()
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), z_fill=ref["z_fill"],
                   rgb=rgb.detach().numpy(), depth=depth.detach().numpy(), latent_grad=nerf.encoder.latent.grad.numpy(),
                   out_frac=np.float64(out_frac), firm=firm)
    for pname, p in nerf.mlp_fine.named_parameters():
        gnp = p.grad.numpy()
        idx = grad_probe_indices(gnp.shape)
        fixture[f"g_sum/{pname}"] = np.float64(gnp.astype(np.float64).sum())
        fixture[f"g_norm/{pname}"] = np.float64(np.sqrt((gnp.astype(np.float64) ** 2).sum()))
        fixture[f"g_probe/{pname}"] = gnp.reshape(-1)[idx]
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return f"NR={rays.shape[1]} out_frac={out_frac:.3f} firm={firm.mean():.4f} |latent_grad|={np.abs(fixture['latent_grad']).max():.3e}"


def main():
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in list(CASES.items()) + list(TRAIN_CASES.items()):
        if only and name not in only:
            continue
        t0 = time.time()
        msg = (gen_train if name in TRAIN_CASES else gen_render)(name, cfg, out_dir)
        path = out_dir / f"{name}.npz"
        print(f"{name}: {cfg['interp']}/{cfg['padding']} {msg} -> {path.name} {path.stat().st_size / 1e6:.2f} MB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
