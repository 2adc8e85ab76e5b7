"""Golden vectors of the bicubic latent lookup (SpatialEncoder index_interp="bicubic", reference src/models/image_encoder.py:24-25,
119-125): the UNMODIFIED reference PixelNeRF built with index_interp="bicubic" and each padding, rendered on the CPU, plus one training
case with the reference's autograd gradients (MLP parameters, latent) and the same case with the gradients to the geometric leaves.
Runs only where the reference source tree exists (``oracle.ref_harness.import_reference``); the tests read the committed
``tests/golden/bicubic_*.npz`` only.

    python tools/gen_bicubic_golden.py            # (re)writes tests/golden/bicubic_*.npz
    python tools/gen_bicubic_golden.py --case=bicubic_zeros

The machinery is that of tools/gen_index_golden.py and tools/gen_camgrad_golden.py (seeded inputs, sha256 digests, the reference's samples
injected), imported, not edited: their ``CASES`` parametrise existing tests.  Bicubic is continuous, so there is no ``firm`` mask: every
sample is compared.  Each fixture records ``straddle_frac``, the share of (view, sample) lookups whose 4 x 4 footprint has some but not all
taps in the map (where the per-tap padding decides the value), and ``inside_frac``, the share with all 16 taps inside.  Names start with
``bicubic_``: tests/conftest.py parametrises over ``g[0-9]*.npz``, the index tests over ``index_*.npz``.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tools import gen_camgrad_golden as gcg  # noqa: E402
from tools import gen_index_golden as gix  # noqa: E402

_SCENE, _RENDER, STANDARD_MLP = gix._SCENE, gix._RENDER, gix.STANDARD_MLP

# render cases: 32 x 32 scene, K = 24, NC = 200, G = 8, ray_stride 3 (342 rays)
CASES = {
    "bicubic_border_h128": dict(interp="bicubic", padding="border", scene=dict(_SCENE, NV=2, seed=200, C=256), num_freqs=6,
                                mlp=dict(d_hidden=128, n_blocks=4, combine_layer=2), wseed=201, nseed=202, **_RENDER),
    "bicubic_zeros": dict(interp="bicubic", padding="zeros", scene=dict(_SCENE, NV=3, seed=203, C=512), num_freqs=6, mlp=STANDARD_MLP,
                          wseed=204, nseed=205, **_RENDER),
    "bicubic_reflection_fpad4": dict(interp="bicubic", padding="reflection", scene=dict(_SCENE, NV=3, seed=206, C=512, feature_padding=4),
                                     num_freqs=6, mlp=STANDARD_MLP, wseed=207, nseed=208, **dict(_RENDER, focal_scale=0.35)),
}
# training: gradients of L = <c_rgb, rgb> + <c_depth, depth> for the standard model, 16 x 16, NV = 2
_TRAIN = dict(interp="bicubic", padding="border", scene=dict(_SCENE, H=16, W=16, NV=2, seed=210, C=512), num_freqs=6, mlp=STANDARD_MLP,
              K=8, NC=64, G=3, ray_stride=4, focal_scale=0.5, wseed=211, bias_scale=0.1, nseed=212, cseed=213)
TRAIN_CASES = {"bicubic_train": dict(_TRAIN)}
# the same case with the reference's gradients to rays, poses, focal, c, image_shape and depths (tools/gen_camgrad_golden.py's kind "index")
CAMGRAD_CASES = {"bicubic_camgrad": dict(_TRAIN, kind="index")}
ALL_CASES = {**CASES, **TRAIN_CASES, **CAMGRAD_CASES}

case_inputs, input_digests, mlp_dims = gix.case_inputs, gix.input_digests, gix.mlp_dims


def lookup_stats(nerf, rays, z):
    """(straddle_frac, inside_frac) of the latent lookups of the sample points, from the uv SpatialEncoder.index receives"""
    import torch
    from tests.bicubic_ref import footprint_stats
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
    uv = cap[0].double()[0]                                   # [NV, P, 2]
    h, w = enc.latent.shape[-2:]
    fp = float(enc.feature_padding)
    return footprint_stats(uv[..., 0] * ((w - 2 * fp) / w), uv[..., 1] * ((h - 2 * fp) / h), h, w)


def gen_render(name, cfg, out_dir):
    from oracle import ref_harness as rh
    sc, w, rays, noise = case_inputs(cfg)
    nerf = gix.build_reference_model(cfg, sc, w)
    ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    straddle, inside = lookup_stats(nerf, rays, ref["z_fill"])
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), rays=rays, z_fill=ref["z_fill"][0],
                   rgbsigma=ref["rgbsigma"][0], weights=ref["weights"][0], rgb=ref["rgb"][0], depth=ref["depth"][0],
                   straddle_frac=np.float64(straddle), inside_frac=np.float64(inside))
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return f"NR={rays.shape[1]} straddle_frac={straddle:.3f} inside_frac={inside:.3f}"


def gen_train(name, cfg, out_dir, leaves):
    """``leaves``: also the gradients to the geometric leaves (tools/gen_camgrad_golden.py's fixture layout), else ``latent_grad``
    (tools/gen_index_golden.py's)"""
    import torch
    from oracle import ref_harness as rh
    from oracle.gen_golden import grad_probe_indices
    sc, w, rays, noise = case_inputs(cfg)
    nerf = gix.build_reference_model(cfg, sc, w)
    ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    straddle, inside = lookup_stats(nerf, rays, ref["z_fill"])
    z = torch.from_numpy(ref["z_fill"])
    enc = nerf.encoder
    enc.latent = enc.latent.clone().requires_grad_(True)
    for p in nerf.mlp_fine.parameters():
        p.requires_grad_(True)
    rays_t = torch.from_numpy(rays).clone()
    if leaves:
        rays_t.requires_grad_(True)
        nerf.poses, nerf.focal, nerf.c = (t.clone().requires_grad_(True) for t in (nerf.poses, nerf.focal, nerf.c))
        nerf.image_shape = nerf.image_shape.clone().requires_grad_(True)
        enc.depths = enc.depths.clone().requires_grad_(True)
    rend = rh.import_reference().NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"],
                                                 white_bkgd=sc.white_bkgd)
    weights, rgb, depth = rend.composite(nerf, rays_t, z)
    c_rgb, c_depth, _ = gcg.cotangents(cfg, rays.shape[1])
    loss = (rgb * torch.from_numpy(c_rgb)).sum() + (depth * torch.from_numpy(c_depth)).sum()
    loss.backward()
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), z_fill=ref["z_fill"],
                   rgb=rgb.detach().numpy(), depth=depth.detach().numpy(), straddle_frac=np.float64(straddle),
                   inside_frac=np.float64(inside))
    lg = enc.latent.grad.numpy()
    if leaves:
        ts = dict(rays=rays_t, poses=nerf.poses, focal=nerf.focal, c=nerf.c, image_shape=nerf.image_shape, depths=enc.depths)
        for k, t in ts.items():
            fixture[f"grad/{k}"] = (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().astype(np.float32)
        fixture["latent_grad_norm"] = np.float64(np.sqrt((lg.astype(np.float64) ** 2).sum()))
        fixture["latent_grad_max"] = np.float64(np.abs(lg).max())
    else:
        fixture["latent_grad"] = lg
    for pname, p in nerf.mlp_fine.named_parameters():
        gnp = p.grad.numpy()
        idx = grad_probe_indices(gnp.shape)
        fixture[f"g_sum/{pname}"] = np.float64(gnp.astype(np.float64).sum())
        fixture[f"g_norm/{pname}"] = np.float64(np.sqrt((gnp.astype(np.float64) ** 2).sum()))
        fixture[f"g_probe/{pname}"] = gnp.reshape(-1)[idx]
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return f"NR={rays.shape[1]} straddle_frac={straddle:.3f} inside_frac={inside:.3f} |latent_grad|={np.abs(lg).max():.3e}"


def main():
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in ALL_CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        msg = gen_render(name, cfg, out_dir) if name in CASES else gen_train(name, cfg, out_dir, leaves=name in CAMGRAD_CASES)
        path = out_dir / f"{name}.npz"
        print(f"{name}: bicubic/{cfg['padding']} {msg} -> {path.name} {path.stat().st_size / 1e6:.2f} MB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
