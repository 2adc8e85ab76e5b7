"""Golden vectors of the shape-general training path (diner_amd/training_gen.py): the UNMODIFIED reference PixelNeRF built with
non-standard ResnetFC / PositionalEncoding configurations, differentiated by its own autograd on the CPU (``NeRFRendererDGS.composite``
+ ``PixelNeRF.forward``, reference src/models/nerf_renderer.py:286-365, src/models/pixelnerf.py:55-145).  Runs only where the reference
source tree exists (``oracle.ref_harness.import_reference``); the GPU tests read the committed ``tests/golden/trainshape_*.npz`` only.

    python tools/gen_trainshape_golden.py            # (re)writes tests/golden/trainshape_*.npz
    python tools/gen_trainshape_golden.py --case=trainshape_a_h128_nv2

Same scheme as tools/gen_camgrad_golden.py: inputs rebuilt from seeds (``case_inputs``), sha256 digests of them, the cotangents of
``oracle.gen_golden.train_cotangents`` (+ ``weights_cotangent`` where a case asks for it), the reference's samples injected.  Each
fixture holds rgb / depth, the sum, norm and probes of every named parameter's gradient, the latent gradient's norm, max and probes, and
the full gradients of the geometric leaves where the case asks for them (``leaves``).  Names start with ``trainshape_``:
tests/conftest.py parametrises over ``g[0-9]*.npz``.
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

from tools import gen_index_golden as gix  # noqa: E402

_SCENE = dict(H=16, W=16, dataset="facescape", feature_padding=4)
_RENDER = dict(K=8, NC=64, G=3, ray_stride=4, focal_scale=1.0, bias_scale=0.1)
LEAVES = ("rays", "poses", "focal", "c", "image_shape", "depths")

# name: lookup mode, scene (NV, seed, C = d_latent), model (ResnetFC kwargs + num_freqs), seeds, cotangents, leaves
CASES = {
    # (a) the constructor's default width, the standard block layout, Facescape's view count
    "trainshape_a_h128_nv2": dict(interp="bilinear", padding="border", scene=dict(_SCENE, NV=2, seed=200, C=512), num_freqs=6,
                                  mlp=dict(d_hidden=128, n_blocks=5, combine_layer=3), wseed=201, nseed=202, cseed=203, leaves=False,
                                  **_RENDER),
    # (b) Softplus activations, a cotangent on the compositing weights
    "trainshape_b_h256_softplus_nv4": dict(interp="bilinear", padding="border", scene=dict(_SCENE, NV=4, seed=204, C=512), num_freqs=6,
                                           mlp=dict(d_hidden=256, n_blocks=4, combine_layer=2, beta=100.0), wseed=205, nseed=206, cseed=207,
                                           weights_cotangent=True, leaves=False, **_RENDER),
    # (c) num_freqs 4 (d_in 39), d_hidden 96, DTU near / far and black background, every camera leaf
    "trainshape_c_h96_f4_dtu": dict(interp="bilinear", padding="border", scene=dict(_SCENE, H=20, W=16, NV=3, seed=208, C=512, dataset="dtu"),
                                    num_freqs=4, mlp=dict(d_hidden=96, n_blocks=5, combine_layer=3), wseed=209, nseed=210, cseed=211,
                                    leaves=True, **dict(_RENDER, K=12, NC=96, G=4)),
    # (d) a smaller encoder (num_layers = 3: 256 latent channels), nearest / zeros lookup, camera leaves
    "trainshape_d_lat256_h64_nearest_zeros": dict(interp="nearest", padding="zeros", scene=dict(_SCENE, NV=2, seed=212, C=256,
                                                                                              feature_padding=0),
                                                  num_freqs=6, mlp=dict(d_hidden=64, n_blocks=3, combine_layer=1), wseed=213, nseed=214,
                                                  cseed=215, leaves=True, **dict(_RENDER, focal_scale=0.5)),
    # (e) the ResnetFC constructor's defaults (d_hidden 128, combine_layer 1000: no mean over views), one view
    "trainshape_e_defaults_nv1": dict(interp="bilinear", padding="border", scene=dict(_SCENE, NV=1, seed=216, C=512), num_freqs=6,
                                      mlp=dict(n_blocks=5), wseed=217, nseed=218, cseed=219, leaves=False, **_RENDER),
    # (f) combine_layer 0: the mean over views right after lin_in, no lin_z (the latent's gradient is zero)
    "trainshape_f_combine0_nv3": dict(interp="bilinear", padding="border", scene=dict(_SCENE, NV=3, seed=220, C=512), num_freqs=6,
                                      mlp=dict(d_hidden=128, n_blocks=3, combine_layer=0), wseed=221, nseed=222, cseed=223, leaves=True,
                                      **_RENDER),
}
LATENT_PROBES = 64


def case_inputs(cfg):
    """(scene, weights, rays, noise) of a case, rebuilt from its seeds (shared by the generator and the tests)"""
    return gix.case_inputs(cfg)


def input_digests(sc, w, rays, noise):
    from oracle.gen_golden import input_digests as _digests
    return _digests(sc, w, rays, noise)


def model_kwargs(cfg):
    """keyword arguments of synthetic.model_stub.model_from_scene for this case"""
    dims = {k: v for k, v in gix.mlp_dims(cfg).items() if k != "d_in"}
    return dict(num_freqs=cfg["num_freqs"], index_interp=cfg["interp"], index_padding=cfg["padding"], **dims)


def cotangents(cfg, NR):
    from oracle.gen_golden import train_cotangents, weights_cotangent
    c_rgb, c_depth = train_cotangents(NR, cfg["cseed"])
    c_w = weights_cotangent(NR, cfg["K"], cfg["cseed"]) if cfg.get("weights_cotangent") else None
    return c_rgb, c_depth, c_w


def latent_probe_indices(shape):
    from oracle.gen_golden import grad_probe_indices
    return grad_probe_indices(shape, n=LATENT_PROBES, seed=7)


def gen(name, cfg, out_dir):
    import torch
    from oracle import ref_harness as rh
    from oracle.gen_golden import grad_probe_indices
    torch.manual_seed(0)
    sc, w, rays, noise = case_inputs(cfg)
    nerf = gix.build_reference_model(cfg, sc, w)
    ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    z = torch.from_numpy(ref["z_fill"])
    enc = nerf.encoder
    enc.latent = enc.latent.clone().requires_grad_(True)
    for p in nerf.mlp_fine.parameters():
        p.requires_grad_(True)
    leaves = cfg["leaves"]
    rays_t = torch.from_numpy(rays).clone().requires_grad_(leaves)
    if leaves:
        nerf.poses = nerf.poses.clone().requires_grad_(True)
        nerf.focal = nerf.focal.clone().requires_grad_(True)
        nerf.c = nerf.c.clone().requires_grad_(True)
        nerf.image_shape = nerf.image_shape.clone().requires_grad_(True)
        enc.depths = enc.depths.clone().requires_grad_(True)
    rend = rh.import_reference().NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"],
                                                 white_bkgd=sc.white_bkgd)
    weights, rgb, depth = rend.composite(nerf, rays_t, z)
    c_rgb, c_depth, c_w = cotangents(cfg, rays.shape[1])
    loss = (rgb * torch.from_numpy(c_rgb)).sum() + (depth * torch.from_numpy(c_depth)).sum()
    if c_w is not None:
        loss = loss + (weights * torch.from_numpy(c_w)).sum()
    loss.backward()
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), z_fill=ref["z_fill"],
                   rgb=rgb.detach().numpy(), depth=depth.detach().numpy())
    if leaves:
        tensors = dict(rays=rays_t, poses=nerf.poses, focal=nerf.focal, c=nerf.c, image_shape=nerf.image_shape, depths=enc.depths)
        for k, t in tensors.items():
            fixture[f"grad/{k}"] = (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().astype(np.float32)
    lgt = enc.latent.grad if enc.latent.grad is not None else torch.zeros_like(enc.latent)   # combine_layer 0: the latent is not used
    lg = lgt.numpy().astype(np.float64)
    fixture["latent_grad_norm"] = np.float64(np.sqrt((lg ** 2).sum()))
    fixture["latent_grad_max"] = np.float64(np.abs(lg).max())
    fixture["latent_grad_probe"] = lgt.numpy().reshape(-1)[latent_probe_indices(lg.shape)]
    for pname, p in nerf.mlp_fine.named_parameters():
        gnp = p.grad.numpy()
        idx = grad_probe_indices(gnp.shape)
        fixture[f"g_sum/{pname}"] = np.float64(gnp.astype(np.float64).sum())
        fixture[f"g_norm/{pname}"] = np.float64(np.sqrt((gnp.astype(np.float64) ** 2).sum()))
        fixture[f"g_probe/{pname}"] = gnp.reshape(-1)[idx]
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return f"NR={rays.shape[1]} dims={gix.mlp_dims(cfg)} |latent grad|={fixture['latent_grad_norm']:.3e}"


def main():
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        msg = gen(name, cfg, out_dir)
        path = out_dir / f"{name}.npz"
        print(f"{name}: {cfg['interp']}/{cfg['padding']} {msg} -> {path.name} {path.stat().st_size / 1e6:.3f} MB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
