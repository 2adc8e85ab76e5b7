"""Golden vectors of the training path's gradients to the geometric leaves: ``rays``, ``model.poses``, ``model.focal``, ``model.c``,
``model.image_shape`` and ``encoder.depths``, from the UNMODIFIED reference's autograd on the CPU (``NeRFRendererDGS.composite`` +
``PixelNeRF.forward``, reference src/models/nerf_renderer.py:286-365, src/models/pixelnerf.py:55-145), next to its MLP / latent
gradient summaries.  Runs only where the reference source tree exists (``oracle.ref_harness.import_reference``); the GPU tests read
the committed ``tests/golden/camgrad_*.npz`` only.

    python tools/gen_camgrad_golden.py            # (re)writes tests/golden/camgrad_*.npz
    python tools/gen_camgrad_golden.py --case=camgrad_zeros

Same scheme as tools/gen_index_golden.py ``gen_train``: inputs rebuilt from seeds (``case_inputs``), sha256 digests of them, the same
cotangents (``oracle.gen_golden.train_cotangents`` / ``weights_cotangent``), the reference's samples injected.  ``out_frac`` records the
fraction of (view, sample) latent lookups whose coordinate was clipped (border, reflection) or left the map (zeros), so that the
zero-gradient branches of grid_sample's grid gradient are known to be exercised.  Names start with ``camgrad_``: tests/conftest.py
parametrises over ``g[0-9]*.npz``.
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

from oracle.gen_golden import TRAIN_CASE, TRAIN_CASE_DTU  # noqa: E402
from tools import gen_index_golden as gix  # noqa: E402

# "oracle": a case of oracle/gen_golden.py (the default lookup mode, the oracle's model builder); "index": a gen_index_golden-style
# case (any lookup mode)
CASES = {
    "camgrad_facescape": dict(TRAIN_CASE, kind="oracle", interp="bilinear", padding="border"),
    "camgrad_dtu": dict(TRAIN_CASE_DTU, kind="oracle", interp="bilinear", padding="border"),
    "camgrad_zeros": dict(gix.TRAIN_CASES["index_train_zeros"], kind="index"),
    "camgrad_reflection": dict(gix.TRAIN_CASES["index_train_zeros"], kind="index", padding="reflection",
                               scene=dict(gix.TRAIN_CASES["index_train_zeros"]["scene"], seed=180), wseed=181, nseed=182, cseed=183),
    "camgrad_nearest": dict(gix.TRAIN_CASES["index_train_nearest"], kind="index"),
}
LEAVES = ("rays", "poses", "focal", "c", "image_shape", "depths")


def case_inputs(cfg):
    """(scene, weights, rays, noise) of a case, rebuilt from its seeds (shared by the generator and the tests)"""
    if cfg["kind"] == "oracle":
        from oracle.gen_golden import case_inputs as ci
        return ci(cfg)
    return gix.case_inputs(cfg)


def input_digests(sc, w, rays, noise):
    from oracle.gen_golden import input_digests as _digests
    return _digests(sc, w, rays, noise)


def model_kwargs(cfg):
    """keyword arguments of synthetic.model_stub.model_from_scene for this case"""
    if cfg["kind"] == "oracle":
        return {}
    dims = {k: v for k, v in gix.mlp_dims(cfg).items() if k != "d_in"}
    return dict(num_freqs=cfg["num_freqs"], index_interp=cfg["interp"], index_padding=cfg["padding"], **dims)


def cotangents(cfg, NR):
    from oracle.gen_golden import train_cotangents, weights_cotangent
    c_rgb, c_depth = train_cotangents(NR, cfg["cseed"])
    c_w = weights_cotangent(NR, cfg["K"], cfg["cseed"]) if cfg.get("weights_cotangent") else None
    return c_rgb, c_depth, c_w


def gen(name, cfg, out_dir):
    import torch
    from oracle import ref_harness as rh
    from oracle.gen_golden import grad_probe_indices
    sc, w, rays, noise = case_inputs(cfg)
    nerf = rh.build_model(sc, w) if cfg["kind"] == "oracle" else gix.build_reference_model(cfg, sc, w)
    ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    out_frac, _ = gix.lookup_stats(nerf, dict(cfg), rays, ref["z_fill"])
    z = torch.from_numpy(ref["z_fill"])
    enc = nerf.encoder
    enc.latent = enc.latent.clone().requires_grad_(True)
    for p in nerf.mlp_fine.parameters():
        p.requires_grad_(True)
    rays_t = torch.from_numpy(rays).clone().requires_grad_(True)
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
    leaves = dict(rays=rays_t, poses=nerf.poses, focal=nerf.focal, c=nerf.c, image_shape=nerf.image_shape, depths=enc.depths)
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), z_fill=ref["z_fill"],
                   rgb=rgb.detach().numpy(), depth=depth.detach().numpy(), out_frac=np.float64(out_frac))
    for k, t in leaves.items():
        fixture[f"grad/{k}"] = (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().astype(np.float32)
    lg = enc.latent.grad.numpy().astype(np.float64)
    fixture["latent_grad_norm"] = np.float64(np.sqrt((lg ** 2).sum()))
    fixture["latent_grad_max"] = np.float64(np.abs(lg).max())
    for pname, p in nerf.mlp_fine.named_parameters():
        gnp = p.grad.numpy()
        idx = grad_probe_indices(gnp.shape)
        fixture[f"g_sum/{pname}"] = np.float64(gnp.astype(np.float64).sum())
        fixture[f"g_norm/{pname}"] = np.float64(np.sqrt((gnp.astype(np.float64) ** 2).sum()))
        fixture[f"g_probe/{pname}"] = gnp.reshape(-1)[idx]
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    mx = " ".join(f"{k}={np.abs(fixture['grad/' + k]).max():.2e}" for k in LEAVES)
    return f"NR={rays.shape[1]} out_frac={out_frac:.3f} max|grad| {mx}"


def main():
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        msg = gen(name, cfg, out_dir)
        path = out_dir / f"{name}.npz"
        print(f"{name}: {cfg['interp']}/{cfg['padding']} {msg} -> {path.name} {path.stat().st_size / 1e6:.2f} MB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
