"""Golden vectors of the gradients to the TARGET camera: the UNMODIFIED reference's ``gen_rays`` (src/util/cam_geometry.py:36-79) ->
``NeRFRendererDGS.composite`` + ``PixelNeRF.forward`` (src/models/nerf_renderer.py:286-365, src/models/pixelnerf.py:55-145) on the CPU,
with autograd to the target ``extrinsics``, ``intrinsics``, ``z_near`` and ``z_far``, next to the MLP / latent gradient norms.  Runs only
where the reference source tree exists (``oracle.ref_harness.import_reference``); the GPU tests read the committed
``tests/golden/targetcam_*.npz`` only.

    python tools/gen_targetcam_golden.py            # (re)writes tests/golden/targetcam_*.npz
    python tools/gen_targetcam_golden.py --case=targetcam_zeros

Same scheme as tools/gen_camgrad_golden.py: inputs rebuilt from seeds (``case_inputs``), sha256 digests of them, the same cotangents,
the reference's own samples injected (its sampler and fill-up run under no_grad on the generated rays; the samples are then constants,
which is what the training path does too -- see DESIGN §7 on near / far).  One small target image (about 200 rays) per case.  Names
start with ``targetcam_``: tests/conftest.py parametrises over ``g[0-9]*.npz``.
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
from synthetic import synth  # noqa: E402
from tools import gen_index_golden as gix  # noqa: E402

# target image: H x W pixels, camera on the scene's circle at `yaw`, focal scaled by (fsx, fsy), principal point moved by (dcx, dcy)
_T = dict(H=10, W=20, yaw=0.15, fsx=1.0, fsy=0.95, dcx=0.6, dcy=-0.4)
CASES = {
    "targetcam_facescape": dict(TRAIN_CASE, kind="oracle", interp="bilinear", padding="border", target=_T),
    "targetcam_dtu": dict(TRAIN_CASE_DTU, kind="oracle", interp="bilinear", padding="border",
                          target=dict(_T, H=12, W=16, yaw=-0.1, fsx=0.9, fsy=1.0, dcx=-0.3, dcy=0.5)),
    "targetcam_zeros": dict(gix.TRAIN_CASES["index_train_zeros"], kind="index", target=dict(_T, yaw=0.2, fsx=0.5, fsy=0.5)),
    # a non-standard fusion MLP (the shape-general training path, train_any_shape)
    "targetcam_gen_h128": dict(interp="bilinear", padding="border", scene=dict(H=16, W=16, dataset="facescape", feature_padding=4, NV=2,
                                                                            seed=300, C=256),
                               num_freqs=6, mlp=dict(d_hidden=128, n_blocks=4, combine_layer=2), K=8, NC=64, G=3, ray_stride=4,
                               focal_scale=1.0, wseed=301, bias_scale=0.1, nseed=302, cseed=303, kind="index",
                               target=dict(_T, H=14, W=14, yaw=-0.2)),
}


def target_camera(cfg, sc):
    """the case's target camera: dict(E [1,4,4], K [1,3,3], near [1], far [1], H, W) in float32"""
    t = cfg["target"]
    H, W = t["H"], t["W"]
    E = synth.look_at_origin_w2c(t["yaw"], sc.meta["cam_radius"])[None]
    K = synth.intrinsics(W, H)
    K[0, 0] *= np.float32(t["fsx"])
    K[1, 1] *= np.float32(t["fsy"])
    K[0, 2] += np.float32(t["dcx"])
    K[1, 2] += np.float32(t["dcy"])
    return dict(E=np.ascontiguousarray(E, np.float32), K=np.ascontiguousarray(K[None], np.float32),
                near=np.array([sc.near], np.float32), far=np.array([sc.far], np.float32), H=H, W=W)


def case_inputs(cfg):
    """(scene, weights, target camera, noise) of a case, rebuilt from its seeds (shared by the generator and the tests)"""
    if cfg["kind"] == "oracle":
        from oracle.gen_golden import case_inputs as ci
        sc, w, _, _ = ci(cfg)
    else:
        sc, w, _, _ = gix.case_inputs(cfg)
    cam = target_camera(cfg, sc)
    noise = synth.make_noise(cam["H"] * cam["W"], cfg["NC"], cfg["G"], cfg["K"], seed=cfg["nseed"])
    return sc, w, cam, noise


def _cam_array(cam):
    return np.concatenate([cam["E"].ravel(), cam["K"].ravel(), cam["near"], cam["far"],
                           np.array([cam["H"], cam["W"]], np.float32)])


def input_digests(sc, w, cam, noise):
    from oracle.gen_golden import input_digests as _digests
    return _digests(sc, w, _cam_array(cam), noise)


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
    sc, w, cam, noise = case_inputs(cfg)
    nerf = rh.build_model(sc, w) if cfg["kind"] == "oracle" else gix.build_reference_model(cfg, sc, w)
    ref = rh.import_reference()
    from src.util.cam_geometry import gen_rays
    H, W = cam["H"], cam["W"]
    NR = H * W
    leaves = {k: torch.from_numpy(cam[k]).clone().requires_grad_(True) for k in ("E", "K", "near", "far")}
    with torch.no_grad():
        rays0 = gen_rays(leaves["E"], leaves["K"], W, H, leaves["near"], leaves["far"]).reshape(1, NR, 8).contiguous()
    run = rh.run_reference(nerf, rays0.numpy(), cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
    z = torch.from_numpy(run["z_fill"])
    enc = nerf.encoder
    enc.latent = enc.latent.clone().requires_grad_(True)
    for p in nerf.mlp_fine.parameters():
        p.requires_grad_(True)
    rays = gen_rays(leaves["E"], leaves["K"], W, H, leaves["near"], leaves["far"]).reshape(1, NR, 8)
    rend = ref.NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"], white_bkgd=sc.white_bkgd)
    weights, rgb, depth = rend.composite(nerf, rays, z)
    c_rgb, c_depth, c_w = cotangents(cfg, NR)
    loss = (rgb * torch.from_numpy(c_rgb)).sum() + (depth * torch.from_numpy(c_depth)).sum()
    if c_w is not None:
        loss = loss + (weights * torch.from_numpy(c_w)).sum()
    loss.backward()
    g = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().astype(np.float32)
    fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, cam, noise)), z_fill=run["z_fill"],
                   rgb=rgb.detach().numpy(), depth=depth.detach().numpy(), **{"grad/extrinsics": g(leaves["E"]),
                   "grad/intrinsics": g(leaves["K"]), "grad/z_near": g(leaves["near"]), "grad/z_far": g(leaves["far"])})
    lg = enc.latent.grad.numpy().astype(np.float64)
    fixture["latent_grad_norm"] = np.float64(np.sqrt((lg ** 2).sum()))
    for pname, p in nerf.mlp_fine.named_parameters():
        fixture[f"g_norm/{pname}"] = np.float64(np.sqrt((p.grad.numpy().astype(np.float64) ** 2).sum()))
    np.savez_compressed(out_dir / f"{name}.npz", **fixture)
    return (f"NR={NR} max|grad| E={np.abs(fixture['grad/extrinsics']).max():.2e} K={np.abs(fixture['grad/intrinsics']).max():.2e} "
            f"far={float(np.abs(fixture['grad/z_far']).max()):.2e} near={float(np.abs(fixture['grad/z_near']).max()):.2e}")


def main():
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        msg = gen(name, cfg, out_dir)
        path = out_dir / f"{name}.npz"
        print(f"{name}: {msg} -> {path.name} {path.stat().st_size / 1e6:.2f} MB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
