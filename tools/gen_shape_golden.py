"""Golden vectors of the shape-general inference path: the UNMODIFIED reference PixelNeRF built with non-standard ResnetFC /
PositionalEncoding configurations, rendered on the CPU.  Runs only where the reference source tree exists
(``oracle.ref_harness.import_reference``); the GPU tests read the committed ``tests/golden/shape_*.npz`` only.

    python tools/gen_shape_golden.py            # (re)writes tests/golden/shape_*.npz
    python tools/gen_shape_golden.py --case=shape_a_h128_nv2

Same scheme as oracle/gen_golden.py: every input is rebuilt from seeds (``case_inputs``, shared with the tests) and the fixture
stores sha256 digests of the seeded inputs next to the reference's outputs.  The samples are the reference's own (sampler with
replayed noise); the tests inject them (``z_samples``), so a last-ulp flip of erf in the short-list cannot change what is
compared.  The names start with ``shape_``: tests/conftest.py parametrises its suites over ``g[0-9]*.npz``.
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

_SCENE = dict(H=32, W=32, dataset="facescape", feature_padding=4)
_RENDER = dict(K=24, NC=200, G=8, ray_stride=3, focal_scale=1.0, bias_scale=0.1)

# name: scene (NV, seed, C = d_latent), model (ResnetFC kwargs the config would carry + num_freqs), seeds
CASES = {
    # (a) the constructor's default width, Facescape's view count
    "shape_a_h128_nv2": dict(scene=dict(_SCENE, NV=2, seed=40, C=512), num_freqs=6,
                             mlp=dict(d_hidden=128, n_blocks=5, combine_layer=3), wseed=41, nseed=42, **_RENDER),
    # (b) Softplus activations
    "shape_b_h256_softplus_nv4": dict(scene=dict(_SCENE, NV=4, seed=43, C=512), num_freqs=6,
                                      mlp=dict(d_hidden=256, n_blocks=4, combine_layer=2, beta=100.0), wseed=44, nseed=45, **_RENDER),
    # (c) only d_in changes (num_freqs = 4: d_in = 39)
    "shape_c_h512_f4_nv3": dict(scene=dict(_SCENE, NV=3, seed=46, C=512), num_freqs=4,
                                mlp=dict(d_hidden=512, n_blocks=5, combine_layer=3), wseed=58, nseed=48, **_RENDER),
    # (d) a smaller encoder (num_layers = 3: 256 latent channels)
    "shape_d_lat256_h64_nv4": dict(scene=dict(_SCENE, NV=4, seed=49, C=256), num_freqs=6,
                                   mlp=dict(d_hidden=64, n_blocks=3, combine_layer=1), wseed=50, nseed=51, **_RENDER),
    # (e) the ResnetFC constructor's defaults as they stand (d_hidden 128, combine_layer 1000: no mean over views, NV = 1)
    "shape_e_defaults_nv1": dict(scene=dict(_SCENE, NV=1, seed=52, C=512), num_freqs=6,
                                 mlp=dict(n_blocks=5), wseed=53, nseed=54, **_RENDER),
}
RESNETFC_DEFAULTS = dict(d_hidden=128, n_blocks=5, combine_layer=1000, beta=0.0)   # resnetfc.py:72-82
ENCODER_LAYERS = {64: 1, 128: 2, 256: 3, 512: 4, 1024: 5}                           # image_encoder.py:56


def mlp_dims(cfg):
    """ResnetFC constructor arguments of a case, defaults filled in, plus d_in / d_latent as PixelNeRF passes them (:18-24)"""
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
    """The reference PixelNeRF with this case's configuration (the YAML keys poscode_conf, encoder_conf, mlp_fine_conf)"""
    import torch
    from oracle import ref_harness as rh
    ref = rh.import_reference()
    mlp_kwargs = dict(cfg["mlp"], combine_type="average")
    nerf = ref.PixelNeRF(
        poscode_conf=NS(kwargs=dict(num_freqs=cfg["num_freqs"], freq_factor=6.28, include_input=True)),
        encoder_conf=NS(module="src.models.image_encoder.SpatialEncoder",
                        kwargs=dict(image_padding=2 * sc.feature_padding, padding_pe=4, pretrained=False,
                                    num_layers=ENCODER_LAYERS[sc.C])),
        mlp_fine_conf=NS(module="src.models.resnetfc.ResnetFC", kwargs=mlp_kwargs))
    res = nerf.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    enc = nerf.encoder
    enc.depths, enc.depths_std, enc.normals = t(sc.depths), t(sc.depths_std), t(sc.normals)
    enc.nviews, enc.nobjects = sc.NV, sc.poses.shape[0]
    enc.latent = t(sc.latent)
    nerf.poses, nerf.focal, nerf.c, nerf.image_shape = t(sc.poses), t(sc.focal), t(sc.c), t(sc.image_shape)
    assert enc.feature_padding == sc.feature_padding and enc.latent_size == sc.C
    return nerf.eval()


def main():
    from oracle import ref_harness as rh
    out_dir = ROOT / "tests" / "golden"
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, cfg in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        sc, w, rays, noise = case_inputs(cfg)
        nerf = build_reference_model(cfg, sc, w)
        ref = rh.run_reference(nerf, rays, cfg["K"], cfg["NC"], cfg["G"], noise, white_bkgd=sc.white_bkgd, want_internals=False)
        fixture = dict(config=json.dumps(cfg), digests=json.dumps(input_digests(sc, w, rays, noise)), rays=rays,
                       z_fill=ref["z_fill"][0], rgbsigma=ref["rgbsigma"][0], weights=ref["weights"][0], rgb=ref["rgb"][0],
                       depth=ref["depth"][0])
        path = out_dir / f"{name}.npz"
        np.savez_compressed(path, **fixture)
        print(f"{name}: NR={rays.shape[1]} dims={mlp_dims(cfg)} sigma_max={ref['rgbsigma'][..., 3].max():.2f} "
              f"-> {path.name} {path.stat().st_size / 1e6:.2f} MB ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
