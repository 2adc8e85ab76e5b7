"""Golden vectors of conv1's input (diner_encoder_input): the UNMODIFIED reference PixelNeRF, built on the CPU through
``oracle.ref_harness`` with the harness's fake trunk, runs ``encode`` (reference src/models/pixelnerf.py:35-53); a forward pre-hook on
``encoder.model.conv1`` captures what ``Normalize`` + the head of ``SpatialEncoder.forward`` (src/models/image_encoder.py:222-232) hand
to the trunk.  Each fixture holds the seeded inputs next to the captured tensor.  Runs only where the reference source tree exists; the
tests read the committed ``tests/golden/encoder_input_*.npz`` only (data, no program text).

    python tools/gen_encoder_input_golden.py            # (re)writes tests/golden/encoder_input_*.npz

``image_padding`` is even in every case: the reference asserts an integral ``feature_padding = image_padding / conv1.stride``.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"

# name -> SB, NV, H, W, image_padding, padding_pe, seed
CASES = {
    "encoder_input_p4_f4": dict(SB=1, NV=2, H=10, W=13, image_padding=4, padding_pe=4, seed=301),     # [2, 21, 18, 21]
    "encoder_input_p2_f0": dict(SB=1, NV=2, H=6, W=7, image_padding=2, padding_pe=0, seed=302),       # F = 0: 5 channels
    "encoder_input_p6_nope": dict(SB=1, NV=2, H=5, W=9, image_padding=6, padding_pe=-1, seed=303),    # pad above H, no encoding
    "encoder_input_p0": dict(SB=1, NV=2, H=8, W=6, image_padding=0, padding_pe=4, seed=304),          # pad 0: the encoding is off
}


def case_inputs(cfg):
    """seeded inputs of ``PixelNeRF.encode``: images in [0, 1), positive depths, pinhole cameras"""
    rs = np.random.RandomState(cfg["seed"])
    SB, NV, H, W = cfg["SB"], cfg["NV"], cfg["H"], cfg["W"]
    images = rs.random_sample((SB, NV, 3, H, W)).astype(np.float32)
    depths = (1.0 + rs.random_sample((SB, NV, 1, H, W))).astype(np.float32)
    depths_std = (0.004 + 0.004 * rs.random_sample((SB, NV, 1, H, W))).astype(np.float32)
    extrinsics = np.tile(np.eye(4, dtype=np.float32), (SB, NV, 1, 1))
    extrinsics[..., :3, 3] = rs.standard_normal((SB, NV, 3)).astype(np.float32)
    intrinsics = np.tile(np.array([[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]], dtype=np.float32), (SB, NV, 1, 1))
    return dict(images=images, depths=depths, depths_std=depths_std, extrinsics=extrinsics, intrinsics=intrinsics)


def generate(name):
    import torch

    from oracle import ref_harness
    cfg = CASES[name]
    ref = ref_harness.import_reference()
    torch.manual_seed(cfg["seed"])       # (the reference draws conv1's weights when the encoding is on)
    nerf = ref.PixelNeRF(
        poscode_conf=NS(kwargs=dict(num_freqs=6, freq_factor=6.28, include_input=True)),
        encoder_conf=NS(module="src.models.image_encoder.SpatialEncoder",
                        kwargs=dict(image_padding=cfg["image_padding"], padding_pe=cfg["padding_pe"], pretrained=False)),
        mlp_fine_conf=NS(module="src.models.resnetfc.ResnetFC", kwargs=dict(n_blocks=5, d_hidden=512, combine_layer=3,
                                                                            combine_type="average"))).eval()
    inp = case_inputs(cfg)
    cap = {}
    hook = nerf.encoder.model.conv1.register_forward_pre_hook(lambda mod, args: cap.setdefault("x", args[0].detach().clone()))
    with torch.no_grad():
        nerf.encode(*(torch.from_numpy(inp[k]) for k in ("images", "depths", "depths_std", "extrinsics", "intrinsics")))
    hook.remove()
    x = cap["x"].numpy()
    pad, F = cfg["image_padding"], cfg["padding_pe"]
    Cpe = 2 * (1 + 2 * F) if F >= 0 and pad > 0 else 0
    assert x.shape == (cfg["SB"] * cfg["NV"], 3 + Cpe, cfg["H"] + 2 * pad, cfg["W"] + 2 * pad) and x.dtype == np.float32, x.shape
    norm = nerf.normalize_rgb
    np.savez_compressed(GOLDEN / f"{name}.npz", config=json.dumps(cfg), conv1_input=x,
                        mean=np.asarray(norm.mean, dtype=np.float32).reshape(3), std=np.asarray(norm.std, dtype=np.float32).reshape(3), **inp)
    print(f"{name}: conv1 input {x.shape}, {(GOLDEN / (name + '.npz')).stat().st_size} bytes")


if __name__ == "__main__":
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--case=")]
    for n in (only or CASES):
        generate(n)
