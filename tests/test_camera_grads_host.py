"""Host-side checks of the training path's gradients to rays, source cameras and depth maps (no GPU): the C ABI's new entry points
and their argument checks, the fixture set of tools/gen_camgrad_golden.py, and the routing of a non-standard model."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
SO = ROOT / "diner_amd" / "lib" / "libdiner_hip.so"
NEW_SYMBOLS = ("diner_composite_backward_far", "diner_train_camera_workspace_floats", "diner_train_point_inputs_backward")


def test_new_symbols_declared_exported_and_abi_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SYMBOLS, name
    if not SO.exists():
        pytest.skip("library not built")
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.diner_version() == 3


def _scene(_lib):
    sc = _lib.DinerScene(SB=1, NV=2, H=4, W=4, h=4, w=4, C=512, num_freqs=6, image_w=4.0, image_h=4.0)
    sc.poses = sc.focal = sc.c = sc.maps = 16   # never dereferenced: every call below is rejected before any launch
    return sc


def test_null_and_inconsistent_arguments_are_invalid_with_a_message():
    from diner_amd import _lib
    if not SO.exists():
        pytest.skip("library not built")
    lib = _lib.lib()
    E = -1   # DINER_E_INVALID
    assert lib.diner_train_camera_workspace_floats(-1, 4, 2) == -1
    assert lib.diner_train_camera_workspace_floats(8, 4, 2) == 8 * 4 * 2 * 24 + 2 * 256 * 18
    sc = _scene(_lib)
    args = lambda **kw: [kw.get(k, 16) for k in ("lat", "rays", "z")] + [8, 4, kw.get("sb", 0)] + \
        [kw.get(k, 16) for k in ("d_in56", "d_zlat")] + [None, kw.get("ws", 16)] + [None] * 6 + [None]
    assert lib.diner_train_point_inputs_backward(None, None, *args()) == E
    assert b"scene" in lib.diner_last_error()
    assert lib.diner_train_point_inputs_backward(C.byref(sc), None, *args(d_zlat=None)) == E
    assert b"NULL" in lib.diner_last_error()
    assert lib.diner_train_point_inputs_backward(C.byref(sc), None, *args(ws=None)) == E
    assert b"NULL" in lib.diner_last_error()
    assert lib.diner_train_point_inputs_backward(C.byref(sc), None, *args(sb=1)) == E
    assert b"sb 1" in lib.diner_last_error()
    bad = _lib.DinerLatentIndex(0, 7)
    assert lib.diner_train_point_inputs_backward(C.byref(sc), C.byref(bad), *args()) == E
    assert b"latent index" in lib.diner_last_error()
    sc.C = 256
    assert lib.diner_train_point_inputs_backward(C.byref(sc), None, *args()) == E
    assert b"latent C 256" in lib.diner_last_error()
    assert lib.diner_composite_backward_far(16, 16, 16, 16, None, None, 4, 2, 0, 16, None, None) == E
    assert b"NULL" in lib.diner_last_error()
    assert lib.diner_composite_backward_far(16, 16, 16, 16, None, None, 4, 0, 0, 16, 16, None) == E
    assert b"N / K" in lib.diner_last_error()


def test_fixture_set_covers_the_five_cases():
    from tools.gen_camgrad_golden import CASES
    assert set(CASES) == {"camgrad_facescape", "camgrad_dtu", "camgrad_zeros", "camgrad_reflection", "camgrad_nearest"}
    modes = {(c["interp"], c["padding"]) for c in CASES.values()}
    assert {("bilinear", "border"), ("bilinear", "zeros"), ("bilinear", "reflection"), ("nearest", "border")} <= modes
    assert CASES["camgrad_facescape"]["scene"]["NV"] == 2 and CASES["camgrad_dtu"]["scene"]["NV"] == 3
    assert CASES["camgrad_dtu"].get("weights_cotangent")
    total = 0
    for name in CASES:
        p = GOLDEN / f"{name}.npz"
        assert p.exists(), p
        assert not re.fullmatch(r"g[0-9].*\.npz", p.name)    # not parametrised by tests/conftest.py
        assert p.stat().st_size < 1 << 20
        total += p.stat().st_size
    assert total < 4 << 20


@pytest.mark.parametrize("name", ["camgrad_facescape", "camgrad_dtu", "camgrad_zeros", "camgrad_reflection", "camgrad_nearest"])
def test_fixture_digests_regenerate_from_their_seeds(name):
    from tools.gen_camgrad_golden import CASES, LEAVES, case_inputs, input_digests
    data = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    cfg = json.loads(str(data["config"]))
    assert cfg == json.loads(json.dumps(CASES[name]))
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    shapes = dict(rays=rays.shape, poses=sc.poses.shape, focal=sc.focal.shape, c=sc.c.shape, image_shape=sc.image_shape.shape,
                  depths=sc.depths.shape)
    for k in LEAVES:
        assert data[f"grad/{k}"].shape == tuple(shapes[k]), k
    assert (data["grad/rays"][..., 6] == 0).all()            # near feeds only the sampler
    assert np.abs(data["grad/poses"]).max() > 0 and np.abs(data["grad/depths"]).max() > 0
    if cfg["padding"] != "border" or cfg["kind"] == "index":
        assert float(data["out_frac"]) > 0.1                 # the clipped / outside-the-map branches are exercised


def test_non_standard_model_with_only_rays_requiring_grad_raises_inference():
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(8, 8, 1, seed=0, feature_padding=2, C=512)
    dims = dict(d_hidden=64, n_blocks=2, combine_layer=1)
    w = synth.make_mlp_weights(1, d_in=55, d_latent=512, **dims)
    m = model_from_scene(sc, w, device="cpu", d_latent=512, **dims)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(False)
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1)
    rays = torch.zeros(1, 2, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="inference"):
        r(m, rays)                                           # raised before any device work
