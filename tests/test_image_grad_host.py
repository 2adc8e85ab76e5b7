"""Host-side checks of the target-camera gradients (no GPU): the backward of gen_rays in the C ABI (declared, exported, bound; argument
validation before any launch), the ``targetcam_*`` fixtures of tools/gen_targetcam_golden.py, and render_image's refusal of a
non-standard model under autograd without train_any_shape."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW_SYMBOLS = ("diner_gen_rays_backward_workspace_floats", "diner_gen_rays_backward")
NAMES = ["targetcam_facescape", "targetcam_dtu", "targetcam_zeros", "targetcam_gen_h128"]
FAKE = C.c_void_p(1 << 20)   # a non-NULL pointer that no call below may dereference: every call fails validation first


def test_new_symbols_declared_exported_and_abi_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3 == _lib.ABI_VERSION
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.diner_version() == 3


def test_bad_arguments_return_invalid_with_a_message():
    from diner_amd import _lib
    lib = _lib.lib()
    E = -1   # DINER_E_INVALID
    assert lib.diner_gen_rays_backward_workspace_floats(-1, 4, 4) == -1
    assert lib.diner_gen_rays_backward_workspace_floats(2, 0, 4) == -1
    assert lib.diner_gen_rays_backward_workspace_floats(2, 10, 20) == 2 * 1 * 18 * 2          # one block per camera, 18 doubles
    assert lib.diner_gen_rays_backward_workspace_floats(1, 1024, 1024) == 256 * 18 * 2       # at most 256 blocks per camera
    ok = dict(e=FAKE, k=FAKE, g=FAKE, B=2, H=4, W=4, de=FAKE, dk=FAKE, dn=FAKE, df=FAKE, ws=FAKE)
    call = lambda **kw: lib.diner_gen_rays_backward(*[kw.get(k, v) for k, v in ok.items()], None)
    assert call(B=-1) == E and b"bad size" in lib.diner_last_error()
    assert call(W=0) == E and b"bad size" in lib.diner_last_error()
    for k in ("e", "k", "g", "de", "dk", "dn", "df", "ws"):
        assert call(**{k: None}) == E, k
        assert b"NULL" in lib.diner_last_error(), k
    assert call(ws=C.c_void_p((1 << 20) + 4)) == E and b"aligned" in lib.diner_last_error()
    assert call(B=0) == 0                                                                   # nothing to do, nothing launched


def test_fixture_set_and_digests():
    from tools.gen_targetcam_golden import CASES, case_inputs, input_digests
    assert set(CASES) == set(NAMES)
    assert CASES["targetcam_facescape"]["scene"]["NV"] == 2 and CASES["targetcam_facescape"]["scene"]["dataset"] == "facescape"
    assert CASES["targetcam_dtu"]["scene"]["NV"] == 3 and CASES["targetcam_dtu"]["scene"]["dataset"] == "dtu"
    assert CASES["targetcam_zeros"]["padding"] == "zeros"
    assert CASES["targetcam_gen_h128"]["kind"] == "index" and CASES["targetcam_gen_h128"]["mlp"]["d_hidden"] == 128
    for name in NAMES:
        p = GOLDEN / f"{name}.npz"
        assert p.exists(), p
        assert not re.fullmatch(r"g[0-9].*\.npz", p.name)    # not parametrised by tests/conftest.py
        assert p.stat().st_size < 1 << 20
        data = np.load(p, allow_pickle=False)
        cfg = json.loads(str(data["config"]))
        assert cfg == json.loads(json.dumps(CASES[name]))
        sc, w, cam, noise = case_inputs(cfg)
        assert json.loads(str(data["digests"])) == input_digests(sc, w, cam, noise)
        NR = cam["H"] * cam["W"]
        assert 150 <= NR <= 260 and data["z_fill"].shape == (1, NR, cfg["K"])
        assert data["grad/extrinsics"].shape == (1, 4, 4) and data["grad/intrinsics"].shape == (1, 3, 3)
        assert (data["grad/extrinsics"][:, 3] == 0).all() and np.abs(data["grad/extrinsics"]).max() > 0
        used = np.zeros((3, 3), bool)
        used[0, 0] = used[1, 1] = used[0, 2] = used[1, 2] = True
        assert (data["grad/intrinsics"][:, ~used] == 0).all() and np.abs(data["grad/intrinsics"]).max() > 0
        assert np.abs(data["grad/z_far"]).max() > 0


def test_non_standard_model_under_autograd_in_render_image_raises_before_device_work():
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(8, 8, 1, seed=0, feature_padding=2, C=512)
    dims = dict(d_hidden=64, n_blocks=2, combine_layer=1)
    m = model_from_scene(sc, synth.make_mlp_weights(1, d_in=55, d_latent=512, **dims), device="cpu", d_latent=512, **dims)
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1)
    E = torch.from_numpy(sc.target_extrinsics)[None]
    K = torch.from_numpy(sc.target_intrinsics)[None]
    with pytest.raises(NotImplementedError, match="train_any_shape"):
        r.render_image(m, E.clone().requires_grad_(True), K, 8, 8, sc.near, sc.far)       # a target camera requires grad
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="train_any_shape"):
        r.render_image(m, E, K, 8, 8, sc.near, sc.far)                                      # forward()'s predicate
    assert r._calls == 0                                                                     # no seed drawn: nothing ran
