"""Rendering inside a scene bounding box (diner_amd/csrc/ray_box.hip; glue.ray_box, glue.box_rays, glue.frame_from_hits) as far as it
goes without a GPU: the float64 restatement of tests/ray_box_ref.py reproduces tests/golden/ray_box.npz -- the outputs of the
UNMODIFIED reference ``get_near_far`` on gen_rays' rays (tools/gen_ray_box_golden.py) -- outside the ambiguous set, the same comparison
rejects deliberately wrong forms, the restatement's own cases that the golden cannot pin (the two deliberate differences from the
reference among them), and the new entry points' declarations, bindings and refusals before any launch."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import ray_box_ref as R

ROOT = Path(__file__).resolve().parents[1]
CAMERAS = ("48x64", "37x53", "32x32")
HIT_SHARES = {"48x64": 0.22, "37x53": 0.30, "32x32": 0.21}
NEW_SYMBOLS = ("diner_ray_box_select_workspace_floats", "diner_ray_box_select", "diner_gen_rays_box", "diner_frame_from_hits")
_fixture = {}


def fixture():
    if not _fixture:
        d = dict(np.load(ROOT / "tests" / "golden" / "ray_box.npz", allow_pickle=False))
        _fixture["index"] = json.loads(str(d.pop("index")))
        _fixture["data"] = d
    return _fixture["index"], _fixture["data"]


def golden_case(name, variant=None):
    """(the restatement's result, the reference's near / far / mask, the ambiguous set) of one golden camera"""
    index, d = fixture()
    cfg = index[name]
    mine = R.ray_box_ref(d[f"{name}.extrinsics"], d[f"{name}.intrinsics"], cfg["H"], cfg["W"], cfg["z_near"], cfg["z_far"], d["bounds"],
                         tuple(d["box_offset"]), variant=variant)
    want = dict(near=d[f"{name}.near"], far=d[f"{name}.far"], mask=d[f"{name}.mask"])
    return mine, want


def test_fixture_holds_the_cases():
    index, d = fixture()
    assert tuple(index) == CAMERAS
    assert np.array_equal(d["bounds"], np.array([[-0.12, -0.16, -0.10], [0.11, 0.15, 0.13]], np.float32))
    assert tuple(d["box_offset"]) == R.BOX_OFFSET
    for name in CAMERAS:
        cfg = index[name]
        assert f"{cfg['H']}x{cfg['W']}" == name and d[f"{name}.mask"].shape == (cfg["H"], cfg["W"])
        assert abs(d[f"{name}.mask"].mean() - HIT_SHARES[name]) < 0.01
        m = d[f"{name}.mask"]
        assert (d[f"{name}.far"][m] > d[f"{name}.near"][m]).all() and (d[f"{name}.near"][m] > 0.5).all()
    assert (ROOT / "tests" / "golden" / "ray_box.npz").stat().st_size < 100_000


@pytest.mark.parametrize("name", CAMERAS)
def test_restatement_reproduces_reference_get_near_far(name):
    mine, want = golden_case(name)
    amb = mine["ambiguous"]
    print(f"{name}: ambiguous set {amb.mean():.2%} of the pixels; mask mismatches outside it {int(((mine['mask'] != want['mask']) & ~amb).sum())}; "
          f"|near| {np.abs(mine['near'] - want['near'])[mine['mask'] & want['mask']].max():.2e}, "
          f"|far| {np.abs(mine['far'] - want['far'])[mine['mask'] & want['mask']].max():.2e}")
    assert amb.mean() <= R.CAP
    assert R.compare(mine, want, amb) == []


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("name", CAMERAS)
def test_wrong_forms_are_rejected(name, variant):
    right, want = golden_case(name)
    wrong, _ = golden_case(name, variant)
    bad = R.compare(wrong, want, right["ambiguous"])        # (the ambiguous set is the right form's: a property of the inputs)
    assert bad, f"{variant} passes the comparison on {name}"
    print(f"{name}: {variant}: {bad[0]}")


# ---- what the golden cannot pin: the restatement's own cases ---------------------------------------------------------------------------
BOX = np.array([[-0.12, -0.16, -0.10], [0.11, 0.15, 0.13]])


def test_camera_inside_the_box_hits_everywhere_from_z_near():
    E, K = R.look_at((0.02, -0.01, 0.0), target=(0.0, 0.0, 1.0)), R.intrinsics(40.0, 17, 31)
    r = R.ray_box_ref(E, K, 17, 31, 0.05, 10.0, BOX)
    assert r["mask"].all() and r["count"] == 17 * 31 and (r["near"] == 0.05).all()
    assert (r["far"] > 0.05).all() and (r["far"] < 0.5).all()
    assert np.array_equal(r["idx"], np.arange(17 * 31)) and np.array_equal(r["slot"], np.arange(17 * 31))
    # z_near beyond the exit: nothing is left of the interval
    assert not R.ray_box_ref(E, K, 17, 31, 0.6, 10.0, BOX)["mask"].any()


def test_box_behind_the_camera_is_a_miss():
    E, K = R.look_at((0.0, 0.0, -1.5), target=(0.0, 0.0, -3.0)), R.intrinsics(70.0, 32, 32)     # looking away from the box
    r = R.ray_box_ref(E, K, 32, 32, 0.1, 10.0, BOX)
    assert not r["mask"].any() and r["count"] == 0 and (r["idx"] == -1).all() and (r["slot"] == -1).all()
    assert (r["near"] == 0.1).all() and (r["far"] == 10.0).all()
    # the same camera turned round sees it: the miss above is the box behind the camera, not a frustum that passes it
    assert R.ray_box_ref(R.look_at((0.0, 0.0, -1.5)), K, 32, 32, 0.1, 10.0, BOX)["mask"].any()


def test_z_far_cuts_the_box_and_z_near_enters_it():
    E, K = R.look_at((0.0, 0.0, -1.5)), R.intrinsics(70.0, 32, 32)
    full = R.ray_box_ref(E, K, 32, 32, 0.1, 10.0, BOX)
    cut = R.ray_box_ref(E, K, 32, 32, 0.1, 1.5, BOX)             # the front face is at t ~ 1.39, the back one at t ~ 1.64
    m = full["mask"]
    assert np.array_equal(cut["mask"], m) and np.array_equal(cut["near"], full["near"])
    assert np.array_equal(cut["far"][m], np.minimum(full["far"][m], 1.5)) and (cut["far"][m] == 1.5).sum() > m.sum() // 2
    entered = R.ray_box_ref(E, K, 32, 32, 1.5, 10.0, BOX)         # rays through the box's rim leave it before 1.5: no hit any more
    assert np.array_equal(entered["mask"], m & (full["far"] > 1.5)) and entered["mask"].sum() > m.sum() // 2
    assert (entered["near"][entered["mask"]] == 1.5).all() and np.array_equal(entered["far"][entered["mask"]], full["far"][entered["mask"]])
    assert not R.ray_box_ref(E, K, 32, 32, 0.1, 1.3, BOX)["mask"].any()       # z_far in front of the box


def test_a_box_the_frustum_misses():
    E, K = R.look_at((0.0, 0.0, -1.5)), R.intrinsics(70.0, 32, 32)
    r = R.ray_box_ref(E, K, 32, 32, 0.1, 10.0, BOX + np.array([2.0, 0.0, 0.0]))
    assert not r["mask"].any() and r["count"] == 0 and r["ambiguous"].mean() <= R.CAP


def test_frame_gather():
    mask = np.zeros((3, 4), bool)
    mask[1, 1:3] = mask[2, 0] = True
    idx, slot, count = R.select_ref(mask)
    assert count == 3 and idx[:3].tolist() == [5, 6, 8] and slot.reshape(3, 4)[1].tolist() == [-1, 0, 1, -1]
    rgb_c = np.arange(9, dtype=np.float32).reshape(3, 3) / 10
    rgb, depth = R.frame_from_hits_ref(rgb_c, np.array([2.0, 3.0, 4.0], np.float32), slot, 3, 4, True)
    assert rgb.shape == (3, 3, 4) and depth.shape == (1, 3, 4)
    assert (rgb[:, ~mask] == 1.0).all() and (depth[0, ~mask] == 0.0).all()
    assert np.array_equal(rgb[:, 1, 2], rgb_c[1]) and depth[0, 2, 0] == 4.0
    assert (R.frame_from_hits_ref(rgb_c, np.zeros(3, np.float32), slot, 3, 4, False)[0][:, ~mask] == 0.0).all()


# ---- the C ABI and the Python surface ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_built_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert "ray_box.hip" in (ROOT / "diner_amd" / "csrc" / "Makefile").read_text()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
        assert m, name
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
        assert getattr(L, name)                                       # exported by the built library
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 3 == L.diner_version()


def _cam(H, W, p=64):
    from diner_amd import _lib
    cam = _lib.DinerTargetCam()
    cam.extrinsics = cam.intrinsics = cam.z_near = cam.z_far = p
    cam.H, cam.W = H, W
    return cam


def test_bad_arguments_return_codes_before_any_launch():
    from diner_amd import _lib
    L = _lib.lib()
    p = 64                                                            # a non-NULL dummy, never dereferenced
    cam = _cam(4, 5)
    sel = lambda cam, SB, b, nf, idx, slot, cnt, ws: L.diner_ray_box_select(cam, SB, b, -0.01, 0.01, nf, idx, slot, cnt, ws, None)
    err = lambda: L.diner_last_error()
    assert sel(None, 1, p, p, p, p, p, p) == -1 and b"NULL camera" in err()
    assert sel(C.byref(cam), 1, None, p, p, p, p, p) == -1 and b"NULL bounds" in err()
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert sel(C.byref(cam), 1, p, p, *args) == -1 and b"NULL pointer" in err()
    assert sel(C.byref(cam), 1, p, None, p, p, p, 66) == -1 and b"aligned" in err()          # a misaligned workspace
    assert sel(C.byref(cam), 1, p, 68, p, p, p, p) == -1 and b"near_far" in err()
    assert sel(C.byref(cam), -1, p, p, p, p, p, p) == -1 and b"negative" in err()
    assert sel(C.byref(_cam(-4, 5)), 1, p, p, p, p, p, p) == -1
    assert sel(C.byref(_cam(65536, 32768)), 1, p, p, p, p, p, p) == -3 and b"2^31" in err()
    assert sel(C.byref(cam), 65536, p, p, p, p, p, p) == -3
    broken = _cam(4, 5)
    broken.z_far = None
    assert sel(C.byref(broken), 1, p, p, p, p, p, p) == -1 and b"camera" in err()
    # nothing to do: DINER_OK without a launch, whatever the pointers
    assert sel(C.byref(cam), 0, None, None, None, None, None, None) == 0
    assert sel(C.byref(_cam(0, 5)), 3, None, None, None, None, None, None) == 0
    # one 4-byte word per workgroup of 256 pixels and scene
    assert L.diner_ray_box_select_workspace_floats(1, 16, 16) == 1
    assert L.diner_ray_box_select_workspace_floats(3, 17, 31) == 3 * 3
    assert L.diner_ray_box_select_workspace_floats(2, 512, 512) == 2 * 1024
    assert L.diner_ray_box_select_workspace_floats(0, 5, 5) == 0 and L.diner_ray_box_select_workspace_floats(-1, 5, 5) == -1
    assert L.diner_ray_box_select_workspace_floats(1, 65536, 32768) == -1

    rays = lambda cam, SB, b, idx, cnt, host, B, out: L.diner_gen_rays_box(cam, SB, b, -0.01, 0.01, idx, cnt, host, B, out, None)
    two = (C.c_int32 * 2)(3, 7)
    assert rays(C.byref(cam), 2, p, p, p, two, 6, p) == -1 and b"below" in err()              # B < max count
    assert rays(C.byref(cam), 2, p, p, p, two, 0, p) == -1
    assert rays(None, 2, p, p, p, None, 7, p) == -1
    assert rays(C.byref(cam), 2, None, p, p, two, 7, p) == -1 and b"bounds" in err()
    assert rays(C.byref(cam), 2, p, None, p, two, 7, p) == -1 and b"NULL pointer" in err()
    assert rays(C.byref(cam), 2, p, p, None, two, 7, p) == -1
    assert rays(C.byref(cam), 2, p, p, p, two, 7, None) == -1
    assert rays(C.byref(cam), 2, p, p, p, two, 7, 72) == -1 and b"aligned" in err()
    assert rays(C.byref(cam), 2, p, p, p, None, -1, p) == -1 and b"negative B" in err()
    assert rays(C.byref(cam), 0, None, None, None, None, 7, None) == 0
    assert rays(C.byref(cam), 2, None, None, None, (C.c_int32 * 2)(0, 0), 0, None) == 0           # B = 0: no launch

    frame = lambda c, d, s, SB, B, H, W, rgb, dep: L.diner_frame_from_hits(c, d, s, SB, B, H, W, 1, rgb, dep, None, None)
    assert frame(p, p, None, 1, 3, 4, 5, p, p) == -1 and b"NULL pointer" in err()
    assert frame(p, p, p, 1, 3, 4, 5, None, p) == -1
    assert frame(p, p, p, 1, 3, 4, 5, p, None) == -1
    assert frame(None, p, p, 1, 3, 4, 5, p, p) == -1 and b"compact" in err()
    assert frame(p, None, p, 1, 3, 4, 5, p, p) == -1
    assert frame(p, p, p, 1, -1, 4, 5, p, p) == -1 and b"negative B" in err()
    assert frame(p, p, p, -1, 3, 4, 5, p, p) == -1
    assert frame(p, p, p, 1, 3, 65536, 32768, p, p) == -3
    assert frame(None, None, None, 0, 0, 4, 5, None, None) == 0
    assert frame(None, None, None, 2, 0, 0, 5, None, None) == 0


def test_glue_refusals_need_no_gpu():
    import torch

    from diner_amd import NeRFRendererDGS, glue
    E, K = torch.eye(4)[None], torch.eye(3)[None]
    for fn in (glue.ray_box, glue.box_rays):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(E, K, 8, 8, 0.1, 2.0, BOX)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.frame_from_hits(torch.zeros(1, 2, 3), torch.zeros(1, 2), torch.zeros(1, 64, dtype=torch.int32), 8, 8, True)
    assert glue.BOX_OFFSET == R.BOX_OFFSET
    import inspect
    sig = inspect.signature(NeRFRendererDGS.render_image).parameters
    assert sig["bounds"].default is None and sig["box_offset"].default == (-0.01, 0.01) and sig["return_mask"].default is False
    assert NeRFRendererDGS().last_box_hits is None
