"""Host-side checks (no GPU) of the lin_z maps of the shape-general render routes (``NeRFRendererDGS(linz_maps_any_shape=True)``,
csrc/linz_maps_gen.hip and the point kernels' lin_z-map forms): the sizes and the argument validation of the new C entry points, the
switch and its memory report, and the property of the zeros-padding fixture that lets the GPU test on it reject a map with the bias
folded in."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests.test_mlp_shapes_host import _shape

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW_SYMBOLS = ["diner_linz_maps_gen_floats", "diner_pack_linz_maps_gen", "diner_render_points_gen_lz", "diner_render_gen_lz",
               "diner_render_image_gen_lz"]
INVALID, UNSUPPORTED = -1, -3


def _scene(SB=2, NV=3, h=5, w=7, Cc=512, pointers=False):
    from diner_amd import _lib
    sc = _lib.DinerScene(SB=SB, NV=NV, H=8, W=8, h=h, w=w, C=Cc, num_freqs=6, image_w=8.0, image_h=8.0)
    if pointers:
        sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 16      # never dereferenced: the call is refused before any launch
    return sc


def test_new_symbols_are_declared_and_exported():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    for stem in ("render_points_gen", "render_gen", "render_image_gen"):      # the _gen_ix list + precision, bicubic padding, maps
        assert _lib.SYMBOLS[f"diner_{stem}_lz"][1] == _lib.SYMBOLS[f"diner_{stem}_ix"][1] + [C.c_int32, C.c_int32, C.c_void_p], stem
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # new entry points only: the ABI version stays


@pytest.mark.parametrize("kw, nlz", [
    (dict(n_blocks=5, combine_layer=3), 3),
    (dict(n_blocks=5, combine_layer=0), 0),
    (dict(n_blocks=2, combine_layer=1000), 2),
    (dict(n_blocks=3, combine_layer=3), 3),
    (dict(d_hidden=32), 3),
    (dict(d_hidden=512), 3),
    (dict(d_latent=8), 3),
    (dict(d_latent=1024), 3),
])
def test_map_size_follows_the_shape(kw, nlz):
    from diner_amd import _lib
    lib = _lib.lib()
    sh = _shape(**kw)
    sc = _scene(Cc=sh.d_latent)
    assert lib.diner_linz_maps_gen_floats(C.byref(sc), C.byref(sh)) == nlz * 2 * 3 * 5 * 7 * sh.d_hidden


@pytest.mark.parametrize("kw", [dict(d_hidden=48), dict(d_hidden=544), dict(d_latent=12), dict(d_latent=1032), dict(n_blocks=0),
                                dict(combine_layer=-1), dict(d_out=5), dict(combine_type=1)])
def test_an_unsupported_shape_returns_the_packers_code(kw):
    from diner_amd import _lib
    lib = _lib.lib()
    sh = _shape(**kw)
    want = lib.diner_mlp_gen_packed_floats(C.byref(sh))
    reason = lib.diner_last_error().decode()
    assert want == UNSUPPORTED
    assert lib.diner_linz_maps_gen_floats(C.byref(_scene()), C.byref(sh)) == want
    assert lib.diner_last_error().decode() == reason
    assert lib.diner_pack_linz_maps_gen(C.byref(_scene(pointers=True)), C.byref(sh), 16, 16, None) == want
    assert lib.diner_render_points_gen_lz(C.byref(_scene(pointers=True)), None, C.byref(sh), 16, None, None, 0, 1, None, None, 0, -1, 16) == want


def test_null_pointers_and_bad_sizes_are_invalid_not_a_crash():
    from diner_amd import _lib
    lib = _lib.lib()
    sh, sc = _shape(), _scene(pointers=True)
    assert lib.diner_linz_maps_gen_floats(None, C.byref(sh)) == INVALID
    assert lib.diner_linz_maps_gen_floats(C.byref(sc), None) == INVALID
    assert lib.diner_linz_maps_gen_floats(C.byref(_scene(h=0)), C.byref(sh)) == INVALID
    assert lib.diner_linz_maps_gen_floats(C.byref(_scene(NV=0)), C.byref(sh)) == INVALID
    for args in ((None, C.byref(sh), 16, 16), (C.byref(sc), None, 16, 16), (C.byref(sc), C.byref(sh), None, 16), (C.byref(sc), C.byref(sh), 16, None)):
        assert lib.diner_pack_linz_maps_gen(*args, None) == INVALID
        assert "NULL" in lib.diner_last_error().decode()
    assert lib.diner_pack_linz_maps_gen(C.byref(_scene()), C.byref(sh), 16, 16, None) == INVALID          # scene->latent NULL
    assert "latent" in lib.diner_last_error().decode()
    assert lib.diner_pack_linz_maps_gen(C.byref(_scene(Cc=256, pointers=True)), C.byref(sh), 16, 16, None) == INVALID
    assert "d_latent" in lib.diner_last_error().decode()
    # the render family: NULL shape, NULL maps with nlz > 0, NULL scene
    assert lib.diner_render_points_gen_lz(C.byref(sc), None, None, 16, None, None, 0, 1, None, None, 0, -1, 16) == INVALID
    assert "shape is NULL" in lib.diner_last_error().decode()
    assert lib.diner_render_points_gen_lz(C.byref(sc), None, C.byref(sh), 16, None, None, 0, 1, None, None, 0, -1, None) == INVALID
    assert "linz_maps_gen is NULL" in lib.diner_last_error().decode()
    assert lib.diner_render_points_gen_lz(None, None, C.byref(sh), 16, None, None, 0, 1, None, None, 0, -1, 16) == INVALID
    assert lib.diner_render_gen_lz(C.byref(sc), None, C.byref(sh), 16, None, 0, None, 1, None, None, None, 0, None, None, None, None, None, None,
                                   1, -1, None) == INVALID
    assert "linz_maps_gen is NULL" in lib.diner_last_error().decode()
    assert lib.diner_render_image_gen_lz(C.byref(sc), None, C.byref(sh), 16, None, None, 1, 0, None, None, None, None, None, None, None,
                                         0, 2, None) == INVALID
    assert "linz_maps_gen is NULL" in lib.diner_last_error().decode()
    # a shape without lin_z layers needs no maps: the call gets as far as the parent's checks (here: NULL mlp_packed)
    assert lib.diner_render_points_gen_lz(C.byref(sc), None, C.byref(_shape(combine_layer=0)), None, None, None, 0, 1, None, None, 0, -1,
                                          None) == INVALID
    assert "mlp_packed is NULL" in lib.diner_last_error().decode()


@pytest.mark.parametrize("precision, padding, what", [(2, -1, "precision=2"), (-1, -1, "precision=-1"), (0, 3, "padding=3"),
                                                     (1, -2, "padding=-2")])
def test_precision_and_bicubic_padding_out_of_range_are_invalid(precision, padding, what):
    from diner_amd import _lib
    lib = _lib.lib()
    sh, sc = _shape(), _scene(pointers=True)
    calls = [
        lambda: lib.diner_render_points_gen_lz(C.byref(sc), None, C.byref(sh), 16, None, None, 0, 1, None, None, precision, padding, 16),
        lambda: lib.diner_render_gen_lz(C.byref(sc), None, C.byref(sh), 16, None, 0, None, 1, None, None, None, 0, None, None, None, None,
                                        None, None, precision, padding, 16),
        lambda: lib.diner_render_image_gen_lz(C.byref(sc), None, C.byref(sh), 16, None, None, 1, 0, None, None, None, None, None, None, None,
                                              precision, padding, 16),
    ]
    for call in calls:
        assert call() == INVALID
        assert what in lib.diner_last_error().decode()


def test_the_switch_is_a_constructor_keyword_off_by_default():
    from diner_amd import NeRFRendererDGS
    assert NeRFRendererDGS().linz_maps_any_shape is False
    assert NeRFRendererDGS(linz_maps_any_shape=True).linz_maps_any_shape is True
    assert NeRFRendererDGS(n_samples=8, linz_maps_any_shape=1).linz_maps_any_shape is True
    for r in (NeRFRendererDGS(), NeRFRendererDGS(linz_maps_any_shape=True)):
        rep = r.memory_report()
        assert rep["cached"]["linz_maps_gen"] == 0 and rep["cached"]["total"] == 0
    r = NeRFRendererDGS(linz_maps_any_shape=True)
    assert r._gen_route(False, None) == "points_mlp_gen" and r._gen_route(True, None) == "points_mlp_gen_f16"
    assert r._gen_route(False, object()) == "points_mlp_gen_lz" and r._gen_route(True, object()) == "points_mlp_gen_f16_lz"


def test_the_zeros_fixture_holds_lookups_whose_tap_weights_sum_to_less_than_one():
    """index_gen_zeros_h128 in float64 numpy: the samples of the fixture projected into every view (pixelnerf.py:91-108), the
    feature_padding rescale and grid_sample's unnormalisation (image_encoder.py:113-125, align_corners=False), the bilinear footprint.
    With zeros padding a tap outside the map contributes nothing, so the weights of such a lookup sum to less than 1: a lin_z map
    with the bias folded in would give that lookup only a part of the bias.  The GPU test on this fixture can reject that mistake
    only if such lookups exist -- here: that they are a real share, clear of rounding."""
    from tools.gen_index_golden import case_inputs
    data = np.load(GOLDEN / "index_gen_zeros_h128.npz", allow_pickle=False)
    cfg = json.loads(str(data["config"]))
    assert (cfg["interp"], cfg["padding"]) == ("bilinear", "zeros") and cfg["mlp"]["combine_layer"] > 0
    sc, w, rays, _ = case_inputs(cfg)
    z = data["z_fill"].astype(np.float64)                                  # [NR, K]
    r = rays[0].astype(np.float64)
    pts = r[:, None, :3] + z[..., None] * r[:, None, 3:6]                  # [NR, K, 3]
    h, wd = sc.latent.shape[-2:]
    iw, ih = (float(v) for v in sc.image_shape)
    sx, sy = (wd - 2.0 * sc.feature_padding) / wd, (h - 2.0 * sc.feature_padding) / h
    partial = total = 0
    min_sum = 1.0
    for v in range(sc.NV):
        P = sc.poses[0, v].astype(np.float64)
        cam = pts @ P[:3, :3].T + P[:3, 3]
        u = (cam[..., 0] / cam[..., 2] * sc.focal[0, v, 0] + sc.c[0, v, 0]) / iw * 2 - 1
        t = (cam[..., 1] / cam[..., 2] * sc.focal[0, v, 1] + sc.c[0, v, 1]) / ih * 2 - 1
        ix, iy = ((u * sx + 1) * wd - 1) / 2, ((t * sy + 1) * h - 1) / 2
        x0, y0 = np.floor(ix), np.floor(iy)
        fx, fy = ix - x0, iy - y0
        wsum = np.zeros_like(ix)
        for dx, wx in ((0, 1 - fx), (1, fx)):
            for dy, wy in ((0, 1 - fy), (1, fy)):
                inside = (x0 + dx >= 0) & (x0 + dx <= wd - 1) & (y0 + dy >= 0) & (y0 + dy <= h - 1)
                wsum += np.where(inside, wx * wy, 0.0)
        clear = wsum < 1 - 1e-3                                            # far from a last-ulp difference of the projection
        partial += int(clear.sum())
        total += clear.size
        min_sum = min(min_sum, float(wsum.min()))
    print(f"index_gen_zeros_h128: {partial} of {total} (view, sample) lookups have tap weights summing below 1 - 1e-3; smallest sum {min_sum:.3f}")
    assert partial >= 0.05 * total
