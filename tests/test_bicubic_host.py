"""Host tests (no GPU) of the bicubic latent lookup (SpatialEncoder index_interp="bicubic"): the restatement of tests/bicubic_ref.py
proven against torch's own F.grid_sample(mode="bicubic") forward and autograd (and a deliberately wrong variant rejected by the same
comparison), the renderer's ``bicubic_index`` switch and its routing, the C ABI of the _bc entry points, and the bicubic_* fixtures of
tools/gen_bicubic_golden.py."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bicubic_ref as br

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
FIXTURES = sorted(p.stem for p in GOLDEN.glob("bicubic_*.npz"))
NEW_SYMBOLS = ["diner_render_points_gen_bc", "diner_render_gen_bc", "diner_render_image_gen_bc", "diner_render_points_gen_f16_bc",
               "diner_render_gen_f16_bc", "diner_render_image_gen_f16_bc", "diner_train_point_inputs_gen_bc",
               "diner_train_point_inputs_backward_gen_bc", "diner_train_bicubic_scatter"]
MAPS = [(2, 3), (4, 4), (5, 7)]


def _coords(h, w, seed):
    """normalised (u, v) whose centre coordinates span -3 .. size + 3 texels: random ones, and every pair of exact integers"""
    g = torch.Generator().manual_seed(seed)
    ix = torch.rand(400, generator=g, dtype=torch.float64) * (w + 6) - 3
    iy = torch.rand(400, generator=g, dtype=torch.float64) * (h + 6) - 3
    gx, gy = torch.meshgrid(torch.arange(-3, w + 4, dtype=torch.float64), torch.arange(-3, h + 4, dtype=torch.float64), indexing="ij")
    ix, iy = torch.cat([ix, gx.reshape(-1)]), torch.cat([iy, gy.reshape(-1)])
    return (2 * ix + 1) / w - 1, (2 * iy + 1) / h - 1                      # ix = ((u + 1) w - 1) / 2


def _torch_lookup(lat, u, v, padding):
    grid = torch.stack([u, v], -1)[None, None]                             # [1, 1, N, 2]
    return F.grid_sample(lat[None], grid, mode="bicubic", padding_mode=padding, align_corners=False)[0, :, 0].t()   # [N, C]


def _errors(h, w, padding, centre_fn):
    g = torch.Generator().manual_seed(h * 10 + w)
    lat = torch.randn(6, h, w, generator=g, dtype=torch.float64)
    u, v = _coords(h, w, seed=h + w)
    cot = torch.randn(u.numel(), 6, generator=g, dtype=torch.float64)
    lat_t, u_t, v_t = lat.clone().requires_grad_(True), u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ref = _torch_lookup(lat_t, u_t, v_t, padding)
    (ref * cot).sum().backward()
    got = br.lookup(lat, u, v, padding, centre_fn=centre_fn)
    d_lat, d_u, d_v = br.lookup_grads(lat, u, v, cot, padding, centre_fn=centre_fn)
    err = lambda a, b: float((a - b).abs().max())
    return err(got, ref.detach()), err(d_lat, lat_t.grad), max(err(d_u, u_t.grad), err(d_v, v_t.grad))


@pytest.mark.parametrize("padding", br.PADDINGS)
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_grid_sample_forward_and_autograd(hw, padding):
    e_fwd, e_lat, e_grid = _errors(*hw, padding, br.centre)
    # float64 on both sides: a few ulp of values of magnitude <= ~10 (the grid gradient carries size / 2 and sums 400 + rows per texel)
    assert e_fwd <= 1e-12 and e_lat <= 1e-10 and e_grid <= 1e-10, (e_fwd, e_lat, e_grid)


@pytest.mark.parametrize("padding", br.PADDINGS)
def test_a_clamped_centre_is_rejected_by_the_same_comparison(padding):
    e_fwd, e_lat, e_grid = _errors(5, 7, padding, br.clamped_centre)
    assert e_fwd > 1e-2 and e_lat > 1e-2 and e_grid > 1e-2, (e_fwd, e_lat, e_grid)


def test_fp32_coordinate_mode_stays_close_to_float64():
    lat = torch.randn(4, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    u, v = _coords(5, 7, seed=3)
    a = br.lookup(lat, u, v, "border")
    b = br.lookup(lat, u.float(), v.float(), "border", coord_dtype=torch.float32)
    near_int = ((br.centre(u, 7) - br.centre(u, 7).round()).abs() < 1e-5) | ((br.centre(v, 5) - br.centre(v, 5).round()).abs() < 1e-5)
    assert float((a - b)[~near_int].abs().max()) < 1e-4      # (border clamps: a floor that flips at an integer changes which texels clamp)


@pytest.mark.parametrize("padding", br.PADDINGS)
def test_fp32_mode_tracks_grid_sample_in_float32(padding):
    """the float32 mode (the kernels' reference) against ATen's own float32 evaluation: the same weights operation for operation; ATen
    un-normalises as ((u + 1) w - 1) / 2 (the coordinate may differ by an ulp, 1e-6 texel at magnitude 10) and sums in float32"""
    lat = (torch.rand(6, 5, 7, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    u, v = (t.float() for t in _coords(5, 7, seed=4))
    ref = _torch_lookup(lat, u, v, padding).double()
    got = br.lookup(lat, u, v, padding, coord_dtype=torch.float32)
    assert float((got - ref).abs().max()) <= 1e-5


# ---- the switch and the routing -----------------------------------------------------------------------------------------------------
def _model(padding, interp="bicubic", **dims):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(8, 8, 2, seed=1, feature_padding=2)
    d = dict(d_in=55, d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3)
    d.update(dims)
    w = synth.make_mlp_weights(2, d_in=d["d_in"], d_latent=d["d_latent"], d_hidden=d["d_hidden"], n_blocks=d["n_blocks"],
                               combine_layer=d["combine_layer"])
    return model_from_scene(sc, w, device="cpu", index_interp=interp, index_padding=padding, **{k: v for k, v in d.items() if k != "d_in"})


def test_default_renderer_refuses_bicubic_and_names_the_switch():
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS()
    assert r.bicubic_index is False
    for call in (lambda: NeRFRendererDGS._validate_model(_model("border")), lambda: r._route(_model("zeros")),
                 lambda: NeRFRendererDGS(bicubic_index=True)._validate_model(_model("border"))):    # the static check never accepts it
        with pytest.raises(NotImplementedError, match="bicubic_index"):
            call()
    with pytest.raises(NotImplementedError):
        NeRFRendererDGS(bicubic_index=True)._route(_model("wrap"))


@pytest.mark.parametrize("padding", br.PADDINGS)
def test_switch_routes_bicubic_like_a_non_standard_shape(padding):
    import warnings
    from diner_amd import NeRFRendererDGS, _lib
    from diner_amd.renderer import STANDARD_SHAPE
    m = _model(padding)
    r = NeRFRendererDGS(bicubic_index=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        shape = r._route(m)
    assert shape == STANDARD_SHAPE and r._bicubic_pad(m) == _lib.INDEX_PADDING[padding]
    assert r._use_gen(shape, m) and not r._use_gen_f16(shape, m) and r.effective_precision == "fp32"
    assert len(w) == 1 and "fp32" in str(w[0].message)                      # the one-time precision warning
    fn, name, look = r._gen_lookup("render_points_gen", False, m)
    assert name == "diner_render_points_gen_bc" and look == (_lib.INDEX_PADDING[padding],)
    r16 = NeRFRendererDGS(bicubic_index=True, f16x3_any_shape=True)
    shape = r16._route(m)
    assert r16._use_gen_f16(shape, m) and r16.effective_precision == "f16x3"
    assert r16._gen_lookup("render_image_gen", True, m)[1] == "diner_render_image_gen_f16_bc"
    r16.precision = "fp32"
    assert not r16._use_gen_f16(r16._route(m), m)
    # training needs train_any_shape (and train_f16x3_any_shape for f16x3)
    assert not r._use_gen_train(shape, m)
    with pytest.raises(NotImplementedError, match="train_any_shape"):
        r._gen_training_unsupported(shape, m)
    rt = NeRFRendererDGS(bicubic_index=True, train_any_shape=True)
    assert rt._use_gen_train(shape, m) and not rt._use_gen_train_f16(shape, m)      # (no call before it: nothing is remembered)
    rt16 = NeRFRendererDGS(bicubic_index=True, train_any_shape=True, train_f16x3_any_shape=True)
    assert rt16._use_gen_train_f16(shape, m)
    # the routing is read from the model of the call, never from an earlier one
    other = _model("border", interp="bilinear")
    shape = r._route(other)
    assert r._bicubic_pad(other) is None and not r._use_gen(shape, other) and r._use_gen(shape, m)
    assert r._gen_lookup("render_points_gen", False, other)[1] == "diner_render_points_gen"
    assert r._index(other) is None and r._index(m) is None and r._index(_model("zeros", interp="nearest")).interp == 1


def test_memory_report_of_a_bicubic_model_on_a_fresh_renderer_only_reports():
    from diner_amd import NeRFRendererDGS
    m = _model("zeros")
    rep = NeRFRendererDGS(bicubic_index=True).memory_report(m, rays_per_call=64)
    assert rep["bicubic_index"] is True
    base = NeRFRendererDGS(bicubic_index=True).memory_report(_model("zeros", interp="bilinear"), rays_per_call=64, n_views=1)
    assert base["bicubic_index"] is False
    one = NeRFRendererDGS(bicubic_index=True).memory_report(m, rays_per_call=64, n_views=1)
    assert one["training_step"]["saved_activations"] - base["training_step"]["saved_activations"] == 64 * 40 * 4 * 8   # 16-float tap records
    # it reports, it does not validate: a model no kernel serves, and a renderer without the switch
    assert NeRFRendererDGS().memory_report(m)["bicubic_index"] is False
    assert "cached" in NeRFRendererDGS().memory_report(_model("wrap", interp="area"))


def test_training_without_train_any_shape_raises_naming_the_switch():
    from diner_amd import NeRFRendererDGS
    m = _model("border")
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    r = NeRFRendererDGS(bicubic_index=True)
    with pytest.raises(NotImplementedError, match="train_any_shape"):
        r(m, torch.zeros(1, 4, 8))


def test_non_standard_shape_with_bicubic():
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(bicubic_index=True)
    r.precision = "fp32"
    shape = r._route(_model("reflection", d_hidden=128, n_blocks=4, combine_layer=2))
    m = _model("reflection", d_hidden=128, n_blocks=4, combine_layer=2)
    assert not shape.standard and r._use_gen(shape, m) and r._bicubic_pad(m) == 2


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_exported_and_abi_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3 == _lib.ABI_VERSION
    assert _lib.INDEX_INTERP == {"bilinear": 0, "nearest": 1}
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(const DinerScene \*scene, int32_t padding,|\b{name}\(const float \*dz", header), name
        assert name in _lib.SYMBOLS, name
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.diner_version() == 3


def test_bad_padding_is_invalid_with_a_message():
    from diner_amd import _lib
    lib = _lib.lib()
    sc = _lib.DinerScene(SB=1, NV=1, H=4, W=4, h=4, w=4, C=512, num_freqs=6, image_w=4.0, image_h=4.0)
    sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 16      # never dereferenced: the padding is rejected before any launch
    shape = _lib.DinerMlpShape(55, 512, 512, 5, 3, 6, 0.0, 4, 0)
    cfg = _lib.DinerSamplerCfg(8, 4, 2, 0.05)
    cam = _lib.DinerTargetCam(16, 16, 16, 16, 2, 2)
    for bad in (3, -1, 17):
        for sfx in ("", "_f16"):
            pts = getattr(lib, f"diner_render_points_gen{sfx}_bc")
            assert pts(C.byref(sc), bad, C.byref(shape), 16, 16, 16, 1, 1, 16, None) == -1
            assert b"bicubic padding" in lib.diner_last_error()
            ren = getattr(lib, f"diner_render_gen{sfx}_bc")
            assert ren(C.byref(sc), bad, C.byref(shape), 16, 16, 1, C.byref(cfg), 1, None, None, None, 0, 16, 16, 16, None, None, None) == -1
            assert b"bicubic padding" in lib.diner_last_error()
            img = getattr(lib, f"diner_render_image_gen{sfx}_bc")
            assert img(C.byref(sc), bad, C.byref(shape), 16, C.byref(cam), C.byref(cfg), 1, 0, 16, None, 16, 16, None, None, None) == -1
            assert b"bicubic padding" in lib.diner_last_error()
        assert lib.diner_train_point_inputs_gen_bc(C.byref(sc), bad, 16, 16, 16, 1, 1, 0, 16, 56, 16, 16, None) == -1
        assert b"bicubic padding" in lib.diner_last_error()
        assert lib.diner_train_point_inputs_backward_gen_bc(C.byref(sc), bad, 16, 16, 16, 1, 1, 0, 16, 56, 16, None, 16, None, None, None,
                                                            None, None, None, None) == -1
        assert b"bicubic padding" in lib.diner_last_error()
    # the _ix entry points keep rejecting interp = 2
    ix = _lib.DinerLatentIndex(2, 0)
    assert lib.diner_render_points_gen_ix(C.byref(sc), C.byref(ix), C.byref(shape), 16, 16, 16, 1, 1, 16, None) == -1
    assert b"latent index" in lib.diner_last_error()


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def test_fixture_set():
    from tools.gen_bicubic_golden import ALL_CASES, CAMGRAD_CASES, CASES, TRAIN_CASES
    assert FIXTURES == sorted(ALL_CASES)
    assert {c["padding"] for c in CASES.values()} == set(br.PADDINGS) and all(c["interp"] == "bicubic" for c in ALL_CASES.values())
    assert any(c["mlp"]["d_hidden"] != 512 for c in CASES.values()) and any(c["mlp"]["d_hidden"] == 512 for c in CASES.values())
    assert any(c["scene"]["feature_padding"] > 0 for c in CASES.values())
    assert TRAIN_CASES and CAMGRAD_CASES
    assert all((GOLDEN / f"{n}.npz").stat().st_size < 1 << 20 for n in FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_digests_and_footprint_coverage(name):
    from tools.gen_bicubic_golden import ALL_CASES, case_inputs, input_digests
    data = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    cfg = json.loads(str(data["config"]))
    assert cfg == ALL_CASES[name]
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    assert float(data["straddle_frac"]) >= 0.10, "the per-tap padding must decide a real share of the lookups"
    assert float(data["inside_frac"]) >= 0.10, "a real share of the lookups must have all 16 taps in the map"
    assert "firm" not in data.files
