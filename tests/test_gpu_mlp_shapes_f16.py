"""GPU tests of the shape-general f16x3 inference path (points_mlp_gen_f16.hip through the *_gen_f16 entry points, selected by
``NeRFRendererDGS(f16x3_any_shape=True)`` with ``precision == "f16x3"``):
(1) the ``shape_*`` fixtures of the unmodified reference (tools/gen_shape_golden.py) within the bars tests/test_gpu_mlp_shapes.py
    holds the fp32 route to: 1e-4 abs on rgb, depth and weights, sigma relative to max(1, sigma/12);
(2) against the fp32 shape-general route on the same inputs, same bars, also on a 128 x 128 frame the fixtures do not reach;
(3) the latent lookup modes; (4) render_image == forward bit for bit; (5) an activation beyond the fp16 range is raised, not
    returned; (6) the switch off is the parent's behaviour; (7) the standard model keeps its own kernel.
Every comparison prints its measured maxima before it asserts."""
import warnings

import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_shapes import SHAPE_FIXTURES, ShapeCase, T

pytestmark = pytest.mark.gpu

ROUTE = "points_mlp_gen_f16"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_cases = {}


def _shape_case(name, dev):
    if name not in _cases:
        _cases[name] = ShapeCase(name, dev)
    return _cases[name]


def _renderer(c, precision="f16x3", switch=True):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=c.K, n_depth_candidates=c.cfg["NC"], n_gaussian=c.cfg["G"], white_bkgd=c.scene.white_bkgd,
                        f16x3_any_shape=switch)
    r.precision = precision
    return r


def _rgbsigma_errors(got, ref, mask=None):
    if mask is not None:
        got, ref = got[mask], ref[mask]
    err_rgb = float(np.abs(got[..., :3] - ref[..., :3]).max())
    s_ref = ref[..., 3]
    err_s = float((np.abs(got[..., 3] - s_ref) / np.maximum(1.0, s_ref / 12.0)).max())   # the sigma bar of tests/test_gpu_parity.py
    return err_rgb, err_s


def _assert_rgbsigma(got, ref, what, mask=None):
    err_rgb, err_s = _rgbsigma_errors(got, ref, mask)
    print(f"{what}: |rgb| {err_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {err_s:.2e}, sigma max {float(ref[..., 3].max()):.3g}")
    assert np.isfinite(got).all(), what
    assert err_rgb <= 1e-4 and err_s <= 1e-4, f"{what}: |rgb| {err_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {err_s:.2e}"


def _assert_frames(out, ref, what, rays=None):
    for key in ("rgb", "depth", "weights"):
        a, b = out[key], ref[key]
        if rays is not None:
            a, b = a[rays], b[rays]
        err = float(np.abs(a - b).max())
        print(f"{what}: |{key}| {err:.2e}")
        assert err <= 1e-4, f"{what}: |{key}| {err:.2e}"


def _frames(o):
    return {"rgb": o.rgb.cpu().numpy()[0], "depth": o.depth.cpu().numpy()[0], "weights": o.weights.cpu().numpy()[0]}


# ---- 1. parity against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPE_FIXTURES)
def test_fixture_vs_reference(name, dev):
    """Measured on the MI355X (max over the fixture; rgb-sigma per sample | rgb, depth, weights per ray): see DESIGN.md §2."""
    c = _shape_case(name, dev)
    r = _renderer(c)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # no precision= warning on this route
        with torch.no_grad():
            pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
            assert r.last_route == ROUTE and r.last_binding == "ctypes" and r.effective_precision == "f16x3"
            out = r(c.model, rays, want_weights=True, z_samples=z).fine
    assert r.last_route == ROUTE and r.last_binding == "ctypes" and r.effective_precision == "f16x3"
    assert r.memory_report()["cached"]["mlp_gen_f16_packed"] > 0 and r.memory_report()["cached"]["mlp_gen_packed"] == 0
    _assert_rgbsigma(pts, c.data["rgbsigma"], f"{name} render_points vs reference")
    _assert_frames(_frames(out), c.data, f"{name} forward vs reference")


# ---- 2. against the fp32 shape-general route ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPE_FIXTURES)
def test_fixture_vs_fp32_route(name, dev):
    c = _shape_case(name, dev)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    res = {}
    with torch.no_grad():
        for prec in ("fp32", "f16x3"):
            r = _renderer(c, prec)
            pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
            out = r(c.model, rays, want_weights=True, z_samples=z).fine
            assert r.last_route == ("points_mlp_gen" if prec == "fp32" else ROUTE) and r.effective_precision == prec
            res[prec] = (pts, _frames(out))
    _assert_rgbsigma(res["f16x3"][0], res["fp32"][0], f"{name} render_points vs the fp32 route")
    _assert_frames(res["f16x3"][1], res["fp32"][1], f"{name} forward vs the fp32 route")


def test_whole_frame_vs_fp32_route(dev):
    """a 128 x 128 frame of the synthetic scene, d_hidden 256, NV 2, K 40: whole forward() (sampler -> point kernel -> compositing)
    with replayed noise on both routes"""
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    K, NC, G = 40, 200, 15
    dims = dict(d_hidden=256, n_blocks=5, combine_layer=3)
    sc = synth.make_scene(128, 128, 2, seed=4, feature_padding=8)
    w = synth.make_mlp_weights(3, bias_scale=0.1, d_latent=sc.C, **dims)
    m = model_from_scene(sc, w, device=dev, d_latent=sc.C, **dims)
    rays = sc.target_rays()
    NR = rays.shape[1]
    assert NR == 128 * 128
    noise = tuple(T(n, dev)[None] for n in synth.make_noise(NR, NC, G, K, seed=6))
    res = {}
    with torch.no_grad():
        for prec in ("fp32", "f16x3"):
            r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=sc.white_bkgd, f16x3_any_shape=True)
            r.precision = prec
            out = r(m, T(rays, dev), want_weights=True, noise=noise).fine
            assert r.last_route == ("points_mlp_gen" if prec == "fp32" else ROUTE) and r.effective_precision == prec
            res[prec] = _frames(out)
    assert np.isfinite(res["f16x3"]["rgb"]).all()
    _assert_frames(res["f16x3"], res["fp32"], "128 x 128 frame, d_hidden 256, NV 2, K 40, vs the fp32 route")


# ---- 3. index modes -----------------------------------------------------------------------------------------------------------
def test_index_modes(dev):
    """zeros padding against the reference fixture index_gen_zeros_h128; nearest and reflection on the same model against the fp32
    shape-general route"""
    from tests.test_gpu_index_modes import _case as index_case
    c = index_case("index_gen_zeros_h128", dev)
    assert not c.standard
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        r = _renderer(c)
        pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
        assert r.last_route == ROUTE and r.effective_precision == "f16x3"
        out = r(c.model, rays, want_weights=True, z_samples=z).fine
    _assert_rgbsigma(pts, c.data["rgbsigma"], "index_gen_zeros_h128 render_points vs reference", mask=c.firm)
    fr = c.firm_rays
    assert fr.mean() >= 0.9
    for key in ("rgb", "depth"):
        err = float(np.abs(_frames(out)[key][fr] - c.data[key][fr]).max())
        print(f"index_gen_zeros_h128 forward vs reference: |{key}| {err:.2e}")
        assert err <= 1e-4, (key, err)
    for interp, padding in (("nearest", "border"), ("nearest", "zeros"), ("bilinear", "reflection"), ("nearest", "reflection")):
        m = c.make_model(interp, padding, dev)
        with torch.no_grad():
            a = _renderer(c, "fp32")
            ref = a.render_points(m, rays, z).cpu().numpy()[0]
            assert a.last_route == "points_mlp_gen"
            b = _renderer(c)
            got = b.render_points(m, rays, z).cpu().numpy()[0]
            assert b.last_route == ROUTE
        _assert_rgbsigma(got, ref, f"{interp} / {padding} vs the fp32 route")


# ---- 4. render_image == forward -----------------------------------------------------------------------------------------------
def test_render_image_equals_forward(dev):
    """render_image (diner_render_image_gen_f16) against gen_rays -> forward (diner_render_gen_f16) with the same seed: bit for bit"""
    from diner_amd import glue
    c = _shape_case("shape_a_h128_nv2", dev)
    r = _renderer(c)
    sc = c.scene
    H, W = 20, 28
    E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
    Kt = torch.tensor([[[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
    near, far = float(sc.near), float(sc.far)
    r.seed, r._calls = 3, 0
    rgb, depth = r.render_image(c.model, E, Kt, H, W, near, far, return_depth=True)
    assert r.last_route == ROUTE and r.effective_precision == "f16x3"
    rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        ref = r(c.model, rays).fine
    assert r.last_route == ROUTE
    assert torch.equal(rgb, ref.rgb.view(1, H, W, 3).permute(0, 3, 1, 2))
    assert torch.equal(depth, ref.depth.view(1, H, W, 1).permute(0, 3, 1, 2))


# ---- 5. loud failure ----------------------------------------------------------------------------------------------------------
def test_an_activation_beyond_the_fp16_range_is_raised(dev):
    """the construction of tests/test_gpu_magnitude.py (latent x30, weights x3, bias 1) on a 128-wide model: the hidden state leaves
    the fp16 range (65504 * 16), the samples come out non-finite and the guard names precision='fp32'; in fp32 the same model renders
    finite values"""
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    K = 16
    dims = dict(d_hidden=128, n_blocks=5, combine_layer=3)
    sc = synth.make_scene(24, 24, 3, seed=5, feature_padding=4, latent_scale=30.0)
    w = synth.make_mlp_weights(7, bias_scale=1.0, d_latent=sc.C, **dims)
    # that sweep's loudest cell is weights x3; x4 here: every residual block then grows the state about 17-fold from a lin_z term of
    # order 30 * 4, far past the fp16 ceiling of the scaled state (1.05e6) and far inside fp32
    w = {k: (v * np.float32(4.0) if k.endswith("weight") else v) for k, v in w.items()}
    m = model_from_scene(sc, w, device=dev, d_latent=sc.C, **dims)
    rays = sc.target_rays()[:, ::7]
    z = np.sort(np.random.RandomState(1).uniform(sc.near, sc.far, (1, rays.shape[1], K)).astype(np.float32), -1)
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=64, n_gaussian=4, white_bkgd=True, f16x3_any_shape=True)
    with torch.no_grad():
        pts = r.render_points(m, T(rays, dev), T(z, dev))
        assert r.last_route == ROUTE
        assert not bool(torch.isfinite(pts).all()), "the construction does not leave the fp16 range"
        r(m, T(rays, dev), z_samples=T(z, dev))
        with pytest.raises(RuntimeError, match="precision = 'fp32'"):
            r.check_finite()
        r.precision = "fp32"
        o = r(m, T(rays, dev), z_samples=T(z, dev))
        r.check_finite()
        assert r.last_route == "points_mlp_gen" and bool(torch.isfinite(o.fine.rgb).all())


# ---- 6. switch off = the parent -----------------------------------------------------------------------------------------------
def test_switch_off_is_the_fp32_route(dev):
    c = _shape_case("shape_a_h128_nv2", dev)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    r = _renderer(c, "f16x3", switch=False)
    assert r.f16x3_any_shape is False
    with pytest.warns(UserWarning, match="fp32"):
        with torch.no_grad():
            a = r(c.model, rays, want_weights=True, z_samples=z).fine
    assert r.last_route == "points_mlp_gen" and r.effective_precision == "fp32"
    e = _renderer(c, "fp32", switch=True)                   # precision "fp32" keeps the fp32 kernel whatever the switch says
    with torch.no_grad():
        b = e(c.model, rays, want_weights=True, z_samples=z).fine
    assert e.last_route == "points_mlp_gen" and e.effective_precision == "fp32"
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth) and torch.equal(a.weights, b.weights)


# ---- 7. the standard model is untouched ---------------------------------------------------------------------------------------
def test_standard_model_keeps_its_kernel(dev):
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(32, 32, 4, seed=0, feature_padding=4)
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1), device=dev)
    rays = T(sc.target_rays()[:, ::4], dev)
    out = {}
    for switch in (False, True):
        r = NeRFRendererDGS(n_samples=16, n_depth_candidates=100, n_gaussian=6, f16x3_any_shape=switch)
        r.seed = 5
        with torch.no_grad():
            out[switch] = r(m, rays).fine.rgb
        assert r.last_route == "points_mlp_f16" and r.effective_precision == "f16x3"
    assert torch.equal(out[False], out[True])
