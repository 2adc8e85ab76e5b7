"""GPU test of the inference doors of ``NeRFRendererDGS``, route by route: on every route the renderer has, ``forward()`` in one call,
``forward()`` with ``stage_events`` (the three stage entry points), ``composite(render_points(...))`` on the same samples and
``render_image()`` of the same rays run the same three kernels with the same arguments, so they must agree bit for bit -- no tolerance.
``last_route`` / ``last_binding`` / ``effective_precision`` are asserted behind every door.

Scene: 8 x 8 maps, 2 views; a 5 x 13 target frame = 65 rays x 8 samples = 520 points: eight full 64-point tiles and a tail of 8;
16 depth candidates, 3 gaussian samples.  Models: the standard MLP and d_hidden 64 / d_latent 32 / 2 blocks / combine_layer 1 /
num_freqs 2.  Each route with the default lookup and one other."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, K, NC, G = 5, 13, 8, 16, 3
NONSTD = dict(d_hidden=64, n_blocks=2, combine_layer=1)

# id: (model, precision, renderer switches, (index_interp, index_padding), last_route, effective_precision)
CASES = {
    "std_f16x3": ("std", "f16x3", {}, ("bilinear", "border"), "points_mlp_f16", "f16x3"),
    "std_f16x3_nearest_zeros": ("std", "f16x3", {}, ("nearest", "zeros"), "points_mlp_f16", "f16x3"),
    "std_fp32": ("std", "fp32", {}, ("bilinear", "border"), "points_mlp", "fp32"),
    "std_fp32_nearest_zeros": ("std", "fp32", {}, ("nearest", "zeros"), "points_mlp", "fp32"),
    "gen_fp32": ("nonstd", "fp32", {}, ("bilinear", "border"), "points_mlp_gen", "fp32"),
    "gen_fp32_bicubic_reflection": ("nonstd", "fp32", dict(bicubic_index=True), ("bicubic", "reflection"), "points_mlp_gen", "fp32"),
    "gen_f16x3": ("nonstd", "f16x3", dict(f16x3_any_shape=True), ("bilinear", "border"), "points_mlp_gen_f16", "f16x3"),
    "gen_f16x3_nearest_zeros": ("nonstd", "f16x3", dict(f16x3_any_shape=True), ("nearest", "zeros"), "points_mlp_gen_f16", "f16x3"),
    "gen_lz_fp32": ("nonstd", "fp32", dict(linz_maps_any_shape=True), ("bilinear", "border"), "points_mlp_gen_lz", "fp32"),
    "gen_lz_fp32_nearest_zeros": ("nonstd", "fp32", dict(linz_maps_any_shape=True), ("nearest", "zeros"), "points_mlp_gen_lz", "fp32"),
    "gen_lz_f16x3": ("nonstd", "f16x3", dict(f16x3_any_shape=True, linz_maps_any_shape=True), ("bilinear", "border"),
                     "points_mlp_gen_f16_lz", "f16x3"),
    "gen_lz_f16x3_bicubic_border": ("nonstd", "f16x3", dict(f16x3_any_shape=True, linz_maps_any_shape=True, bicubic_index=True),
                                    ("bicubic", "border"), "points_mlp_gen_f16_lz", "f16x3"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_inputs = {}


def _model(kind, lookup, dev):
    """(model, target extrinsics, intrinsics, near, far, the frame's rays [1, 65, 8]) -- built once per (kind, lookup), never modified"""
    if (kind, lookup) not in _inputs:
        from diner_amd import glue
        from synthetic import synth
        from synthetic.model_stub import model_from_scene
        interp, padding = lookup
        if kind == "std":
            sc = synth.make_scene(8, 8, 2, seed=3, feature_padding=2)
            m = model_from_scene(sc, synth.make_mlp_weights(4, bias_scale=0.1), device=dev, index_interp=interp, index_padding=padding)
        else:
            sc = synth.make_scene(8, 8, 2, seed=3, feature_padding=2, C=32)
            w = synth.make_mlp_weights(4, bias_scale=0.1, d_in=7 + 8 * 2, d_latent=32, **NONSTD)
            m = model_from_scene(sc, w, device=dev, num_freqs=2, d_latent=32, index_interp=interp, index_padding=padding, **NONSTD)
        E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
        Kt = torch.tensor([[[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
        near, far = float(sc.near), float(sc.far)
        rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
        _inputs[kind, lookup] = (m, E, Kt, near, far, rays)
    return _inputs[kind, lookup]


def _renderer(precision, switches, white, **attrs):
    """renderers constructed alike: the same seed and a fresh call counter"""
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=white, **switches)
    r.precision, r.seed = precision, 5
    for k, v in attrs.items():
        setattr(r, k, v)
    return r


def _state(r):
    return r.last_route, r.last_binding, r.effective_precision


@pytest.mark.parametrize("name", list(CASES))
def test_every_door_of_a_route_gives_the_same_bits(name, dev):
    from diner_amd import ops
    kind, precision, switches, lookup, route, eff = CASES[name]
    m, E, Kt, near, far, rays = _model(kind, lookup, dev)
    assert tuple(rays.shape) == (1, 65, 8)
    # the torch_ops binding serves the standard model with the default lookup, where the extension is built: the renderer's default
    op = "torch_ops" if kind == "std" and lookup == ("bilinear", "border") and ops.available() else "ctypes"
    with torch.no_grad():
        # (a) forward() in one call, in the default binding and through ctypes
        ra = _renderer(precision, switches, True)
        a = ra(m, rays, want_weights=True).fine
        assert _state(ra) == (route, op, eff)
        assert tuple(a.rgb.shape) == (1, 65, 3) and tuple(a.depth.shape) == (1, 65) and tuple(a.weights.shape) == (1, 65, K)
        assert bool(torch.isfinite(a.rgb).all()) and float(a.weights.sum(-1).max()) > 0.5, "the frame must composite something"
        rc = _renderer(precision, switches, True, binding="ctypes")
        c = rc(m, rays, want_weights=True).fine
        assert _state(rc) == (route, "ctypes", eff)
        # (b) forward() stage by stage
        rb = _renderer(precision, switches, True, stage_events=[])
        b = rb(m, rays, want_weights=True).fine
        assert _state(rb) == (route, "ctypes", eff)
        assert len(rb.stage_events) == 1 and len(rb.stage_events[0]) == 4
        # (c) the stages as the caller's own calls, on the samples (b) drew: a renderer constructed alike draws the same ones
        rs = _renderer(precision, switches, True)
        z = rs._sample(rays, m, K, NC, G, 0.05, None, None)["z"]
        rgbsigma = rs.render_points(m, rays, z)
        assert _state(rs) == (route, "ctypes", eff)
        assert tuple(rgbsigma.shape) == (1, 65, K, 4)
        weights, rgb, depth = rs.composite(m, rays, z, rgbsigma=rgbsigma)
        # ... and with injected samples: forward(z_samples=...) goes through composite()
        rz = _renderer(precision, switches, True)
        zs = rz(m, rays, want_weights=True, z_samples=z).fine
        assert _state(rz) == (route, "ctypes", eff) and rz._calls == 0
        # (d) render_image of the 5 x 13 frame
        ri = _renderer(precision, switches, True)
        img, img_depth = ri.render_image(m, E, Kt, H, W, near, far, return_depth=True)
        assert _state(ri) == (route, op, eff)
        assert ra._calls == rb._calls == rc._calls == rs._calls == ri._calls == 1      # one seed per call
    for what, other in (("ctypes", c), ("staged", b), ("injected samples", zs)):
        for field in ("rgb", "depth", "weights"):
            assert torch.equal(a[field], other[field]), (name, what, field)
    assert torch.equal(a.rgb, rgb) and torch.equal(a.depth, depth) and torch.equal(a.weights, weights), (name, "composite(render_points)")
    assert torch.equal(img, a.rgb.view(1, H, W, 3).permute(0, 3, 1, 2)), (name, "render_image rgb")
    assert torch.equal(img_depth, a.depth.view(1, H, W, 1).permute(0, 3, 1, 2)), (name, "render_image depth")
