"""GPU tests of lin_z hoisted into per-texel maps on the shape-general render routes (``NeRFRendererDGS(linz_maps_any_shape=True)``:
csrc/linz_maps_gen.hip builds M_b = lin_z[b].weight . latent once per encode(), the lin_z-map forms of the point kernels --
points_mlp_gen_lz.hip, points_mlp_gen_f16_lz.hip and their bicubic twins -- gather d_hidden channels of it per point):
(1) the map builder against a float64 matmul, inside the forward error bound of an fp32 dot product, nothing written past the maps;
(2) every ``shape_*`` fixture of the unmodified reference in both precisions under the bars of tests/test_gpu_mlp_shapes.py, and a
    d_hidden 32 / d_latent 1024 / NV 3 case against the switch off;  (3) the switch on against off;
(4) the lookup modes: zeros padding against its reference fixture (a map with the bias folded in fails here:
    tests/test_linz_maps_gen_host.py), nearest / reflection against the switch off, the bicubic fixtures against their reference;
(5) the fall-backs equal the parent bit for bit;  (6) the cache follows the latent and the weights;
(7) render_image == forward bit for bit, a whole 32 x 32 frame on against off;  (8) training builds no maps.
Every comparison prints its measured maxima before it asserts."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from tests.test_gpu_mlp_shapes import SHAPE_FIXTURES, ShapeCase, T
from tests.test_gpu_mlp_shapes_f16 import _assert_frames, _assert_rgbsigma, _frames

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "f16x3"]
ROUTE = {"fp32": "points_mlp_gen", "f16x3": "points_mlp_gen_f16"}
ROUTE_LZ = {p: r + "_lz" for p, r in ROUTE.items()}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_cases = {}


def _shape_case(name, dev):
    if name not in _cases:
        _cases[name] = ShapeCase(name, dev)
    return _cases[name]


def _renderer(K=8, NC=64, G=4, white=True, precision="fp32", on=True, **kw):
    """``on`` None: built without the keyword at all (the parent's constructor call)"""
    from diner_amd import NeRFRendererDGS
    if on is not None:
        kw["linz_maps_any_shape"] = on
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=white, f16x3_any_shape=precision == "f16x3", **kw)
    r.precision = precision
    return r


def _case_renderer(c, precision, on=True, **kw):
    return _renderer(c.K, c.cfg["NC"], c.cfg["G"], c.scene.white_bkgd, precision, on, **kw)


def _predicted_bytes(r, model):
    """4 x diner_linz_maps_gen_floats for the scene the renderer has cached"""
    from diner_amd import _lib
    shape = r._validate(model)
    sc, _ = r._scene(model, need_latent=True)
    cs = shape.c_struct()
    return 4 * int(_lib.lib().diner_linz_maps_gen_floats(C.byref(sc), C.byref(cs)))


def _synthetic(dev, dims, NV, C_lat=512, HW=24, seed=11, K=8, stride=7, interp="bilinear", padding="border", fpad=4):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(HW, HW, NV, seed=seed, feature_padding=fpad, C=C_lat)
    w = synth.make_mlp_weights(seed + 1, bias_scale=0.1, d_latent=C_lat, **{k: v for k, v in dims.items() if k != "beta"})
    m = model_from_scene(sc, w, device=dev, d_latent=C_lat, index_interp=interp, index_padding=padding, **dims)
    rays = sc.target_rays()[:, ::stride]
    z = np.sort(np.random.RandomState(seed).uniform(sc.near, sc.far, (1, rays.shape[1], K)).astype(np.float32), -1)
    return sc, w, m, T(rays, dev), T(z, dev)


# ---- 1. the map builder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlz", [1, 3])
@pytest.mark.parametrize("d_latent, d_hidden", [(512, 128), (1024, 32), (8, 512)])
def test_builder_against_float64(d_latent, d_hidden, nlz, dev):
    """SB * NV = 3 maps of 5 x 7 texels: 105 texels, neither a square nor a multiple of the 64-texel tile.  Tolerance per element:
    d_latent * 2^-24 * (|W| @ |F|), the forward error bound of an fp32 dot product of that length in any order."""
    from diner_amd import _lib
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    dims = dict(d_hidden=d_hidden, n_blocks=3, combine_layer=nlz)
    sc0 = synth.make_scene(8, 8, 1, seed=2, feature_padding=2, C=d_latent)
    w = synth.make_mlp_weights(5, bias_scale=0.3, d_latent=d_latent, **dims)
    m = model_from_scene(sc0, w, device=dev, d_latent=d_latent, **dims)
    r = _renderer()
    shape = r._validate(m)
    packed = r._mlp_shape_general(m, shape, False)
    SB, NV, h, wd = 1, 3, 5, 7
    F = np.random.RandomState(9).standard_normal((SB, NV, h, wd, d_latent)).astype(np.float32)
    lat = T(F, dev)
    sc = _lib.DinerScene(SB=SB, NV=NV, H=8, W=8, h=h, w=wd, C=d_latent, num_freqs=6, image_w=8.0, image_h=8.0)
    sc.latent = lat.data_ptr()
    cs = shape.c_struct()
    n = int(_lib.lib().diner_linz_maps_gen_floats(C.byref(sc), C.byref(cs)))
    assert n == nlz * SB * NV * h * wd * d_hidden
    margin, sentinel = 4096, -7.25
    buf = torch.full((n + 2 * margin,), sentinel, dtype=torch.float32, device=dev)
    out = buf[margin:margin + n]
    _lib.check(_lib.lib().diner_pack_linz_maps_gen(C.byref(sc), C.byref(cs), packed.data_ptr(), out.data_ptr(), None), "diner_pack_linz_maps_gen")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:margin] == sentinel).all() and (got[margin + n:] == sentinel).all(), "the builder wrote outside the maps"
    got = got[margin:margin + n].reshape(nlz, SB * NV * h * wd, d_hidden).astype(np.float64)
    F64 = F.reshape(-1, d_latent).astype(np.float64)
    worst = 0.0
    for b in range(nlz):
        W = w[f"lin_z.{b}.weight"].astype(np.float64)
        ref, bound = F64 @ W.T, d_latent * 2.0 ** -24 * (np.abs(F64) @ np.abs(W).T)
        ratio = float((np.abs(got[b] - ref) / bound).max())
        worst = max(worst, ratio)
        print(f"builder d_latent {d_latent} d_hidden {d_hidden} map {b}/{nlz}: max |err| {np.abs(got[b] - ref).max():.2e}, max err / bound {ratio:.3f}")
    assert worst <= 1.0


# ---- 2. parity against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", SHAPE_FIXTURES)
def test_fixture_vs_reference(name, precision, dev):
    """Measured on the MI355X: see DESIGN.md §2."""
    c = _shape_case(name, dev)
    r = _case_renderer(c, precision)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    nlz = min(c.dims.get("combine_layer", 3), c.dims.get("n_blocks", 5))
    want_route = ROUTE_LZ[precision] if nlz > 0 else ROUTE[precision]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad():
            pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
            assert (r.last_route, r.last_binding, r.effective_precision) == (want_route, "ctypes", precision)
            out = r(c.model, rays, want_weights=True, z_samples=z).fine
    assert (r.last_route, r.last_binding, r.effective_precision) == (want_route, "ctypes", precision)
    cached = r.memory_report()["cached"]["linz_maps_gen"]
    assert cached == _predicted_bytes(r, c.model) and (cached > 0) == (nlz > 0)
    _assert_rgbsigma(pts, c.data["rgbsigma"], f"{name} {precision} lz render_points vs reference")
    _assert_frames(_frames(out), c.data, f"{name} {precision} lz forward vs reference")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_narrow_hidden_wide_latent_on_vs_off(precision, dev):
    """d_hidden 32 (one column tile, <1,1> with idle waves), d_latent 1024 (the builder's two 512-column pieces), NV 3, 53 rays x 7
    samples = 371 points: not a multiple of the 64-point tile"""
    dims = dict(d_hidden=32, n_blocks=3, combine_layer=2)
    sc, w, m, rays, z = _synthetic(dev, dims, NV=3, C_lat=1024, K=7, stride=11)
    assert (rays.shape[1] * 7) % 64 != 0
    res = {}
    with torch.no_grad():
        for on in (False, True):
            r = _renderer(7, precision=precision, on=on)
            pts = r.render_points(m, rays, z).cpu().numpy()[0]
            out = r(m, rays, want_weights=True, z_samples=z).fine
            assert r.last_route == (ROUTE_LZ if on else ROUTE)[precision]
            res[on] = (pts, _frames(out))
    _assert_rgbsigma(res[True][0], res[False][0], f"d_hidden 32, d_latent 1024, NV 3, {precision}: lz on vs off, render_points")
    _assert_frames(res[True][1], res[False][1], f"d_hidden 32, d_latent 1024, NV 3, {precision}: lz on vs off, forward")


# ---- 3. on against off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", SHAPE_FIXTURES)
def test_fixture_on_vs_off(name, precision, dev):
    c = _shape_case(name, dev)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    res = {}
    with torch.no_grad():
        for on in (False, True):
            r = _case_renderer(c, precision, on)
            pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
            out = r(c.model, rays, want_weights=True, z_samples=z).fine
            res[on] = (pts, _frames(out))
            assert (r.memory_report()["cached"]["linz_maps_gen"] > 0) == (on and r.last_route.endswith("_lz"))
    _assert_rgbsigma(res[True][0], res[False][0], f"{name} {precision}: lz on vs off, render_points")
    _assert_frames(res[True][1], res[False][1], f"{name} {precision}: lz on vs off, forward")


# ---- 4. lookup modes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_index_modes(precision, dev):
    from tests.test_gpu_index_modes import _case as index_case
    c = index_case("index_gen_zeros_h128", dev)
    assert not c.standard
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        r = _case_renderer(c, precision)
        pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
        assert (r.last_route, r.effective_precision) == (ROUTE_LZ[precision], precision)
        out = r(c.model, rays, want_weights=True, z_samples=z).fine
    _assert_rgbsigma(pts, c.data["rgbsigma"], f"index_gen_zeros_h128 {precision} lz render_points vs reference", mask=c.firm)
    fr = c.firm_rays
    assert fr.mean() >= 0.9
    for key in ("rgb", "depth"):
        err = float(np.abs(_frames(out)[key][fr] - c.data[key][fr]).max())
        print(f"index_gen_zeros_h128 {precision} lz forward vs reference: |{key}| {err:.2e}")
        assert err <= 1e-4, (key, err)
    for interp, padding in (("nearest", "border"), ("nearest", "zeros"), ("bilinear", "reflection"), ("nearest", "reflection")):
        m = c.make_model(interp, padding, dev)
        with torch.no_grad():
            a = _case_renderer(c, precision, on=False)
            ref = a.render_points(m, rays, z).cpu().numpy()[0]
            assert a.last_route == ROUTE[precision]
            b = _case_renderer(c, precision)
            got = b.render_points(m, rays, z).cpu().numpy()[0]
            assert b.last_route == ROUTE_LZ[precision]
        _assert_rgbsigma(got, ref, f"{interp} / {padding} {precision}: lz on vs off")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["bicubic_border_h128", "bicubic_zeros", "bicubic_reflection_fpad4"])
def test_bicubic_vs_reference(name, precision, dev):
    from tests.test_gpu_bicubic import _case as bicubic_case
    c = bicubic_case(name, dev)
    r, m = c.renderer(precision, linz_maps_any_shape=True), c.model()
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        pts = r.render_points(m, rays, z).cpu().numpy()[0]
        assert (r.last_route, r.last_binding, r.effective_precision) == (ROUTE_LZ[precision], "ctypes", precision)
        out = r(m, rays, want_weights=True, z_samples=z).fine
        assert r.last_route == ROUTE_LZ[precision]
    assert r.memory_report()["cached"]["linz_maps_gen"] == _predicted_bytes(r, m) > 0
    _assert_rgbsigma(pts, c.data["rgbsigma"], f"{name} {precision} lz render_points vs reference")
    for key in ("rgb", "depth"):
        err = float(np.abs(_frames(out)[key] - c.data[key]).max())
        print(f"{name} {precision} lz forward vs reference: |{key}| {err:.2e}")
        assert err <= 1e-4, (key, err)


# ---- 5. fall-backs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fallbacks_are_the_parent_bit_for_bit(precision, dev):
    c = _shape_case("shape_a_h128_nv2", dev)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]

    def run(r, model, rays, z):
        with torch.no_grad():
            pts = r.render_points(model, rays, z)
            o = r(model, rays, want_weights=True, z_samples=z).fine
        return pts, o.rgb, o.depth, o.weights

    parent = run(_case_renderer(c, precision, on=None), c.model, rays, z)
    budget = _case_renderer(c, precision)
    budget.linz_maps_max_bytes = 0
    off = _case_renderer(c, precision, on=False)
    for what, r in (("linz_maps_max_bytes = 0", budget), ("the switch left False", off)):
        got = run(r, c.model, rays, z)
        assert r.last_route == ROUTE[precision], what
        assert r.memory_report()["cached"]["linz_maps_gen"] == 0 and r._linz_gen_pack is None, what
        assert all(torch.equal(a, b) for a, b in zip(got, parent)), what
    # a model without lin_z layers
    dims = dict(d_hidden=64, n_blocks=2, combine_layer=0)
    sc, w, m, rays0, z0 = _synthetic(dev, dims, NV=3)
    on, par = _renderer(precision=precision), _renderer(precision=precision, on=None)
    got, want = run(on, m, rays0, z0), run(par, m, rays0, z0)
    assert on.last_route == par.last_route == ROUTE[precision]
    assert on.memory_report()["cached"]["linz_maps_gen"] == 0 and on._linz_gen_pack is None
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_the_standard_model_keeps_its_kernels(dev):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(32, 32, 4, seed=0, feature_padding=4)
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1), device=dev)
    rays = T(sc.target_rays()[:, ::4], dev)
    for precision, route in (("f16x3", "points_mlp_f16"), ("fp32", "points_mlp")):
        out = {}
        for on in (False, True):
            r = _renderer(16, 100, 6, precision=precision, on=on)
            r.seed = 5
            with torch.no_grad():
                out[on] = r(m, rays).fine.rgb
            assert r.last_route == route and r.effective_precision == precision
            assert r.memory_report()["cached"]["linz_maps_gen"] == 0
        assert torch.equal(out[False], out[True])


# ---- 6. the cache ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_cache_follows_its_sources(precision, dev):
    from diner_amd import glue
    dims = dict(d_hidden=64, n_blocks=3, combine_layer=2)
    sc, w, m, rays, z = _synthetic(dev, dims, NV=2, C_lat=256)

    def fresh():
        f = _renderer(precision=precision)
        with torch.no_grad():
            return f.render_points(m, rays, z)

    r = _renderer(precision=precision)
    with torch.no_grad():
        a = r.render_points(m, rays, z)
        maps = r._linz_gen_pack
        assert maps is not None and r.last_route == ROUTE_LZ[precision]
        b = r.render_points(m, rays, z)
        assert r._linz_gen_pack is maps and torch.equal(a, b)           # two identical calls build the maps once
        r(m, rays, z_samples=z)
        assert r._linz_gen_pack is maps
        # an in-place weight update
        m.mlp_fine.lin_z[0].weight.add_(0.05)
        c1 = r.render_points(m, rays, z)
        maps1 = r._linz_gen_pack
        assert maps1 is not maps and not torch.equal(c1, a) and torch.equal(c1, fresh())
        # a re-bound latent (what every encode() does)
        m.encoder.latent = (m.encoder.latent * 0.5).contiguous()
        c2 = r.render_points(m, rays, z)
        maps2 = r._linz_gen_pack
        assert maps2 is not maps1 and not torch.equal(c2, c1) and torch.equal(c2, fresh())
        # a latent in glue.assemble_latent's layout: the renderer reads the encoder's own buffer
        NV, Cc, h, wd = m.encoder.latent.shape[1:]
        m.encoder.latent = glue.assemble_latent([(m.encoder.latent[0] * 3.0).contiguous()], 1, NV)
        assert glue.latent_is_packed(m.encoder.latent)
        c3 = r.render_points(m, rays, z)
        assert r._linz_gen_pack is not maps2 and r.memory_report()["latent_zero_copy"]
        assert not torch.equal(c3, c2) and torch.equal(c3, fresh())
        assert r.memory_report()["cached"]["linz_maps_gen"] == 4 * 2 * 1 * NV * h * wd * 64
    m.mlp_fine.lin_z[0].weight.sub_(0.05)


# ---- 7. whole frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_render_image_equals_forward(precision, dev):
    from diner_amd import glue
    c = _shape_case("shape_a_h128_nv2", dev)
    r = _case_renderer(c, precision)
    sc = c.scene
    H = W = 16
    E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
    Kt = torch.tensor([[[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
    near, far = float(sc.near), float(sc.far)
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        rgb, depth = r.render_image(c.model, E, Kt, H, W, near, far, return_depth=True)
    assert (r.last_route, r.last_binding, r.effective_precision) == (ROUTE_LZ[precision], "ctypes", precision)
    rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        ref = r(c.model, rays).fine
    assert r.last_route == ROUTE_LZ[precision]
    assert torch.equal(rgb, ref.rgb.view(1, H, W, 3).permute(0, 3, 1, 2))
    assert torch.equal(depth, ref.depth.view(1, H, W, 1).permute(0, 3, 1, 2))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_frame_on_vs_off(precision, dev):
    """a 32 x 32 frame, d_hidden 256 (<2,1>), NV 2, K 40, NC 200: the whole forward() -- sampler, point kernel, compositing -- with
    replayed noise on both routes"""
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    K, NC, G = 40, 200, 15
    dims = dict(d_hidden=256, n_blocks=5, combine_layer=3)
    sc = synth.make_scene(32, 32, 2, seed=4, feature_padding=8)
    w = synth.make_mlp_weights(3, bias_scale=0.1, d_latent=sc.C, **dims)
    m = model_from_scene(sc, w, device=dev, d_latent=sc.C, **dims)
    rays = sc.target_rays()
    NR = rays.shape[1]
    assert NR == 32 * 32
    noise = tuple(T(n, dev)[None] for n in synth.make_noise(NR, NC, G, K, seed=6))
    res = {}
    with torch.no_grad():
        for on in (False, True):
            r = _renderer(K, NC, G, sc.white_bkgd, precision, on)
            out = r(m, T(rays, dev), want_weights=True, noise=noise).fine
            assert r.last_route == (ROUTE_LZ if on else ROUTE)[precision] and r.effective_precision == precision
            res[on] = _frames(out)
    assert np.isfinite(res[True]["rgb"]).all()
    _assert_frames(res[True], res[False], f"32 x 32 frame, d_hidden 256, NV 2, K 40, {precision}: lz on vs off")


# ---- 8. training ----------------------------------------------------------------------------------------------------------------
def test_training_is_untouched(dev):
    dims = dict(d_hidden=64, n_blocks=3, combine_layer=2)
    sc, w, m, rays, z = _synthetic(dev, dims, NV=2, C_lat=256)
    r = _renderer(precision="fp32", train_any_shape=True)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    try:
        out = r(m, rays, z_samples=z).fine
        assert r.last_route == "train_gen" and out.rgb.requires_grad
        out.rgb.sum().backward()
        assert m.mlp_fine.lin_z[0].weight.grad is not None
        assert r.memory_report()["cached"]["linz_maps_gen"] == 0 and r._linz_gen_pack is None
    finally:
        for p in m.mlp_fine.parameters():
            p.requires_grad_(False)
            p.grad = None
