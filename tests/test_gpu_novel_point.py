"""The NOVEL point model on the GPU (diner_amd.novel.NeRFRendererDGS.render_points_novel; csrc/points_mlp_gen_nv.hip and
points_mlp_gen_f16_nv.hip through diner_render_points_novel):
(i)   every ``novel_point_*`` fixture -- the unmodified reference's NOVEL PixelNeRF on the CPU (tools/gen_novel_point_golden.py) -- in fp32
      and f16x3 at the bars tests/test_gpu_mlp_shapes*.py hold the same kernels to (rgb 1e-4 abs, sigma 1e-4 relative to max(1, sigma/12)),
      every point compared, and a second run bit-equal;
(ii)  with gen_latent = 0, xyz_gen = xyz_in and points formed from rays and depths the output is ``render_points`` of the plain renderer
      on the shape-general kernel bit for bit (the sum is formed before lin_z, so adding a zero lookup changes nothing);
(iii) the cache of the packed general latent follows an in-place change;
(iv)  ``composite()`` and ``forward()`` with ``hip_point_model`` against the PyTorch route on the restated model (tests/novel_point_ref.py),
      on the geometry of tests/golden/novel_sampler.npz, and ``last_route`` in every routing case.
tests/test_novel_point_host.py proves the restatement against the same fixtures on the CPU."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from synthetic import synth
from tests import novel_point_ref as R
from tests import novel_sampler_ref as N
from tools.gen_novel_point_golden import CASES, case_inputs, input_digests

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
BOUND = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


_cases = {}


def case(name, dev):
    """(inputs rebuilt from seeds and digest-checked, the stand-in model on the device, the reference's rgb-sigma): built once"""
    if name not in _cases:
        inp, g = case_inputs(CASES[name]), np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
        assert json.loads(str(g["digests"])) == input_digests(inp)
        _cases[name] = (inp, R.model_from_inputs(inp, device=dev), g["rgbsigma"])
    return _cases[name]


def renderer(precision="fp32", **kw):
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(f16x3_any_shape=precision == "f16x3", **kw)
    r.precision = precision
    return r


ROUTE = {"fp32": "novel_points_gen", "f16x3": "novel_points_gen_f16"}


# ---- (i) golden parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_points_novel_meets_the_reference(name, precision, dev):
    inp, m, ref = case(name, dev)
    r = renderer(precision)
    args = [T(inp[k], dev) for k in ("xyz_in", "xyz_gen", "viewdirs")]
    out = r.render_points_novel(m, *args)
    assert r.last_route == ROUTE[precision] and r.last_binding == "ctypes" and r.effective_precision == precision
    assert out.shape == ref.shape and m.calls == 0
    e_rgb, e_sigma = R.rgbsigma_errors(out.cpu().numpy(), ref)
    print(f"{name} {precision}: |rgb| {e_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {e_sigma:.2e}")
    assert e_rgb <= BOUND and e_sigma <= BOUND
    again = renderer(precision).render_points_novel(m, *args)              # another renderer: packs of its own
    assert torch.equal(out, again) and torch.equal(out, r.render_points_novel(m, *args))


def test_precision_without_the_any_shape_switch_runs_fp32_and_says_so(dev):
    inp, m, ref = case("novel_point_b", dev)
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS()                                                   # precision "f16x3", f16x3_any_shape False
    with pytest.warns(UserWarning, match="fp32"):
        out = r.render_points_novel(m, *[T(inp[k], dev) for k in ("xyz_in", "xyz_gen", "viewdirs")])
    assert r.last_route == "novel_points_gen" and r.effective_precision == "fp32"
    assert torch.equal(out, renderer("fp32").render_points_novel(m, *[T(inp[k], dev) for k in ("xyz_in", "xyz_gen", "viewdirs")]))


def test_no_points(dev):
    inp, m, _ = case("novel_point_b", dev)
    e = torch.empty((1, 0, 3), device=dev)
    assert renderer().render_points_novel(m, e, e, e).shape == (1, 0, 4)


# ---- (ii) against the plain renderer's shape-general kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, precision", [("novel_point_a", "fp32"), ("novel_point_d", "fp32"), ("novel_point_d", "f16x3")])
def test_zero_general_latent_is_the_plain_point_kernel_bit_for_bit(name, precision, dev):
    """bilinear / border; (a): the standard shape, on the shape-general kernel under _force_gen; (d): two gather pieces"""
    from diner_amd import NeRFRendererDGS
    inp, m, _ = case(name, dev)
    SB, P, K = inp["poses"].shape[0], inp["xyz_in"].shape[1], 5
    B = P // K
    rs = np.random.RandomState(9)
    d = rs.standard_normal((SB, B, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = inp["xyz_in"][:, :B] - 1.75 * d            # every sample within 0.75 of the fixture's box: in front of every source camera
    rays = T(np.concatenate([o, d, np.full((SB, B, 1), 1.0), np.full((SB, B, 1), 2.5)], -1), dev)
    z = T(np.sort(rs.uniform(1.0, 2.5, (SB, B, K)), -1), dev)
    pts = (rays[..., None, :3] + z[..., None] * rays[..., None, 3:6]).reshape(SB, B * K, 3).contiguous()      # nerf_renderer.py:304
    dirs = rays[..., None, 3:6].expand(-1, -1, K, -1).reshape(SB, B * K, 3).contiguous()
    plain = NeRFRendererDGS(n_samples=K)
    plain.precision, plain.f16x3_any_shape, plain._force_gen = precision, precision == "f16x3", name == "novel_point_a"
    keep = m.gen_latent.detach().clone()
    try:
        with torch.no_grad():
            m.gen_latent.zero_()
        with torch.no_grad():
            want = plain.render_points(m, rays, z).reshape(SB, B * K, 4)
        assert plain.last_route == ("points_mlp_gen_f16" if precision == "f16x3" else "points_mlp_gen")
        got = renderer(precision).render_points_novel(m, pts, pts, dirs)
    finally:
        with torch.no_grad():
            m.gen_latent.copy_(keep)                  # (in place on the parameter itself: its version counter moves)
    assert torch.isfinite(want).all() and float(want[..., 3].max()) > 0
    assert torch.equal(got, want), float((got - want).abs().max())


# ---- (iii) the cache ---------------------------------------------------------------------------------------------------------------------------
def test_general_latent_cache_follows_an_in_place_change(dev):
    inp, m, ref = case("novel_point_c", dev)
    r = renderer()
    args = [T(inp[k], dev) for k in ("xyz_in", "xyz_gen", "viewdirs")]
    a = r.render_points_novel(m, *args)
    pack = r._gen_latent_pack
    assert r.render_points_novel(m, *args) is not a and r._gen_latent_pack is pack                # unchanged: the same pack
    rep = r.memory_report(m)["cached"]
    assert rep["gen_latent_nhwc"] == inp["gen_latent"].size * 4 and rep["total"] == sum(v for k, v in rep.items() if k != "total")
    keep = m.gen_latent.detach().clone()
    try:
        with torch.no_grad():
            m.gen_latent.mul_(0.5)                                                                   # what an optimizer step does
        b = r.render_points_novel(m, *args)
        assert r._gen_latent_pack is not pack and not torch.equal(a, b)
        assert torch.equal(b, renderer().render_points_novel(m, *args))
    finally:
        with torch.no_grad():
            m.gen_latent.copy_(keep)                  # (in place on the parameter itself: its version counter moves)
    assert max(R.rgbsigma_errors(r.render_points_novel(m, *args).cpu().numpy(), ref)) <= BOUND
    # the general cameras are read again after encode_gen writes them in place
    with torch.no_grad():
        m.gen_c.add_(3.0)
        try:
            assert not torch.equal(r.render_points_novel(m, *args), a)
        finally:
            m.gen_c.sub_(3.0)


# ---- (iv) composite(), forward() and the routing ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler_case(dev):
    """the nc64 case of tests/golden/novel_sampler.npz (its rays, filled z, vertices and both offset sets) with a NOVEL stand-in model
    on its scene: the standard-width lookup into a 64-channel latent, a 128-wide MLP"""
    g = np.load(GOLDEN / "novel_sampler.npz")
    c = N.GOLDEN_CASES["nc64"].build()
    rec = {k: g[f"nc64.{k}"] for k in ("rays", "z", "vertices", "offsets_in", "offsets_gen")}
    assert np.array_equal(rec["rays"], c.rays) and np.array_equal(rec["vertices"], c.vertices)
    sc = c.batched_scene()
    rs = np.random.RandomState(31)
    Cc, fp = 64, 4
    dims = dict(d_latent=Cc, d_hidden=128, n_blocks=3, combine_layer=2, beta=0.0)
    inp = {k: getattr(sc, k) for k in ("poses", "focal", "c", "image_shape", "depths", "depths_std", "normals")}
    inp["latent"] = rs.standard_normal((1, c.NV, Cc, 12 + 2 * fp, 12 + 2 * fp)).astype(np.float32)
    inp["weights"] = synth.make_mlp_weights(32, bias_scale=0.1, d_in=55, **{k: v for k, v in dims.items() if k != "beta"})
    inp["gen_latent"] = rs.standard_normal((Cc, 28, 20)).astype(np.float32)
    inp["gen_poses"] = synth.look_at_origin_w2c(0.7, 1.7)[None, None]
    inp["gen_focal"], inp["gen_c"] = np.array([[[60.0, 63.0]]], np.float32), np.array([[[21.5, 26.0]]], np.float32)
    inp["gen_image_shape"] = np.array([40, 56], np.float32)
    inp["cfg"] = dict(scene=dict(feature_padding=fp), num_freqs=6, index_interp="bilinear", index_padding="border")
    inp["dims"] = dims
    return c, {k: T(v, dev) for k, v in rec.items()}, R.model_from_inputs(inp, device=dev)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_composite_and_forward_match_the_torch_route(sampler_case, precision, dev):
    c, rec, m = sampler_case
    geo = (rec["vertices"], rec["offsets_in"], rec["offsets_gen"])
    on = renderer(precision, n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G, hip_point_model=True)
    off = renderer("fp32", n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G)
    m.calls = 0
    with torch.no_grad():
        want = off.composite(m, rec["rays"], rec["z"], *geo)
        assert off.last_route == "torch" and m.calls == 1
        got = on.composite(m, rec["rays"], rec["z"], *geo)
        assert on.last_route == ROUTE[precision] and on.effective_precision == precision and m.calls == 1
        on.check_finite()
        for k, a, b in zip(("weights", "rgb", "depth"), got, want):
            err = float((a - b).abs().max())
            print(f"composite {precision}: max |d {k}| = {err:.2e}")
            assert err <= BOUND, k
        assert float(want[0].sum(-1).max()) > 0.5 and float(want[1].std()) > 1e-2                   # (a frame with content)
        for r in (on, off):
            r.seed, r._calls = 7, 0
        fw = off(m, rec["rays"], *geo, want_weights=True).fine
        fg = on(m, rec["rays"], *geo, want_weights=True).fine
        assert on.last_route == ROUTE[precision] and off.last_route == "torch" and m.calls == 2
        for k in ("rgb", "depth", "weights"):
            err = float((fg[k] - fw[k]).abs().max())
            print(f"forward {precision}: max |d {k}| = {err:.2e}")
            assert err <= BOUND, k


def test_routing_cases(sampler_case, dev):
    from diner_amd.novel import NeRFRendererDGS
    c, rec, m = sampler_case
    call = lambda r, model=m: r.composite(model, rec["rays"], rec["z"], rec["vertices"], rec["offsets_in"], rec["offsets_gen"])
    kw = dict(n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G)
    r = renderer("fp32", hip_point_model=True, **kw)
    m.calls = 0
    call(r)                                                                     # grad mode on, no parameter requires grad: the kernel
    assert r.last_route == "novel_points_gen" and m.calls == 0
    m.gen_latent.requires_grad_(True)                                           # training: PyTorch, with a graph to the parameter
    try:
        w, rgb, depth = call(r)
        assert r.last_route == "torch" and m.calls == 1 and rgb.requires_grad
        g, = torch.autograd.grad(rgb.sum(), m.gen_latent)
        assert float(g.abs().max()) > 0
        with torch.no_grad():
            call(r)
        assert r.last_route == "novel_points_gen" and m.calls == 1
    finally:
        m.gen_latent.requires_grad_(False)
    with torch.no_grad():
        r.hip_point_model = False                                               # a plain attribute
        call(r)
        assert r.last_route == "torch" and m.calls == 2
        r.hip_point_model = True
        m.encoder.index_interp = "bicubic"
        try:
            call(r)
            assert r.last_route == "torch" and m.calls == 3
        finally:
            m.encoder.index_interp = "bilinear"
        m.encoder.index_padding = "reflection"                                  # a served mode: the kernel, like the PyTorch route
        try:
            got = call(r)
            assert r.last_route == "novel_points_gen" and m.calls == 3
            want = call(renderer("fp32", **kw))
            assert float((got[1] - want[1]).abs().max()) <= BOUND and m.calls == 4
        finally:
            m.encoder.index_padding = "border"
        rp = NeRFRendererDGS(pass_points=True, hip_point_model=True, **kw)
        seen = []
        fn = lambda a, b, p, viewdirs=None: seen.append(1) or m(a, b, viewdirs=viewdirs)
        call(rp, fn)
        assert rp.last_route == "torch" and seen == [1]
