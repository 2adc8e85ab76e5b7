"""GPU tests of the shape-general inference path (points_mlp_gen.hip through the *_gen entry points):
(i) the ``shape_*`` fixtures -- the unmodified reference built with non-standard ResnetFC / PositionalEncoding configurations
    (tools/gen_shape_golden.py) -- within 1e-4 abs on rgb, sigma and depth, with the reference's samples injected;
(ii) at the standard shape the generic kernel against the existing oracle-pinned fp32 kernel (goldens g0, g4), and the default
    route unchanged;
(iii) edge shapes, checked by identities the reference's arithmetic implies: a model padded with zero hidden units / zero latent
    channels computes the same function, a scene rendered in a batch equals it rendered alone, a point's result does not
    depend on where the tile boundaries fall."""
import json
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
SHAPE_FIXTURES = sorted(p.stem for p in GOLDEN.glob("shape_*.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class ShapeCase:
    def __init__(self, name, dev):
        from synthetic.model_stub import model_from_scene
        from tools.gen_shape_golden import case_inputs, input_digests, mlp_dims
        self.name = name
        self.data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
        self.cfg = json.loads(str(self.data["config"]))
        self.scene, self.weights, self.rays, noise = case_inputs(self.cfg)
        assert json.loads(str(self.data["digests"])) == input_digests(self.scene, self.weights, self.rays, noise)
        d = mlp_dims(self.cfg)
        self.dims = {k: v for k, v in d.items() if k not in ("d_in",)}
        self.model = model_from_scene(self.scene, self.weights, device=dev, num_freqs=self.cfg["num_freqs"], **self.dims)
        self.K = self.cfg["K"]

    def renderer(self, precision="fp32"):
        from diner_amd import NeRFRendererDGS
        r = NeRFRendererDGS(n_samples=self.K, n_depth_candidates=self.cfg["NC"], n_gaussian=self.cfg["G"],
                            white_bkgd=self.scene.white_bkgd)
        r.precision = precision
        return r


_cases = {}


@pytest.fixture(params=SHAPE_FIXTURES)
def case(request, dev):
    if request.param not in _cases:
        _cases[request.param] = ShapeCase(request.param, dev)
    return _cases[request.param]


def _assert_rgbsigma(got, ref, what):
    err_rgb = np.abs(got[..., :3] - ref[..., :3]).max()
    s_ref = ref[..., 3]
    err_s = (np.abs(got[..., 3] - s_ref) / np.maximum(1.0, s_ref / 12.0)).max()   # the sigma bar of tests/test_gpu_parity.py
    assert err_rgb <= 1e-4 and err_s <= 1e-4, f"{what}: |rgb| {err_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {err_s:.2e}"


def test_render_points_vs_reference(case, dev):
    r = case.renderer()
    with torch.no_grad():
        out = r.render_points(case.model, T(case.rays, dev), T(case.data["z_fill"], dev)[None]).cpu().numpy()[0]
    assert r.last_route == "points_mlp_gen" and r.last_binding == "ctypes" and r.effective_precision == "fp32"
    _assert_rgbsigma(out, case.data["rgbsigma"], case.name)


def test_forward_with_injected_samples_vs_reference(case, dev):
    r = case.renderer(precision="f16x3")               # the default: runs fp32 for this model and says so
    with pytest.warns(UserWarning, match="fp32"):
        with torch.no_grad():
            out = r(case.model, T(case.rays, dev), want_weights=True, z_samples=T(case.data["z_fill"], dev)[None]).fine
    assert r.last_route == "points_mlp_gen" and r.effective_precision == "fp32"
    rgb, depth, w = (out.rgb.cpu().numpy()[0], out.depth.cpu().numpy()[0], out.weights.cpu().numpy()[0])
    assert np.abs(rgb - case.data["rgb"]).max() <= 1e-4, case.name
    assert np.abs(depth - case.data["depth"]).max() <= 1e-4, case.name
    assert np.abs(w - case.data["weights"]).max() <= 1e-4, case.name


def test_forward_end_to_end_runs_the_generic_route(case, dev):
    """sampler -> generic point kernel -> compositing in one diner_render_gen call: finite images in range, and the stage-event
    form (the three entry points one by one) computes the same frame"""
    r = case.renderer()
    r.seed, r._calls = 7, 0
    with torch.no_grad():
        a = r(case.model, T(case.rays, dev)).fine
        r.seed, r._calls, r.stage_events = 7, 0, []
        b = r(case.model, T(case.rays, dev)).fine
    assert r.last_route == "points_mlp_gen" and len(r.stage_events) == 1
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.depth, b.depth)
    assert torch.isfinite(a.rgb).all() and float(a.rgb.min()) >= 0 and float(a.rgb.max()) <= 1 + 1e-5


def test_training_a_non_standard_model_raises(dev):
    c = ShapeCase(SHAPE_FIXTURES[0], dev)
    r = c.renderer()
    for p in c.model.mlp_fine.parameters():
        p.requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError, match="inference"):
            r.composite(c.model, T(c.rays, dev), T(c.data["z_fill"], dev)[None])
    finally:
        for p in c.model.mlp_fine.parameters():
            p.requires_grad_(False)


def test_no_mean_over_views_with_several_views_is_not_implemented(dev):
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(16, 16, 2, seed=3, feature_padding=4)
    dims = dict(d_hidden=64, n_blocks=2, combine_layer=1000)
    m = model_from_scene(sc, synth.make_mlp_weights(2, **dims), device=dev, **dims)
    rays = T(sc.target_rays()[:, ::8], dev)
    z = torch.linspace(1.2, 2.2, 8, device=dev).expand(1, rays.shape[1], 8).contiguous()
    r = NeRFRendererDGS(n_samples=8)
    r.precision = "fp32"
    with torch.no_grad(), pytest.raises(NotImplementedError, match="pixelnerf.py:137"):
        r.render_points(m, rays, z)


# ---- standard shape: the generic kernel against the existing fp32 kernel -------------------------------------------------------
@pytest.mark.parametrize("gname", ["g0_nv4_k16", "g4_nv4_k128_headline"])
def test_generic_kernel_matches_the_fp32_kernel_at_the_standard_shape(gname, dev):
    from diner_amd import NeRFRendererDGS
    from synthetic.model_stub import model_from_scene
    g = load_golden(gname)
    m = model_from_scene(g.scene, g.weights, device=dev)
    rays, z = T(g.rays, dev), T(g["z_fill"], dev)[None]
    ref = NeRFRendererDGS(n_samples=g.K, n_depth_candidates=g.NC, n_gaussian=g.G, white_bkgd=g.scene.white_bkgd)
    ref.precision = "fp32"
    gen = NeRFRendererDGS(n_samples=g.K, n_depth_candidates=g.NC, n_gaussian=g.G, white_bkgd=g.scene.white_bkgd)
    gen.precision = "fp32"
    gen._force_gen = True
    with torch.no_grad():
        a = ref.render_points(m, rays, z)
        assert ref.last_route == "points_mlp"
        b = gen.render_points(m, rays, z)
        assert gen.last_route == "points_mlp_gen"
        fa = ref(m, rays, z_samples=z).fine
        fb = gen(m, rays, z_samples=z).fine
    assert float((a - b).abs().max()) <= 1e-5
    assert float((fa.rgb - fb.rgb).abs().max()) <= 1e-5 and float((fa.depth - fb.depth).abs().max()) <= 1e-5
    assert gen.memory_report()["cached"]["mlp_gen_packed"] > 0 and ref.memory_report()["cached"]["mlp_gen_packed"] == 0


def test_default_renderer_keeps_the_existing_kernels_for_the_standard_model(dev):
    from diner_amd import NeRFRendererDGS
    from synthetic.model_stub import model_from_scene
    g = load_golden("g0_nv4_k16")
    m = model_from_scene(g.scene, g.weights, device=dev)
    rays = T(g.rays, dev)
    r = NeRFRendererDGS(n_samples=g.K, n_depth_candidates=g.NC, n_gaussian=g.G, white_bkgd=g.scene.white_bkgd)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*precision=")
        with torch.no_grad():
            r(m, rays)
            assert r.last_route == "points_mlp_f16" and r.effective_precision == "f16x3"
            r.render_points(m, rays, T(g["z_fill"], dev)[None])
            assert r.last_route == "points_mlp_f16"
            r.precision = "fp32"
            r(m, rays)
            assert r.last_route == "points_mlp" and r.effective_precision == "fp32"
    assert r.memory_report()["cached"]["mlp_gen_packed"] == 0


# ---- render_image ---------------------------------------------------------------------------------------------------------------
def test_render_image_equals_forward_for_a_non_standard_model(dev):
    """render_image (rays generated inside the sampler, diner_render_image_gen) against gen_rays -> forward (diner_render_gen) with
    the same seed: the same samples, so the same image, bit for bit (as tests/test_glue.py checks for the standard model)"""
    from diner_amd import glue
    c = ShapeCase("shape_a_h128_nv2", dev)
    r = c.renderer()
    sc = c.scene
    H, W = 20, 28
    E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
    Kt = torch.tensor([[[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
    near, far = float(sc.near), float(sc.far)
    r.seed, r._calls = 3, 0
    rgb, depth = r.render_image(c.model, E, Kt, H, W, near, far, return_depth=True)
    assert r.last_route == "points_mlp_gen"
    rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        ref = r(c.model, rays).fine
    assert torch.equal(rgb, ref.rgb.view(1, H, W, 3).permute(0, 3, 1, 2))
    assert torch.equal(depth, ref.depth.view(1, H, W, 1).permute(0, 3, 1, 2))


# ---- edge shapes --------------------------------------------------------------------------------------------------------------
def _pad_model_weights(w, dims, d_hidden_to=None, d_latent_to=None):
    """the same function with zero hidden units / zero latent channels appended: a zero row of W (and bias) makes the unit 0, its
    activation relu(0) = 0, and a zero column of the next W drops it; zero latent channels meet zero lin_z columns"""
    H, Hp = dims["d_hidden"], d_hidden_to or dims["d_hidden"]
    out = {}
    for k, v in w.items():
        v = np.asarray(v)
        if k.endswith("bias"):
            n = Hp if v.shape[0] == H and not k.startswith("lin_out") else v.shape[0]
            out[k] = np.concatenate([v, np.zeros(n - v.shape[0], np.float32)])
            continue
        rows = Hp if not k.startswith("lin_out") else v.shape[0]
        cols = v.shape[1]
        if k.startswith(("blocks", "lin_out")):
            cols = Hp
        elif k.startswith("lin_z") and d_latent_to:
            cols = d_latent_to
        p = np.zeros((rows, cols), np.float32)
        p[:v.shape[0], :v.shape[1]] = v
        out[k] = p
    return out


def _edge_render(dev, NV, dims, seed=11, C=512, latent=None, SB_scenes=None, K=12, stride=7, weights=None, rays_sel=None):
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(24, 24, NV, seed=seed, feature_padding=4, C=C)
    if latent is not None:
        sc.latent = latent
    w = weights if weights is not None else synth.make_mlp_weights(seed + 1, bias_scale=0.1, **{k: v for k, v in dims.items() if k != "beta"})
    m = model_from_scene(sc, w, device=dev, d_latent=C, **dims)
    rays = sc.target_rays()[:, ::stride] if rays_sel is None else rays_sel
    NR = rays.shape[1]
    z = np.sort(np.random.RandomState(seed).uniform(sc.near, sc.far, (1, NR, K)).astype(np.float32), -1)
    r = NeRFRendererDGS(n_samples=K)
    r.precision = "fp32"
    with torch.no_grad():
        out = r.render_points(m, T(rays, dev), T(z, dev))
    assert r.last_route == "points_mlp_gen"
    return out.cpu().numpy(), sc, w, rays, z


@pytest.mark.parametrize("dims, NV", [
    (dict(d_hidden=32, n_blocks=2, combine_layer=1), 8),
    (dict(d_hidden=32, n_blocks=1, combine_layer=0), 3),
    (dict(d_hidden=96, n_blocks=1, combine_layer=1000), 1),
    (dict(d_hidden=64, n_blocks=3, combine_layer=2, beta=5.0), 2),
])
def test_zero_padded_hidden_units_change_nothing(dev, dims, NV):
    """a d_hidden model against the same model padded with zero units to 160 (<2,1> instantiation) and 320 (<2,2>): exercises every
    tile-to-wave mapping, n_blocks = 1, combine_layer 0 and >= n_blocks, NV 1 .. 8 (ReLU only for the padding identity: softplus(0)
    is not 0 -- its case is compared at its own width)"""
    base, sc, w, rays, z = _edge_render(dev, NV, dims)
    assert np.isfinite(base).all()
    if dims.get("beta", 0) > 0:
        return
    for Hp in (160, 320):
        wp = _pad_model_weights(w, dims, d_hidden_to=Hp)
        padded, *_ = _edge_render(dev, NV, dict(dims, d_hidden=Hp), weights=wp)
        np.testing.assert_allclose(padded, base, rtol=0, atol=1e-6, err_msg=f"padded to {Hp}")


def test_wide_latent_runs_in_pieces(dev):
    """d_latent = 1024 (two 512-column pieces of the LDS image) with the upper 512 channels of zero weight equals d_latent = 512"""
    dims = dict(d_hidden=64, n_blocks=3, combine_layer=2)
    base, sc, w, rays, z = _edge_render(dev, 2, dims, C=512)
    rs = np.random.RandomState(5)
    wide = np.concatenate([sc.latent, rs.standard_normal(sc.latent.shape).astype(np.float32)], axis=2)
    wp = _pad_model_weights(w, dims, d_latent_to=1024)
    got, *_ = _edge_render(dev, 2, dims, C=1024, latent=wide, weights=wp)
    np.testing.assert_allclose(got, base, rtol=0, atol=1e-6)


def test_tile_boundaries_and_ray_counts(dev):
    """ray counts that are not a multiple of the 64-point tile: each subset's points equal the same points in the full batch"""
    dims = dict(d_hidden=128, n_blocks=3, combine_layer=1)
    from diner_amd import NeRFRendererDGS
    from synthetic.model_stub import model_from_scene
    full, sc, w, rays, z = _edge_render(dev, 2, dims, K=7, stride=5)
    m = model_from_scene(sc, w, device=dev, **dims)
    r = NeRFRendererDGS(n_samples=7)
    r.precision = "fp32"
    for lo, hi in ((0, 1), (3, 12), (5, rays.shape[1])):
        with torch.no_grad():
            part = r.render_points(m, T(rays[:, lo:hi], dev), T(z[:, lo:hi], dev)).cpu().numpy()
        assert np.array_equal(part, full[:, lo:hi]), (lo, hi)


def test_two_scenes_in_a_batch(dev):
    """SB = 2: each scene of the batch equals the scene rendered alone"""
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    dims = dict(d_hidden=64, n_blocks=3, combine_layer=2)
    a, sa, w, rays, z = _edge_render(dev, 3, dims, seed=21)
    b, sb_, _, _, z_b = _edge_render(dev, 3, dims, seed=22, weights=w, rays_sel=rays)
    both = synth.make_scene(24, 24, 3, seed=21, feature_padding=4)
    for f in ("poses", "focal", "c", "depths", "depths_std", "normals", "latent"):
        setattr(both, f, np.concatenate([getattr(sa, f), getattr(sb_, f)], 0))
    m = model_from_scene(both, w, device=dev, **dims)
    r = NeRFRendererDGS(n_samples=z.shape[-1])
    r.precision = "fp32"
    with torch.no_grad():
        out = r.render_points(m, T(np.concatenate([rays, rays]), dev), T(np.concatenate([z, z_b]), dev)).cpu().numpy()
    assert np.array_equal(out[:1], a) and np.array_equal(out[1:], b)
