"""GPU tests of the bicubic latent lookup (SpatialEncoder index_interp="bicubic", reference src/models/image_encoder.py:24-25,119-125;
renderer switch ``bicubic_index``):
(i) the ``bicubic_*`` render fixtures -- the unmodified reference built with index_interp="bicubic" and each padding
    (tools/gen_bicubic_golden.py) -- within tests/test_gpu_index_modes.py's bar with the reference's samples injected, in fp32 on
    points_mlp_gen and in f16x3 on points_mlp_gen_f16, every sample compared; the bilinear render of the same model is far from it;
(ii) render_image equal to forward(gen_rays(...)) bit for bit;
(iii) stage level: diner_train_point_inputs_gen_bc's zlat against tests/bicubic_ref.py and diner_train_bicubic_scatter against torch
    autograd's input gradient, on maps smaller than the footprint;
(iv) training: the gradients of the training and camera-gradient fixtures in fp32 and f16x3 (tests/test_training.py's and
    tests/test_gpu_camera_grads.py's tolerances), and a whole frame's backward against forward(gen_rays(...)) under autograd."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bicubic_ref as br

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
RENDER = ["bicubic_border_h128", "bicubic_reflection_fpad4", "bicubic_zeros"]
PRECISIONS = ["fp32", "f16x3"]
ROUTE = {"fp32": "points_mlp_gen", "f16x3": "points_mlp_gen_f16"}
TRAIN_ROUTE = {"fp32": "train_gen", "f16x3": "train_gen_f16"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Case:
    def __init__(self, name, dev):
        from tools.gen_bicubic_golden import case_inputs, input_digests, mlp_dims
        self.data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
        self.cfg = json.loads(str(self.data["config"]))
        self.scene, self.weights, self.rays, noise = case_inputs(self.cfg)
        assert json.loads(str(self.data["digests"])) == input_digests(self.scene, self.weights, self.rays, noise)
        self.dims = {k: v for k, v in mlp_dims(self.cfg).items() if k != "d_in"}
        self.dev = dev

    def model(self, interp="bicubic"):
        from synthetic.model_stub import model_from_scene
        return model_from_scene(self.scene, self.weights, device=self.dev, num_freqs=self.cfg["num_freqs"], index_interp=interp,
                                index_padding=self.cfg["padding"], **self.dims)

    def renderer(self, precision, **switches):
        from diner_amd import NeRFRendererDGS
        r = NeRFRendererDGS(n_samples=self.cfg["K"], n_depth_candidates=self.cfg["NC"], n_gaussian=self.cfg["G"],
                            white_bkgd=self.scene.white_bkgd, bicubic_index=True, f16x3_any_shape=precision == "f16x3", **switches)
        r.precision = precision
        return r


_cases = {}


def _case(name, dev):
    if name not in _cases:
        _cases[name] = Case(name, dev)
    return _cases[name]


# ---- (i) render against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", RENDER)
def test_render_vs_reference(name, precision, dev):
    c = _case(name, dev)
    r, m = c.renderer(precision), c.model()
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        pts = r.render_points(m, rays, z).cpu().numpy()[0]
        assert (r.last_route, r.last_binding, r.effective_precision) == (ROUTE[precision], "ctypes", precision)
        assert r._linz_pack is None                                      # no lin_z maps are built for a bicubic model
        out = r(m, rays, z_samples=z).fine
        assert (r.last_route, r.last_binding) == (ROUTE[precision], "ctypes")
    ref = c.data["rgbsigma"]
    err_rgb = np.abs(pts[..., :3] - ref[..., :3]).max()
    err_s = (np.abs(pts[..., 3] - ref[..., 3]) / np.maximum(1.0, ref[..., 3] / 12.0)).max()     # tests/test_gpu_index_modes.py's bar
    print(f"{name} {precision}: |rgb| {err_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {err_s:.2e}")
    assert err_rgb <= 1e-4 and err_s <= 1e-4, (err_rgb, err_s)
    np.testing.assert_allclose(out.rgb.cpu().numpy()[0], c.data["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.depth.cpu().numpy()[0], c.data["depth"], rtol=0, atol=1e-4)


@pytest.mark.parametrize("name", RENDER)
def test_the_mode_matters(name, dev):
    c = _case(name, dev)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        base = c.renderer("fp32").render_points(c.model("bilinear"), rays, z).cpu().numpy()[0]
    assert np.abs(base - c.data["rgbsigma"]).max() > 1e-2


def test_default_renderer_still_refuses(dev):
    from diner_amd import NeRFRendererDGS
    c = _case("bicubic_zeros", dev)
    with pytest.raises(NotImplementedError, match="bicubic_index"), torch.no_grad():
        NeRFRendererDGS(n_samples=c.cfg["K"])(c.model(), T(c.rays, dev))


def test_sampler_and_memory_report_on_a_fresh_renderer(dev):
    """the stages that never validate a model serve a bicubic one without any call before them (the sampler does not use the latent
    lookup), and give what a renderer that has rendered the model gives"""
    c = _case("bicubic_zeros", dev)
    m, rays = c.model(), T(c.rays, dev)
    K, NC, G = c.cfg["K"], c.cfg["NC"], c.cfg["G"]
    fresh, used = c.renderer("fp32"), c.renderer("fp32")
    with torch.no_grad():
        used(m, rays)
        used.seed, used._calls, fresh.seed, fresh._calls = 7, 0, 7, 0
        z_used = used.sample_depthguided(rays, m, K, NC, n_gaussian=G)
        z_fresh = fresh.sample_depthguided(rays, m, K, NC, n_gaussian=G)
    assert torch.equal(z_fresh, z_used) and bool(torch.isfinite(z_fresh).all())
    rep = c.renderer("fp32").memory_report(m, rays_per_call=64)
    assert rep["bicubic_index"] is True and rep["cached"]["linz_maps"] == 0


# ---- (ii) render_image ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("bicubic_zeros", "f16x3"), ("bicubic_reflection_fpad4", "fp32"), ("bicubic_border_h128", "fp32")])
def test_render_image_equals_forward(name, precision, dev):
    from diner_amd import glue
    c = _case(name, dev)
    r, m, sc = c.renderer(precision), c.model(), c.scene
    H, W = 20, 28
    E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
    Kt = torch.tensor([[[0.6 * W, 0, W / 2], [0, 0.6 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
    near, far = float(sc.near), float(sc.far)
    r.seed, r._calls = 3, 0
    rgb, depth = r.render_image(m, E, Kt, H, W, near, far, return_depth=True)
    assert (r.last_route, r.last_binding) == (ROUTE[precision], "ctypes")
    rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        ref = r(m, rays).fine
    assert (r.last_route, r.last_binding) == (ROUTE[precision], "ctypes")
    assert torch.equal(rgb, ref.rgb.view(1, H, W, 3).permute(0, 3, 1, 2))
    assert torch.equal(depth, ref.depth.view(1, H, W, 1).permute(0, 3, 1, 2))


# ---- (iii) stage level ------------------------------------------------------------------------------------------------------------
class Stage:
    """One scene of NV identity cameras looking down +z at points of depth 1, so that a point's normalised coordinate in view v is the
    fp32 value ((x + cx_v) / 2 * 2 - 1) of its ray origin (focal 1, image_shape 2): the kernel's coordinate is known to the last bit and
    the reference (tests/bicubic_ref.py, coord_dtype=float32) starts from the same number."""

    def __init__(self, h, w, Cc, P, NV, dev, seed):
        from diner_amd import _lib
        g = torch.Generator().manual_seed(seed)
        self.h, self.w, self.C, self.P, self.NV, self.dev = h, w, Cc, P, NV, dev
        self.latent = torch.rand((NV, Cc, h, w), generator=g) * 2 - 1                         # unit scale, NCHW
        self.lat_nhwc = self.latent.permute(0, 2, 3, 1).contiguous().to(dev)
        # centre coordinates from -3 to size + 3 texels: the first half a slow sweep (consecutive rows share footprints), then random,
        # then near-integers
        n_sw = P // 2
        # (a lone point sits inside the map: outside, under zeros padding, its whole gradient would be an outer weight's rounding)
        t = torch.cat([torch.linspace(0, 1, n_sw), torch.rand(P - n_sw, generator=g)]) if P > 1 else torch.tensor([0.5])
        s = torch.cat([torch.linspace(0.2, 0.8, n_sw), torch.rand(P - n_sw, generator=g)]) if P > 1 else torch.tensor([0.45])
        ix, iy = t * (w + 6) - 3, s * (h + 6) - 3
        if P > 8:
            ix[-4:], iy[-4:] = torch.tensor([-1.0, 0.0, w - 1.0, w + 1.0]), torch.tensor([0.0, h - 1.0, -2.0, 1.0])
        ox, oy = (2 * ix + 1) / w, (2 * iy + 1) / h                                           # u + 1
        self.c = torch.tensor([[0.0, 0.0], [0.25, -0.5], [-0.375, 0.125]])[:NV].contiguous()
        rays = torch.zeros((1, P, 8))
        rays[0, :, 0], rays[0, :, 1], rays[0, :, 5], rays[0, :, 7] = ox, oy, 1.0, 2.0
        self.u = torch.stack([(ox + self.c[v, 0]) / 2 * 2 - 1 for v in range(NV)])            # fp32, the kernel's operations
        self.v = torch.stack([(oy + self.c[v, 1]) / 2 * 2 - 1 for v in range(NV)])
        self.t = dict(rays=rays.to(dev), z=torch.ones((1, P, 1), device=dev), poses=torch.eye(4).repeat(1, NV, 1, 1).contiguous().to(dev),
                      focal=torch.ones((1, NV, 2), device=dev), c=self.c[None].contiguous().to(dev),
                      maps=torch.zeros((1, NV, 2, 2, 8), device=dev))
        sc = _lib.DinerScene(SB=1, NV=NV, H=2, W=2, h=h, w=w, C=Cc, num_freqs=1, image_w=2.0, image_h=2.0, feature_padding=0.0,
                             freq_factor=1.0)
        sc.poses, sc.focal, sc.c, sc.maps = (self.t[k].data_ptr() for k in ("poses", "focal", "c", "maps"))
        sc.latent = self.lat_nhwc.data_ptr()
        self.scene = sc

    def point_inputs(self, pad):
        from diner_amd import _lib
        from diner_amd.renderer import _ptr, _stream
        R = self.NV * self.P
        inp, zl, taps = (torch.full((R, n), float("nan"), device=self.dev) for n in (16, self.C, 16))
        rc = _lib.lib().diner_train_point_inputs_gen_bc(C.byref(self.scene), pad, _ptr(self.lat_nhwc), _ptr(self.t["rays"]), _ptr(self.t["z"]),
                                                        self.P, 1, 0, _ptr(inp), 16, _ptr(zl), _ptr(taps), _stream(self.dev))
        assert rc == 0, _lib.lib().diner_last_error()
        torch.cuda.synchronize()
        return zl, taps


STAGE_SHAPES = [(Cc, P, NV) for Cc in (8, 72, 1024) for P in (1, 65) for NV in (1, 3)]


@pytest.mark.parametrize("padding", br.PADDINGS)
@pytest.mark.parametrize("hw", [(2, 3), (5, 7)], ids=["2x3", "5x7"])
def test_stage_zlat_against_the_restatement(hw, padding, dev):
    from diner_amd import _lib
    h, w = hw
    worst = 0.0
    for i, (Cc, P, NV) in enumerate(STAGE_SHAPES):
        st = Stage(h, w, Cc, P, NV, dev, seed=100 + i)
        zl, taps = st.point_inputs(_lib.INDEX_PADDING[padding])
        zl, taps = zl.cpu().double().view(NV, P, Cc), taps.cpu().view(NV, P, 16)
        idx = taps[..., :8].contiguous().view(torch.int32)
        assert int(idx[..., :4].min()) >= 0 and int(idx[..., :4].max()) <= w - 1 and int(idx[..., 4:].min()) >= 0 and int(idx[..., 4:].max()) <= h - 1
        for v in range(NV):
            ref = br.lookup(st.latent[v], st.u[v], st.v[v], padding, coord_dtype=torch.float32)
            worst = max(worst, float((zl[v] - ref).abs().max()))
    print(f"zlat {h}x{w} {padding}: max |kernel - restatement| {worst:.2e}")
    # same coordinate and same float32 weights on both sides (tests/bicubic_ref.py); what is left is the kernel's 16 contracted fp32 terms
    # on unit-scale texels.  (Against weights evaluated in float64 the same kernel measured 1.84e-06 on the 2x3 border case: ATen's
    # float32 Horner form of the outer weight is itself up to 1.1e-6 from the exact polynomial.)
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("padding", br.PADDINGS)
@pytest.mark.parametrize("hw", [(2, 3), (5, 7)], ids=["2x3", "5x7"])
def test_stage_scatter_against_autograd(hw, padding, dev):
    from diner_amd import _lib
    from diner_amd.renderer import _ptr, _stream
    h, w = hw
    shapes = STAGE_SHAPES + ([(72, 4099, 3)] if hw == (2, 3) else [])          # thousands of rows on a 2 x 3 map
    for i, (Cc, P, NV) in enumerate(shapes):
        st = Stage(h, w, Cc, P, NV, dev, seed=200 + i)
        _, taps = st.point_inputs(_lib.INDEX_PADDING[padding])
        g = torch.Generator().manual_seed(300 + i)
        dz = torch.randn((NV * P, Cc), generator=g)
        d_lat = torch.zeros((1, NV, h, w, Cc), device=dev)
        dz_d = dz.to(dev)
        rc = _lib.lib().diner_train_bicubic_scatter(_ptr(dz_d), _ptr(taps), P, Cc, h, w, NV, 0, _ptr(d_lat), _stream(dev))
        assert rc == 0, _lib.lib().diner_last_error()
        torch.cuda.synchronize()
        got = d_lat[0].permute(0, 3, 1, 2).cpu().double()                       # [NV, C, h, w]
        lat = st.latent.double().requires_grad_(True)
        grid = torch.stack([st.u.double(), st.v.double()], -1)[:, None]         # [NV, 1, P, 2]
        out = F.grid_sample(lat, grid, mode="bicubic", padding_mode=padding, align_corners=False)[:, :, 0].permute(0, 2, 1)   # [NV, P, C]
        (out * dz.double().view(NV, P, Cc)).sum().backward()
        ref = lat.grad
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        assert err <= 2e-4 * scale, (Cc, P, NV, err, scale)                     # tests/test_training.py's latent_grad tolerance


# ---- (iv) training ----------------------------------------------------------------------------------------------------------------
def _train_renderer(c, precision):
    r = c.renderer(precision, train_any_shape=True, train_f16x3_any_shape=precision == "f16x3")
    return r


@pytest.mark.parametrize("precision", PRECISIONS)
def test_training_gradients_match_reference_autograd(precision, dev):
    from oracle.gen_golden import grad_probe_indices, train_cotangents
    c = Case("bicubic_train", dev)
    gold, m = c.data, c.model()
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent = m.encoder.latent.clone().requires_grad_(True)
    r = _train_renderer(c, precision)
    out = r(m, T(c.rays, dev), want_weights=True, z_samples=T(gold["z_fill"], dev))
    assert (r.last_route, r.last_binding, r.effective_precision) == (TRAIN_ROUTE[precision], "ctypes", precision)
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), gold["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.fine.depth.detach().cpu().numpy(), gold["depth"], rtol=0, atol=1e-4)
    c_rgb, c_depth = train_cotangents(c.rays.shape[1], c.cfg["cseed"])
    ((out.fine.rgb * T(c_rgb, dev)).sum() + (out.fine.depth * T(c_depth, dev)).sum()).backward()
    gl, ref = m.encoder.latent.grad.cpu().numpy(), gold["latent_grad"]
    scale = np.abs(ref).max()
    print(f"bicubic_train {precision}: latent_grad max err {np.abs(gl - ref).max():.2e} of {scale:.2e}")
    assert np.abs(gl - ref).max() <= 2e-4 * scale, (np.abs(gl - ref).max(), scale)
    assert (ref != 0).mean() > 0.001
    for pname, p in m.mlp_fine.named_parameters():
        g = p.grad.cpu().numpy()
        norm = float(gold[f"g_norm/{pname}"])
        assert norm > 0, pname
        assert abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - norm) <= 1e-4 * norm, pname
        assert abs(g.astype(np.float64).sum() - float(gold[f"g_sum/{pname}"])) <= 2e-4 * norm * np.sqrt(g.size), pname
        idx = grad_probe_indices(g.shape)
        np.testing.assert_allclose(g.reshape(-1)[idx], gold[f"g_probe/{pname}"], rtol=0, atol=2e-4 * norm / np.sqrt(g.size) * 30 + 1e-7,
                                   err_msg=pname)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_camera_gradients_match_reference_autograd(precision, dev):
    from tools.gen_camgrad_golden import cotangents
    c = Case("bicubic_camgrad", dev)
    data, m = c.data, c.model()
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent = m.encoder.latent.detach().clone().requires_grad_(True)
    rays_t = T(c.rays, dev).requires_grad_(True)
    for k in ("poses", "focal", "c", "image_shape"):
        setattr(m, k, getattr(m, k).detach().clone().requires_grad_(True))
    m.encoder.depths = m.encoder.depths.detach().clone().requires_grad_(True)
    r = _train_renderer(c, precision)
    out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.last_route == TRAIN_ROUTE[precision]
    c_rgb, c_depth, _ = cotangents(c.cfg, c.rays.shape[1])
    ((out.fine.rgb * T(c_rgb, dev)).sum() + (out.fine.depth * T(c_depth, dev)).sum()).backward()
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), data["rgb"], rtol=0, atol=1e-4)
    leaves = dict(rays=rays_t, poses=m.poses, focal=m.focal, c=m.c, image_shape=m.image_shape, depths=m.encoder.depths)
    for k, t in leaves.items():
        ref = data[f"grad/{k}"]
        assert t.grad is not None, k
        g = t.grad.detach().cpu().numpy()
        assert g.shape == ref.shape, k
        scale = np.abs(ref).max()
        print(f"bicubic_camgrad {precision} {k}: max err {np.abs(g - ref).max():.2e} of {scale:.2e}")
        assert np.abs(g - ref).max() <= 2e-4 * scale + 1e-6, (k, np.abs(g - ref).max(), scale)    # tests/test_gpu_camera_grads.py's tolerance
    assert scale_nonzero(data)
    gl = m.encoder.latent.grad.detach().cpu().numpy().astype(np.float64)
    assert abs(np.sqrt((gl ** 2).sum()) - float(data["latent_grad_norm"])) <= 2e-4 * float(data["latent_grad_norm"])
    for pname, p in m.mlp_fine.named_parameters():
        g = p.grad.detach().cpu().numpy().astype(np.float64)
        norm = float(data[f"g_norm/{pname}"])
        assert abs(np.sqrt((g ** 2).sum()) - norm) <= 1e-4 * norm, pname


def scale_nonzero(data):
    """the lookup's gradient reaches the cameras: the reference's focal / c gradients are not zero"""
    return all(np.abs(data[f"grad/{k}"]).max() > 0 for k in ("rays", "poses", "focal", "c", "image_shape"))


def test_training_without_train_any_shape_raises(dev):
    c = Case("bicubic_train", dev)
    m = c.model()
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="train_any_shape"):
        c.renderer("fp32")(m, T(c.rays, dev), z_samples=T(c.data["z_fill"], dev))


def test_whole_frame_backward_equals_forward_of_gen_rays(dev):
    """render_image under autograd (the frame's backward in chunks of grad_chunk_rays) against forward(gen_rays(...)) under autograd"""
    from diner_amd import glue
    c = Case("bicubic_train", dev)
    m, sc = c.model(), c.scene
    params = list(m.mlp_fine.parameters())
    for p in params:
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    H = W = 16
    E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
    Kt = torch.tensor([[[0.6 * W, 0, W / 2], [0, 0.6 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
    zn, zf = torch.tensor([float(sc.near)], device=dev), torch.tensor([float(sc.far)], device=dev)
    r = _train_renderer(c, "fp32")
    r.grad_chunk_rays = 100                                              # 256 rays: two whole chunks and a part
    cot = torch.randn((1, 3, H, W), generator=torch.Generator().manual_seed(5)).to(dev)
    grads = []
    for use_image in (True, False):
        for t in params + [m.encoder.latent]:
            t.grad = None
        r.seed, r._calls = 3, 0
        if use_image:
            rgb = r.render_image(m, E, Kt, H, W, zn, zf)
        else:
            rgb = r(m, glue.gen_rays(E, Kt, W, H, zn, zf).view(1, H * W, 8)).fine.rgb.view(1, H, W, 3).permute(0, 3, 1, 2)
        assert rgb.grad_fn is not None
        (rgb * cot).sum().backward()
        grads.append((rgb.detach(), [t.grad.clone() for t in params + [m.encoder.latent]]))
    np.testing.assert_allclose(grads[0][0].cpu().numpy(), grads[1][0].cpu().numpy(), rtol=0, atol=1e-4)
    for a, b in zip(grads[0][1], grads[1][1]):
        scale = float(b.abs().max())
        assert scale > 0 and float((a - b).abs().max()) <= 1e-4 * scale + 1e-7       # fp32 sums in another order (chunks, atomics)
