"""GPU tests of the gradients to the target camera and of render_image under autograd:
(1) glue.gen_rays under autograd (diner_gen_rays_backward) against a float64 restatement of the reference's gen_rays;
(2) render_image under autograd: the no-grad frame bit for bit, and the gradients of forward(glue.gen_rays(...)) on the same samples,
    for SB = 1, 2 and both precisions, whatever the chunking of its backward;
(3) the reference's autograd through gen_rays -> composite (tools/gen_targetcam_golden.py fixtures);
(4) the peak memory of a whole-frame backward against one chunk run alone;
(5) in-place updates between forward and backward raise.

Tolerances: gradients compared with each other are held to 1e-5 of the tensor's largest entry (the weight-gradient GEMMs accumulate with
atomics, and a chunked backward sums in another order); against the reference the bound of tests/test_gpu_camera_grads.py."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _close(a, b, what, rel=1e-5):
    assert a is not None and b is not None, what
    assert a.shape == b.shape and a.dtype == b.dtype, what
    err, scale = (a.double() - b.double()).abs().max().item(), b.double().abs().max().item()
    assert err <= rel * scale + 1e-12, (what, err, scale)


# ---- (1) gen_rays --------------------------------------------------------------------------------------------------------------
def _cameras(B, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    E = torch.zeros(B, 4, 4, dtype=torch.float64)
    for b in range(B):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        E[b, :3, :3] = q
        E[b, :3, 3] = torch.randn(3, generator=g, dtype=torch.float64)
    E[:, 3, 3] = 1
    Kt = torch.zeros(B, 3, 3, dtype=torch.float64)
    Kt[:, 0, 0], Kt[:, 1, 1] = W * (0.8 + 0.4 * rnd(B)), H * (0.8 + 0.4 * rnd(B))
    Kt[:, 0, 2], Kt[:, 1, 2] = W * (0.4 + 0.2 * rnd(B)), H * (0.4 + 0.2 * rnd(B))
    Kt[:, 0, 1] = 0.3          # a skew entry gen_rays does not read: its gradient is exactly 0
    Kt[:, 2, 2] = 1
    zn = 0.5 + rnd(B)
    return [t.float().to(dev) for t in (E, Kt, zn, zn + 2)]


def _gen_rays_f64(E, Kt, W, H, zn, zf):
    """reference src/util/cam_geometry.py:36-79, restated"""
    B = E.shape[0]
    focal, c = Kt[:, [0, 1], [0, 1]], Kt[:, [0, 1], [-1, -1]]
    ys, xs = torch.meshgrid(torch.arange(0.5, H, 1, dtype=E.dtype, device=E.device), torch.arange(0.5, W, 1, dtype=E.dtype, device=E.device),
                            indexing="ij")
    p = (torch.stack([xs, ys], -1)[None] - c.view(B, 1, 1, 2)) / focal.view(B, 1, 1, 2)
    p = torch.cat([p, torch.ones_like(p[..., :1])], -1)
    d = p / p.pow(2).sum(-1, keepdim=True).sqrt()
    R = E[:, :3, :3].transpose(1, 2)
    dw = (R @ d.reshape(B, -1, 3).transpose(1, 2)).transpose(1, 2).reshape(B, H, W, 3)
    o = (-R @ E[:, :3, 3:]).view(B, 1, 1, 3).expand(-1, H, W, -1)
    return torch.cat([o, dw, zn.view(B, 1, 1, 1).expand(-1, H, W, 1), zf.view(B, 1, 1, 1).expand(-1, H, W, 1)], -1)


def test_gen_rays_backward_matches_float64_autograd(dev):
    from diner_amd import glue
    B, H, W = 3, 37, 53
    cams = _cameras(B, H, W, dev)
    with torch.no_grad():
        plain = glue.gen_rays(cams[0], cams[1], W, H, cams[2], cams[3])
    leaves = [t.clone().requires_grad_(True) for t in cams]
    rays = glue.gen_rays(leaves[0], leaves[1], W, H, leaves[2], leaves[3])
    assert rays.requires_grad and torch.equal(rays.detach(), plain)
    cot = torch.randn(rays.shape, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    grads = torch.autograd.grad(rays, leaves, cot)
    l64 = [t.detach().double().requires_grad_(True) for t in cams]
    ref = torch.autograd.grad(_gen_rays_f64(l64[0], l64[1], W, H, l64[2], l64[3]), l64, cot.double())
    for name, g, r in zip(("extrinsics", "intrinsics", "z_near", "z_far"), grads, ref):
        assert g.dtype == torch.float32 and g.shape == r.shape, name
        err, scale = (g.double() - r).abs().max().item(), r.abs().max().item()
        assert err <= 1e-5 * scale, (name, err, scale)
    assert (grads[0][:, 3, :] == 0).all()
    used = torch.zeros(3, 3, dtype=torch.bool, device=dev)
    used[0, 0] = used[1, 1] = used[0, 2] = used[1, 2] = True
    assert (grads[1][:, ~used] == 0).all() and (grads[1][:, used] != 0).all()
    again = torch.autograd.grad(glue.gen_rays(leaves[0], leaves[1], W, H, leaves[2], leaves[3]), leaves, cot)
    for a, b in zip(grads, again):
        assert torch.equal(a, b)                     # fixed-order sums: bitwise reproducible


def test_gen_rays_gradient_dtypes_shapes_and_scalar_near_far(dev):
    from diner_amd import glue
    B, H, W = 2, 8, 12
    E, Kt, _, _ = _cameras(B, H, W, dev, seed=1)
    E64 = E.double().requires_grad_(True)
    zf = torch.tensor(3.0, device=dev, requires_grad=True)
    rays = glue.gen_rays(E64, Kt, W, H, 0.5, zf)       # z_near a Python float, z_far a 0-d tensor
    with torch.no_grad():
        plain = glue.gen_rays(E, Kt, W, H, torch.full((B,), 0.5, device=dev), torch.full((B,), 3.0, device=dev))
    assert torch.equal(rays.detach(), plain)
    rays.sum().backward()
    assert E64.grad.dtype == torch.float64 and E64.grad.shape == E64.shape
    assert zf.grad.shape == () and float(zf.grad) == B * H * W


# ---- (2) render_image under autograd against forward(gen_rays(...)) ---------------------------------------------------------
def _model(dev, SB):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(24, 32, 3, seed=5, feature_padding=4)
    m = model_from_scene(sc, synth.make_mlp_weights(6, bias_scale=0.1), device=dev)
    enc = m.encoder
    if SB > 1:
        cat = lambda t: torch.cat([t] * SB).contiguous()
        m.poses, m.focal, m.c = cat(m.poses), cat(m.focal), cat(m.c)
        enc.latent, enc.depths, enc.depths_std, enc.normals = cat(enc.latent), cat(enc.depths), cat(enc.depths_std), cat(enc.normals)
        enc.nobjects = SB
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    enc.latent.requires_grad_(True)
    return sc, m


def _targets(sc, SB, H, W, dev):
    from synthetic import synth
    E = T(np.stack([synth.look_at_origin_w2c(0.1 - 0.25 * i, sc.meta["cam_radius"]) for i in range(SB)]), dev)
    Kt = torch.tensor([[1.2 * W, 0, W / 2 + 0.7], [0, 1.1 * W, H / 2 - 0.4], [0, 0, 1]], dtype=torch.float32, device=dev).repeat(SB, 1, 1)
    return E, Kt, torch.full((SB,), float(sc.near), device=dev), torch.full((SB,), float(sc.far), device=dev)


def _grads_of(r, m, SB, H, W, cams, use_image, chunk=None):
    from diner_amd import glue
    E, Kt, zn, zf = cams
    leaves = [t.clone().requires_grad_(True) for t in (E, Kt, zf)]
    params = list(m.mlp_fine.parameters())
    for t in params + [m.encoder.latent]:
        t.grad = None
    if chunk is not None:
        r.grad_chunk_rays = chunk
    r.seed, r._calls = 3, 0
    if use_image:
        rgb, depth = r.render_image(m, leaves[0], leaves[1], H, W, zn, leaves[2], return_depth=True)
    else:
        out = r(m, glue.gen_rays(leaves[0], leaves[1], W, H, zn, leaves[2]).view(SB, H * W, 8)).fine
        rgb, depth = out.rgb.view(SB, H, W, 3).permute(0, 3, 1, 2), out.depth.view(SB, H, W, 1).permute(0, 3, 1, 2)
    g = torch.Generator(device=rgb.device).manual_seed(11)
    c_rgb = torch.randn(rgb.shape, generator=g, device=rgb.device)
    c_depth = torch.randn(depth.shape, generator=g, device=rgb.device)
    ((rgb * c_rgb).sum() + (depth * c_depth).sum()).backward()
    names = ["extrinsics", "intrinsics", "z_far", "latent"] + [n for n, _ in m.mlp_fine.named_parameters()]
    return rgb.detach(), depth.detach(), dict(zip(names, [t.grad for t in leaves] + [m.encoder.latent.grad] + [p.grad for p in params]))


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("SB", [1, 2])
def test_render_image_under_autograd_equals_forward_of_gen_rays(precision, SB, dev):
    from diner_amd import NeRFRendererDGS
    H, W = 20, 28
    sc, m = _model(dev, SB)
    cams = _targets(sc, SB, H, W, dev)
    r = NeRFRendererDGS(n_samples=16, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd)
    r.precision = precision
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        rgb0, depth0 = r.render_image(m, *cams[:2], H, W, *cams[2:], return_depth=True)
    rgb, depth, g_img = _grads_of(r, m, SB, H, W, cams, True)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)       # the inference frame, bit for bit
    _, _, g_fwd = _grads_of(r, m, SB, H, W, cams, False)
    for k in g_fwd:
        _close(g_img[k], g_fwd[k], k)
    assert (g_img["extrinsics"][:, 3] == 0).all() and g_img["intrinsics"][:, 0, 1].eq(0).all()


def test_chunked_backward_equals_one_chunk(dev):
    from diner_amd import NeRFRendererDGS
    H, W = 20, 28
    sc, m = _model(dev, 1)
    cams = _targets(sc, 1, H, W, dev)
    r = NeRFRendererDGS(n_samples=16, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd)
    r.precision = "fp32"
    _, _, whole = _grads_of(r, m, 1, H, W, cams, True, chunk=H * W)
    _, _, chunked = _grads_of(r, m, 1, H, W, cams, True, chunk=97)   # 97 divides nothing here
    for k in whole:
        _close(chunked[k], whole[k], k)


# ---- (3) against the reference's autograd ------------------------------------------------------------------------------------
FIXTURES = [("targetcam_facescape", "fp32"), ("targetcam_facescape", "f16x3"), ("targetcam_dtu", "fp32"), ("targetcam_dtu", "f16x3"),
            ("targetcam_zeros", "fp32"), ("targetcam_zeros", "f16x3"), ("targetcam_gen_h128", "fp32")]


@pytest.mark.parametrize("name,precision", FIXTURES)
def test_target_camera_gradients_match_reference_autograd(name, precision, dev):
    from diner_amd import NeRFRendererDGS, glue
    from synthetic.model_stub import model_from_scene
    from tools.gen_targetcam_golden import case_inputs, cotangents, input_digests, model_kwargs
    data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
    cfg = json.loads(str(data["config"]))
    sc, w, cam, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, cam, noise)
    m = model_from_scene(sc, w, device=dev, **model_kwargs(cfg))
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    H, W, NR = cam["H"], cam["W"], cam["H"] * cam["W"]
    E, Kt, zf = [T(cam[k], dev).requires_grad_(True) for k in ("E", "K", "far")]
    rays = glue.gen_rays(E, Kt, W, H, T(cam["near"], dev), zf).view(1, NR, 8)
    r = NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"], white_bkgd=sc.white_bkgd, train_any_shape=True)
    r.precision = precision
    out = r(m, rays, want_weights=True, z_samples=T(data["z_fill"], dev)).fine
    c_rgb, c_depth, c_w = cotangents(cfg, NR)
    loss = (out.rgb * T(c_rgb, dev)).sum() + (out.depth * T(c_depth, dev)).sum()
    if c_w is not None:
        loss = loss + (out.weights * T(c_w, dev)).sum()
    loss.backward()
    np.testing.assert_allclose(out.rgb.detach().cpu().numpy(), data["rgb"], rtol=0, atol=1e-4)
    for k, t in (("extrinsics", E), ("intrinsics", Kt), ("z_far", zf)):
        ref, g = data[f"grad/{k}"], t.grad.detach().cpu().numpy()
        scale = np.abs(ref).max()
        assert g.shape == ref.shape and np.abs(g - ref).max() <= 2e-4 * scale + 1e-6, (k, np.abs(g - ref).max(), scale)
    gl = m.encoder.latent.grad.detach().cpu().numpy().astype(np.float64)
    assert abs(np.sqrt((gl ** 2).sum()) - float(data["latent_grad_norm"])) <= 1e-4 * float(data["latent_grad_norm"])
    for pname, p in m.mlp_fine.named_parameters():
        norm = float(data[f"g_norm/{pname}"])
        assert abs(np.sqrt((p.grad.detach().cpu().numpy().astype(np.float64) ** 2).sum()) - norm) <= 1e-4 * norm, pname


# ---- (4) memory ---------------------------------------------------------------------------------------------------------------
def test_whole_frame_backward_peak_memory_is_one_chunk_plus_saved_tensors(dev):
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    H = W = 256
    K, NV = 40, 2
    sc = synth.make_scene(H, W, NV, seed=0, with_latent=False)
    h, w = sc.latent_hw
    latent = torch.randn((1, NV, 512, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    m = model_from_scene(sc, synth.make_mlp_weights(1, bias_scale=0.1), device=dev, latent=latent)
    params = list(m.mlp_fine.parameters())
    for p in params:
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=1000, n_gaussian=15, white_bkgd=sc.white_bkgd)
    E = T(sc.target_extrinsics, dev)[None]
    Kt = T(sc.target_intrinsics, dev)[None]
    zn, zf = torch.tensor([sc.near], device=dev), torch.tensor([sc.far], device=dev)
    with torch.no_grad():
        r.render_image(m, E, Kt, H, W, zn, zf)            # the packs (maps, latent, lin_z maps, MLP) are resident from here on

    def measure(fn):
        for t in params + [m.encoder.latent]:
            t.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def frame():
        r.render_image(m, E, Kt, H, W, zn, zf).sum().backward()

    NR, chunk = H * W, int(r.grad_chunk_rays)
    with torch.no_grad():
        rays = glue.gen_rays(E, Kt, W, H, zn, zf).view(1, NR, 8)[:, :chunk].contiguous()
        z = torch.sort(zn + (zf - zn) * torch.rand((1, chunk, K), device=dev), dim=-1).values

    def one_chunk():
        r(m, rays, z_samples=z).fine.rgb.sum().backward()

    peak_frame, peak_chunk = measure(frame), measure(one_chunk)
    saved = NR * (8 + K + 3 + 1) * 4                      # rays, samples, rgb, depth
    assert peak_frame <= saved + 2 * peak_chunk, (peak_frame, saved, peak_chunk)


# ---- (5) in-place updates -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["target_extrinsics", "mlp_weight"])
def test_in_place_update_between_forward_and_backward_raises(what, dev):
    from diner_amd import NeRFRendererDGS
    H, W = 12, 16
    sc, m = _model(dev, 1)
    E, Kt, zn, zf = _targets(sc, 1, H, W, dev)
    E = E.clone().requires_grad_(True)
    r = NeRFRendererDGS(n_samples=16, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd)
    loss = r.render_image(m, E, Kt, H, W, zn, zf).sum()
    with torch.no_grad():
        (E if what == "target_extrinsics" else m.mlp_fine.lin_out.weight).mul_(1.0)     # an optimizer step
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()
