"""GPU tests of the training path's gradients to the geometric leaves -- rays, model.poses / focal / c / image_shape and
encoder.depths -- against the reference's autograd (tools/gen_camgrad_golden.py fixtures) in both precisions, plus identities that
hold independently of any fixture: the render is invariant under a shift of the world and under a common scale of focal, c and
image_shape.  Also: camera-only training takes the training route, an SB = 2 batch equals its scenes rendered alone, and an in-place
update of a camera tensor between forward and backward raises."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NAMES = ["camgrad_facescape", "camgrad_dtu", "camgrad_zeros", "camgrad_reflection", "camgrad_nearest"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _setup(name, dev):
    from synthetic.model_stub import model_from_scene
    from tools.gen_camgrad_golden import case_inputs, input_digests, model_kwargs
    data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
    cfg = json.loads(str(data["config"]))
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    m = model_from_scene(sc, w, device=dev, **model_kwargs(cfg))
    return data, cfg, sc, m, rays


def _renderer(cfg, sc, precision):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"], white_bkgd=sc.white_bkgd)
    r.precision = precision
    return r


def _leaves(m, rays_t):
    return dict(rays=rays_t, poses=m.poses, focal=m.focal, c=m.c, image_shape=m.image_shape, depths=m.encoder.depths)


def _require(m, rays, dev, mlp=True, cams=("rays", "poses", "focal", "c", "image_shape", "depths")):
    for p in m.mlp_fine.parameters():
        p.requires_grad_(mlp)
    m.encoder.latent = m.encoder.latent.detach().clone().requires_grad_(mlp)
    rays_t = T(rays, dev).requires_grad_("rays" in cams)
    for k in ("poses", "focal", "c", "image_shape"):
        setattr(m, k, getattr(m, k).detach().clone().requires_grad_(k in cams))
    m.encoder.depths = m.encoder.depths.detach().clone().requires_grad_("depths" in cams)
    return rays_t


def _loss(out, cfg, NR, dev):
    from tools.gen_camgrad_golden import cotangents
    c_rgb, c_depth, c_w = cotangents(cfg, NR)
    loss = (out.fine.rgb * T(c_rgb, dev)).sum() + (out.fine.depth * T(c_depth, dev)).sum()
    if c_w is not None:
        loss = loss + (out.fine.weights * T(c_w, dev)).sum()
    return loss


def _run(name, dev, precision="fp32", mlp=True, cams=("rays", "poses", "focal", "c", "image_shape", "depths")):
    data, cfg, sc, m, rays = _setup(name, dev)
    rays_t = _require(m, rays, dev, mlp=mlp, cams=cams)
    r = _renderer(cfg, sc, precision)
    out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    _loss(out, cfg, rays.shape[1], dev).backward()
    return data, cfg, m, rays_t, out


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", NAMES)
def test_camera_gradients_match_reference_autograd(name, precision, dev):
    data, cfg, m, rays_t, out = _run(name, dev, precision)
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), data["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.fine.depth.detach().cpu().numpy(), data["depth"], rtol=0, atol=1e-4)
    for k, t in _leaves(m, rays_t).items():
        ref = data[f"grad/{k}"]
        assert t.grad is not None, k
        g = t.grad.detach().cpu().numpy()
        assert g.shape == ref.shape and t.grad.dtype == t.dtype and t.grad.device == t.device, k
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= 2e-4 * scale + 1e-6, (k, np.abs(g - ref).max(), scale)
    assert (rays_t.grad[..., 6] == 0).all()
    assert (m.poses.grad[..., 3, :] == 0).all()
    assert m.encoder.depths_std.grad is None and m.encoder.normals.grad is None
    # the MLP / latent gradients are unchanged by the camera leaves
    gl = m.encoder.latent.grad.detach().cpu().numpy().astype(np.float64)
    assert abs(np.sqrt((gl ** 2).sum()) - float(data["latent_grad_norm"])) <= 2e-4 * float(data["latent_grad_norm"])
    for pname, p in m.mlp_fine.named_parameters():
        g = p.grad.detach().cpu().numpy().astype(np.float64)
        norm = float(data[f"g_norm/{pname}"])
        assert abs(np.sqrt((g ** 2).sum()) - norm) <= 1e-4 * norm, pname


@pytest.mark.parametrize("name", ["camgrad_facescape", "camgrad_zeros"])
def test_world_shift_and_intrinsics_scale_identities(name, dev):
    _, _, m, rays_t, _ = _run(name, dev)
    d_o = rays_t.grad[0, :, 0:3].double().sum(0)
    R = m.poses.detach()[0, :, :3, :3].double()
    d_t = m.poses.grad[0, :, :3, 3].double()
    rt = torch.einsum("vij,vi->j", R, d_t)
    mag = rays_t.grad[0, :, 0:3].double().abs().sum() + torch.einsum("vij,vi->vj", R, d_t).abs().sum()
    assert (d_o - rt).abs().max() <= 1e-4 * mag, (d_o, rt, mag)
    f, c, s = m.focal.detach().double(), m.c.detach().double(), m.image_shape.detach().double()
    terms = [f * m.focal.grad.double(), c * m.c.grad.double(), s * m.image_shape.grad.double()]
    tot = sum(t.sum() for t in terms)
    mag = sum(t.abs().sum() for t in terms)
    assert mag > 0
    assert tot.abs() <= 1e-4 * mag, (tot, mag)


def test_camera_only_training_takes_the_training_route(dev):
    _, _, m_full, _, _ = _run("camgrad_facescape", dev)
    _, _, m, rays_t, out = _run("camgrad_facescape", dev, mlp=False, cams=("poses",))
    assert out.fine.rgb.grad_fn is not None
    assert rays_t.grad is None and m.focal.grad is None and m.encoder.latent.grad is None
    assert all(p.grad is None for p in m.mlp_fine.parameters())
    torch.testing.assert_close(m.poses.grad, m_full.poses.grad, rtol=1e-6, atol=1e-6)


def test_batch_of_two_equals_the_scenes_alone(dev):
    data, cfg, sc, m, rays = _setup("camgrad_dtu", dev)
    z = data["z_fill"]
    rays_b, z_b = rays[:, ::-1].copy(), z[:, ::-1].copy()
    single = []
    for rr, zz in ((rays, z), (rays_b, z_b)):
        _, _, _, m1, _ = _setup("camgrad_dtu", dev)
        rt = _require(m1, rr, dev, mlp=False)
        out = _renderer(cfg, sc, "fp32")(m1, rt, want_weights=True, z_samples=T(zz, dev))
        _loss(out, cfg, rr.shape[1], dev).backward()
        single.append((rt.grad, m1.poses.grad, m1.focal.grad, m1.c.grad, m1.encoder.depths.grad))
    enc = m.encoder
    cat = lambda t: torch.cat([t, t]).contiguous()
    m.poses, m.focal, m.c = cat(m.poses), cat(m.focal), cat(m.c)
    enc.latent, enc.depths, enc.depths_std, enc.normals = cat(enc.latent), cat(enc.depths), cat(enc.depths_std), cat(enc.normals)
    enc.nobjects = 2
    rays2 = np.concatenate([rays, rays_b])
    rt = _require(m, rays2, dev, mlp=False)
    out = _renderer(cfg, sc, "fp32")(m, rt, want_weights=True, z_samples=T(np.concatenate([z, z_b]), dev))
    from tools.gen_camgrad_golden import cotangents
    c_rgb, c_depth, c_w = cotangents(cfg, rays.shape[1])
    ct = lambda a: T(np.concatenate([a, a]), dev)
    loss = (out.fine.rgb * ct(c_rgb)).sum() + (out.fine.depth * ct(c_depth)).sum() + (out.fine.weights * ct(c_w)).sum()
    loss.backward()
    for sb in range(2):
        g_rays, g_poses, g_focal, g_c, g_depths = single[sb]
        torch.testing.assert_close(rt.grad[sb:sb + 1], g_rays, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.poses.grad[sb:sb + 1], g_poses, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.focal.grad[sb:sb + 1], g_focal, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.c.grad[sb:sb + 1], g_c, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.encoder.depths.grad[sb:sb + 1], g_depths, rtol=1e-5, atol=1e-5)


def test_in_place_update_of_poses_between_forward_and_backward_raises(dev):
    data, cfg, sc, m, rays = _setup("camgrad_facescape", dev)
    rays_t = _require(m, rays, dev, mlp=False, cams=("poses",))
    out = _renderer(cfg, sc, "fp32")(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    loss = _loss(out, cfg, rays.shape[1], dev)
    with torch.no_grad():
        m.poses.add_(0.0)          # an optimizer step on the pose
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()
