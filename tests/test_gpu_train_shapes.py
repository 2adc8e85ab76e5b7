"""GPU tests of the shape-general training path (diner_amd/training_gen.py, renderer ``train_any_shape``): gradients of non-standard
fusion MLPs against the reference's own autograd (tools/gen_trainshape_golden.py fixtures), the standard shape forced through the new
path against the standard training fixtures, its forward against the shape-general inference route, and the contract of the standard
path (in-place updates raise, precision settles on fp32, a batch of two scenes equals the scenes alone, an optimizer lowers the loss).

Tolerances: those of tests/test_training.py and tests/test_gpu_camera_grads.py (exact fp32 GEMMs with another summation order than the
reference's and atomically accumulated weight gradients)."""
import json
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NAMES = ["trainshape_a_h128_nv2", "trainshape_b_h256_softplus_nv4", "trainshape_c_h96_f4_dtu", "trainshape_d_lat256_h64_nearest_zeros",
         "trainshape_e_defaults_nv1", "trainshape_f_combine0_nv3"]
LEAVES = ("rays", "poses", "focal", "c", "image_shape", "depths")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _setup(name, dev):
    from synthetic.model_stub import model_from_scene
    from tools.gen_trainshape_golden import case_inputs, input_digests, model_kwargs
    data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
    cfg = json.loads(str(data["config"]))
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    m = model_from_scene(sc, w, device=dev, **model_kwargs(cfg))
    return data, cfg, sc, m, rays


def _renderer(cfg, sc, precision="fp32", **kw):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"], white_bkgd=sc.white_bkgd, **kw)
    r.precision = precision
    return r


def _require(m, rays, dev, cams=()):
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent = m.encoder.latent.detach().clone().requires_grad_(True)
    rays_t = T(rays, dev).requires_grad_("rays" in cams)
    for k in ("poses", "focal", "c", "image_shape"):
        setattr(m, k, getattr(m, k).detach().clone().requires_grad_(k in cams))
    m.encoder.depths = m.encoder.depths.detach().clone().requires_grad_("depths" in cams)
    return rays_t


def _loss(out, cotangents, NR, dev, cfg):
    c_rgb, c_depth, c_w = cotangents(cfg, NR)
    loss = (out.fine.rgb * T(c_rgb, dev)).sum() + (out.fine.depth * T(c_depth, dev)).sum()
    if c_w is not None:
        loss = loss + (out.fine.weights * T(c_w, dev)).sum()
    return loss


def _check_params(m, data):
    from oracle.gen_golden import grad_probe_indices
    for pname, p in m.mlp_fine.named_parameters():
        g = p.grad.detach().cpu().numpy()
        norm = float(data[f"g_norm/{pname}"])
        assert abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - norm) <= 1e-4 * norm, (pname, np.sqrt((g.astype(np.float64) ** 2).sum()), norm)
        assert abs(g.astype(np.float64).sum() - float(data[f"g_sum/{pname}"])) <= 2e-4 * norm * np.sqrt(g.size), pname
        idx = grad_probe_indices(g.shape)
        np.testing.assert_allclose(g.reshape(-1)[idx], data[f"g_probe/{pname}"], rtol=0, atol=2e-4 * norm / np.sqrt(g.size) * 30 + 1e-7,
                                   err_msg=pname)


def _check_leaves(m, rays_t, data):
    for k, t in dict(rays=rays_t, poses=m.poses, focal=m.focal, c=m.c, image_shape=m.image_shape, depths=m.encoder.depths).items():
        ref = data[f"grad/{k}"]
        assert t.grad is not None, k
        g = t.grad.detach().cpu().numpy()
        assert g.shape == ref.shape, k
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= 2e-4 * scale + 1e-6, (k, np.abs(g - ref).max(), scale)


@pytest.mark.parametrize("name", NAMES)
def test_non_standard_training_matches_reference_autograd(name, dev):
    from tools.gen_trainshape_golden import cotangents, latent_probe_indices
    data, cfg, sc, m, rays = _setup(name, dev)
    cams = LEAVES if cfg["leaves"] else ()
    rays_t = _require(m, rays, dev, cams)
    r = _renderer(cfg, sc, train_any_shape=True)
    out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.last_route == "train_gen" and r.effective_precision == "fp32"
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), data["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.fine.depth.detach().cpu().numpy(), data["depth"], rtol=0, atol=1e-4)
    _loss(out, cotangents, rays.shape[1], dev, cfg).backward()
    gl = m.encoder.latent.grad.detach().cpu().numpy()
    lmax, lnorm = float(data["latent_grad_max"]), float(data["latent_grad_norm"])
    assert abs(np.sqrt((gl.astype(np.float64) ** 2).sum()) - lnorm) <= 1e-4 * lnorm + 1e-6
    assert abs(np.abs(gl).max() - lmax) <= 2e-4 * lmax + 1e-6
    np.testing.assert_allclose(gl.reshape(-1)[latent_probe_indices(gl.shape)], data["latent_grad_probe"], rtol=0, atol=2e-4 * lmax + 1e-6)
    if cfg["mlp"].get("combine_layer", 1000) == 0:
        assert (gl == 0).all()
    _check_params(m, data)
    if cfg["leaves"]:
        _check_leaves(m, rays_t, data)


@pytest.mark.parametrize("case", ["train", "train_dtu"])
def test_standard_shape_through_the_new_path_matches_train_fixtures(case, dev):
    from diner_amd import NeRFRendererDGS
    from oracle.gen_golden import TRAIN_CASES, case_inputs, train_cotangents, weights_cotangent
    from synthetic.model_stub import model_from_scene
    gold = dict(np.load(GOLDEN / f"{case}.npz", allow_pickle=False))
    cfg = json.loads(str(gold["config"]))
    assert cfg == TRAIN_CASES[case]
    sc, w, rays, _ = case_inputs(cfg)
    m = model_from_scene(sc, w, device=dev)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent = m.encoder.latent.clone().requires_grad_(True)
    r = NeRFRendererDGS(n_samples=cfg["K"], n_depth_candidates=cfg["NC"], n_gaussian=cfg["G"], white_bkgd=sc.white_bkgd)
    r.precision = "fp32"
    r._force_gen_train = True
    out = r(m, T(rays, dev), want_weights=True, z_samples=T(gold["z_fill"], dev))
    assert r.last_route == "train_gen"
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), gold["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.fine.depth.detach().cpu().numpy(), gold["depth"], rtol=0, atol=1e-4)
    c_rgb, c_depth = train_cotangents(rays.shape[1], cfg["cseed"])
    loss = (out.fine.rgb * T(c_rgb, dev)).sum() + (out.fine.depth * T(c_depth, dev)).sum()
    if cfg.get("weights_cotangent"):
        loss = loss + (out.fine.weights * T(weights_cotangent(rays.shape[1], cfg["K"], cfg["cseed"]), dev)).sum()
    loss.backward()
    gl = m.encoder.latent.grad.cpu().numpy()
    ref = gold["latent_grad"]
    assert np.abs(gl - ref).max() <= 2e-4 * np.abs(ref).max(), (np.abs(gl - ref).max(), np.abs(ref).max())
    _check_params(m, gold)


def test_standard_shape_through_the_new_path_matches_camgrad_dtu(dev):
    from tools.gen_camgrad_golden import case_inputs, cotangents, input_digests, model_kwargs
    from synthetic.model_stub import model_from_scene
    data = dict(np.load(GOLDEN / "camgrad_dtu.npz", allow_pickle=False))
    cfg = json.loads(str(data["config"]))
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    m = model_from_scene(sc, w, device=dev, **model_kwargs(cfg))
    rays_t = _require(m, rays, dev, LEAVES)
    r = _renderer(cfg, sc)
    r._force_gen_train = True
    out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.last_route == "train_gen"
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), data["rgb"], rtol=0, atol=1e-4)
    _loss(out, cotangents, rays.shape[1], dev, cfg).backward()
    _check_leaves(m, rays_t, data)
    gl = m.encoder.latent.grad.detach().cpu().numpy().astype(np.float64)
    assert abs(np.sqrt((gl ** 2).sum()) - float(data["latent_grad_norm"])) <= 2e-4 * float(data["latent_grad_norm"])
    for pname, p in m.mlp_fine.named_parameters():
        g = p.grad.detach().cpu().numpy().astype(np.float64)
        norm = float(data[f"g_norm/{pname}"])
        assert abs(np.sqrt((g ** 2).sum()) - norm) <= 1e-4 * norm, pname


@pytest.mark.parametrize("name", ["trainshape_b_h256_softplus_nv4", "trainshape_d_lat256_h64_nearest_zeros", "trainshape_e_defaults_nv1"])
def test_forward_equals_the_shape_general_inference_route(name, dev):
    data, cfg, sc, m, rays = _setup(name, dev)
    z = T(data["z_fill"], dev)
    r = _renderer(cfg, sc)
    with torch.no_grad():
        ref = r(m, T(rays, dev), want_weights=True, z_samples=z)
    assert r.last_route == "points_mlp_gen"
    rays_t = _require(m, rays, dev)
    r2 = _renderer(cfg, sc, train_any_shape=True)
    out = r2(m, rays_t, want_weights=True, z_samples=z)
    assert r2.last_route == "train_gen"
    for k in ("rgb", "depth", "weights"):
        torch.testing.assert_close(out.fine[k].detach(), ref.fine[k], rtol=0, atol=2e-5)
    # composite() takes the same route
    w_, rgb, depth = r2.composite(m, rays_t, z)
    assert r2.last_route == "train_gen" and rgb.grad_fn is not None
    torch.testing.assert_close(rgb.detach(), ref.fine.rgb, rtol=0, atol=2e-5)


def test_in_place_update_between_forward_and_backward_raises(dev):
    from tools.gen_trainshape_golden import cotangents
    data, cfg, sc, m, rays = _setup("trainshape_a_h128_nv2", dev)
    rays_t = _require(m, rays, dev)
    out = _renderer(cfg, sc, train_any_shape=True)(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    loss = _loss(out, cotangents, rays.shape[1], dev, cfg)
    with torch.no_grad():
        m.mlp_fine.blocks[2].fc_0.weight.add_(0.0)   # an optimizer step between forward and backward
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()


def test_f16x3_precision_warns_and_runs_in_fp32(dev):
    from tools.gen_trainshape_golden import cotangents
    data, cfg, sc, m, rays = _setup("trainshape_a_h128_nv2", dev)
    rays_t = _require(m, rays, dev)
    r = _renderer(cfg, sc, precision="f16x3", train_any_shape=True)
    with pytest.warns(UserWarning, match="precision="):
        out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.effective_precision == "fp32" and r.precision == "f16x3"
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), data["rgb"], rtol=0, atol=1e-4)
    _loss(out, cotangents, rays.shape[1], dev, cfg).backward()
    _check_params(m, data)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))   # once only


def test_batch_of_two_equals_the_scenes_alone(dev):
    from tools.gen_trainshape_golden import cotangents
    name = "trainshape_c_h96_f4_dtu"
    data, cfg, sc, m, rays = _setup(name, dev)
    z = data["z_fill"]
    rays_b, z_b = rays[:, ::-1].copy(), z[:, ::-1].copy()
    single = []
    for rr, zz in ((rays, z), (rays_b, z_b)):
        _, _, _, m1, _ = _setup(name, dev)
        rt = _require(m1, rr, dev, LEAVES)
        out = _renderer(cfg, sc, train_any_shape=True)(m1, rt, want_weights=True, z_samples=T(zz, dev))
        _loss(out, cotangents, rr.shape[1], dev, cfg).backward()
        single.append(dict(rays=rt.grad, poses=m1.poses.grad, focal=m1.focal.grad, c=m1.c.grad, depths=m1.encoder.depths.grad,
                           latent=m1.encoder.latent.grad, params={k: p.grad for k, p in m1.mlp_fine.named_parameters()}))
    enc = m.encoder
    cat = lambda t: torch.cat([t, t]).contiguous()
    m.poses, m.focal, m.c = cat(m.poses), cat(m.focal), cat(m.c)
    enc.latent, enc.depths, enc.depths_std, enc.normals = cat(enc.latent), cat(enc.depths), cat(enc.depths_std), cat(enc.normals)
    enc.nobjects = 2
    rt = _require(m, np.concatenate([rays, rays_b]), dev, LEAVES)
    out = _renderer(cfg, sc, train_any_shape=True)(m, rt, want_weights=True, z_samples=T(np.concatenate([z, z_b]), dev))
    c_rgb, c_depth, c_w = cotangents(cfg, rays.shape[1])
    ct = lambda a: T(np.concatenate([a, a]), dev)
    loss = (out.fine.rgb * ct(c_rgb)).sum() + (out.fine.depth * ct(c_depth)).sum()
    if c_w is not None:
        loss = loss + (out.fine.weights * ct(c_w)).sum()
    loss.backward()
    for sb in range(2):
        s = single[sb]
        torch.testing.assert_close(rt.grad[sb:sb + 1], s["rays"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.poses.grad[sb:sb + 1], s["poses"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.focal.grad[sb:sb + 1], s["focal"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.c.grad[sb:sb + 1], s["c"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.encoder.depths.grad[sb:sb + 1], s["depths"], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.encoder.latent.grad[sb:sb + 1], s["latent"], rtol=1e-5, atol=1e-5)
    for k, p in m.mlp_fine.named_parameters():   # parameter gradients add up over the batch
        torch.testing.assert_close(p.grad, single[0]["params"][k] + single[1]["params"][k], rtol=1e-4, atol=1e-5)


def test_three_adam_steps_lower_the_loss(dev):
    data, cfg, sc, m, rays = _setup("trainshape_b_h256_softplus_nv4", dev)
    rays_t = _require(m, rays, dev)
    r = _renderer(cfg, sc, train_any_shape=True)
    target = torch.full((1, rays.shape[1], 3), 0.5, device=dev)
    opt = torch.optim.Adam(list(m.mlp_fine.parameters()) + [m.encoder.latent], lr=1e-4)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        out = r(m, rays_t, z_samples=T(data["z_fill"], dev))
        loss = ((out.fine.rgb - target) ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 4:
            break
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.mlp_fine.parameters())
        assert torch.isfinite(m.encoder.latent.grad).all()
        opt.step()
    assert losses[-1] < losses[0], losses
