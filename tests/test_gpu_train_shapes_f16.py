"""GPU tests of the shape-general training path in f16x3 (diner_amd/csrc/train_gen_f16.hip, renderer ``train_f16x3_any_shape`` together
with ``train_any_shape`` and precision "f16x3"): gradients of non-standard fusion MLPs against the reference's own autograd (the
``trainshape_*`` fixtures), the standard shape forced through the path against the standard training fixtures, its forward against the
fp32 shape-general training forward, the GEMM itself against float64 next to the fp32 kernel, and the contract of the fp32 path (in-place
updates raise, a batch of two scenes equals the scenes alone, an optimizer lowers the loss, the switch off is the fp32 path).

Tolerances: those of tests/test_gpu_train_shapes.py (helpers copied), which the standard path meets in f16x3 in tests/test_training.py."""
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
    r = _renderer(cfg, sc, precision="f16x3", train_any_shape=True, train_f16x3_any_shape=True)
    out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.last_route == "train_gen_f16" and r.effective_precision == "f16x3"
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
    r.precision, r.train_f16x3_any_shape = "f16x3", True
    r._force_gen_train = True
    out = r(m, T(rays, dev), want_weights=True, z_samples=T(gold["z_fill"], dev))
    assert r.last_route == "train_gen_f16" and r.effective_precision == "f16x3"
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
    r = _renderer(cfg, sc, precision="f16x3", train_f16x3_any_shape=True)
    r._force_gen_train = True
    out = r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.last_route == "train_gen_f16" and r.effective_precision == "f16x3"
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
def test_forward_equals_the_fp32_training_forward(name, dev):
    data, cfg, sc, m, rays = _setup(name, dev)
    z = T(data["z_fill"], dev)
    rays_t = _require(m, rays, dev)
    r = _renderer(cfg, sc, train_any_shape=True)
    ref = r(m, rays_t, want_weights=True, z_samples=z)
    assert r.last_route == "train_gen"
    r2 = _renderer(cfg, sc, precision="f16x3", train_any_shape=True, train_f16x3_any_shape=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no precision warning on this route
        out = r2(m, rays_t, want_weights=True, z_samples=z)
    assert r2.last_route == "train_gen_f16" and r2.effective_precision == "f16x3"
    for k in ("rgb", "depth", "weights"):
        print(name, k, "max |f16x3 - fp32| =", float((out.fine[k].detach() - ref.fine[k].detach()).abs().max()))
    for k in ("rgb", "depth", "weights"):
        torch.testing.assert_close(out.fine[k].detach(), ref.fine[k].detach(), rtol=0, atol=2e-5)
    # composite() takes the same route
    w_, rgb, depth = r2.composite(m, rays_t, z)
    assert r2.last_route == "train_gen_f16" and rgb.grad_fn is not None
    torch.testing.assert_close(rgb.detach(), ref.fine.rgb.detach(), rtol=0, atol=2e-5)


def test_in_place_update_between_forward_and_backward_raises(dev):
    from tools.gen_trainshape_golden import cotangents
    data, cfg, sc, m, rays = _setup("trainshape_a_h128_nv2", dev)
    rays_t = _require(m, rays, dev)
    out = _renderer(cfg, sc, precision="f16x3", train_any_shape=True, train_f16x3_any_shape=True)(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    loss = _loss(out, cotangents, rays.shape[1], dev, cfg)
    with torch.no_grad():
        m.mlp_fine.blocks[2].fc_0.weight.add_(0.0)   # an optimizer step between forward and backward
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()


def test_switch_off_is_the_fp32_path_with_its_warning(dev):
    data, cfg, sc, m, rays = _setup("trainshape_a_h128_nv2", dev)
    rays_t = _require(m, rays, dev)
    for kw in (dict(train_any_shape=True), dict(train_any_shape=True, f16x3_any_shape=True)):
        r = _renderer(cfg, sc, precision="f16x3", **kw)
        assert r.train_f16x3_any_shape is False
        with pytest.warns(UserWarning, match="precision="):
            r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
        assert r.last_route == "train_gen" and r.effective_precision == "fp32"
    r = _renderer(cfg, sc, precision="fp32", train_any_shape=True, train_f16x3_any_shape=True)   # fp32 asked for: fp32 runs, silently
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r(m, rays_t, want_weights=True, z_samples=T(data["z_fill"], dev))
    assert r.last_route == "train_gen" and r.effective_precision == "fp32"


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
        out = _renderer(cfg, sc, precision="f16x3", train_any_shape=True, train_f16x3_any_shape=True)(m1, rt, want_weights=True, z_samples=T(zz, dev))
        _loss(out, cotangents, rr.shape[1], dev, cfg).backward()
        single.append(dict(rays=rt.grad, poses=m1.poses.grad, focal=m1.focal.grad, c=m1.c.grad, depths=m1.encoder.depths.grad,
                           latent=m1.encoder.latent.grad, params={k: p.grad for k, p in m1.mlp_fine.named_parameters()}))
    enc = m.encoder
    cat = lambda t: torch.cat([t, t]).contiguous()
    m.poses, m.focal, m.c = cat(m.poses), cat(m.focal), cat(m.c)
    enc.latent, enc.depths, enc.depths_std, enc.normals = cat(enc.latent), cat(enc.depths), cat(enc.depths_std), cat(enc.normals)
    enc.nobjects = 2
    rt = _require(m, np.concatenate([rays, rays_b]), dev, LEAVES)
    out = _renderer(cfg, sc, precision="f16x3", train_any_shape=True, train_f16x3_any_shape=True)(m, rt, want_weights=True, z_samples=T(np.concatenate([z, z_b]), dev))
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
    r = _renderer(cfg, sc, precision="f16x3", train_any_shape=True, train_f16x3_any_shape=True)
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


# ---- the GEMM itself: forward / dX / dW against float64, next to diner_train_gemm_act (the fp32 MFMA kernel) on the same data -------
SHAPES = [(1000, 96, 40), (1000, 256, 256), (1000, 64, 1024), (1000, 4, 128)]


def _act64(x, act, beta):
    if act == 1:
        return np.maximum(x, 0.0)
    if act == 2:
        return np.where(x * beta > 20.0, x, np.log1p(np.exp(np.minimum(x * beta, 20.0))) / beta)
    return x


def _dact64(s, act, beta):
    if act == 1:
        return (s > 0).astype(np.float64)
    if act == 2:
        z = np.exp(np.minimum(s * beta, 20.0))
        return np.where(s * beta > 20.0, 1.0, z / (z + 1.0))
    return np.ones_like(s)


def _err(c, ref):
    return float(np.abs(c.double().cpu().numpy() - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("act,beta", [(1, 1.0), (2, 3.0)])
@pytest.mark.parametrize("gscale", [1.0, 1e-12, 1e9])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_act_f16x3_is_fp32_grade(M, N, K, gscale, act, beta, dev):
    """criterion of tests/test_training.py::test_train_gemm_f16x3_is_fp32_grade: error of the new kernel < max(3 x the error of the fp32
    kernel on the same data, 1e-6), relative to max|result|; rows of mixed magnitude in the gradient operand"""
    import ctypes as C
    from diner_amd import _lib
    from diner_amd.training import EXP_ACT, EXP_W
    from diner_amd.training_gen import SplitWeight
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(M + 7 * N + 13 * K)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    X, W, b = (rn(M, K) * 2.0).to(dev), (rn(N, K) / np.sqrt(K)).to(dev), rn(N).to(dev)
    rowmag = torch.pow(10.0, torch.randint(-3, 1, (M, 1), generator=g).float())
    dY = (rn(M, N) * rowmag * gscale).to(dev)
    S = X.clone()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    X64, W64, b64, dY64 = (t.double().cpu().numpy() for t in (X, W, b, dY))
    amax = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(L.diner_train_amax(p(dY), dY.numel(), p(amax), st), "amax")

    # forward: act(X) W^T + b
    ref = _act64(X64, act, beta) @ W64.T + b64
    c32, c16, c16s = (torch.empty(M, N, device=dev) for _ in range(3))
    _lib.check(L.diner_train_gemm_act(p(X), p(W), p(b), None, p(c32), M, N, K, K, 1, 1, K, N, 0, act, 0, 0, beta, 0, 0, 0, st), "fp32")
    sw = SplitWeight(W, False)
    _lib.check(L.diner_train_gemm_act_f16x3_w(p(X), K, p(sw.hi), p(sw.lo), p(b), None, 0, p(c16), N, M, N, K, act, 0, beta, 0, None, EXP_ACT,
                                              EXP_W, st), "f16x3_w")
    _lib.check(L.diner_train_gemm_act_f16x3(p(X), p(W), p(b), None, p(c16s), M, N, K, K, 1, 1, K, N, 0, act, 0, 0, beta, 0, 0, 0, None, None,
                                            EXP_ACT, EXP_W, st), "f16x3")
    e32, e16, e16s = _err(c32, ref), _err(c16, ref), _err(c16s, ref)
    print(f"fwd  {M}x{N}x{K} act {act} gscale {gscale:g}: fp32 {e32:.3e} f16x3(pre-split) {e16:.3e} f16x3(streamed) {e16s:.3e}")
    assert e32 < 2e-6, e32                          # the yardstick itself: the bar tests/test_training.py puts on the fp32 kernel
    assert e16 < max(3 * e32, 1e-6) and e16s < max(3 * e32, 1e-6)

    # dX: (dY W) * act'(S), S = the [M, K] pre-activation
    ref = (dY64 @ W64) * _dact64(X64, act, beta)
    c32, c16, c16s = (torch.empty(M, K, device=dev) for _ in range(3))
    _lib.check(L.diner_train_gemm_act(p(dY), p(W), None, p(S), p(c32), M, K, N, N, 1, K, 1, K, K, 0, 0, act, beta, 0, 0, 0, st), "fp32")
    swt = SplitWeight(W, True)
    _lib.check(L.diner_train_gemm_act_f16x3_w(p(dY), N, p(swt.hi), p(swt.lo), None, p(S), K, p(c16), K, M, K, N, 0, act, beta, 0, p(amax), 0,
                                              EXP_W, st), "f16x3_w")
    _lib.check(L.diner_train_gemm_act_f16x3(p(dY), p(W), None, p(S), p(c16s), M, K, N, N, 1, K, 1, K, K, 0, 0, act, beta, 0, 0, 0, p(amax), None,
                                            0, EXP_W, st), "f16x3")
    e32, e16, e16s = _err(c32, ref), _err(c16, ref), _err(c16s, ref)
    print(f"dX   {M}x{N}x{K} act {act} gscale {gscale:g}: fp32 {e32:.3e} f16x3(pre-split) {e16:.3e} f16x3(streamed) {e16s:.3e}")
    assert e32 < 2e-6, e32                          # the yardstick itself: the bar tests/test_training.py puts on the fp32 kernel
    assert e16 < max(3 * e32, 1e-6) and e16s < max(3 * e32, 1e-6)

    # dW: dY^T act(X), split over the rows, atomics
    ref = dY64.T @ _act64(X64, act, beta)
    c32, c16 = torch.zeros(N, K, device=dev), torch.zeros(N, K, device=dev)
    _lib.check(L.diner_train_gemm_act(p(dY), p(X), None, None, p(c32), N, K, M, 1, N, K, 1, K, 0, 0, act, 0, beta, 0, 1, 256, st), "fp32")
    _lib.check(L.diner_train_gemm_act_f16x3(p(dY), p(X), None, None, p(c16), N, K, M, 1, N, K, 1, K, 0, 0, act, 0, beta, 0, 1, 256, p(amax), None,
                                            0, EXP_ACT, st), "f16x3")
    e32, e16 = _err(c32, ref), _err(c16, ref)
    print(f"dW   {M}x{N}x{K} act {act} gscale {gscale:g}: fp32 {e32:.3e} f16x3 {e16:.3e}")
    assert e32 < 2e-6, e32
    assert e16 < max(3 * e32, 1e-6)


# ---- render_image under autograd: the frame is the inference kernel's, its backward re-runs the training path in chunks -----------
def _close(a, b, what, rel=1e-5):
    """tests/test_gpu_image_grad.py's comparison: 1e-5 of the tensor's largest entry (atomically accumulated weight gradients)"""
    assert a is not None and b is not None, what
    assert a.shape == b.shape and a.dtype == b.dtype, what
    err, scale = (a.double() - b.double()).abs().max().item(), b.double().abs().max().item()
    assert err <= rel * scale + 1e-12, (what, err, scale)


def _image_grads(r, m, SB, H, W, cams, use_image):
    from diner_amd import glue
    E, Kt, zn, zf = cams
    leaves = [t.clone().requires_grad_(True) for t in (E, Kt, zf)]
    params = list(m.mlp_fine.parameters())
    for t in params + [m.encoder.latent]:
        t.grad = None
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
    return dict(zip(names, [t.grad for t in leaves] + [m.encoder.latent.grad] + [p.grad for p in params]))


@pytest.mark.parametrize("dims,chunk", [(dict(d_hidden=128), None), (dict(d_hidden=96, n_blocks=3, combine_layer=1, beta=2.0), 97)])
def test_render_image_under_autograd_takes_the_new_route_in_its_chunks(dims, chunk, dev):
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    H, W, SB = 20, 28, 1
    sc = synth.make_scene(24, 32, 3, seed=5, feature_padding=4)
    m = model_from_scene(sc, synth.make_mlp_weights(6, bias_scale=0.1, **{k: v for k, v in dims.items() if k != "beta"}), device=dev, **dims)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent.requires_grad_(True)
    E = T(np.stack([synth.look_at_origin_w2c(0.1, sc.meta["cam_radius"])]), dev)
    Kt = torch.tensor([[1.2 * W, 0, W / 2 + 0.7], [0, 1.1 * W, H / 2 - 0.4], [0, 0, 1]], dtype=torch.float32, device=dev).repeat(SB, 1, 1)
    cams = (E, Kt, torch.full((SB,), float(sc.near), device=dev), torch.full((SB,), float(sc.far), device=dev))
    r = NeRFRendererDGS(n_samples=16, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd, train_any_shape=True,
                        train_f16x3_any_shape=True)
    r.precision = "f16x3"
    if chunk is not None:
        r.grad_chunk_rays = chunk
    with pytest.warns(UserWarning, match="precision="):     # the frame itself is the fp32 shape-general inference kernel, and says so
        g_img = _image_grads(r, m, SB, H, W, cams, True)
    assert r.last_route == "train_gen_f16" and r.effective_precision == "f16x3"      # what the backward's chunks ran
    g_fwd = _image_grads(r, m, SB, H, W, cams, False)
    assert r.last_route == "train_gen_f16"
    for k in g_fwd:
        _close(g_img[k], g_fwd[k], k)
    r.train_f16x3_any_shape = False                          # switch off: the chunks run the fp32 path
    _image_grads(r, m, SB, H, W, cams, True)
    assert r.last_route == "train_gen" and r.effective_precision == "fp32"


# ---- beyond the fp16 range: non-finite, never clamped, no error (as diner_train_gemm's f16x3 mode) ------------------------------------
def test_activation_beyond_the_fp16_range_gives_non_finite_results(dev):
    import ctypes as C
    from diner_amd import _lib
    from diner_amd.training import EXP_ACT, EXP_W
    from diner_amd.training_gen import SplitWeight
    L = _lib.lib()
    M, N, K = 256, 128, 64
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device="cpu").manual_seed(3)
    X, W = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / 8).to(dev)
    X[5, 7] = 65504.0 * 16 * 1.01                    # * 2^-4 lies above the largest fp16
    X[9, 3] = 65504.0 * 16 * 0.5                     # half of it: in range, row 9 stays finite
    sw = SplitWeight(W, False)
    outs = [torch.empty(M, N, device=dev) for _ in range(3)]
    _lib.check(L.diner_train_gemm_act_f16x3_w(p(X), K, p(sw.hi), p(sw.lo), None, None, 0, p(outs[0]), N, M, N, K, 0, 0, 1.0, 0, None, EXP_ACT,
                                              EXP_W, st), "f16x3_w")
    _lib.check(L.diner_train_gemm_act_f16x3(p(X), p(W), None, None, p(outs[1]), M, N, K, K, 1, 1, K, N, 0, 0, 0, 0, 1.0, 0, 0, 0, None, None,
                                            EXP_ACT, EXP_W, st), "f16x3")
    _lib.check(L.diner_train_gemm(p(X), p(W), None, None, p(outs[2]), M, N, K, K, 1, 1, K, N, 0, 0, 0, 0, 0, 0, 1, None, None, EXP_ACT, EXP_W, st),
               "diner_train_gemm")                   # the standard path's f16x3 GEMM on the same data
    torch.cuda.synchronize()
    for c in outs:
        assert not torch.isfinite(c[5]).any()        # every product of the row's +inf hi half: inf, or inf - inf = NaN; nothing clamped
        rest = torch.ones(M, dtype=torch.bool, device=dev)
        rest[5] = False
        assert torch.isfinite(c[rest]).all()
    assert torch.equal(torch.isnan(outs[0]), torch.isnan(outs[2])) and torch.equal(torch.isnan(outs[1]), torch.isnan(outs[2]))
    ref = X[9].double() @ W.double().T
    assert (outs[0][9].double() - ref).abs().max() <= 1e-6 * ref.abs().max()


# ---- the pre-split planes: values, and the zero padding the GEMM reads without bounds -----------------------------------------------------
@pytest.mark.parametrize("rows,cols,transpose", [(96, 40, False), (40, 96, True), (4, 128, False), (128, 4, True), (130, 33, False), (200, 72, True)])
def test_split_weight_planes_and_padding(rows, cols, transpose, dev):
    from diner_amd.training import EXP_W
    from diner_amd.training_gen import SplitWeight
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    ld = cols + 4                                     # a row stride larger than the row
    buf = torch.randn(rows, ld, generator=g).to(dev)
    W = buf[:, :cols]
    sw = SplitWeight(W, transpose)
    B = (W.t() if transpose else W).contiguous()      # B^T rows: plane[n][k]
    N, K = B.shape
    npad, kpad = (N + 127) // 128 * 128, (K + 31) // 32 * 32
    assert sw.hi.numel() == sw.lo.numel() == npad * kpad
    hi, lo = sw.hi.view(npad, kpad), sw.lo.view(npad, kpad)
    t = B * 2.0 ** EXP_W
    h = t.half()
    assert torch.equal(hi[:N, :K], h) and torch.equal(lo[:N, :K], (t - h.float()).half())
    pad = torch.ones(npad, kpad, dtype=torch.bool, device=dev)
    pad[:N, :K] = False
    assert pad.any() and (hi[pad] == 0).all() and (lo[pad] == 0).all()
    # hi + lo carries the weight to ~2^-22 relative
    assert ((hi[:N, :K].double() + lo[:N, :K].double()) - t.double()).abs().max() <= 2.0 ** -21 * t.abs().max()
