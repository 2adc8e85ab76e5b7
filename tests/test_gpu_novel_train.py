"""Training the NOVEL point model on the GPU (diner_amd/training_novel.py; csrc/train_novel.hip + the shape-general training GEMMs):
(i)   every ``novel_train_*`` fixture -- the unmodified reference's autograd on the CPU (tools/gen_novel_train_golden.py) -- in fp32 and
      f16x3 at the bars of tests/novel_train_ref.py::check_fixture: the forward at tests/test_gpu_novel_point.py's (rgb 1e-4, sigma 1e-4
      relative), the parameter and latent gradients at tests/test_gpu_train_shapes.py's (norm 1e-4, sum 2e-4 norm sqrt(n), probes,
      2e-4 max for the latents; tests/test_gpu_train_shapes_f16.py holds f16x3 to the same), gen_latent's whole gradient at
      2e-4 max|ref| + 1e-6 where it is stored whole; case e: both latent gradients exactly 0;
(ii)  ``composite()`` and ``forward()`` with ``train_hip_point_model`` against the PyTorch route on the restated model, same GPU, on the
      nc64 geometry of tests/golden/novel_sampler.npz for the loss rgb c1 + depth c2 + weights c3: outputs at 2e-5, gradients at (i)'s bars;
(iii) the contract: only what requires grad receives one, an in-place update between forward and backward and a double backward raise, ten
      Adam steps lower the loss and the packed gen_latent follows them, a batch of two scenes gives the scenes' gradients summed.
tests/test_novel_train_host.py proves fixtures, restatement and comparison on the CPU; tests/test_gpu_novel_train_stage.py the two new
kernels alone."""
import numpy as np
import pytest
import torch

from synthetic import synth
from tests import novel_point_ref as R
from tests import novel_sampler_ref as N
from tests import novel_train_ref as TR
from tools.gen_novel_train_golden import CASES, cotangent

pytestmark = pytest.mark.gpu
ROUTE = {"fp32": "novel_train_gen", "f16x3": "novel_train_gen_f16"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def renderer(precision="fp32", **kw):
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(hip_point_model=True, train_hip_point_model=True, train_f16x3_any_shape=precision == "f16x3", **kw)
    r.precision = precision
    return r


def trainable(inp, dev, mlp=True, latent=True, gen=True):
    """the stand-in model of a case with fresh leaves; called, it is the restatement with its graph kept (TR.TrainableNovelModel)"""
    m = R.model_from_inputs(inp, device=dev)
    m.__class__, m.case_inputs = TR.TrainableNovelModel, inp
    for p in m.mlp_fine.parameters():
        p.requires_grad_(mlp)
    m.encoder.latent = m.encoder.latent.detach().clone().requires_grad_(latent)
    m.gen_latent.requires_grad_(gen)
    return m


def points_with_grad(r, m, inp, dev):
    from diner_amd import training_novel
    f16 = r.precision == "f16x3"
    args = [T(inp[k], dev) for k in ("xyz_in", "xyz_gen", "viewdirs")]
    return training_novel.render_points_with_grad(r, m, *args, r._validate(m), f16=f16)


def grads_of(m, out=None):
    z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().cpu().numpy()
    g = dict(params={k: z(p) for k, p in m.mlp_fine.named_parameters()}, latent=z(m.encoder.latent), gen=z(m.gen_latent))
    if out is not None:
        g["rgbsigma"] = out.detach().cpu().numpy()
    return g


# ---- (i) golden parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_training_matches_the_reference_autograd(name, precision, dev):
    inp, data = TR.load(name)
    cfg = CASES[name]
    m = trainable(inp, dev)
    out = points_with_grad(renderer(precision), m, inp, dev)
    assert out.shape == data["rgbsigma"].shape and out.requires_grad and m.calls == 0
    (out * T(cotangent(cfg), dev)).sum().backward()
    got = grads_of(m, out)
    if min(cfg["mlp"].get("combine_layer", 1000), cfg["mlp"]["n_blocks"]) == 0:       # case e: neither latent is read
        assert (got["latent"] == 0).all() and (got["gen"] == 0).all()
    TR.check_fixture(got, data, cfg, label=f"{name} {precision}")


# ---- (ii) composite() and forward() against the PyTorch route -----------------------------------------------------------------------------------
SAMPLER_CFG = dict(mlp=dict(n_blocks=3, combine_layer=2), scene=dict(C=64), gen_h=28, gen_w=20)


@pytest.fixture(scope="module")
def sampler_inputs():
    """the nc64 case of tests/golden/novel_sampler.npz with the model of tests/test_gpu_novel_point.py's ``sampler_case``: a 64-channel
    latent, a 128-wide MLP"""
    g = np.load(TR.GOLDEN / "novel_sampler.npz")
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
    cs = np.random.RandomState(33)
    B = rec["rays"].shape[1]
    cot = dict(rgb=cs.standard_normal((1, B, 3)), depth=cs.standard_normal((1, B)), weights=cs.standard_normal((1, B, c.K)))
    return c, rec, inp, cot


_torch_route = {}


def torch_route(sampler_inputs, dev, call):
    """outputs and gradients of the PyTorch route (computed once per call kind, never changed)"""
    if call not in _torch_route:
        c, rec, inp, cot = sampler_inputs
        m = trainable(inp, dev)
        r = renderer("fp32", n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G)
        r.train_hip_point_model = False
        out = run(r, m, rec, dev, call)
        assert r.last_route == "torch" and m.calls == 1
        loss_of(out, cot, dev).backward()
        _torch_route[call] = ({k: v.detach() for k, v in out.items()}, grads_of(m))
    return _torch_route[call]


def run(r, m, rec, dev, call):
    geo = [T(rec[k], dev) for k in ("vertices", "offsets_in", "offsets_gen")]
    if call == "composite":
        w, rgb, depth = r.composite(m, T(rec["rays"], dev), T(rec["z"], dev), *geo)
        return dict(rgb=rgb, depth=depth, weights=w)
    r.seed, r._calls = 7, 0
    f = r(m, T(rec["rays"], dev), *geo, want_weights=True).fine
    return dict(rgb=f.rgb, depth=f.depth, weights=f.weights)


def loss_of(out, cot, dev):
    return sum((out[k] * T(cot[k], dev)).sum() for k in ("rgb", "depth", "weights"))


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("call", ["composite", "forward"])
def test_composite_and_forward_match_the_torch_route(sampler_inputs, call, precision, dev):
    c, rec, inp, cot = sampler_inputs
    want, want_grads = torch_route(sampler_inputs, dev, call)
    m = trainable(inp, dev)
    r = renderer(precision, n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G)
    out = run(r, m, rec, dev, call)
    assert r.last_route == ROUTE[precision] and r.effective_precision == precision and r.last_binding == "ctypes"
    assert m.calls == 0                                                             # the model's own forward never ran
    for k in ("rgb", "depth", "weights"):
        err = float((out[k].detach() - want[k]).abs().max())
        print(f"{call} {precision}: max |d {k}| = {err:.2e}")
        assert err <= 2e-5, k
    assert float(want["weights"].sum(-1).max()) > 0.5
    loss_of(out, cot, dev).backward()
    TR.check_fixture(grads_of(m), TR.as_fixture(want_grads, SAMPLER_CFG), SAMPLER_CFG, label=f"{call} {precision}", forward=False)
    assert float(np.abs(want_grads["gen"]).max()) > 0 and float(np.abs(want_grads["latent"]).max()) > 0


# ---- (iii) the contract ------------------------------------------------------------------------------------------------------------------------
def test_only_what_requires_grad_receives_a_gradient(dev):
    inp, data = TR.load("novel_train_c")
    cot = T(cotangent(CASES["novel_train_c"]), dev)
    full = trainable(inp, dev)
    (points_with_grad(renderer(), full, inp, dev) * cot).sum().backward()
    m = trainable(inp, dev, mlp=False, latent=False, gen=True)
    (points_with_grad(renderer(), m, inp, dev) * cot).sum().backward()
    assert all(p.grad is None for p in m.mlp_fine.parameters()) and m.encoder.latent.grad is None
    torch.testing.assert_close(m.gen_latent.grad, full.gen_latent.grad, rtol=1e-4, atol=1e-5)
    m = trainable(inp, dev, mlp=True, latent=False, gen=False)
    (points_with_grad(renderer(), m, inp, dev) * cot).sum().backward()
    assert m.gen_latent.grad is None and m.encoder.latent.grad is None
    for (k, p), q in zip(m.mlp_fine.named_parameters(), full.mlp_fine.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-5, msg=k)


def test_in_place_update_of_gen_latent_between_forward_and_backward_raises(dev):
    inp, _ = TR.load("novel_train_b")
    m = trainable(inp, dev)
    loss = points_with_grad(renderer(), m, inp, dev).sum()
    with torch.no_grad():
        m.gen_latent.add_(0.0)                                                      # an optimizer step between forward and backward
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()


def test_double_backward_raises(dev):
    inp, _ = TR.load("novel_train_b")
    m = trainable(inp, dev)
    out = points_with_grad(renderer(), m, inp, dev)
    g, = torch.autograd.grad(out.sum(), m.gen_latent, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_ten_adam_steps_lower_the_loss_and_the_packed_gen_latent_follows(dev):
    inp, _ = TR.load("novel_train_a")
    m = trainable(inp, dev, latent=False)
    r = renderer()
    target = torch.full((inp["cfg"]["SB"], inp["cfg"]["P"], 3), 0.5, device=dev)
    opt = torch.optim.Adam(list(m.mlp_fine.parameters()) + [m.gen_latent], lr=1e-3)
    losses = []
    for _ in range(11):
        opt.zero_grad()
        loss = ((points_with_grad(r, m, inp, dev)[..., :3] - target) ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 11:
            break
        loss.backward()
        assert torch.isfinite(m.gen_latent.grad).all() and float(m.gen_latent.grad.abs().max()) > 0
        opt.step()
    assert losses[-1] < losses[0], losses
    args = [T(inp[k], dev) for k in ("xyz_in", "xyz_gen", "viewdirs")]
    with torch.no_grad():
        after = r.render_points_novel(m, *args)
        fresh = renderer().render_points_novel(m, *args)
    assert torch.equal(after, fresh)


def test_batch_of_two_gives_the_sum_of_the_scenes_alone(dev):
    inp, _ = TR.load("novel_train_a")
    cot = cotangent(CASES["novel_train_a"])
    m = trainable(inp, dev)
    (points_with_grad(renderer(), m, inp, dev) * T(cot, dev)).sum().backward()
    per_scene = ("poses", "focal", "c", "depths", "depths_std", "normals", "latent", "gen_poses", "gen_focal", "gen_c", "xyz_in", "xyz_gen", "viewdirs")
    total, params = 0, {}
    for sb in range(2):
        one = dict(inp)
        for k in per_scene:
            one[k] = np.ascontiguousarray(inp[k][sb:sb + 1])
        m1 = trainable(one, dev)
        (points_with_grad(renderer(), m1, one, dev) * T(cot[sb:sb + 1], dev)).sum().backward()
        total = total + m1.gen_latent.grad
        for k, p in m1.mlp_fine.named_parameters():
            params[k] = params.get(k, 0) + p.grad
        torch.testing.assert_close(m.encoder.latent.grad[sb:sb + 1], m1.encoder.latent.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(m.gen_latent.grad, total, rtol=1e-4, atol=1e-5)
    for k, p in m.mlp_fine.named_parameters():
        torch.testing.assert_close(p.grad, params[k], rtol=1e-4, atol=1e-5, msg=k)
