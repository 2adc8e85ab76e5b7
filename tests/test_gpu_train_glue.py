"""GPU tests of a training step's ray selection and photometric losses (glue.gen_rays_at, glue.photo_loss, glue.calc_losses;
diner_amd/csrc/train_glue.hip) on every case of tests/golden/train_glue.npz, against the float64 restatement of tests/train_glue_ref.py
(tests/test_train_glue_host.py proves on the CPU that it reproduces the reference and that its comparisons reject wrong forms).

Bounds:
* gen_rays_at: bit-equal to the indexed glue.gen_rays; its camera gradients within GRAD_REL = 1e-5 of the tensor's largest entry -- the
  bound tests/test_gpu_image_grad.py holds diner_gen_rays_backward to (the same fp64 store-and-sum scheme), taken by value;
* gt_colors: bit-equal to the fixture; mse / antibias: within 4 x the reference's own recorded fp32 deviation for the case (a different
  but legitimate fp32 association; the kernel's fp64 partials leave one final rounding, which is never worse than the reference's own:
  its result is a float too, and ours is the float nearest the exact value);
* d_pred: elementwise within 2 ulp (fp32) of the MSE term + half an ulp of the total (the one rounding no fp32 output can avoid where the
  exact antibias constant dominates it); the antibias part alone (g_mse = 0) is the fp32-rounded constant times the sign, exactly, and an
  exact 0 in the equal cell and in the dropped remainder;
* every backward twice: bit-equal.

Largest error / bound ratios measured on an MI355X over all cases: see DESIGN.md §7 "Training-step glue"."""
import numpy as np
import pytest
import torch

from tests import train_glue_ref as R
from tests.test_train_glue_host import CASES, fixture

pytestmark = pytest.mark.gpu
GRAD_REL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name", CASES)
def test_gen_rays_at_is_bit_equal_to_indexed_gen_rays(name, dev):
    from diner_amd import glue
    cfg, d = fixture()[name]
    H, W, SB = cfg["H"], cfg["W"], cfg["SB"]
    cams = [T(d[k], dev) for k in ("E", "K", "zn", "zf")]
    idx = T(d["idx"], dev)
    full = glue.gen_rays(cams[0], cams[1], W, H, cams[2], cams[3]).view(SB, H * W, 8)
    want = torch.stack([full[b, idx[b]] for b in range(SB)])
    got = glue.gen_rays_at(cams[0], cams[1], W, H, cams[2], cams[3], idx, check_indices=True)
    assert got.shape == (SB, cfg["B"], 8) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(glue.gen_rays_at(cams[0], cams[1], W, H, cams[2], cams[3], idx.int()), got)           # int32 indices
    leaves = [t.clone().requires_grad_(True) for t in cams]
    under = glue.gen_rays_at(leaves[0], leaves[1], W, H, leaves[2], leaves[3], idx)
    assert under.requires_grad and torch.equal(under.detach(), got)


def test_out_of_range_indices_are_clamped_not_followed(dev):
    from diner_amd import glue
    cfg, d = fixture()["random_b130"]
    H, W = cfg["H"], cfg["W"]
    cams = [T(d[k], dev) for k in ("E", "K", "zn", "zf")]
    idx = T(d["idx"], dev).clone()
    idx[0, 3], idx[1, 4] = -7, H * W + 5
    with pytest.raises(IndexError):
        glue.gen_rays_at(cams[0], cams[1], W, H, cams[2], cams[3], idx, check_indices=True)
    got = glue.gen_rays_at(cams[0], cams[1], W, H, cams[2], cams[3], idx)
    want = glue.gen_rays_at(cams[0], cams[1], W, H, cams[2], cams[3], idx.clamp(0, H * W - 1))
    assert torch.equal(got, want)
    _, _, gt = glue.photo_loss(T(d["pred"], dev), T(d["target"], dev), idx)
    _, _, gt_c = glue.photo_loss(T(d["pred"], dev), T(d["target"], dev), idx.clamp(0, H * W - 1))
    assert torch.equal(gt, gt_c)


@pytest.mark.parametrize("name", CASES)
def test_gen_rays_at_camera_gradients_match_float64(name, dev):
    from diner_amd import glue
    cfg, d = fixture()[name]
    H, W = cfg["H"], cfg["W"]
    idx, cot = T(d["idx"], dev), T(d["d_rays"], dev)
    leaves = [T(d[k], dev).requires_grad_(True) for k in ("E", "K", "zn", "zf")]
    grads = torch.autograd.grad(glue.gen_rays_at(leaves[0], leaves[1], W, H, leaves[2], leaves[3], idx), leaves, cot)
    ref = R.gen_rays_at_grads_ref(d["E"], d["K"], W, H, d["zn"], d["zf"], d["idx"], d["d_rays"])
    for what, g, r in zip(("extrinsics", "intrinsics", "z_near", "z_far"), grads, ref):
        assert g.dtype == torch.float32 and g.shape == r.shape, what
        err, scale = (g.double().cpu() - r).abs().max().item(), r.abs().max().item()
        print(f"{name}: {what}: err {err:.3e} scale {scale:.3e} ratio to bound {err / (GRAD_REL * scale):.3e}")
        assert err <= GRAD_REL * scale, (what, err, scale)
    assert (grads[0][:, 3, :] == 0).all()
    used = torch.zeros(3, 3, dtype=torch.bool, device=dev)
    used[0, 0] = used[1, 1] = used[0, 2] = used[1, 2] = True
    assert (grads[1][:, ~used] == 0).all()
    again = torch.autograd.grad(glue.gen_rays_at(leaves[0], leaves[1], W, H, leaves[2], leaves[3], idx), leaves, cot)
    for a, b in zip(grads, again):
        assert torch.equal(a, b)                     # fixed-order sums: bitwise reproducible
    g32 = torch.autograd.grad(glue.gen_rays_at(leaves[0], leaves[1], W, H, leaves[2], leaves[3], idx.int()), leaves, cot)
    for a, b in zip(grads, g32):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_photo_loss_values(name, dev):
    from diner_amd import glue
    cfg, d = fixture()[name]
    patch, n = cfg.get("s"), cfg.get("n", 3)
    pred, target, idx = T(d["pred"], dev), T(d["target"], dev), T(d["idx"], dev)
    mse, ab, gt = glue.photo_loss(pred, target, idx, patch=patch, antibias_downsampling=n)
    assert mse.shape == ab.shape == () and mse.dtype == ab.dtype == gt.dtype == torch.float32
    assert np.array_equal(gt.cpu().numpy().view(np.uint32), d["gt"].view(np.uint32))
    mse64, ab64, _ = R.photo_loss_ref(d["pred"], d["target"], d["idx"], patch, n)
    for what, got, want in (("mse", mse, mse64), ("ab", ab, ab64)):
        err, bound = abs(float(got.double().cpu()) - float(want)), 4.0 * float(d["dev_" + what])
        print(f"{name}: {what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0.0:.3f}")
        assert err <= bound, (what, err, bound)
    if patch is None:
        assert float(ab) == 0.0
    mse2, ab2, gt2 = glue.photo_loss(pred, target, idx.int(), patch=patch, antibias_downsampling=n)
    assert torch.equal(mse, mse2) and torch.equal(ab, ab2) and torch.equal(gt, gt2)
    under = glue.photo_loss(pred.clone().requires_grad_(True), target, idx, patch=patch, antibias_downsampling=n)
    assert torch.equal(under[0].detach(), mse) and torch.equal(under[1].detach(), ab) and not under[2].requires_grad


@pytest.mark.parametrize("name", CASES)
def test_photo_loss_d_pred(name, dev):
    from diner_amd import glue
    cfg, d = fixture()[name]
    patch, n, SB = cfg.get("s"), cfg.get("n", 3), cfg["SB"]
    target, idx = T(d["target"], dev), T(d["idx"], dev)
    g_mse, g_ab = float(d["g"][0]), float(d["g"][1])

    def d_pred(wm, wa):
        pred = T(d["pred"], dev).requires_grad_(True)
        mse, ab, _ = glue.photo_loss(pred, target, idx, patch=patch, antibias_downsampling=n)
        (wm * mse + wa * ab).backward()
        return pred.grad

    got = d_pred(g_mse, g_ab)
    assert torch.equal(got, d_pred(g_mse, g_ab))                                       # two runs: bit-equal
    want, mse_term, ab_term = (t.numpy() for t in R.photo_loss_dpred_ref(d["pred"], d["gt"], patch, n, g_mse, g_ab))
    err = np.abs(got.double().cpu().numpy() - want)
    bound = 2.0 * ulp32(mse_term) + 0.5 * ulp32(want)
    print(f"{name}: d_pred: worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    if patch is None:
        return
    # the antibias part alone: the exact constant times the sign; 0 in an equal cell and in the dropped remainder
    only = d_pred(0.0, g_ab).cpu().numpy()
    _, _, ab_only = R.photo_loss_dpred_ref(d["pred"], d["gt"], patch, n, 0.0, g_ab)
    assert np.array_equal(only, ab_only.numpy().astype(np.float32))
    p = 2 ** n
    img = only.reshape(SB, patch, patch, 3)
    nc = patch // p
    assert (img[:, nc * p:] == 0).all() and (img[:, :, nc * p:] == 0).all()
    assert (np.abs(img[:, :nc * p, :nc * p]) > 0).sum() == img[:, :nc * p, :nc * p].size - (3 * p * p if cfg.get("equal") else 0)
    if cfg.get("equal"):
        assert (img[0, p:2 * p, :p] == 0).all()
        both = got.cpu().numpy().reshape(SB, patch, patch, 3)[0, p:2 * p, :p]
        assert (both == 0).all()             # pred == gt there: the MSE term is an exact 0 too


def test_calc_losses_on_the_stub_model(dev):
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    H, W, s, n = 24, 32, 8, 2
    sc = synth.make_scene(H, W, 3, seed=5, feature_padding=4)
    m = model_from_scene(sc, synth.make_mlp_weights(6, bias_scale=0.1), device=dev)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    seen = []
    m.encode = lambda **kw: seen.append(sorted(kw))             # the stub's maps are already in place
    class Recording:
        """the renderer, keeping what calc_losses hands it and what it returns"""
        def __init__(self):
            self.r = NeRFRendererDGS(n_samples=16, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd)

        def forward(self, model, rays):
            self.rays, self.out = rays, self.r.forward(model=model, rays=rays)
            return self.out

    r = Recording()
    g = torch.Generator(device=dev).manual_seed(3)
    batch = dict(src_rgbs=None, src_depths=None, src_depth_stds=None, src_extrinsics=None, src_intrinsics=None,
                 target_rgb=torch.rand((1, 3, H, W), device=dev, generator=g),
                 target_extrinsics=T(sc.target_extrinsics, dev)[None].clone().requires_grad_(True),
                 target_intrinsics=T(sc.target_intrinsics, dev)[None])
    ys, xs = torch.meshgrid(torch.arange(s, device=dev), torch.arange(s, device=dev), indexing="ij")
    pix_idcs = ((W // 2 - s // 2 + xs) + (H // 2 - s // 2 + ys) * W).reshape(1, -1)
    w_ab = 0.25
    out = glue.calc_losses(m, r, batch, sc.near, sc.far, pix_idcs, patch=s, w_antibias=w_ab, antibias_downsampling=n)
    assert seen == [["depths", "depths_std", "extrinsics", "images", "intrinsics"]]
    assert set(out) == {"rgb_fine", "vgg_fine", "antibias", "total"} and out["vgg_fine"] == 0.
    assert torch.equal(out["total"], out["rgb_fine"] + w_ab * out["antibias"])
    assert out["total"] is not out["rgb_fine"]
    # rgb_fine / antibias from the pieces: the rays calc_losses made and the colours the renderer returned for them
    with torch.no_grad():
        assert torch.equal(r.rays.detach(), glue.gen_rays_at(batch["target_extrinsics"], batch["target_intrinsics"], W, H, sc.near, sc.far, pix_idcs))
        mse, ab, _ = glue.photo_loss(r.out.fine.rgb.detach(), batch["target_rgb"], pix_idcs, patch=s, antibias_downsampling=n)
    assert torch.equal(mse, out["rgb_fine"].detach()) and torch.equal(ab, out["antibias"].detach())
    out["total"].backward()
    for name, p in m.mlp_fine.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert sum(float(p.grad.abs().sum()) for p in m.mlp_fine.parameters()) > 0
    assert float(m.mlp_fine.lin_out.weight.grad.abs().max()) > 0
    gE = batch["target_extrinsics"].grad
    assert gE is not None and bool(torch.isfinite(gE).all()) and float(gE[:, :3].abs().max()) > 0
    # without the antibias weight: no pooling, the float 0. of the reference
    with torch.no_grad():
        plain = glue.calc_losses(m, r, batch, sc.near, sc.far, pix_idcs)
        mse, ab, _ = glue.photo_loss(r.out.fine.rgb, batch["target_rgb"], pix_idcs)
    assert plain["antibias"] == 0. and plain["total"] is plain["rgb_fine"] and torch.equal(plain["rgb_fine"], mse) and float(ab) == 0.0
