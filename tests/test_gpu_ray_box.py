"""Rendering inside a scene bounding box on the MI355X (diner_amd/csrc/ray_box.hip; glue.ray_box, glue.box_rays, glue.frame_from_hits,
NeRFRendererDGS.render_image(bounds=)):

* the select kernels against the float64 restatement of tests/ray_box_ref.py at the sizes where the ordered compaction can go wrong
  (one pixel, less than a wave, exactly one 256-pixel workgroup, one workgroup and a partial one, many), one scene and three (no hit,
  every pixel hit, mixed): mask outside the ambiguous set, near / far within 1e-6 max(1, far), count, idx, slot, two runs bit-equal;
* the compact rays bit-equal to gen_rays_at's and to ray_box's near / far, the padding as specified;
* render_image(bounds=) bit-equal to frame_from_hits(forward(box_rays(...))) on the standard and on a shape-general model, the
  background exact, last_box_hits, a box no ray meets, the frame without bounds unchanged, and the refusal under autograd."""
import numpy as np
import pytest
import torch

from tests import ray_box_ref as R

pytestmark = pytest.mark.gpu

BOX = np.array([[-0.12, -0.16, -0.10], [0.11, 0.15, 0.13]], np.float32)
SIZES = ((1, 1), (5, 7), (16, 16), (17, 31), (48, 64))      # RB_THREADS = 256 pixels per workgroup
Z_NEAR, Z_FAR = 0.05, 10.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def cameras(kind, H, W):
    """(E [4,4], K [3,3]) float32: 'mixed' sees the box over about a third of the image, 'inside' sits in it, 'away' has it behind"""
    if kind == "mixed":
        return R.look_at((0.3, -0.2, -1.8)).astype(np.float32), R.intrinsics(2.3 * max(H, W), H, W).astype(np.float32)
    if kind == "inside":
        return R.look_at((0.02, -0.01, 0.0), target=(0.0, 0.0, 1.0)).astype(np.float32), R.intrinsics(0.8 * max(H, W), H, W).astype(np.float32)
    return R.look_at((0.0, 0.0, -1.5), target=(0.0, 0.0, -3.0)).astype(np.float32), R.intrinsics(1.5 * max(H, W), H, W).astype(np.float32)


_refs = {}


def reference(kinds, H, W):
    """the restatement's result per scene, computed once per case and left unchanged"""
    key = (kinds, H, W)
    if key not in _refs:
        cams = [cameras(k, H, W) for k in kinds]
        _refs[key] = (cams, [R.ray_box_ref(E, K, H, W, Z_NEAR, Z_FAR, BOX) for E, K in cams])
    return _refs[key]


@pytest.mark.parametrize("kinds", [("mixed",), ("away", "inside", "mixed")], ids=["SB1", "SB3"])
@pytest.mark.parametrize("H,W", SIZES)
def test_select_and_rays_against_the_restatement(H, W, kinds, dev):
    from diner_amd import glue
    cams, refs = reference(kinds, H, W)
    SB, npix = len(kinds), H * W
    E, K = T(np.stack([c[0] for c in cams]), dev), T(np.stack([c[1] for c in cams]), dev)
    bounds = T(BOX, dev) if SB == 1 else np.tile(BOX, (SB, 1, 1))          # a [2,3] tensor, or an [SB,2,3] array
    near, far, mask = glue.ray_box(E, K, W, H, Z_NEAR, Z_FAR, bounds)
    rays, idx, slot, counts = glue.box_rays(E, K, W, H, Z_NEAR, Z_FAR, bounds)
    assert tuple(near.shape) == tuple(far.shape) == tuple(mask.shape) == (SB, H, W) and mask.dtype == torch.bool
    B = int(counts.max())
    assert tuple(rays.shape) == (SB, B, 8) and tuple(idx.shape) == (SB, B) and tuple(slot.shape) == (SB, npix) and tuple(counts.shape) == (SB,)
    assert idx.dtype == slot.dtype == counts.dtype == torch.int32
    assert torch.equal(mask.view(SB, npix), slot >= 0)
    for sb, (kind, ref) in enumerate(zip(kinds, refs)):
        got = dict(near=near[sb].cpu().numpy(), far=far[sb].cpu().numpy(), mask=mask[sb].cpu().numpy(), idx=idx[sb].cpu().numpy(),
                   slot=slot[sb].cpu().numpy(), count=int(counts[sb]))
        amb = ref["ambiguous"]
        both = got["mask"] & ref["mask"] & ~amb
        print(f"{H}x{W} {kind}: hits {got['count']} of {npix}, ambiguous {amb.mean():.2%}, "
              f"|near| {np.abs(got['near'] - ref['near'])[both].max(initial=0):.2e}, |far| {np.abs(got['far'] - ref['far'])[both].max(initial=0):.2e}")
        assert R.compare(got, ref, amb) == [], (kind, H, W)
        assert (got["near"][~got["mask"]] == np.float32(Z_NEAR)).all() and (got["far"][~got["mask"]] == np.float32(Z_FAR)).all()
        assert (got["idx"][got["count"]:] == -1).all()
        if kind == "inside":
            assert got["count"] == npix and (got["near"] == np.float32(Z_NEAR)).all()
        if kind == "away":
            assert got["count"] == 0
    if "mixed" in kinds and npix > 1:
        c = int(counts[-1])
        assert 0 < c < npix

    # two runs give the same bytes (fresh buffers each)
    cam, b, lo, hi, _keep = glue._box_args(E, K, W, H, Z_NEAR, Z_FAR, bounds, glue.BOX_OFFSET, "test")
    one = glue._ray_box_select(cam, SB, b, lo, hi, dev, True)
    two = glue._ray_box_select(cam, SB, b, lo, hi, dev, True)
    for a, c in zip(one, two):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, c.view(torch.int32) if c.dtype == torch.float32 else c)
    assert torch.equal(one[0].view(SB, H, W, 2)[..., 0], near) and torch.equal(one[2], slot)

    # the compact rays: gen_rays_at's origin and direction and ray_box's near / far at idx, bit for bit; the padding
    if B == 0:
        return
    full = glue.gen_rays_at(E, K, W, H, Z_NEAR, Z_FAR, idx.clamp(min=0))
    nf = torch.stack((near.view(SB, npix), far.view(SB, npix)), dim=-1)
    for sb in range(SB):
        c = int(counts[sb])
        assert torch.equal(rays[sb, :c, :6], full[sb, :c, :6])
        assert torch.equal(rays[sb, :c, 6:], nf[sb, idx[sb, :c].long()])
        if c == 0:
            pix0 = glue.gen_rays_at(E[sb:sb + 1], K[sb:sb + 1], W, H, Z_NEAR, Z_FAR, torch.zeros((1, 1), dtype=torch.int32, device=dev))[0, 0]
            assert torch.equal(rays[sb], pix0.expand(B, 8))
        elif c < B:
            assert torch.equal(rays[sb, c:], rays[sb, c - 1].expand(B - c, 8))


def test_frame_from_hits_against_the_restatement(dev):
    from diner_amd import glue
    H, W = 17, 31
    cams, refs = reference(("away", "inside", "mixed"), H, W)
    slot = T(np.stack([r["slot"] for r in refs]), dev)
    B = max(r["count"] for r in refs)
    g = torch.Generator().manual_seed(3)
    rgb_c, depth_c = torch.rand((3, B, 3), generator=g).to(dev), (1.0 + torch.rand((3, B), generator=g)).to(dev)
    for white in (True, False):
        rgb, depth, mask = glue.frame_from_hits(rgb_c, depth_c, slot, H, W, white, return_mask=True)
        assert tuple(rgb.shape) == (3, 3, H, W) and tuple(depth.shape) == (3, 1, H, W) and tuple(mask.shape) == (3, 1, H, W)
        for sb, ref in enumerate(refs):
            want_rgb, want_depth = R.frame_from_hits_ref(rgb_c[sb].cpu().numpy(), depth_c[sb].cpu().numpy(), ref["slot"], H, W, white)
            assert np.array_equal(rgb[sb].cpu().numpy(), want_rgb) and np.array_equal(depth[sb].cpu().numpy(), want_depth)
            assert np.array_equal(mask[sb, 0].cpu().numpy(), ref["mask"])
    empty = glue.frame_from_hits(torch.empty((3, 0, 3), device=dev), torch.empty((3, 0), device=dev), torch.full_like(slot, -1), H, W, True)
    assert (empty[0] == 1.0).all() and (empty[1] == 0.0).all()


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------
FRAME_H, FRAME_W, FRAME_K = 24, 32, 16
SCENE_BOX = np.array([[-0.3, -0.35, -0.3], [0.3, 0.25, 0.3]], np.float32)      # inside the synthetic scene's sphere of radius 0.45
GEN_DIMS = dict(d_hidden=256, n_blocks=5, combine_layer=3)
_models = {}


def scene_and_model(kind, dev):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    if kind not in _models:
        sc = synth.make_scene(FRAME_H, FRAME_W, 3, seed=5, feature_padding=4)
        if kind == "standard":
            m = model_from_scene(sc, synth.make_mlp_weights(6, bias_scale=0.1), device=dev)
        else:
            m = model_from_scene(sc, synth.make_mlp_weights(3, bias_scale=0.1, d_latent=sc.C, **GEN_DIMS), device=dev, d_latent=sc.C, **GEN_DIMS)
        _models[kind] = (sc, m)
    return _models[kind]


def renderer(sc, precision="f16x3"):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=FRAME_K, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd)
    r.seed, r.precision = 3, precision
    return r


def target(sc, dev):
    E = T(np.asarray(sc.target_extrinsics, np.float32), dev)[None]
    Kt = torch.tensor([[[1.2 * FRAME_W, 0, FRAME_W / 2], [0, 1.2 * FRAME_W, FRAME_H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
    return E, Kt, float(sc.near), float(sc.far)


@pytest.mark.parametrize("kind,precision,route", [("standard", "f16x3", "points_mlp_f16"), ("shape_general", "fp32", "points_mlp_gen")])
def test_render_image_in_a_box_equals_its_three_steps(kind, precision, route, dev):
    from diner_amd import glue
    sc, m = scene_and_model(kind, dev)
    E, Kt, near, far = target(sc, dev)
    H, W = FRAME_H, FRAME_W
    a = renderer(sc, precision)
    rgb, depth, mask = a.render_image(m, E, Kt, H, W, near, far, return_depth=True, bounds=SCENE_BOX, return_mask=True)
    assert tuple(rgb.shape) == (1, 3, H, W) and tuple(depth.shape) == (1, 1, H, W) and tuple(mask.shape) == (1, 1, H, W)
    assert a.last_route.startswith(route) and a.last_binding in ("torch_ops", "ctypes")
    hits = int(mask.sum())
    assert a.last_box_hits == [hits] and 0.1 * H * W < hits < 0.9 * H * W
    # a second renderer built alike, no earlier call: the same Philox seed
    b = renderer(sc, precision)
    rays, idx, slot, counts = glue.box_rays(E, Kt, W, H, near, far, SCENE_BOX)
    assert counts.tolist() == [hits]
    with torch.no_grad():
        fine = b(m, rays).fine
    assert b.last_route == a.last_route
    want_rgb, want_depth = glue.frame_from_hits(fine.rgb, fine.depth, slot, H, W, sc.white_bkgd)
    assert torch.equal(rgb, want_rgb) and torch.equal(depth, want_depth)
    assert torch.equal(mask.view(1, H * W), slot >= 0)
    # the background is exact, the rendered pixels are the compact results
    bg = 1.0 if sc.white_bkgd else 0.0
    miss = ~mask.expand(1, 3, H, W)
    assert (rgb[miss] == bg).all() and (depth[~mask] == 0.0).all()
    assert torch.equal(rgb.permute(0, 2, 3, 1).reshape(H * W, 3)[idx[0].long()], fine.rgb[0])
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all() and float(depth.max()) > 0.0
    # rgb alone, and rgb + mask
    only = renderer(sc, precision).render_image(m, E, Kt, H, W, near, far, bounds=T(SCENE_BOX, dev)[None])
    assert isinstance(only, torch.Tensor) and torch.equal(only, rgb)
    pair = renderer(sc, precision).render_image(m, E, Kt, H, W, near, far, bounds=SCENE_BOX, return_mask=True)
    assert len(pair) == 2 and torch.equal(pair[1], mask)


def test_a_box_no_ray_meets_is_the_background_without_a_render(dev):
    sc, m = scene_and_model("standard", dev)
    E, Kt, near, far = target(sc, dev)
    r = renderer(sc)
    rgb, depth, mask = r.render_image(m, E, Kt, FRAME_H, FRAME_W, near, far, return_depth=True, bounds=SCENE_BOX + np.float32(50.0), return_mask=True)
    assert r.last_box_hits == [0] and not mask.any()
    assert (rgb == (1.0 if sc.white_bkgd else 0.0)).all() and (depth == 0.0).all()
    assert r._calls == 0 and r.last_route is None             # no seed was drawn, no route taken: nothing was rendered


def test_without_bounds_the_frame_is_forward_of_gen_rays(dev):
    from diner_amd import glue
    sc, m = scene_and_model("standard", dev)
    E, Kt, near, far = target(sc, dev)
    H, W = FRAME_H, FRAME_W
    r = renderer(sc)
    rgb, depth = r.render_image(m, E, Kt, H, W, near, far, return_depth=True)
    assert r.last_box_hits is None
    rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
    r.seed, r._calls = 3, 0
    with torch.no_grad():
        ref = r(m, rays).fine
    assert torch.equal(rgb, ref.rgb.view(1, H, W, 3).permute(0, 3, 1, 2))
    assert torch.equal(depth, ref.depth.view(1, H, W, 1).permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="return_mask"):
        r.render_image(m, E, Kt, H, W, near, far, return_mask=True)


def test_bounds_under_autograd_is_refused(dev):
    sc, m = scene_and_model("standard", dev)
    E, Kt, near, far = target(sc, dev)
    r = renderer(sc)
    with pytest.raises(NotImplementedError, match=r"glue\.box_rays"):
        r.render_image(m, E.clone().requires_grad_(True), Kt, FRAME_H, FRAME_W, near, far, bounds=SCENE_BOX)
    assert r._calls == 0 and r.last_box_hits is None
