"""The sampler's in-kernel Philox noise (what every production call draws: ``forward(noise=None)``, ``render_image``, the torch ops, the
training step's sampler) against the host restatement of tests/philox_ref.py, whose dense tensors put the production mode on the
footing of the injected mode.  tests/test_philox_ref_host.py proves the restatement and that these comparisons reject wrong variants.
Cases: philox_ref.PHILOX_CASES (every ``sampler_kernel<CPL>``, NC not a multiple of 64 / 256, K and G beyond 64, G = 0, G = K, SB 1 and
2, call seeds below 2^32 and from 2^63); every case keeps >= 20 surface and >= 5 missing rays per scene and no ray is filtered.

(a) one stream in the kernel, the other two injected, against all three injected: candidates and fill-up bit for bit (likelihood,
    z_dg, z); the gaussian against n_gauss64 (rounded to float32) injected: short-list bit for bit, gaussian slots and the sorted z
    within dn * gstd[ray] + 2e-6, dn = 4 x max |n_gauss32 - n_gauss64| over the case's own draws (CPU only), gstd from the float64
    ``select_from_likelihood`` (n = 1 minus n = 0);
(b) all three in the kernel against the oracle on the restated tensors: the stage checks and bars of test_gpu_stage_kernels.py's
    ``test_sampler_stages`` plus the dn term;
(c) the standalone sample_coarse / fill_up kernels with a seed against their injected forms: bit for bit;
(d) ``forward(noise=None)`` == ``forward(z_samples=_sample(noise=None)["z"])`` at the same call seed, bit for bit, for fp32 / f16x3,
    the ctypes and torch-op bindings and the shape-general route (the op takes the seed as int64: seeds from 2^63 included);
(e) ray numbering: a ``render_image`` frame (gray = sb H W + pixel) and a boxed one (gray = sb B + compact slot of ``glue.box_rays``)
    with G = 0 against ``forward`` on restated noise, bit for bit; with G > 0 the frame equals ``forward(noise=None)``; the training
    forward under autograd with noise=None is the inference frame of the same call seed within 2e-5.

Largest values observed on the MI355X over all cases (every bit-for-bit comparison of (a), (c), (d) and (e) held without exception; the
standard deviation of a ray's gaussian is 0.03 .. 0.09 on these scenes, so the 2e-6 floor is most of each bound):

                                            CPU side                                largest bound   GPU error
    (a) gaussian stream in the kernel       max |n_gauss32 - n_gauss64| 1.31e-06    2.48e-06        1.19e-07 (gaussian slots and z: 1 ulp)
    (b) all streams, against the oracle     float32 oracle's error 1.79e-06         9.35e-06        3.38e-07
    (e) training forward / inference call   bar 2e-5                                                rgb 2.21e-06, weights 2.03e-06
"""
import copy

import numpy as np
import pytest
import torch

from tests import philox_ref as pr
from tests import stage_refs as sr
from tests.philox_ref import PHILOX_CASES

pytestmark = pytest.mark.gpu
IDS = [c.id for c in PHILOX_CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


_weights = []


def sampler_model(scene, dev):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    if not _weights:
        _weights.append(synth.make_mlp_weights(1))        # the sampler reads none of them
    return model_from_scene(scene, _weights[0], device=dev)


def renderer(K, NC, G, **kw):
    from diner_amd import NeRFRendererDGS
    return NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, **kw)


def at(r, seed, calls=1):
    """the renderer's next call is call number ``calls`` of base seed ``seed``"""
    r.seed, r._calls = seed, calls - 1
    return r


def sample(r, pc, rays, m, noise, **kw):
    at(r, pc.seed, pc.calls)
    out = r._sample(rays, m, pc.K, pc.NC, pc.G, 0.05, noise, None, **kw)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


# ---- (a) one stream at a time ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PHILOX_CASES, ids=IDS)
def test_one_stream_in_the_kernel(pc, dev):
    c = pc.build()
    K, NC, G, SB, keep = pc.K, pc.NC, pc.G, pc.SB, pc.K - pc.G
    for s in range(SB):
        assert c.surface[s].sum() >= 20 and (~c.surface[s]).sum() >= 5
    r, m, rays = renderer(K, NC, G), sampler_model(c.batched_scene(), dev), T(c.rays, dev)
    u_c, n_g, u_f = T(c.u_coarse, dev), T(c.n_gauss, dev), T(c.u_fill, dev)
    ref = sample(r, pc, rays, m, (u_c, n_g, u_f), want_dg=True, want_lik=True)
    assert int((ref["z_dg"] == 0).all(-1).sum()) >= 5 * SB          # rays that take all K ranks of the fill-up stream
    # candidates
    got = sample(r, pc, rays, m, (None, n_g, u_f), want_dg=True, want_lik=True)
    for k in ("likelihood", "z_dg", "z"):
        assert pr.compare_bits(got[k], ref[k], f"candidates in the kernel: {k}") == []
    # fill-up
    got = sample(r, pc, rays, m, (u_c, n_g, None), want_dg=True)
    assert pr.compare_bits(got["z_dg"], ref["z_dg"], "fill-up in the kernel: z_dg") == []
    assert pr.compare_bits(got["z"], ref["z"], "fill-up in the kernel: z") == []
    # gaussian
    got = sample(r, pc, rays, m, (u_c, None, u_f), want_dg=True, want_lik=True)
    assert pr.compare_bits(got["likelihood"], ref["likelihood"], "gaussian in the kernel: likelihood") == []
    assert pr.compare_bits(got["z_dg"][..., :keep], ref["z_dg"][..., :keep], "gaussian in the kernel: short-list") == []
    for s in range(SB):
        gstd = pr.gauss_std(ref["likelihood"][s], c.z_cand[s], K, G)
        bad_g, err_g, tol = pr.compare_gauss(got["z_dg"][s][:, keep:], ref["z_dg"][s][:, keep:], gstd, pc.dn, "gaussian slots")
        bad_z, err_z, _ = pr.compare_gauss(got["z"][s], ref["z"][s], gstd, pc.dn, "z")
        print(f"{pc.id}[{s}]: max |n32 - n64| {pc.n32_err:.2e} gstd max {gstd.max():.2e} bound {tol:.2e} gpu err gaussian slots {err_g:.2e} z {err_z:.2e}")
        assert bad_g == [] and bad_z == []
        if G:
            assert (got["z_dg"][s][:, keep:] != 0).any(-1).sum() >= 20


# ---- (b) all three streams in the kernel, against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("pc", PHILOX_CASES, ids=IDS)
def test_all_streams_in_the_kernel_against_the_oracle(pc, dev):
    from oracle.oracle import Oracle
    c = pc.build()
    K, NC, G, SB, keep = pc.K, pc.NC, pc.G, pc.SB, pc.K - pc.G
    r, m, rays = renderer(K, NC, G), sampler_model(c.batched_scene(), dev), T(c.rays, dev)
    # 1. candidates: the standalone kernel's draw at the call seed against the oracle on the restated u_coarse
    zc = at(r, pc.seed, pc.calls).sample_coarse(rays, n_coarse=NC).cpu().numpy()
    for s in range(SB):
        np.testing.assert_allclose(zc[s], c.z_cand[s], rtol=0, atol=2.5e-7 * float(c.rays[s, :, 7].max()))
    # 2.-4. one fused call, no noise passed
    out = sample(r, pc, rays, m, None, want_dg=True, want_lik=True)
    L, z_dg, z = out["likelihood"], out["z_dg"], out["z"]
    for s in range(SB):
        orc = Oracle(c.scenes[s], None)
        assert sr.compare_likelihood(L[s], orc.likelihood(c.rays[s], zc[s])) == []      # on the kernel's own candidates (1 ulp from the oracle's)
        orc_ref, _ = sr.select_rows(c.orc_L[s], c.z_cand[s], K, G, c.n_gauss[s])
        base, cpu_err = sr.gauss_bound(c.orc_z_dg[s], orc_ref, K, G)                      # the existing bar, from CPU values alone
        ref, hit = sr.select_rows(L[s], zc[s], K, G, c.n_gauss[s])
        assert sr.compare_decisions(z_dg[s], ref, hit, K, G, np.inf) == []               # short-list as a set bit for bit, hit / no-hit
        gstd = pr.gauss_std(L[s], zc[s], K, G)
        bad, err, tol = pr.compare_gauss(z_dg[s][:, keep:], ref[:, keep:], gstd, pc.dn, "gaussian slots", base=base - sr.FLOOR_GAUSS)
        print(f"{pc.id}[{s}]: gaussian slots: oracle err {cpu_err:.2e} bound {tol:.2e} gpu err {err:.2e}; surface rays "
              f"{int(c.surface[s].sum())}/{c.surface[s].size}")
        assert bad == []
        np.testing.assert_array_equal(z[s], orc.fill_up(c.rays[s], z_dg[s], c.u_fill[s]))


# ---- (c) standalone kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PHILOX_CASES, ids=IDS)
def test_standalone_kernels(pc, dev):
    c = pc.build()
    r, rays = renderer(pc.K, pc.NC, pc.G), T(c.rays, dev)
    a = at(r, pc.seed, pc.calls).sample_coarse(rays, n_coarse=pc.NC)
    b = r.sample_coarse(rays, n_coarse=pc.NC, u_coarse=T(c.u_coarse, dev))
    assert tuple(a.shape) == (pc.SB, c.rays.shape[1], pc.NC)
    assert pr.compare_bits(a.cpu().numpy(), b.cpu().numpy(), "sample_coarse") == []
    z_dg = T(c.orc_z_dg, dev)
    assert int((z_dg == 0).all(-1).sum()) >= 5 * pc.SB       # (rays with some slots empty: test_philox_ref_host.py counts them per case)
    a = at(r, pc.seed, pc.calls).fill_up_uniform_samples(z_dg, rays)
    b = r.fill_up_uniform_samples(z_dg, rays, u_fill=T(c.u_fill, dev))
    assert pr.compare_bits(a.cpu().numpy(), b.cpu().numpy(), "fill_up_uniform_samples") == []


# ---- (d) production entry points -------------------------------------------------------------------------------------------------
FH, FW = 24, 32                                     # the source maps
GEN_DIMS = dict(d_hidden=256, n_blocks=5, combine_layer=3)
_scenes, _models = {}, {}


def two_scenes():
    from synthetic import synth
    if not _scenes:
        a = synth.make_scene(FH, FW, 3, seed=5, feature_padding=4)
        b = synth.make_scene(FH, FW, 3, seed=6, feature_padding=4, bg_sigma_zero=True, target_yaw=-0.25)
        both = copy.copy(a)
        for name in ("poses", "focal", "c", "depths", "depths_std", "normals", "latent"):
            setattr(both, name, np.concatenate([getattr(a, name), getattr(b, name)], 0))
        _scenes.update(a=a, b=b, both=both)
    return _scenes


def model(kind, dev, fresh=False):
    """'standard' / 'shape_general': scene a; 'both': the standard model on the batch of two scenes"""
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    if kind in _models and not fresh:
        return _models[kind]
    sc = two_scenes()["both" if kind == "both" else "a"]
    if kind == "shape_general":
        m = model_from_scene(sc, synth.make_mlp_weights(3, bias_scale=0.1, d_latent=sc.C, **GEN_DIMS), device=dev, d_latent=sc.C, **GEN_DIMS)
    else:
        m = model_from_scene(sc, synth.make_mlp_weights(6, bias_scale=0.1), device=dev)
    if not fresh:
        _models[kind] = m
    return m


ENTRY_K, ENTRY_NC, ENTRY_G = 16, 200, 5
ENTRY_SEEDS = ((3, 2), (0, 7))                      # call seeds 0xDAA66D2C7DDF7441 (>= 2^63) and 7 (< 2^32)


@pytest.mark.parametrize("kind,precision,binding,route", [
    ("standard", "fp32", "ctypes", "points_mlp"), ("standard", "fp32", "torch_ops", "points_mlp"),
    ("standard", "f16x3", "ctypes", "points_mlp_f16"), ("standard", "f16x3", "torch_ops", "points_mlp_f16"),
    ("shape_general", "fp32", "ctypes", "points_mlp_gen")])
def test_forward_draws_the_samples_of_the_sampler_call(kind, precision, binding, route, dev):
    """forward(noise=None) is the point kernel and the compositing on the samples _sample(noise=None) draws at the same call seed
    -- which (a) to (c) tie to the oracle -- bit for bit: the whole-path entry points launch the very kernels of the stage entry points"""
    sc, m = two_scenes()["a"], model(kind, dev)
    rays = T(sc.target_rays()[:, ::7], dev)
    r = renderer(ENTRY_K, ENTRY_NC, ENTRY_G, white_bkgd=sc.white_bkgd)
    r.precision, r.binding = precision, binding
    seen = []
    for seed, calls in ENTRY_SEEDS:
        assert (pr.call_seed(seed, calls) >= 1 << 63) == (seed == 3)
        with torch.no_grad():
            a = at(r, seed, calls)(m, rays, want_weights=True).fine
            assert r.last_binding == binding and r.last_route == route and r._calls == calls
            z = at(r, seed, calls)._sample(rays, m, ENTRY_K, ENTRY_NC, ENTRY_G, 0.05, None, None)["z"]
            b = r(m, rays, want_weights=True, z_samples=z).fine
        for k in ("rgb", "depth", "weights"):
            print(f"{kind} {precision} {binding} seed {pr.call_seed(seed, calls):#x}: max |d {k}| = {float((a[k] - b[k]).abs().max()):.2e}")
            assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(a.rgb).all() and float(a.weights.sum(-1).max()) > 0.5
        seen.append(z)
    assert not torch.equal(seen[0], seen[1])


# ---- (e) ray numbering -----------------------------------------------------------------------------------------------------------
IMG_H, IMG_W = 20, 28
SCENE_BOX = np.array([[-0.3, -0.35, -0.3], [0.3, 0.25, 0.3]], np.float32)      # inside the synthetic scenes' sphere of radius 0.45


def targets(dev):
    s = two_scenes()
    E = T(np.stack([s["a"].target_extrinsics, s["b"].target_extrinsics]), dev)
    Kt = torch.tensor([[1.2 * IMG_W, 0, IMG_W / 2], [0, 1.2 * IMG_W, IMG_H / 2], [0, 0, 1]], dtype=torch.float32, device=dev).expand(2, 3, 3).contiguous()
    return E, Kt, float(s["a"].near), float(s["a"].far)


def restated(seed, calls, SB, NR, NC, K, G, dev):
    u_c, n_g, u_f = pr.noise(pr.call_seed(seed, calls), SB, NR, NC, K, G)
    return T(u_c, dev), (T(n_g, dev) if G else None), T(u_f, dev)


@pytest.mark.parametrize("binding", ["ctypes", "torch_ops"])
def test_render_image_numbers_its_rays_by_scene_and_pixel(binding, dev):
    from diner_amd import glue
    m = model("both", dev)
    E, Kt, near, far = targets(dev)
    H, W, K, NC, seed, calls = IMG_H, IMG_W, 16, 200, 1, 1            # call seed 0x9E3779B97F4A7C16
    r = renderer(K, NC, 0, white_bkgd=True)
    r.binding = binding
    rgb, depth = at(r, seed, calls).render_image(m, E, Kt, H, W, near, far, return_depth=True)
    assert r.last_binding == binding
    rays = glue.gen_rays(E, Kt, W, H, torch.full((2,), near, device=dev), torch.full((2,), far, device=dev)).view(2, H * W, 8)
    with torch.no_grad():
        ref = at(r, seed, calls)(m, rays, noise=restated(seed, calls, 2, H * W, NC, K, 0, dev)).fine
    assert torch.equal(rgb, ref.rgb.view(2, H, W, 3).permute(0, 3, 1, 2)) and torch.equal(depth, ref.depth.view(2, H, W, 1).permute(0, 3, 1, 2))
    assert float((rgb[0] - rgb[1]).abs().max()) > 0.05 and float(depth.max()) > 0.5
    # G > 0: the frame is forward(noise=None) of the generated rays at the same call seed
    r = renderer(K, NC, 5, white_bkgd=True)
    r.binding = binding
    rgb, depth = at(r, seed, calls).render_image(m, E, Kt, H, W, near, far, return_depth=True)
    with torch.no_grad():
        ref = at(r, seed, calls)(m, rays).fine
    assert torch.equal(rgb, ref.rgb.view(2, H, W, 3).permute(0, 3, 1, 2)) and torch.equal(depth, ref.depth.view(2, H, W, 1).permute(0, 3, 1, 2))


def test_boxed_render_image_numbers_its_rays_by_compact_slot(dev):
    from diner_amd import glue
    m = model("both", dev)
    E, Kt, near, far = targets(dev)
    H, W, K, NC, seed, calls = IMG_H, IMG_W, 16, 200, 3, 1            # call seed 0xDAA66D2C7DDF7440
    r = renderer(K, NC, 0, white_bkgd=True)
    rgb, depth, mask = at(r, seed, calls).render_image(m, E, Kt, H, W, near, far, return_depth=True, bounds=SCENE_BOX, return_mask=True)
    rays, idx, slot, counts = glue.box_rays(E, Kt, W, H, near, far, SCENE_BOX)
    B = rays.shape[1]
    hits = counts.tolist()
    assert r.last_box_hits == hits and hits[0] != hits[1] and all(0.1 * H * W < h < 0.9 * H * W for h in hits)
    with torch.no_grad():
        fine = at(r, seed, calls)(m, rays, noise=restated(seed, calls, 2, B, NC, K, 0, dev)).fine      # row = sb * B + compact slot
    want_rgb, want_depth = glue.frame_from_hits(fine.rgb, fine.depth, slot, H, W, True)
    assert torch.equal(rgb, want_rgb) and torch.equal(depth, want_depth)
    assert float(depth.max()) > 0.5


def test_training_forward_draws_the_inference_calls_samples(dev):
    """forward under autograd, noise=None: the sampler call of the training path takes the call seed the inference call takes"""
    sc, m = two_scenes()["a"], model("standard", dev, fresh=True)
    rays = T(sc.target_rays()[:, ::7], dev)
    r = renderer(ENTRY_K, ENTRY_NC, ENTRY_G, white_bkgd=sc.white_bkgd)
    r.precision = "fp32"
    seed, calls = 3, 2
    with torch.no_grad():
        a = at(r, seed, calls)(m, rays, want_weights=True).fine
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    b = at(r, seed, calls)(m, rays, want_weights=True).fine
    assert b.rgb.requires_grad and r._calls == calls
    for k in ("rgb", "weights"):
        print(f"training forward against the inference call: max |d {k}| = {float((a[k] - b[k].detach()).abs().max()):.2e}")
        np.testing.assert_allclose(b[k].detach().cpu().numpy(), a[k].cpu().numpy(), rtol=0, atol=2e-5)
    with torch.no_grad():                                # and another call seed is another frame
        other = at(r, seed, calls + 1)(m, rays, want_weights=True).fine
    assert float((other.weights - a.weights).abs().max()) > 1e-3
