"""The NOVEL renderer on the GPU (diner_amd/novel.py; csrc/sampler_points.hip): its sampler of deformed candidates against the host
restatement of tests/novel_sampler_ref.py, its compositing against what the unmodified reference recorded, and the autograd of that
compositing.  tests/test_novel_sampler_host.py proves the restatement on the CPU and that the offsets change the likelihood on at least
a quarter of the rays of every case here.  No ray is filtered out of any comparison.

Sampler, per case of novel_sampler_ref.GRID (every ``sampler_points_kernel<CPL>`` on both sides of its boundary; V = 1031 takes the
pruned search), with dense noise: (1) the candidates' points bit-equal to the restated deformation; (2) the likelihood against the
restated one at the bar of ``compare_likelihood``; (3) the same likelihood bit-equal to what the EXISTING sampler kernel returns on one
pseudo-ray per candidate (origin = the point, near = 0, far = (far - near) / NC, z = 0): the same device function on the same operands;
(4) z_dg against ``select_rows`` of the kernel's own likelihood: short-list as a set and hit / no-hit on every ray, gaussian slots
within 4 x the float32 oracle's error on the same rays undeformed + 2e-6 (the moments are the same sums over the same depths); (5) z
against ``fill_up_f32``; (6) a second run returns the same bits.
"""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import knn_ref
from tests import novel_sampler_ref as N
from tests import philox_ref as pr
from tests import stage_refs as sr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "novel_sampler.npz"
IDS = lambda cases: [c.id for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


class Model:
    """all the NOVEL renderer asks of a model: the cameras, the encoder's three maps, and a call (no mlp_fine, no poscode)"""

    def __init__(self, scene, dev, fn=None):
        self.poses, self.focal, self.c, self.image_shape = [T(getattr(scene, k), dev) for k in ("poses", "focal", "c", "image_shape")]
        self.encoder = SimpleNamespace(**{k: T(getattr(scene, k), dev) for k in ("depths", "depths_std", "normals")})
        self.fn, self.calls = fn, []

    def __call__(self, *pts, viewdirs=None):
        self.calls.append(tuple(pts) + (viewdirs,))
        return self.fn(*pts, viewdirs)


def standin(in_pts, gen_pts, *rest):
    """tools/gen_novel_sampler_golden.py's stand-in model, restated in torch (``rest``: [points,] viewdirs)"""
    a, b, d = in_pts, gen_pts, rest[-1]
    rgb = 0.5 + 0.5 * torch.sin(3.0 * a + 2.0 * b[..., [1, 2, 0]] + d)
    r2 = (a * a).sum(-1) + 0.5 * (b * b).sum(-1)
    sigma = 12.0 * torch.exp(-4.0 * r2) * (1.2 + torch.cos(5.0 * b[..., 0] + d[..., 2])) - 1.0
    return torch.cat([rgb, sigma[..., None]], -1)


def renderer(K, NC, G, **kw):
    from diner_amd.novel import NeRFRendererDGS
    return NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, **kw)


def at(r, seed, calls=1):
    r.seed, r._calls = seed, calls - 1
    return r


def sample(r, c, m, dev, noise):
    z_dg, out = r.sample_depthguided(T(c.rays, dev), m, c.K, c.NC, T(c.vertices, dev), T(c.offsets, dev), n_gaussian=c.G, noise=noise,
                                     return_internals=True)
    assert out["z_dg"] is z_dg
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


_weights = []


def existing_sampler_likelihood(c, xyz, dev):
    """the existing sampler kernel (diner_sample_depthguided) on the pseudo-rays of the candidates -> [SB,NR,NC]"""
    from diner_amd import NeRFRendererDGS
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    if not _weights:
        _weights.append(synth.make_mlp_weights(1))        # the sampler reads none of them
    m = model_from_scene(c.batched_scene(), _weights[0], device=dev)
    p = np.stack([N.pseudo_rays(c.rays[s], xyz[s]) for s in range(c.SB)])
    _, out = NeRFRendererDGS(n_samples=1, n_depth_candidates=1, n_gaussian=0).sample_depthguided(
        T(p, dev), m, 1, 1, n_gaussian=0, z_cand=torch.zeros((c.SB, p.shape[1], 1), device=dev), return_internals=True)
    return out["likelihood"].cpu().numpy().reshape(c.SB, c.NR, c.NC)


# ---- the sampler, dense noise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.GRID, ids=IDS(N.GRID))
def test_sampler_of_deformed_candidates(case, dev):
    from oracle.oracle import Oracle
    c = case.refs()
    K, NC, G, SB = c.K, c.NC, c.G, c.SB
    r, m = renderer(K, NC, G), Model(c.batched_scene(), dev)
    noise = (T(c.u_coarse, dev), T(c.n_gauss, dev), T(c.u_fill, dev))
    out = sample(r, c, m, dev, noise)
    assert out["xyz_cand"].shape == (SB, c.NR, NC, 3) and out["z"].shape == (SB, c.NR, K)
    for s in range(SB):
        np.testing.assert_allclose(out["z_cand"][s], c.z_cand[s], rtol=0, atol=2.5e-7 * float(c.rays[s, :, 7].max()))
    # the restatement on the KERNEL's candidates (1 ulp from the oracle's at most): the points are then bit for bit
    xyz, _ = N.deformed_candidates(c.rays, out["z_cand"], c.vertices, c.offsets)
    assert pr.compare_bits(out["xyz_cand"], xyz, "deformed candidates") == []
    L = out["likelihood"]
    assert pr.compare_bits(L, existing_sampler_likelihood(c, xyz, dev), "likelihood against the existing sampler kernel") == []
    for s, sc in enumerate(c.scenes):
        assert (c.L[s] > 0).any(-1).sum() >= 5 and (c.L[s] == 0).all(-1).sum() >= 5
        restated = N.likelihood(sc, c.rays[s], xyz[s]).astype(np.float64)
        assert sr.compare_likelihood(L[s], restated) == []
        orc_z, orc_L = Oracle(sc, None).sample_depthguided(c.rays[s], c.z_cand[s], K, G, c.n_gauss[s], want_L=True)
        tol, cpu_err = sr.gauss_bound(orc_z, sr.select_rows(orc_L, c.z_cand[s], K, G, c.n_gauss[s])[0], K, G)     # from CPU values alone
        ref, hit = sr.select_rows(L[s], out["z_cand"][s], K, G, c.n_gauss[s])
        print(f"{c.id}[{s}]: gaussian slots: oracle err {cpu_err:.2e} bound {tol:.2e} gpu err {sr.gauss_error(out['z_dg'][s], ref, K, G):.2e}; "
              f"rays with a likelihood {int((L[s] > 0).any(-1).sum())}/{c.NR}; max |L - restated| "
              f"{np.abs(L[s].astype(np.float64) - restated).max():.2e}")
        assert sr.compare_decisions(out["z_dg"][s], ref, hit, K, G, tol) == []
        assert pr.compare_bits(out["z"][s], sr.fill_up_f32(out["z_dg"][s], c.rays[s], c.u_fill[s]), "z against the fill-up") == []
    again = sample(r, c, m, dev, noise)
    for k in ("z_cand", "xyz_cand", "likelihood", "z_dg", "z"):
        assert pr.compare_bits(again[k], out[k], f"second run: {k}") == []


# ---- the in-kernel noise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.PHILOX_CASES, ids=IDS(N.PHILOX_CASES))
def test_noise_is_the_stream_contract_of_one_seed(case, dev):
    """noise=None: the candidates are philox_ref's coarse stream of the call's seed bit for bit; one stream in the kernel at a time
    against all three injected, as tests/test_gpu_philox.py (a) checks diner_sample_depthguided"""
    c = case.build()
    K, NC, G, SB, keep = c.K, c.NC, c.G, c.SB, c.K - c.G
    seed, calls = 3, 2                                    # call seed 0xDAA66D2C7DDF7441: both key words set
    r, m = renderer(K, NC, G), Model(c.batched_scene(), dev)
    u_c, n_g, u_f = [T(a, dev) for a in pr.noise(pr.call_seed(seed, calls), SB, c.NR, NC, K, G)]
    dn, n32_err = pr.delta_n(pr.call_seed(seed, calls), SB * c.NR, G)
    ref = sample(at(r, seed, calls), c, m, dev, (u_c, n_g, u_f))
    assert ref["seed"] == pr.call_seed(seed, calls) and r._calls == calls          # one seed per call
    assert int((ref["z_dg"] == 0).all(-1).sum()) >= 5 and int((ref["z_dg"] != 0).any(-1).sum()) >= 10
    full = sample(at(r, seed, calls), c, m, dev, None)
    assert pr.compare_bits(full["z_cand"], ref["z_cand"], "noise=None: z_cand") == []
    assert pr.compare_bits(full["likelihood"], ref["likelihood"], "noise=None: likelihood") == []
    got = sample(at(r, seed, calls), c, m, dev, (None, n_g, u_f))
    for k in ("z_cand", "xyz_cand", "likelihood", "z_dg", "z"):
        assert pr.compare_bits(got[k], ref[k], f"candidates in the kernel: {k}") == []
    got = sample(at(r, seed, calls), c, m, dev, (u_c, n_g, None))
    for k in ("z_dg", "z"):
        assert pr.compare_bits(got[k], ref[k], f"fill-up in the kernel: {k}") == []
    for what, got in (("gaussian in the kernel", sample(at(r, seed, calls), c, m, dev, (u_c, None, u_f))), ("noise=None", full)):
        assert pr.compare_bits(got["z_dg"][..., :keep], ref["z_dg"][..., :keep], f"{what}: short-list") == []
        for s in range(SB):
            gstd = pr.gauss_std(ref["likelihood"][s], ref["z_cand"][s], K, G)
            bad_g, err_g, tol = pr.compare_gauss(got["z_dg"][s][:, keep:], ref["z_dg"][s][:, keep:], gstd, dn, "gaussian slots")
            bad_z, err_z, _ = pr.compare_gauss(got["z"][s], ref["z"][s], gstd, dn, "z")
            print(f"{c.id}[{s}] {what}: max |n32 - n64| {n32_err:.2e} bound {tol:.2e} gpu err gaussian slots {err_g:.2e} z {err_z:.2e}")
            assert bad_g == [] and bad_z == []
    other = sample(at(r, seed, calls + 1), c, m, dev, None)
    assert not np.array_equal(other["z_cand"], full["z_cand"])


# ---- the copy of the decisions against the ray sampler's own --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.PHILOX_CASES, ids=IDS(N.PHILOX_CASES))
def test_undeformed_points_give_the_ray_samplers_bits(case, dev):
    """xyz = o + z d (a multiplication, then an addition, as sampler_kernel forms it): diner_sample_depthguided_points and
    diner_sample_depthguided with the same injected depths return bit-equal likelihood, z_dg and z, for one NC per instantiation, with
    dense noise and with the kernels' own gaussian and fill-up streams.  sampler_blocks.hpp's shortlist_gauss_fill is a copy of
    sampler_kernel's statements: this is what keeps the two alike."""
    import ctypes as C
    from diner_amd import NeRFRendererDGS, _lib
    from diner_amd.novel import _MapsModel
    from diner_amd.renderer import _ptr, _stream, check
    c = case.refs()
    K, NC, G, SB, NR = c.K, c.NC, c.G, c.SB, c.NR
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G)
    m = Model(c.batched_scene(), dev)
    sc, _keep = r._scene(_MapsModel(m), need_latent=False)
    cfg = r._cfg(K, NC, G)
    rays, z_cand = T(c.rays, dev), T(c.z_cand, dev)
    xyz = (rays[..., None, :3] + z_cand[..., None] * rays[..., None, 3:6]).contiguous()
    assert pr.compare_bits(xyz.cpu().numpy().reshape(SB, NR * NC, 3), knn_ref.ray_points(c.rays, c.z_cand), "o + z d") == []
    L, st = _lib.lib(), _stream(dev)
    for what, n_g, u_f in (("dense noise", T(c.n_gauss, dev), T(c.u_fill, dev)), ("Philox streams 1 and 2", None, None)):
        a, b = [[torch.full(s, float("nan"), device=dev) for s in ((SB, NR, K), (SB, NR, K), (SB, NR, NC))] for _ in range(2)]
        check(L.diner_sample_depthguided(C.byref(sc), _ptr(rays), NR, C.byref(cfg), None, _ptr(n_g), _ptr(u_f), _ptr(z_cand), 77,
                                         _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), st), "diner_sample_depthguided")
        check(L.diner_sample_depthguided_points(C.byref(sc), _ptr(rays), _ptr(z_cand), _ptr(xyz), NR, C.byref(cfg), _ptr(n_g), _ptr(u_f), 77,
                                                _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), st), "diner_sample_depthguided_points")
        for k, x, y in zip(("z", "z_dg", "likelihood"), a, b):
            assert pr.compare_bits(y.cpu().numpy(), x.cpu().numpy(), f"{what}: {k}") == []
        assert int((a[1] != 0).any(-1).sum()) >= 10 and int((a[1] == 0).all(-1).sum()) >= 5
        if G:
            assert int((a[1][..., K - G:] != 0).any(-1).sum()) >= 10          # gaussian slots drawn


# ---- compositing and forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(N.GOLDEN_CASES))
def test_composite_meets_the_reference(name, dev):
    """the recorded filled z, the stand-in model in torch: the unmodified reference's weights / rgb / depth at the project's 1e-4"""
    g = np.load(GOLDEN)
    ix = json.loads(str(g["index"]))[name]
    c = N.GOLDEN_CASES[name].build()
    rec = lambda k: g[f"{name}.{k}"]
    r, m = renderer(c.K, c.NC, c.G, white_bkgd=ix["white_bkgd"]), Model(c.batched_scene(), dev, standin)
    w, rgb, depth = r.composite(m, T(rec("rays"), dev), T(rec("z"), dev), T(rec("vertices"), dev), T(rec("offsets_in"), dev),
                                T(rec("offsets_gen"), dev))
    r.check_finite()
    for k, got in (("weights", w), ("rgb", rgb), ("depth", depth)):
        print(f"{name}: max |d {k}| = {np.abs(got.cpu().numpy() - rec(k)).max():.2e}")
        np.testing.assert_allclose(got.cpu().numpy(), rec(k), rtol=0, atol=1e-4)
    assert len(m.calls) == 1 and len(m.calls[0]) == 3 and float(w.sum(-1).max()) > 0.5


def test_forward_returns_the_reference_object(dev):
    c = N.NovelCase(256, 16, 5, 3, V=1031, SB=2).build()
    r, m = renderer(c.K, c.NC, c.G, eval_batch_size=1000), Model(c.batched_scene(), dev, standin)
    rays, v = T(c.rays, dev), T(c.vertices, dev)
    o_in, o_gen = T(c.offsets, dev), T(c.offsets[::-1], dev)
    with torch.no_grad():
        out = at(r, 7)(m, rays, v, o_in, o_gen)
        assert set(out.keys()) == {"fine"} and set(out.fine.keys()) == {"rgb", "depth"}
        assert out.fine.rgb.shape == (2, c.NR, 3) and out.fine.depth.shape == (2, c.NR)
        chunk = (1000 - 1) // 2 + 1                       # the reference's chunks of points per scene
        assert [t[0].shape[1] for t in m.calls] == [chunk] * (c.NR * c.K // chunk) + [c.NR * c.K % chunk] * bool(c.NR * c.K % chunk)
        w = at(r, 7)(m, rays, v, o_in, o_gen, want_weights=True).fine
        assert set(w.keys()) == {"rgb", "depth", "weights"} and w.weights.shape == (2, c.NR, c.K)
        assert torch.equal(w.rgb, out.fine.rgb) and torch.equal(w.depth, out.fine.depth)      # the same call seed: the same frame
        # ... which is composite on the samples sample_depthguided + fill_up_uniform_samples return at that seed
        z_dg, internals = at(r, 7).sample_depthguided(rays, m, c.K, c.NC, v, o_in, return_internals=True)
        assert torch.equal(r.composite(m, rays, internals["z"], v, o_in, o_gen)[1], out.fine.rgb)
        u_f = T(pr.u_fill(pr.call_seed(7, 1), 2 * c.NR, c.K).reshape(2, c.NR, c.K), dev)
        assert torch.equal(r.fill_up_uniform_samples(z_dg, rays, u_fill=u_f), internals["z"])
    assert torch.isfinite(out.fine.rgb).all() and float(w.weights.sum(-1).max()) > 0.5


def test_pass_points_hands_the_model_three_point_tensors(dev):
    c = N.NovelCase(64, 8, 4, 3).build()
    r, m = renderer(c.K, c.NC, c.G, pass_points=True), Model(c.batched_scene(), dev, standin)
    z = np.sort(1.0 + 1.5 * np.random.RandomState(0).random_sample((1, c.NR, c.K)), -1).astype(np.float32)
    off2 = c.offsets[:, ::-1].copy()
    with torch.no_grad():
        r.composite(m, T(c.rays, dev), T(z, dev), T(c.vertices, dev), T(c.offsets, dev), T(off2, dev))
    (a, b, p, d), = m.calls
    pts = knn_ref.ray_points(c.rays, z)
    idx, _ = knn_ref.nearest_batch(pts, c.vertices)
    assert pr.compare_bits(p.cpu().numpy(), pts, "undeformed points") == []
    assert pr.compare_bits(a.cpu().numpy(), knn_ref.deform(pts, idx, c.offsets), "in-deformed points") == []
    assert pr.compare_bits(b.cpu().numpy(), knn_ref.deform(pts, idx, off2), "gen-deformed points") == []
    assert np.array_equal(d.cpu().numpy(), np.repeat(c.rays[:, :, None, 3:6], c.K, 2).reshape(1, -1, 3))
    m.calls.clear()
    renderer(c.K, c.NC, c.G).composite(m, T(c.rays, dev), T(z, dev), T(c.vertices, dev), T(c.offsets, dev), T(off2, dev))
    assert len(m.calls[0]) == 3                            # pass_points=False: (in, gen, viewdirs)


# ---- autograd of the compositing ---------------------------------------------------------------------------------------------------------------
GRAD_CASES = [sr.CompositeCase(1, 5, True, "moderate", "uniform", "rgbdw"), sr.CompositeCase(64, 64, False, "opaque_one", "repeated", "rgbd"),
              sr.CompositeCase(300, 64, True, "negative", "last_beyond_far", "rgb")]


@pytest.mark.parametrize("case", GRAD_CASES, ids=IDS(GRAD_CASES))
def test_composite_autograd(case, dev):
    """torch.autograd.grad through composite(): the direct diner_composite_backward call bit for bit, composite_ref's gradient under
    compare_composite_grads.  The model hands out a leaf rgb-sigma in one chunk: with several, autograd sums the chunks' zero-padded
    gradients into the leaf, which turns the backward's -0.0 (a zero weight times a negative cotangent) into +0.0."""
    from diner_amd import _lib
    from diner_amd.renderer import _ptr, _stream, check
    c = case.refs()
    N_, K = c.z.shape
    leaf = T(c.rgbsigma, dev).view(1, N_ * K, 4).requires_grad_(True)
    pos = [0]

    def fn(a, b, d):
        s = pos[0]
        pos[0] += a.shape[1]
        return leaf[:, s:pos[0]]

    sc = N.NovelCase(64, 8, 4, 1).build()
    m = Model(sc.batched_scene(), dev, fn)
    r = renderer(K, 64, 0, white_bkgd=c.white)
    rays, z = T(c.rays[None], dev), T(c.z[None], dev)
    v, o = T(sc.vertices, dev), T(sc.offsets, dev)
    w, rgb, depth = r.composite(m, rays, z, v, o, o)
    assert len(m.calls) == 1 and w.requires_grad and rgb.requires_grad
    assert sr.compare_composite(w[0].detach().cpu().numpy(), rgb[0].detach().cpu().numpy(), depth[0].detach().cpu().numpy(), c) == []
    g, gd, gw = [T(a, dev) for a in c.cotangents()]
    loss = (rgb[0] * g).sum()
    if gd is not None:
        loss = loss + (depth[0] * gd).sum()
    if gw is not None:
        loss = loss + (w[0] * gw).sum()
    got, = torch.autograd.grad(loss, [leaf])
    direct = torch.full((N_, K, 4), float("nan"), device=dev)
    check(_lib.lib().diner_composite_backward(_ptr(rays), _ptr(z), _ptr(leaf.detach()), _ptr(g), _ptr(gd), _ptr(gw), N_, K, int(c.white),
                                              _ptr(direct), _stream(dev)), "diner_composite_backward")
    if K == 1:          # the hand-written backward is once-differentiable: its result carries no graph, so a double backward raises
        first, = torch.autograd.grad((r.composite(m_again(m, pos), rays, z, v, o, o)[1][0] * g).sum(), [leaf], create_graph=True)
        with pytest.raises(RuntimeError, match="does not require grad|once_differentiable|differentiated twice"):
            torch.autograd.grad(first.sum(), [leaf])
    got = got.view(N_, K, 4).cpu().numpy()
    assert pr.compare_bits(got, direct.cpu().numpy(), "autograd against the direct backward") == []
    print(f"{c.id}: gradient errors {sr.grad_errors(got, c.grad_ref[4], c)} bounds {c.gbound}")
    assert sr.compare_composite_grads(got, None, c) == []


def m_again(m, pos):
    """the leaf-handing model of test_composite_autograd, rewound for another composite call"""
    pos[0] = 0
    return m


def test_rays_that_require_grad_raise(dev):
    c = N.NovelCase(64, 8, 4, 1).build()
    r, m = renderer(c.K, c.NC, c.G), Model(c.batched_scene(), dev, standin)
    rays = T(c.rays, dev).requires_grad_(True)
    z = T(np.sort(1.0 + 1.5 * np.random.RandomState(0).random_sample((1, c.NR, c.K)), -1), dev)
    with pytest.raises(NotImplementedError, match="training"):
        r.composite(m, rays, z, T(c.vertices, dev), T(c.offsets, dev), T(c.offsets, dev))
    with pytest.raises(NotImplementedError, match="training"):
        r(m, rays, T(c.vertices, dev), T(c.offsets, dev), T(c.offsets, dev))
    # ... and so do vertices or offsets: data, as in the reference, never silently left without a gradient
    rays = T(c.rays, dev)
    for hole in range(3):
        args = [T(c.vertices, dev), T(c.offsets, dev), T(c.offsets, dev)]
        args[hole].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="data"):
            r.composite(m, rays, z, *args)
        with pytest.raises(NotImplementedError, match="data"):
            r(m, rays, *args)
        with torch.no_grad():
            r.composite(m, rays, z, *args)
        m.calls.clear()
    assert m.calls == []
