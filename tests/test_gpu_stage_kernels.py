"""The kernels around the point/MLP kernel, stage by stage on the GPU through the C ABI: the depth-guided sampler (all four
``sampler_kernel<CPL>`` instantiations), the fill-up sort, the in-kernel Philox noise, the alpha compositing, both hand-written
compositing backwards, gen_rays and depth2normal.  Expectations, case sets, comparison functions and bounds are those of
tests/stage_refs.py; tests/test_stage_refs_host.py proves on the CPU that they reproduce the oracle and the goldens and that every
comparison rejects a wrong implementation.  No ray is filtered out of any comparison (no "firm ray" mask).

Sampler, per case: (1) candidates against Oracle.sample_coarse at 2.5e-7 far; (2) the kernel's likelihood against Oracle.likelihood at
1.2e-7 with zero / non-zero flips only below that and on <= 2e-3 of the values; (3) z_dg against ``select_from_likelihood`` of the
kernel's OWN likelihood (just checked elementwise, so the last ulp of erf drops out): short-list as a set bit for bit and hit / no-hit
on every ray, gaussian slots within 4 x the float32 oracle's error + 2e-6; (4) fill-up bit-exact against Oracle.fill_up, the fused
kernel's z bit-equal to it.

Compositing forward against float64 ``composite_ref``: bound = 4 x the worse of two float32 CPU evaluations' error + the stage bars
(1e-6 weights, 2e-6 rgb / depth).  Backward against autograd of ``composite_ref``: float64 in the regular regime (every delta relu(sigma)
<= 9), float32 autograd in the opaque regime (float64 does not round 1 - alpha + 1e-10 as float32 does).  A sigma / far gradient's error is
measured relative to the per-element scale (|dL/dw| T + |S| / keep) delta e in float64, where |dL/dw| and |S| take the absolute value of
every term they sum (the magnitude the gradient is rounded at, whether or not it cancels), + 1e-30; a colour gradient's per unit of d_rgb.
Bound = 4 x the float32 CPU side's normalised error (regular: against float64; opaque: the disagreement of float32 autograd and the
sequential float32 sweep with a correctly rounded exp) + 2e-6.

Largest errors observed over all cases (CPU side: the float32 evaluation the bound is taken from; GPU side: MI355X; sigma / far
gradients in units of their scale, colour gradients per unit of d_rgb); the largest GPU error / bound ratio of any case was 0.31:

    family                                  CPU float32 side   GPU
    gaussian slots, N(0,1) noise            1.99e-06           4.12e-07
    gaussian slots, |n| up to ~1e4          7.93e-05           3.12e-05
    compositing weights                     2.71e-07           3.91e-07
    compositing rgb                         1.00e-06           3.26e-07
    compositing depth                       1.53e-06           8.31e-07
    backward sigma, regular                 9.30e-07           1.56e-06
    backward sigma, opaque                  1.32e-06           2.01e-06
    backward far, regular                   8.44e-07           1.63e-06
    backward far, opaque                    1.34e-06           1.97e-06
    backward colour, regular                8.59e-08           8.59e-08
    backward colour, opaque                 2.68e-07           4.05e-07
"""
import numpy as np
import pytest
import torch

from tests import stage_refs as sr
from tests.stage_refs import COMPOSITE_CASES, SAMPLER_CASES

pytestmark = pytest.mark.gpu
IDS = lambda cases: [c.id for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


_weights = []


def model_for(scene, dev):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    if not _weights:
        _weights.append(synth.make_mlp_weights(1))        # the sampler reads none of them: one set for every stub
    return model_from_scene(scene, _weights[0], device=dev)


def renderer(K, NC, G):
    from diner_amd import NeRFRendererDGS
    return NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G)


# ---- sampler -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SAMPLER_CASES, ids=IDS(SAMPLER_CASES))
def test_sampler_stages(case, dev):
    from oracle.oracle import Oracle
    c = case.oracle()
    K, NC, G, SB = c.K, c.NC, c.G, c.SB
    for s in range(SB):
        assert c.surface[s].sum() >= 20 and (~c.surface[s]).sum() >= 5
    r, m = renderer(K, NC, G), model_for(c.batched_scene(), dev)
    rays = T(c.rays, dev)
    # 1. candidates
    zc = r.sample_coarse(rays, n_coarse=NC, u_coarse=T(c.u_coarse, dev)).cpu().numpy()
    for s in range(SB):
        ref = Oracle(c.scenes[s], None).sample_coarse(c.rays[s], NC, c.u_coarse[s])
        np.testing.assert_allclose(zc[s], ref, rtol=0, atol=2.5e-7 * float(c.rays[s, :, 7].max()))
    # 2.-4. one fused call with the oracle's candidates injected: likelihood, z_dg and the final z
    out = r._sample(rays, m, K, NC, G, 0.05, (None, T(c.n_gauss, dev), T(c.u_fill, dev)), T(c.z_cand, dev), want_dg=True, want_lik=True)
    L, z_dg, z = [out[k].cpu().numpy() for k in ("likelihood", "z_dg", "z")]
    fill = r.fill_up_uniform_samples(out["z_dg"], rays, u_fill=T(c.u_fill, dev)).cpu().numpy()
    for s in range(SB):
        assert sr.compare_likelihood(L[s], c.orc_L[s]) == []
        orc_ref, _ = sr.select_rows(c.orc_L[s], c.z_cand[s], K, G, c.n_gauss[s])
        tol, cpu_err = sr.gauss_bound(c.orc_z_dg[s], orc_ref, K, G)                      # from CPU values alone
        ref, hit = sr.select_rows(L[s], c.z_cand[s], K, G, c.n_gauss[s])
        print(f"{c.id}[{s}]: gaussian slots: oracle err {cpu_err:.2e} bound {tol:.2e} gpu err {sr.gauss_error(z_dg[s], ref, K, G):.2e}; "
              f"surface rays {int(c.surface[s].sum())}/{c.surface[s].size}")
        assert sr.compare_decisions(z_dg[s], ref, hit, K, G, tol) == []
        np.testing.assert_array_equal(fill[s], Oracle(c.scenes[s], None).fill_up(c.rays[s], z_dg[s], c.u_fill[s]))
        np.testing.assert_array_equal(z[s], fill[s])


# ---- Philox ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", sr.PHILOX_NC)
def test_philox_fused_equals_standalone_candidates(NC, dev):
    """with no u_coarse the fused sampler draws the candidates the standalone sample_coarse kernel draws for the same seed"""
    c = sr.SamplerCase(NC, 40, 15).oracle()
    r, m = renderer(c.K, NC, c.G), model_for(c.batched_scene(), dev)
    rays = T(c.rays, dev)
    noise = (None, T(c.n_gauss, dev), T(c.u_fill, dev))
    r.seed, r._calls = 11, 0
    a = r._sample(rays, m, c.K, NC, c.G, 0.05, noise, None, want_dg=True)
    r.seed, r._calls = 11, 0
    zc = r.sample_coarse(rays, n_coarse=NC)
    r.seed, r._calls = 11, 0
    b = r._sample(rays, m, c.K, NC, c.G, 0.05, noise, zc, want_dg=True)
    assert torch.equal(a["z_dg"], b["z_dg"]) and torch.equal(a["z"], b["z"])
    assert int((a["z_dg"] != 0).any(-1).sum()) >= 20


def test_philox_candidates_stratified_and_uniform(dev):
    NC, N = 64, 1600                                     # 102400 draws
    rays = np.zeros((1, N, 8), np.float32)
    rays[..., 5], rays[..., 6], rays[..., 7] = 1, 1.0, 2.5
    r = renderer(8, NC, 0)
    r.seed, r._calls = 5, 0
    z = r.sample_coarse(T(rays, dev), n_coarse=NC).cpu().numpy()[0].astype(np.float64)
    t = (z - 1.0) / 1.5
    j = np.arange(NC) / NC
    tol = 2.5e-7 * 2.5 / 1.5                              # the candidate bar, in units of t
    assert (t >= j - tol).all() and (t < j + 1 / NC + tol).all()
    u = (t - j) * NC
    n = u.size
    # 5 sigma of the sample mean (var 1/12) and of the sample variance (var (1/80 - 1/144)/n) of n uniform draws
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n)
    assert abs(u.var() - 1 / 12) <= 5 * np.sqrt((1 / 80 - 1 / 144) / n)


# ---- compositing -------------------------------------------------------------------------------------------------------------
def _composite(c, dev, rays=None, z=None, rgbsigma=None, weights=True):
    from diner_amd import _lib
    from diner_amd.renderer import _ptr, _stream, check
    rays, z, cc = [T(a, dev) for a in (c.rays if rays is None else rays, c.z if z is None else z, c.rgbsigma if rgbsigma is None else rgbsigma)]
    N, K = z.shape
    w = torch.full((N, K), float("nan"), device=dev) if weights else None
    rgb, depth = torch.full((N, 3), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.lib().diner_composite(_ptr(rays), _ptr(z), _ptr(cc), N, K, int(c.white), _ptr(rgb), _ptr(depth), _ptr(w), _ptr(status),
                                     _stream(dev)), "diner_composite")
    return (None if w is None else w.cpu().numpy()), rgb.cpu().numpy(), depth.cpu().numpy(), int(status.cpu()[0])


@pytest.mark.parametrize("case", COMPOSITE_CASES, ids=IDS(COMPOSITE_CASES))
def test_composite_forward(case, dev):
    c = case.refs()
    w, rgb, depth, status = _composite(c, dev, weights=c.want_weights)
    e = lambda got, i: float(np.abs(got - c.r64[i]).max())
    print(f"{c.id}: cpu err {c.cpu_err} gpu err weights {e(w, 0) if w is not None else None} rgb {e(rgb, 1):.2e} depth {e(depth, 2):.2e}")
    assert sr.compare_composite(w, rgb, depth, c) == []
    assert status == 0                                    # finite input never raises the flag
    if c.N > 1:                                           # a permutation of the rays permutes the outputs bit for bit
        p = np.random.RandomState(1).permutation(c.N)
        w2, rgb2, depth2, _ = _composite(c, dev, c.rays[p], c.z[p], c.rgbsigma[p], weights=c.want_weights)
        assert np.array_equal(rgb2, rgb[p]) and np.array_equal(depth2, depth[p]) and (w is None or np.array_equal(w2, w[p]))


@pytest.mark.parametrize("K,N,where,value", [(65, 5, (4, 64, 3), np.nan), (40, 3, (0, 0, 0), np.inf), (129, 64, (63, 128, 1), -np.inf), (1, 1, (0, 0, 3), np.nan)])
def test_composite_nonfinite_flag(K, N, where, value, dev):
    c = sr.CompositeCase(K, N, True, "moderate", "uniform", "rgb").build()
    assert _composite(c, dev)[3] == 0
    bad = c.rgbsigma.copy()
    bad[where] = value
    assert _composite(c, dev, rgbsigma=bad)[3] == 1      # DINER_STATUS_NONFINITE (include/diner_hip.h)
    assert _composite(c, dev, rgbsigma=bad, weights=False)[3] == 1


def _backward(c, dev, far, d_depth, d_weights):
    from diner_amd import _lib
    from diner_amd.renderer import _ptr, _stream, check
    rays, z, cc, g = [T(a, dev) for a in (c.rays, c.z, c.rgbsigma, c.d_rgb)]
    gd, gw = T(d_depth, dev), T(d_weights, dev)
    N, K = z.shape
    out = torch.full((N, K, 4), float("nan"), device=dev)
    L = _lib.lib()
    if far:
        d_far = torch.full((N,), float("nan"), device=dev)
        check(L.diner_composite_backward_far(_ptr(rays), _ptr(z), _ptr(cc), _ptr(g), _ptr(gd), _ptr(gw), N, K, int(c.white), _ptr(out), _ptr(d_far),
                                             _stream(dev)), "diner_composite_backward_far")
        return out.cpu().numpy(), d_far.cpu().numpy()
    check(L.diner_composite_backward(_ptr(rays), _ptr(z), _ptr(cc), _ptr(g), _ptr(gd), _ptr(gw), N, K, int(c.white), _ptr(out), _stream(dev)),
          "diner_composite_backward")
    return out.cpu().numpy(), None


@pytest.mark.parametrize("case", COMPOSITE_CASES, ids=IDS(COMPOSITE_CASES))
def test_composite_backward(case, dev):
    """both entry points against autograd of composite_ref (the cotangents a case does not have are passed as NULL), d_far included;
    the two kernels are the same arithmetic: d_rgbsigma bit-identical"""
    c = case.refs()
    if c.opaque:
        assert c.opaque_followed(8) >= 1
    else:
        assert not c.keep_is_eps().any()
    a, _ = _backward(c, dev, False, c.d_depth, c.d_weights)
    b, d_far = _backward(c, dev, True, c.d_depth, c.d_weights)
    print(f"{c.id}: {'opaque' if c.opaque else 'regular'}: cpu err {c.cpu_gerr} bound {c.gbound} gpu err {sr.grad_errors(b, d_far, c)}")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sr.compare_composite_grads(a, None, c) == []
    assert sr.compare_composite_grads(b, d_far, c) == []


# ---- gen_rays / depth2normal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sr.GLUE_SIZES)
def test_gen_rays_and_depth2normal_sizes(W, H, dev):
    from diner_amd import glue as hip
    g = sr.glue_case(W, H)
    rays = hip.gen_rays(T(g["extrinsics"], dev), T(g["intrinsics"], dev), W, H, T(g["z_near"], dev), T(g["z_far"], dev)).cpu().numpy()
    assert rays.shape == (3, H, W, 8)
    for b in range(3):
        ref = sr.gen_rays64(g["extrinsics"][b], g["intrinsics"][b], W, H, g["z_near"][b], g["z_far"][b])
        np.testing.assert_allclose(rays[b], ref, rtol=0, atol=3e-7)
    n = hip.depth2normal(T(g["dmap"], dev), T(g["intrinsics"], dev)).cpu().numpy()
    ref = sr.depth2normal64(g["dmap"], g["intrinsics"])
    assert np.array_equal(np.isnan(n), np.isnan(ref))
    np.testing.assert_allclose(np.nan_to_num(n), np.nan_to_num(ref), rtol=0, atol=2e-5)
    assert np.all(n.transpose(0, 2, 3, 1)[g["dmap"][:, 0] == 0] == 0)
