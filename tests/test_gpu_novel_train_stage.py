"""The two kernels of the NOVEL point model's training path (csrc/train_novel.hip), alone on the GPU through the C ABI:

(a) ``diner_train_point_inputs_novel``: in_out, zlat, taps and gen_taps against float64.  The encoder's side is tests/train_stage_refs.py's
    ``TrainStageCase.refs`` (the points handed over are fp32(o + z d), the kernel's own first step on the plain path, the viewdirs the ray
    directions), the general side ``point_inputs_ref`` on a one-view scene made of the general camera and gen_latent, with the points as
    ray origins (z = 0).  Bounds: those of tests/test_gpu_train_stage_kernels.py::test_point_inputs_gen_forward -- the families'
    ``bounds`` of ``refs`` for in_out and taps, the same recipe (4 x the worse float32 CPU evaluation's error + an ulp of the magnitude)
    for the general lookup and its taps; zlat, the sum of the two lookups: the two lookups' bounds + one ulp of the sum's magnitude (the
    one more rounding).  Every 4-tap mode; sb = 1 of a two-scene batch, with its own general camera.
(b) with gen_latent = 0, xyz_gen = xyz_in = o + z d (torch, fp32) and viewdirs = d: in_out, zlat and taps are
    ``diner_train_point_inputs_gen``'s, bit for bit.  (zeros padding: equal as values -- where every tap of a row has weight 0 the
    encoder's lookup can be -0, and -0 + the general lookup's +0 is +0 in any IEEE arithmetic.)
(c) ``diner_train_novel_gen_scatter`` against float64 sums (the view sum, then ``scatter_plain``) at 2e-4 max|ref|: P in {1, 63, 65, 200} x
    NV in {1, 3, 4} x C in {8, 72, 512}; all points on one texel; a lone point; all taps of weight 0 (the buffer stays exactly 0); texels
    no tap names stay exactly 0.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import train_stage_refs as ts
from tests.test_gpu_train_stage_kernels import NAN, P_, ST, T, call, index_of, on_device
from tests.train_stage_refs import MODES, MODE_IDS

pytestmark = pytest.mark.gpu
F32 = np.float32
GEN_HW = (4, 6)                      # the general map: another size than either encoder map
GEN_IMAGE = (14.0, 9.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---- the general side of a case ---------------------------------------------------------------------------------------------------------------
_general = {}


def general(case, sb):
    """scene ``sb``'s general camera, gen_latent (one for all scenes) and xyz_gen [P,3], seeded; every general projection at least
    2.5 DECISION_MARGIN texels from a decision boundary of the general map (the offenders are re-drawn), a third to a half of them outside the map"""
    key = (case.id, sb)
    if key in _general:
        return _general[key]
    c = case.build()
    rs = np.random.RandomState(c.seed + 77)
    hg, wg = GEN_HW
    glat = rs.uniform(-1, 1, (1, c.C, hg, wg)).astype(F32)                       # (drawn first: the same for every sb)
    rs = np.random.RandomState(c.seed + 78 + sb)
    pose = np.eye(4)
    pose[:3, :3] = ts._rot(*rs.uniform(-0.35, 0.35, 3))
    pose[:3, 3] = [rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2), 2.3 + rs.uniform(-0.2, 0.2)]
    iw, ih = GEN_IMAGE
    sxg, syg = (wg - 2 * c.fpad) / wg, (hg - 2 * c.fpad) / hg                 # (the focal lengths undo the feature padding's shrink)
    scene = SimpleNamespace(poses=pose[None].astype(F32), focal=np.array([[iw * 1.3 / sxg, ih * 1.1 / syg]], F32) * F32(rs.uniform(0.9, 1.1)),
                            c=np.array([[iw / 2 + rs.uniform(-1, 1), ih / 2 + rs.uniform(-1, 1)]], F32), image_shape=np.array([iw, ih], F32),
                            depths=np.full((1, 2, 2), 2.0, F32), latent=glat, feature_padding=F32(c.fpad), freq_factor=F32(6.28), num_freqs=c.F)
    rays, z = torch.from_numpy(c.rays[sb]), torch.from_numpy(c.z[sb])
    xyz_in = (rays[:, None, :3] + z[..., None] * rays[:, None, 3:6]).reshape(c.P, 3).numpy()      # fp32, nerf_renderer.py:304
    draw = lambda n: (rs.uniform(-0.08, 0.08, (n, 3)) + 0.01).astype(F32)
    xyz_gen = xyz_in + draw(c.P)
    as_rays = lambda p: np.concatenate([p, np.zeros((len(p), 5), F32)], -1)
    z0 = np.zeros((c.P, 1), F32)
    for _ in range(200):
        f = ts.point_inputs_ref(scene, as_rays(xyz_gen), z0, coords_only=True)
        viol = np.zeros(c.P, bool)
        for x in (f.ix, f.iy):
            x2 = x.numpy() * 2.0
            viol |= (np.abs(x2 - np.round(x2)) < 2.5 * ts.DECISION_MARGIN * 2.0).any(0)
        if not viol.any():
            break
        xyz_gen[viol] = xyz_in[viol] + draw(int(viol.sum()))
    assert not viol.any()
    out = SimpleNamespace(scene=scene, xyz_in=xyz_in, xyz_gen=xyz_gen, rays=as_rays(xyz_gen), z0=z0, refs={})
    _general[key] = out
    return out


def general_refs(case, sb, mode):
    """float64 expectations of the general lookup and its taps with test_point_inputs_gen_forward's bounds, computed once"""
    g = general(case, sb)
    if mode not in g.refs:
        P = case.P
        f64 = ts.point_inputs_ref(g.scene, g.rays, g.z0, mode, torch.float64)
        runs = [ts.point_inputs_ref(g.scene, g.rays, g.z0, mode, torch.float32, V) for V in (0, 1)]
        for f in runs:
            assert torch.equal(f.idx, f64.idx)
        flat = lambda a: a.detach().double().numpy().reshape(P, -1)
        r = SimpleNamespace(zlat=flat(f64.zlat), idx=f64.idx.numpy().reshape(P, 4), wt=flat(f64.wt), bounds={})
        for name in ("zlat", "wt"):
            cpu = max(float(np.abs(flat(getattr(f, name)) - getattr(r, name)).max()) for f in runs)
            r.bounds[name] = ts.MARGIN * cpu + ts.EPS32 * float(np.abs(getattr(r, name)).max())
        ix, iy = f64.ix.numpy(), f64.iy.numpy()
        r.outside = float(((ix < 0) | (ix > GEN_HW[1] - 1) | (iy < 0) | (iy > GEN_HW[0] - 1)).mean())
        g.refs[mode] = r
    return g.refs[mode]


def gen_struct(case, d, sb_count, glat_nhwc, dev, keep):
    """DinerNovelGen of all scenes' general cameras"""
    from diner_amd import _lib
    gs = [general(case, sb) for sb in range(sb_count)]
    poses, focal, c = (T(np.stack([getattr(g.scene, k)[0] for g in gs]), dev) for k in ("poses", "focal", "c"))
    keep += [poses, focal, c, glat_nhwc]
    s = _lib.DinerNovelGen()
    s.latent, s.h, s.w, s.C = glat_nhwc.data_ptr(), GEN_HW[0], GEN_HW[1], case.C
    s.poses, s.focal, s.c = poses.data_ptr(), focal.data_ptr(), c.data_ptr()
    s.image_w, s.image_h = GEN_IMAGE
    return s


def run_novel(case, mode, dev, sb=0, zero_gen=False, same_points=False):
    """-> in [R, ld], zlat [R, C], idx, wt, gen idx [P,4], gen wt [P,4] (numpy)"""
    d = on_device(case, dev)
    c = d.case
    keep = []
    glat = general(c, 0).scene.latent[0].transpose(1, 2, 0)
    gen = gen_struct(c, d, c.SB, T(np.zeros_like(glat) if zero_gen else glat, dev), dev, keep)
    xi = T(np.stack([general(c, s).xyz_in for s in range(c.SB)]), dev)
    xg = xi if same_points else T(np.stack([general(c, s).xyz_gen for s in range(c.SB)]), dev)
    vd = d.t["rays"][:, :, None, 3:6].expand(-1, -1, c.K, -1).reshape(c.SB, c.P, 3).contiguous()
    inp, zl, taps, gtaps = (torch.full((rows, n), NAN, device=dev) for rows, n in ((d.R, c.ld_in), (d.R, c.C), (d.R, 8), (c.P, 8)))
    ix = index_of(mode)
    call("diner_train_point_inputs_novel", C.byref(d.scene), None if mode == MODES[0] else C.byref(ix), P_(d.t["lat_nhwc"]), C.byref(gen),
         P_(xi), P_(xg), P_(vd), c.P, sb, P_(inp), c.ld_in, P_(zl), P_(taps), P_(gtaps), ST(dev))
    tp, gp = taps.cpu(), gtaps.cpu()
    ints = lambda t: t[:, :4].contiguous().view(torch.int32).numpy()
    return inp.cpu().numpy(), zl.cpu().numpy(), ints(tp), tp[:, 4:].numpy(), ints(gp), gp[:, 4:].numpy()


# ---- (a) against float64 ----------------------------------------------------------------------------------------------------------------------
def check_novel(case, mode, dev, sb):
    c = case.build()
    r, g = c.refs(mode, sb=sb, backward=False), general_refs(c, sb, mode)
    inp, zl, idx, wt, gidx, gwt = run_novel(c, mode, dev, sb=sb)
    assert ts.compare_taps(idx, wt, r.idx, r.wt, r.bounds["wt"], c.h * c.w) == []
    assert ts.compare_inputs(inp, r.in55, r.bounds, c.F) == []
    assert ts.compare_taps(gidx, gwt, g.idx, g.wt, g.bounds["wt"], GEN_HW[0] * GEN_HW[1]) == []
    ref = r.zlat + np.tile(g.zlat, (c.NV, 1))                                   # rows are view-major: the general lookup repeats per view
    bound = r.bounds["zlat"] + g.bounds["zlat"] + ts.EPS32 * float(np.abs(ref).max())
    print(f"FIG {c.id} {mode} sb{sb}: zlat {np.abs(zl - ref).max():.3e} bound {bound:.3e}; gen weights {np.abs(gwt - g.wt).max():.3e} bound "
          f"{g.bounds['wt']:.3e}; general projections outside the map {g.outside:.2f}")
    assert ts.compare_abs("zlat", zl, ref, bound) == []
    assert float(np.abs(np.tile(g.zlat, (c.NV, 1))).max()) > 100 * bound           # (the general lookup is not lost in the bound)
    return g


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_point_inputs_novel_forward(mode, dev):
    g = check_novel(ts.GEN_CASES[1], mode, dev, sb=0)
    assert 0.05 <= g.outside <= 0.6


@pytest.mark.parametrize("mode", [MODES[0], MODES[4]], ids=[MODE_IDS[0], MODE_IDS[4]])
def test_sb_1_reads_the_second_scene_and_its_general_camera(mode, dev):
    c = ts.SB2_CASE.build()
    g0, g1 = general_refs(c, 0, mode), general_refs(c, 1, mode)
    assert not np.array_equal(g0.idx, g1.idx)
    check_novel(ts.SB2_CASE, mode, dev, sb=1)
    check_novel(ts.SB2_CASE, mode, dev, sb=0)


def test_no_lin_z_reads_no_latent(dev):
    """zlat = NULL (combine_layer 0): in_out alone is written; latent, taps and gen_taps may be NULL"""
    from diner_amd import _lib
    case = ts.GEN_CASES[1]
    d = on_device(case, dev)
    c = d.case
    mode = MODES[0]
    want = run_novel(c, mode, dev)[0]
    keep = []
    gen = gen_struct(c, d, c.SB, torch.zeros(1, device=dev), dev, keep)
    gen.latent = None
    xi = T(general(c, 0).xyz_in[None], dev)
    vd = d.t["rays"][:, :, None, 3:6].expand(-1, -1, c.K, -1).reshape(c.SB, c.P, 3).contiguous()
    inp = torch.full((d.R, c.ld_in), NAN, device=dev)
    call("diner_train_point_inputs_novel", C.byref(d.scene), None, None, C.byref(gen), P_(xi), P_(xi), P_(vd), c.P, 0, P_(inp), c.ld_in, None, None,
         None, ST(dev))
    assert ts.compare_bits("in_out", inp.cpu().numpy(), want) == []
    assert _lib.lib().diner_version() == 3


# ---- (b) against the plain entry point, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [ts.GEN_CASES[1], ts.GEN_CASES[2]], ids=[ts.GEN_CASES[1].id, ts.GEN_CASES[2].id])
def test_zero_general_latent_is_the_plain_point_inputs_bit_for_bit(case, mode, dev):
    d = on_device(case, dev)
    p_in, p_zl, p_idx, p_wt = d.forward("gen", mode)
    inp, zl, idx, wt, gidx, gwt = run_novel(d.case, mode, dev, zero_gen=True, same_points=True)
    assert ts.compare_bits("in_out", inp, p_in) == []
    assert np.array_equal(idx, p_idx) and ts.compare_bits("tap weights", wt, p_wt) == []
    if mode[1] == "zeros":
        assert np.array_equal(zl, p_zl)                                          # as values (the module docstring says why)
        rows_on_the_map = (p_wt != 0).any(-1)
        assert ts.compare_bits("zlat", zl[rows_on_the_map], p_zl[rows_on_the_map]) == []
    else:
        assert ts.compare_bits("zlat", zl, p_zl) == []
    assert np.isfinite(gwt).all() and gidx.min() >= 0 and gidx.max() < GEN_HW[0] * GEN_HW[1]


# ---- (c) the general latent's scatter -------------------------------------------------------------------------------------------------------------
def scatter(P, NV, Cc, idx, wt, dz, dev, hw=GEN_HW):
    taps = torch.cat([torch.from_numpy(np.ascontiguousarray(idx, np.int32)).view(torch.float32), torch.from_numpy(np.ascontiguousarray(wt, F32))], 1).to(dev)
    out = torch.zeros((hw[0] * hw[1], Cc), device=dev)
    call("diner_train_novel_gen_scatter", P_(T(dz, dev)), P_(taps), P, Cc, hw[0], hw[1], NV, P_(out), ST(dev))
    return out.cpu().numpy()


def scatter_ref(P, NV, Cc, idx, wt, dz, hw=GEN_HW):
    """float64: the sum over the NV view rows of every point, then the plain scatter of one 'view' -> (sums [hw, C], terms per texel [hw])"""
    summed = np.asarray(dz, np.float64).reshape(NV, P, Cc).sum(0)
    out, cnt = ts.scatter_plain(idx, wt, summed, P, 1, hw[0] * hw[1])
    return out[0], cnt[0]


def check_scatter(P, NV, Cc, idx, wt, dz, dev):
    got = scatter(P, NV, Cc, idx, wt, dz, dev)
    ref, cnt = scatter_ref(P, NV, Cc, idx, wt, dz)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print(f"FIG scatter P{P} NV{NV} C{Cc}: max error {err:.3e}, bound {2e-4 * scale:.3e}, texels reached {int((cnt > 0).sum())}")
    assert err <= 2e-4 * scale
    assert np.all(got[cnt == 0] == 0)                                            # texels no tap names stay exactly 0
    return got, ref, cnt


def random_taps(rs, P, hw=GEN_HW):
    """footprints that repeat along runs of points (so that runs merge and break), bilinear-like weights with some zeros"""
    n = hw[0] * hw[1]
    base = rs.randint(0, n - hw[1] - 1, size=(P + 3) // 4).repeat(4)[:P]
    idx = np.stack([base, base + 1, base + hw[1], base + hw[1] + 1], -1).astype(np.int32)
    wt = rs.uniform(0, 1, (P, 4)).astype(F32)
    wt[rs.uniform(size=(P, 4)) < 0.15] = 0
    return idx, wt


@pytest.mark.parametrize("Cc", [8, 72, 512])
@pytest.mark.parametrize("NV", [1, 3, 4])
@pytest.mark.parametrize("P", [1, 63, 65, 200])
def test_gen_scatter_matches_float64(P, NV, Cc, dev):
    rs = np.random.RandomState(1000 * P + 10 * NV + Cc)
    idx, wt = random_taps(rs, P)
    dz = rs.standard_normal((NV * P, Cc)).astype(F32)
    got, ref, cnt = check_scatter(P, NV, Cc, idx, wt, dz, dev)
    assert (cnt > 0).any() and (P > 8 or (cnt == 0).any())


def test_gen_scatter_contention_on_one_texel(dev):
    P, NV, Cc = 200, 3, 72
    rs = np.random.RandomState(5)
    idx = np.full((P, 4), 7, np.int32)
    wt = np.concatenate([rs.uniform(0.5, 1, (P, 1)), np.zeros((P, 3))], -1).astype(F32)          # a nearest lookup's record
    dz = rs.standard_normal((NV * P, Cc)).astype(F32)
    got, ref, cnt = check_scatter(P, NV, Cc, idx, wt, dz, dev)
    assert int((cnt > 0).sum()) == 1 and np.count_nonzero(got.any(-1)) == 1


def test_gen_scatter_of_a_lone_point(dev):
    rs = np.random.RandomState(6)
    idx, wt = np.array([[3, 4, 9, 10]], np.int32), np.array([[0.4, 0.1, 0.3, 0.2]], F32)
    check_scatter(1, 4, 8, idx, wt, rs.standard_normal((4, 8)).astype(F32), dev)


def test_gen_scatter_with_all_weights_zero_leaves_the_buffer_untouched(dev):
    P, NV, Cc = 65, 3, 72
    rs = np.random.RandomState(7)
    idx, _ = random_taps(rs, P)
    got = scatter(P, NV, Cc, idx, np.zeros((P, 4), F32), rs.standard_normal((NV * P, Cc)).astype(F32), dev)
    assert np.all(got == 0) and not np.signbit(got).any()
