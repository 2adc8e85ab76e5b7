"""CPU checks of tests/train_stage_refs.py (no GPU): the restatement reproduces the CPU oracle, the reference's stored MLP inputs and
torch's grid_sample; the decision margin holds for every case and is noticed when it does not; every case reaches the edges it is meant to
reach; every comparison function rejects a deliberately wrong implementation, mutant by mutant; and the bounds are finite, positive and
tighter than the whole-step fixture bars (tests/test_training.py, tests/test_gpu_camera_grads.py: 2e-4 x max|ref|).

Bounds against the fixture bars.  Largest bound / (2e-4 x max|ref|) over the grid and the six lookup modes (CPU values only): focal
0.065, c 0.063, the latent scatter 0.099 at C = 512 -- the tenth the new tests were asked to reach -- and 0.16 at C = 8 (fewer channels
share a maximum), image_shape 0.18, rays 0.17, depths 0.21,
poses 0.05 with more than one point, 0.85 for a lone point.  Why not a tenth everywhere: 4 x the float32 CPU side alone is 0.17 on rays and
0.20 on depths (a row's gradient cancels between its 55 inputs, so the per-row terms these are measured against are small next to the
roundings of the inputs they sum); image_shape's terms have both signs, so the worst-case summation floor, (depth of the reduction) x
2^-24 of sum |terms|, is 0.17 of the bar by itself while the float32 side is 0.006; a lone point's d_R is one outer product whose
small elements carry the large ones' rounding.  test_bounds_sanity asserts these figures family by family; all are below the fixture bar.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_stage_refs as ts
from tests.train_stage_refs import MODES, MODE_IDS, TRAIN_STAGE_CASES

F32 = np.float32
ALL_CASES = TRAIN_STAGE_CASES + ts.GEN_CASES[:2] + [ts.SB2_CASE, ts.SCATTER_CONTENTION, ts.SCATTER_ONE] + ts.REDUCE_CASES
IDS = lambda cases: [c.id for c in cases]
FAKE = C.c_void_p(1 << 20)   # a non-NULL pointer that no call below may dereference
MUT = TRAIN_STAGE_CASES[6]   # 5x7, feature_padding 1, NV 3, (13, 5): the case most mutants are applied to
MUT23 = TRAIN_STAGE_CASES[2]  # 2x3, NV 3, (13, 5): a scatter run that merges across a view boundary


def scene_of(sc, num_freqs=6, freq_factor=6.28):
    """a synthetic.synth.Scene in the restatement's form"""
    from types import SimpleNamespace
    return SimpleNamespace(poses=sc.poses[0], focal=sc.focal[0], c=sc.c[0], image_shape=sc.image_shape, depths=sc.depths[0, :, 0],
                           latent=sc.latent[0], feature_padding=F32(sc.feature_padding), freq_factor=F32(freq_factor), num_freqs=num_freqs)


def port_tolerance(ref_in, F_=6, freq_factor=6.28):
    """what a float32 port of the chain can differ by: a few ulps on the plain columns; on a positional code the argument's rounding,
    f x ulp(x), besides the sine's last ulp"""
    xmax = float(np.abs(ref_in[..., :3]).max())
    tol = {}
    for name, cols in ts.in_families(F_).items():
        if name.startswith("code"):
            f = freq_factor * 2.0 ** int(name.rsplit("f", 1)[1])
            tol[name] = 4.0 * f * ts.EPS32 * xmax + 3e-7
        else:
            tol[name] = 8.0 * ts.EPS32 * xmax
    return tol


def assert_inputs_close(got567, f, scene, F_=6):
    """[NV,n,512+55] of a float32 port against a float64 run of the restatement"""
    ref_in, ref_z = f.in55.numpy(), f.zlat.numpy()
    tol = port_tolerance(ref_in)
    for name, cols in ts.in_families(F_).items():
        err = np.abs(got567[..., [512 + c for c in cols]] - ref_in[..., cols]).max()
        assert err <= tol[name], (name, err, tol[name])
    # the lookup: a float32 coordinate is carried at ulp(map size) texels, and a texel of error moves the value by a texel difference
    size = max(scene.latent.shape[-2:])
    assert np.abs(got567[..., :512] - ref_z).max() <= 4 * ts.EPS32 * size * float(scene.latent.max() - scene.latent.min())


# ---- the forward restatement against existing CPU evidence ------------------------------------------------------------------------
def test_reproduces_the_oracle_on_a_synthetic_scene():
    from oracle.oracle import Oracle
    from synthetic import synth
    sc = synth.make_scene(24, 24, 3, seed=5, feature_padding=2)
    rays = sc.target_rays(focal_scale=0.7)[0][::5]                  # a wide field of view: rays leave the source images
    rs = np.random.RandomState(3)
    z = np.sort(rs.uniform(sc.near, sc.far, (rays.shape[0], 4)), -1).astype(F32)
    xyz = rays[:, None, :3] + z[..., None] * rays[:, None, 3:6]
    got = Oracle(sc, None).point_inputs(xyz.reshape(-1, 3), np.broadcast_to(rays[:, None, 3:6], xyz.shape).reshape(-1, 3))
    f = ts.point_inputs_ref(scene_of(sc), rays, z)
    assert_inputs_close(got, f, sc)
    assert float(((f.ix < 0) | (f.ix > sc.latent.shape[-1] - 1)).double().mean()) > 0.02


@pytest.mark.parametrize("name", ["g0_nv4_k16", "g3_nv3_k40_wide"])
def test_reproduces_the_reference_mlp_inputs(name):
    from tests.conftest import load_golden
    g = load_golden(name)
    rays, zf, K = g.rays[0], g["z_fill"], g.K
    sel = g["mlp_input_sel_full"]
    f = ts.point_inputs_ref(scene_of(g.scene), rays[sel // K], zf[sel // K, sel % K][:, None])
    assert_inputs_close(g["mlp_input_full"], f, g.scene)
    sel = g["mlp_input_sel_tail"]
    f = ts.point_inputs_ref(scene_of(g.scene), rays[sel // K], zf[sel // K, sel % K][:, None])
    tail = np.concatenate([f.zlat.numpy(), g["mlp_input_tail"]], -1)   # the tail rows store the 55 inputs only
    assert_inputs_close(tail, f, g.scene)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [TRAIN_STAGE_CASES[2], MUT, ts.BOUNDARY_CASES[0]], ids=lambda c: c.id)
def test_zlat_equals_grid_sample(case, mode):
    """float64, every mode, values and both gradients; the boundary family included (ATen's conventions ON the boundaries)"""
    c = case.build()
    f = c.forward64(mode, grad=True)
    sc = c.scenes[0]
    lat = torch.from_numpy(sc.latent).double().requires_grad_(True)
    fp = float(sc.feature_padding)
    scale = torch.tensor([(c.w - 2 * fp) / c.w, (c.h - 2 * fp) / c.h], dtype=torch.float64)
    uv = torch.stack([f.u, f.v], -1).detach().requires_grad_(True)
    out = F.grid_sample(lat, (uv * scale)[:, None], mode=mode[0], padding_mode=mode[1], align_corners=False)[:, :, 0].permute(0, 2, 1)
    assert float((out - f.zlat).detach().abs().max()) <= 1e-12
    g = torch.from_numpy(c.d_zlat[0]).double().view(out.shape)
    g_uv, g_lat = torch.autograd.grad((out * g).sum(), [uv, lat])
    m_lat, m_u, m_v = torch.autograd.grad((f.zlat * g).sum(), [f.latent, f.u, f.v], allow_unused=True, materialize_grads=True)
    assert float((g_lat - m_lat).abs().max()) <= 1e-11
    assert float((g_uv - torch.stack([m_u, m_v], -1)).abs().max()) <= 1e-11 * max(1.0, float(g_uv.abs().max()))


# ---- decision margins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=IDS(ALL_CASES))
def test_decision_margin_holds(case):
    c = case.build()
    for sb in range(c.SB):
        f = ts.point_inputs_ref(c.scenes[sb], c.rays[sb], c.z[sb])
        assert ts.decision_margin(f) >= ts.DECISION_MARGIN
        for x, n in ((f.ix, c.w), (f.iy, c.h), (f.dx, c.W), (f.dy, c.H)):          # ... and no coordinate so far out that float32 loses it
            assert float(x.abs().max()) <= 12 * n


def test_decision_margin_notices_a_point_on_a_boundary():
    c = copy.deepcopy(MUT.build())
    c._refs = {}
    # slide ray 0's origin along x until point 0 of view 0 sits on the integer ix = 2
    ix_of = lambda s: float(ts.point_inputs_ref(c.scenes[0], _moved(c, s), c.z[0], coords_only=True).ix[0, 0])
    lo, hi = -3.0, 3.0
    assert (ix_of(lo) - 2.0) * (ix_of(hi) - 2.0) < 0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if (ix_of(lo) - 2.0) * (ix_of(mid) - 2.0) > 0 else (lo, mid)
    c.rays[0] = _moved(c, lo)
    with pytest.raises(AssertionError, match="decision boundary"):
        c.refs(MODES[0], backward=False)


def _moved(c, s):
    r = c.rays[0].copy()
    r[0, 0] = F32(s)
    return r


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=IDS(ALL_CASES))
def test_cases_reach_their_edges(case):
    c = case.build()
    for sb in range(c.SB):
        assert c.coverage_missing(sb) == []
    R = c.P * c.NV
    assert c.P == 1 or R % 64 or (c.NR, c.K) == (4, 16)


def test_the_grid_as_a_whole_covers_every_edge():
    cov = [c.build().coverage() for c in TRAIN_STAGE_CASES]
    for side in ("left", "right", "above", "below"):
        assert sum(getattr(v, side) > 0 for v in cov) >= 3
    assert sum(v.repeats > 0 for v in cov) >= 5 and sum(v.merge_at_view > 0 for v in cov) >= 2
    for hw in ((2, 3), (5, 7)):
        assert {c.fpad > 0 for c in TRAIN_STAGE_CASES if (c.h, c.w) == hw} == {False, True}
    assert {(c.NV, c.NR, c.K) for c in TRAIN_STAGE_CASES} >= {(nv, 1, 1) for nv in (1, 3)} | {(3, 13, 5), (1, 4, 16), (3, 4, 16)}
    b = ts.BOUNDARY_CASES[0].build().forward64(MODES[0])
    for x, n in ((b.ix, 8), (b.iy, 4)):
        vals = set(x.numpy().reshape(-1).tolist())
        assert {-1.0, 0.0, n - 1.0, n + 1.0} <= vals
    assert float((b.dx * 2 % 2 == 1).double().mean()) > 0.3          # half-integers on the depth map


# ---- mutants: every comparison rejects a wrong implementation ------------------------------------------------------------------------------
def _fwd_findings(c, mode, defect):
    r = c.refs(mode, backward=False)
    f = c.forward64(mode, defect=defect)
    flat = lambda a: a.detach().numpy().reshape(c.NV * c.P, -1)
    return dict(taps=ts.compare_taps(flat(f.idx), flat(f.wt).astype(F32), r.idx, r.wt, r.bounds["wt"], c.h * c.w),
                inputs=ts.compare_inputs(flat(f.in55), r.in55, r.bounds, c.F),
                zlat=ts.compare_abs("zlat", flat(f.zlat), r.zlat, r.bounds["zlat"]))


def test_the_float64_restatement_passes_its_own_comparisons():
    for mode in MODES:
        assert all(v == [] for v in _fwd_findings(MUT.build(), mode, None).values())


@pytest.mark.parametrize("defect, mode, caught_by", [
    ("align_corners", MODES[0], ("taps", "zlat")), ("depth_floor", MODES[0], ("inputs",)), ("no_feature_padding", MODES[0], ("taps", "zlat")),
    ("swap_ne_sw", MODES[0], ("taps", "zlat")), ("border_keeps_weight", MODES[1], ("taps", "zlat")),
    ("align_corners", MODES[3], ("taps", "zlat")), ("border_keeps_weight", MODES[4], ("taps", "zlat")),
])
def test_forward_mutants_are_rejected(defect, mode, caught_by):
    found = _fwd_findings(MUT.build(), mode, defect)
    for k in caught_by:
        assert found[k] != [], (defect, k)


def _leaf_findings(c, mode, grads, start_ishape=None):
    r = c.refs(mode)
    bad = {}
    for k in ts.LEAVES:
        ref = r.grads[k] + (start_ishape if k == "image_shape" and start_ishape is not None else 0.0)
        bad[k] = ts.compare_scaled(k, grads[k], ref, r.scales[k], r.rel[k])
    return bad


def _grads(c, mode, defect=None, bwd_defect=None):
    n = 7 + 8 * c.F
    f = c.forward64(mode, defect=defect, grad=True)
    return ts.backward_ref(f, c.d_in[0][:, :n], c.d_zlat[0], c.d_far[0], c.NR, c.K, c.scenes[0].depths.shape, bwd_defect)[0]


def test_every_declared_defect_has_a_mutant_test():
    marks = {m.name: m for m in test_forward_mutants_are_rejected.pytestmark}
    assert {a[0] for a in marks["parametrize"].args[1]} == set(ts.FWD_DEFECTS)
    marks = {m.name: m for m in test_backward_mutants_are_rejected.pytestmark}
    used = {a[0] for a in marks["parametrize"].args[1]} | {a[1] for a in marks["parametrize"].args[1]}
    assert set(ts.GRAD_DEFECTS) | set(ts.BWD_DEFECTS) <= used


def test_the_float64_gradients_pass_their_own_comparison():
    c = MUT.build()
    for mode in MODES:
        assert all(v == [] for v in _leaf_findings(c, mode, _grads(c, mode)).values())


@pytest.mark.parametrize("defect, bwd_defect, mode, leaf", [
    (None, "dR_transposed", MODES[0], "poses"), (None, "dfocal_no_invz", MODES[0], "focal"), ("border_grad_kept", None, MODES[0], "c"),
    ("reflection_sign", None, MODES[2], "focal"), ("depth_floor", None, MODES[0], "depths"),
])
def test_backward_mutants_are_rejected(defect, bwd_defect, mode, leaf):
    c = MUT.build()
    assert _leaf_findings(c, mode, _grads(c, mode, defect, bwd_defect))[leaf] != []


def test_image_shape_that_overwrites_is_rejected():
    c = MUT.build()
    g = _grads(c, MODES[0])
    start = np.array([0.75, -1.5])
    assert _leaf_findings(c, MODES[0], g, start)["image_shape"] != []                       # the kernel must ADD to what is there
    assert _leaf_findings(c, MODES[0], dict(g, image_shape=g["image_shape"] + start), start)["image_shape"] == []


def test_scatter_walk_equals_autograd_and_a_missing_view_flush_is_rejected():
    c = MUT23.build()
    assert c.coverage().merge_at_view > 0
    r = c.refs(MODES[0])
    hw = c.h * c.w
    good = ts.scatter_runs(r.idx, r.wt, c.d_zlat[0], c.P, c.NV, hw)
    assert ts.compare_scaled("scatter", good, r.lat_ref, r.lat_scale, 1e-13) == []           # the walk is the plain sum is autograd
    assert ts.compare_abs("scatter", good, r.lat_ref, r.lat_bound) == []
    assert r.cpu_rel["latent"] <= r.cpu_err["wt"] * 1.001                                     # the float32 side: its weights' error
    bad = ts.scatter_runs(r.idx, r.wt, c.d_zlat[0], c.P, c.NV, hw, defect="no_view_flush")
    assert ts.compare_abs("scatter", bad, r.lat_ref, r.lat_bound) != []
    swapped = ts.scatter_plain(r.idx[:, [0, 2, 1, 3]], r.wt, c.d_zlat[0], c.P, c.NV, hw)[0]      # ne / sw indices swapped
    assert ts.compare_abs("scatter", swapped, r.lat_ref, r.lat_bound) != []


def test_reduction_mutants_are_rejected():
    rs = np.random.RandomState(2)
    # view mean: (NV + 1) ulp of sum|x| / NV
    x = rs.standard_normal((3, 257)).astype(F32)
    tol = 4 * ts.U32 * np.abs(x.astype(np.float64)).sum(0) / 3
    assert ts.compare_abs("mean", ts.view_mean_ref(x, 3), ts.view_mean_ref(x, 3), tol) == []
    assert ts.compare_abs("mean", ts.view_mean_ref(x, 3, defect="nv_minus_1"), ts.view_mean_ref(x, 3), tol) != []
    assert ts.compare_abs("mean_bwd", ts.view_mean_ref(x[0], 3, True, "nv_minus_1"), ts.view_mean_ref(x[0], 3, True), np.abs(x[0]) / 3 * ts.EPS32) != []
    # head: the relu gate at exactly 0
    out = np.array([0.3, -0.2, 0.1, 0.0, 0.3, -0.2, 0.1, -0.0, 1.0, 2.0, 3.0, -1e-30, 0.0, 0.0, 0.0, 1e-30], F32)
    y, g = ts.head_ref(out), rs.standard_normal(out.size) + 3.0
    assert ts.compare_abs("head_bwd", ts.head_bwd_ref(out, y, g), ts.head_bwd_ref(out, y, g), 0.0) == []
    assert ts.compare_abs("head_bwd", ts.head_bwd_ref(out, y, g, "relu_ge"), ts.head_bwd_ref(out, y, g), 0.0) != []
    # amax: the n % 4 tail
    a = rs.standard_normal(1023).astype(F32)
    a[-1] = 40.0
    assert ts.compare_bits("amax", ts.amax_ref(a, "no_tail"), ts.amax_ref(a)) != [] and ts.compare_bits("amax", ts.amax_ref(a), F32(40.0)) == []
    # colsum: the rows past the first sweep of the grid
    dY = rs.standard_normal((2048 * 4 + 9, 4)).astype(F32)
    db0 = 0.05 * np.abs(dY).sum(0) * np.array([1, -1, 1, -1])       # a starting value that matters next to the bound
    scale = ts.colsum_ref(dY, None, absolute=True) + np.abs(db0)
    rel = dY.shape[0] * ts.U32
    assert ts.compare_scaled("colsum", ts.colsum_ref(dY, db0), ts.colsum_ref(dY, db0), scale, rel) == []
    assert ts.compare_scaled("colsum", ts.colsum_ref(dY, db0, "first_sweep"), ts.colsum_ref(dY, db0), scale, rel) != []
    assert ts.compare_scaled("colsum", ts.colsum_ref(dY, 0 * db0), ts.colsum_ref(dY, db0), scale, rel) != []      # db is +=
    # layout
    t = rs.standard_normal((6, 35, 72)).astype(F32)
    assert ts.compare_bits("nchw", ts.nhwc_to_nchw_ref(t, 6, 72, 35), t.transpose(0, 2, 1)) == []
    assert ts.compare_bits("nchw", t, t.transpose(0, 2, 1).copy().reshape(t.shape)) != []


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
FIXTURE_BAR = 2e-4          # x max|ref|: tests/test_training.py (latent gradient), tests/test_gpu_camera_grads.py (camera leaves)
SHARE_OF_BAR = dict(focal=0.1, c=0.1, latent=0.2, rays=0.25, depths=0.25, image_shape=0.25, poses=0.25)   # (module docstring)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", TRAIN_STAGE_CASES + ts.GEN_CASES[:2], ids=IDS(TRAIN_STAGE_CASES + ts.GEN_CASES[:2]))
def test_bounds_sanity(case, mode):
    c = case.build()
    r = c.refs(mode)
    for k, b in r.bounds.items():
        assert np.isfinite(b) and b > 0, k
    fam = {k: (r.rel[k] * r.scales[k], r.cpu_rel[k] * r.scales[k], np.abs(r.grads[k]).max()) for k in ts.LEAVES}
    fam["latent"] = (r.lat_bound, r.cpu_rel["latent"] * r.lat_absdz, np.abs(r.lat_ref).max())
    for k, (bound, cpu, ref_max) in fam.items():
        assert np.all(np.isfinite(bound)) and np.all(np.asarray(r.rel[k] if k != "latent" else r.bounds["wt"]) > 0), k
        if ref_max == 0:
            continue                                        # (nearest: no grid gradient; a lone point: nothing to reduce)
        bar = FIXTURE_BAR * ref_max
        print(f"RATIO {k} {bound.max() / bar:.3f} {cpu.max() / bar:.3f} {c.id} {mode}")
        assert bound.max() <= (0.1 if k == "latent" and c.C == 512 else SHARE_OF_BAR[k]) * bar or (k == "poses" and c.P == 1 and bound.max() < bar), (k, bound.max() / bar)


def test_colsum_amax_refuses_widths_it_cannot_tile():
    from diner_amd import _lib
    lib = _lib.lib()
    for N in (96, 6):                                       # 96 / 4 = 24 does not divide 256; 6 % 4 != 0
        assert lib.diner_train_colsum_amax(FAKE, 16, N, N if N % 4 == 0 else 8, FAKE, FAKE, None) == -1      # DINER_E_INVALID
        assert "train_colsum_amax" in lib.diner_last_error().decode() and "N % 4" in lib.diner_last_error().decode()
    assert lib.diner_train_colsum_amax(FAKE, 0, 64, 64, None, None, None) == -1 and "nothing to compute" in lib.diner_last_error().decode()
