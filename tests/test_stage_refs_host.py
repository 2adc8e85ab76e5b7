"""CPU proof of what tests/test_gpu_stage_kernels.py compares with (tests/stage_refs.py): the restatements reproduce the oracle and the
goldens, the case sets are not vacuous, and every comparison function rejects every listed defect of a float32 restatement on the very
inputs the GPU tests use.  No GPU."""
import numpy as np
import pytest

from tests import stage_refs as sr
from tests.stage_refs import COMPOSITE_CASES, SAMPLER_CASES

IDS = lambda cases: [c.id for c in cases]


# ---- sampler -----------------------------------------------------------------------------------------------------------------
def _check_restatement(L, z_cand, z_dg, K, G, n_gauss):
    ref, hit = sr.select_rows(L, z_cand, K, G, n_gauss)
    keep = K - G
    np.testing.assert_array_equal(z_dg[:, :keep], ref[:, :keep].astype(np.float32))       # same slots, same order, bit for bit
    assert np.array_equal(hit, (z_dg != 0).any(-1))
    bound, err = sr.gauss_bound(z_dg, ref, K, G)
    # float32 rounding of mean and std over NC candidates: |n| * few ulp * sqrt-amplified; far below any defect (test below)
    scale = 1 + (np.abs(n_gauss).max() if G else 0)
    assert err <= 2e-5 * scale, err
    return ref, hit


def test_select_reproduces_oracle_on_goldens(golden):
    from oracle.oracle import Oracle
    orc = Oracle(golden.scene, None)
    z, L = orc.sample_depthguided(golden.rays[0], golden["z_cand"], golden.K, golden.G, golden.noise[1], want_L=True)
    _check_restatement(L, golden["z_cand"], z, golden.K, golden.G, golden.noise[1])


@pytest.mark.parametrize("case", SAMPLER_CASES, ids=IDS(SAMPLER_CASES))
def test_select_and_fill_up_reproduce_oracle(case):
    from oracle.oracle import Oracle
    c = case.oracle()
    for s in range(c.SB):
        assert c.surface[s].sum() >= 20 and (~c.surface[s]).sum() >= 5, (int(c.surface[s].sum()), int((~c.surface[s]).sum()))
        _check_restatement(c.orc_L[s], c.z_cand[s], c.orc_z_dg[s], c.K, c.G, c.n_gauss[s])
        fill = Oracle(c.scenes[s], None).fill_up(c.rays[s], c.orc_z_dg[s], c.u_fill[s])
        np.testing.assert_array_equal(sr.fill_up_f32(c.orc_z_dg[s], c.rays[s], c.u_fill[s]), fill)


def test_dedicated_sampler_cases_reach_their_paths():
    by = {c.special: c.oracle() for c in sr.SAMPLER_SPECIAL}
    for neg in (c for c in sr.SAMPLER_SPECIAL if c.special == "gauss_negative"):
        assert ((neg.orc_z_dg[0] < 0).any(-1) & (neg.orc_z_dg[0] == 0).any(-1)).sum() >= 20     # negative samples AND slots to fill
    far = by["gauss_beyond_far"]
    assert (far.orc_z_dg[0] > far.rays[0, :, 7:8]).any(-1).sum() >= 20
    t = by["ties"]
    keep, n = t.K - t.G, 0
    for L, z in zip(t.orc_L[0], t.z_cand[0]):
        cut = np.sort(L)[::-1][keep - 1]
        tied = z[L == cut]
        n += cut > 0 and (L > cut).sum() < keep < (L >= cut).sum() and np.unique(tied).size > keep    # distinct z tie across the cut
    assert n >= 20, n
    assert (t.z_cand[0][0, 4::5] == t.z_cand[0][0, 3::5][: t.z_cand[0][0, 4::5].size]).all()       # and repeated values
    e = by["near_eq_far"]
    assert (e.rays[0, :, 6] == e.rays[0, :, 7]).sum() >= 20
    m = by["miss_all"]
    assert (~m.surface[0]).sum() >= 100


@pytest.mark.parametrize("defect", sr.SAMPLER_DEFECTS)
def test_decision_comparison_rejects(defect):
    """a wrong selection applied to the oracle's likelihood must not pass as the oracle's z_dg's equal"""
    rejected = []
    for c in SAMPLER_CASES:
        c.oracle()
        ref, hit = sr.select_rows(c.orc_L[0], c.z_cand[0], c.K, c.G, c.n_gauss[0])
        tol, _ = sr.gauss_bound(c.orc_z_dg[0], ref, c.K, c.G)
        assert sr.compare_decisions(c.orc_z_dg[0], ref, hit, c.K, c.G, tol) == [], c.id       # the right one passes
        wrong, _ = sr.select_rows(c.orc_L[0], c.z_cand[0], c.K, c.G, c.n_gauss[0], defect)
        if sr.compare_decisions(wrong.astype(np.float32), ref, hit, c.K, c.G, tol):
            rejected.append(c.id)
    print(defect, "rejected on", len(rejected), "of", len(SAMPLER_CASES))
    if defect == "tie_high":
        assert any(i.endswith("ties") for i in rejected)
    elif defect == "keep_zero":     # wherever a hit ray has fewer non-zero likelihoods than slots
        assert len(rejected) >= 10
    else:                           # ignore_hit: every case with gaussian slots has rays without a hit
        assert set(rejected) >= {c.id for c in SAMPLER_CASES if c.G > 0}


def test_fill_up_comparison_rejects_missing_negative_offset():
    c = next(c for c in sr.SAMPLER_SPECIAL if c.special == "gauss_negative").oracle()
    good = sr.fill_up_f32(c.orc_z_dg[0], c.rays[0], c.u_fill[0])
    wrong = sr.fill_up_f32(c.orc_z_dg[0], c.rays[0], c.u_fill[0], defect="no_neg_offset")
    assert (good != wrong).any(-1).sum() >= 20


def test_likelihood_comparison_rejects():
    c = SAMPLER_CASES[8].oracle()
    L = c.orc_L[0]
    assert sr.compare_likelihood(L.copy(), L) == []
    a = L.copy()
    a[L > 0.1] *= np.float32(1 + 1e-6)
    assert sr.compare_likelihood(a, L)
    b = L.copy()
    b.flat[np.argmax(L)] = 0
    assert sr.compare_likelihood(b, L)


# ---- compositing -------------------------------------------------------------------------------------------------------------
def test_composite_ref_reproduces_goldens(golden):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    w, rgb, depth = sr.composite_ref(t(golden.rays[0]), t(golden["z_fill"]), t(golden["rgbsigma"]), golden.scene.white_bkgd, torch.float32)
    np.testing.assert_allclose(w.numpy(), golden["weights"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(rgb.numpy(), golden["rgb"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(depth.numpy(), golden["depth"], rtol=0, atol=2e-6)
    w2, rgb2, depth2, _ = sr.composite_f32(golden.rays[0], golden["z_fill"], golden["rgbsigma"], golden.scene.white_bkgd)
    np.testing.assert_allclose(w2, golden["weights"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(rgb2, golden["rgb"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(depth2, golden["depth"], rtol=0, atol=2e-6)


def test_composite_case_set_covers_the_issue():
    cs = COMPOSITE_CASES
    assert {c.K for c in cs} == {1, 2, 40, 63, 64, 65, 127, 128, 129, 256, 300} and {c.N for c in cs} == {1, 3, 5, 64, 1001}
    for attr, n in (("sigma", 5), ("zfam", 4), ("cot", 3), ("white", 2), ("want_weights", 2)):
        assert len({getattr(c, attr) for c in cs}) == n
    for fam in ("opaque_one", "opaque_all"):
        assert {c.K for c in cs if c.sigma == fam} == {40, 63, 64, 65, 127, 128, 129, 256, 300}


@pytest.mark.parametrize("case", COMPOSITE_CASES, ids=IDS(COMPOSITE_CASES))
def test_composite_cases_and_float32_evaluations(case):
    """the regimes are what the families say, no case is vacuous, and both float32 CPU evaluations pass the comparison they calibrate"""
    c = case.refs()
    assert c.opaque == c.sigma.startswith("opaque")
    if c.opaque:
        assert c.opaque_followed(8) >= 1
    else:
        assert not c.keep_is_eps().any()
    if c.sigma == "negative" and c.N * c.K >= 5:
        s = c.rgbsigma[..., 3]
        assert (s < 0).any() and (s == 0).any() and (s > 0).any()
    for w, rgb, depth, d_c, d_far in (c.r32, c.s32):
        assert sr.compare_composite(w, rgb, depth, c) == []
        assert sr.compare_composite_grads(d_c, d_far, c) == []
    print(c.id, "cpu forward err", c.cpu_err, "cpu backward err", c.cpu_gerr)


def _applies(defect, c):
    """the cases on which a defect changes the result by more than rounding: there it must be rejected"""
    live = c.sigma == "moderate" or (c.sigma == "negative" and c.N * c.K >= 5) or c.opaque
    if defect == "no_carry":     # (K = 65 with the last sample at far: the only sample behind the carry has delta = 0)
        return c.K > 64 and live and c.sigma != "opaque_all" and not (c.K == 65 and c.zfam == "last_eq_far")
    if defect == "last_delta_z":
        return live and c.zfam in ("uniform", "repeated") and c.sigma != "opaque_all" and c.K > 1
    if defect == "no_eps":
        return c.opaque
    if defect == "no_white_grad":
        return c.white and live and c.sigma != "opaque_all"
    if defect == "s_before":
        return live and c.K > 2 and c.sigma != "opaque_all"
    if defect == "relu_ge":
        return c.sigma in ("zero", "negative") and c.K > 2
    raise KeyError(defect)


@pytest.mark.parametrize("defect", sr.FWD_DEFECTS)
def test_forward_comparison_rejects(defect):
    n = 0
    for c in COMPOSITE_CASES:
        c.refs()
        if defect == "no_eps" or not _applies(defect, c):
            continue       # (the forward does not see a missing 1e-10 within its bars: weights behind an opaque sample are ~1e-10)
        w, rgb, depth, _ = sr.composite_f32(c.rays, c.z, c.rgbsigma, c.white, defect)
        assert sr.compare_composite(w, rgb, depth, c), (defect, c.id)
        assert sr.compare_composite(None, rgb, depth, c) or c.sigma == "negative" or c.K == 2, (defect, c.id)
        n += 1
    assert n >= 8 or defect == "no_eps"


@pytest.mark.parametrize("defect", sr.BWD_DEFECTS)
def test_backward_comparison_rejects(defect):
    n = 0
    for c in COMPOSITE_CASES:
        c.refs()
        if not _applies(defect, c):
            continue
        d_c, d_far = sr.composite_backward_f32(c.rays, c.z, c.rgbsigma, c.white, *c.cotangents(), defect=defect)
        assert sr.compare_composite_grads(d_c, d_far, c), (defect, c.id)
        n += 1
    assert n >= 8, n


# ---- gen_rays / depth2normal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sr.GLUE_SIZES)
def test_float64_glue_restatements_agree_with_float32(W, H):
    from synthetic import synth
    g = sr.glue_case(W, H)
    for b in range(3):
        r32 = synth.gen_rays(g["extrinsics"][b], g["intrinsics"][b], W, H, g["z_near"][b], g["z_far"][b])
        r64 = sr.gen_rays64(g["extrinsics"][b], g["intrinsics"][b], W, H, g["z_near"][b], g["z_far"][b])
        np.testing.assert_allclose(r32, r64, rtol=0, atol=3e-7)
    n32, n64 = synth.depth2normal(g["dmap"], g["intrinsics"]), sr.depth2normal64(g["dmap"], g["intrinsics"])
    assert np.array_equal(np.isnan(n32), np.isnan(n64))
    np.testing.assert_allclose(np.nan_to_num(n32), np.nan_to_num(n64), rtol=0, atol=2e-5)
    if W >= 8:
        fg = g["dmap"][:, 0] != 0
        assert fg[:, H // 2, 4].all() and not fg[:, H // 2 - 1, 4].any() and not fg[:, H // 2, 3].any()     # the isolated pixel
