"""CPU proof of tests/philox_ref.py, the restatement tests/test_gpu_philox.py holds the sampler's in-kernel noise to: known answers of
Philox4x32-10 (against a second, scalar implementation as well), distinct counters, the statistics of the three streams as designed,
and the rejection of every listed wrong variant by the comparisons the GPU tests use, applied to the oracle's CPU stages.  No GPU.

Statistics: every bound is analytic at 5 sigma of the estimator under the null hypothesis (independent U[0,1) / N(0,1) draws), on
102400 draws per stream (400 rays x 256 columns) and the three call seeds of STAT_SEEDS; the outcome is deterministic.
  mean of U: sqrt(1/12/n);  variance of U: sqrt((1/80 - 1/144)/n);  mean of N: sqrt(1/n);  variance of N: sqrt(2/n);
  fourth moment of N: sqrt((105 - 9)/n);  a correlation coefficient of n pairs: 1/sqrt(n).
  Kolmogorov distance of n draws from Phi: the Dvoretzky-Kiefer-Wolfowitz inequality (Massart's constant) P(D > e) <= 2 exp(-2 n e^2)
  holds for every n; at the two-sided 5 sigma level p = erfc(5/sqrt 2) = 5.7e-7 it gives e = sqrt(ln(2/p) / (2 n)) = 2.745/sqrt(n)
  = 8.58e-3 for n = 102400.  (The 24-bit grid of the uniforms moves none of these by more than 2^-24.)
"""
import math

import numpy as np
import pytest
import torch

from tests import philox_ref as pr
from tests import stage_refs as sr

F32 = np.float32
STAT_SEEDS = (pr.call_seed(0, 1), pr.call_seed(1, 1), pr.call_seed(3, 2))     # 1, 0x9E3779B97F4A7C16, 0xDAA66D2C7DDF7441
ROWS, COLS = 400, 256
N = ROWS * COLS
KS_LEVEL = math.erfc(5 / math.sqrt(2))


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------------
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox_scalar(ctr, key):
    """the round function of csrc/common.hpp on Python integers: a second implementation"""
    x, y, z, w = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x, 0xCD9E8D57 * z
        x, y, z, w = (p1 >> 32) ^ y ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ w ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return x, y, z, w


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_known_answers(ctr, key, want):
    assert tuple(int(v) for v in pr.philox4x32(ctr, key)) == want
    assert philox_scalar(ctr, key) == want


def test_vectorised_equals_scalar_on_the_dense_layouts():
    """single elements of the dense tensors from the scalar implementation and the counter table, written out once more"""
    rs = np.random.RandomState(0)
    for seed in STAT_SEEDS:
        key = (seed & 0xFFFFFFFF, seed >> 32)
        uc, uf = pr.u_coarse(seed, 40, 4096), pr.u_fill(seed, 40, 256)
        u1, u2 = pr.gauss_uniforms(seed, 40, 256)
        for _ in range(200):
            g, j, i = int(rs.randint(40)), int(rs.randint(4096)), int(rs.randint(256))
            w = philox_scalar(((j & 63) | ((j >> 8) << 6), 0, g, 0), key)[(j >> 6) & 3]
            assert uc[g, j] == F32((w >> 8) / 16777216.0)
            w = philox_scalar((i, 1, g, 0), key)
            assert u1[g, i] == F32((w[0] >> 8) / 16777216.0) and u2[g, i] == F32((w[1] >> 8) / 16777216.0)
            assert uf[g, i] == F32((philox_scalar((i, 2, g, 0), key)[0] >> 8) / 16777216.0)
    # a row index beyond 2^32 reaches counter word 3
    big = (1 << 32) + 5
    a = pr.u_fill(7, 1, 8, gray=[big])
    assert a[0, 3] == F32((philox_scalar((3, 2, 5, 1), (7, 0))[0] >> 8) / 16777216.0)
    assert not np.array_equal(a, pr.u_fill(7, 1, 8, gray=[5]))


def test_call_seed_is_the_renderers_rule():
    from diner_amd.renderer import NeRFRendererDGS
    for seed, calls in pr.SEEDS + ((0xFFFFFFFFFFFFFFFF, 3), (12345678901234567, 40)):
        r = NeRFRendererDGS.__new__(NeRFRendererDGS)       # (_next_seed reads two plain attributes)
        r.__dict__.update(seed=seed, _calls=calls - 1)
        assert NeRFRendererDGS._next_seed(r) == pr.call_seed(seed, calls)
    got = [pr.call_seed(*s) for s in pr.SEEDS]
    assert got == [1, 0x9E3779B97F4A7C16, 0xDAA66D2C7DDF7441, 0x3C6EF372FE94F82F, 7]
    assert any(s >= 1 << 63 for s in got) and any(s < 1 << 32 for s in got)
    cases = {c.call_seed for c in pr.PHILOX_CASES}
    assert any(s >= 1 << 63 for s in cases) and any(s < 1 << 32 for s in cases)


# ---- layout ------------------------------------------------------------------------------------------------------------------
def test_counters_of_one_ray_are_pairwise_distinct():
    x, comp = pr.candidate_counter(np.arange(4096))
    triples = [(int(a), pr.STREAM_CANDIDATES, int(c)) for a, c in zip(x, comp)]
    triples += [(i, pr.STREAM_GAUSS, c) for i in range(256) for c in (0, 1)]
    triples += [(rank, pr.STREAM_FILL, 0) for rank in range(256)]
    assert len(set(triples)) == len(triples) == 4096 + 512 + 256
    assert x.max() < 1 << 10 and set(comp.tolist()) == {0, 1, 2, 3}
    # and the wrong variants are not: the comparison below can tell them apart
    xd, cd = pr.candidate_counter(np.arange(4096), "always_x")
    assert len({(int(a), int(c)) for a, c in zip(xd, cd)}) == 1024
    xd, cd = pr.candidate_counter(np.arange(4096), "shift6")
    assert not np.array_equal(xd, x) and np.array_equal(xd[:64], x[:64])


def test_rows_differ_between_rays_seeds_and_key_halves():
    for fn, n in ((pr.u_coarse, 200), (pr.u_fill, 40), (lambda *a, **k: pr.n_gauss64(*a, **k), 15)):
        a = np.asarray(fn(STAT_SEEDS[1], 64, n))
        assert len({row.tobytes() for row in a}) == 64                       # rows of different gray
        assert (a[:-1] != a[1:]).mean() > 0.99
        b = np.asarray(fn(STAT_SEEDS[1] + 1, 64, n))                         # another seed
        assert (a != b).mean() > 0.99
        hi = np.asarray(fn(STAT_SEEDS[1] ^ (1 << 40), 64, n))                # the same low word, another high word
        assert (a != hi).mean() > 0.99
        assert np.array_equal(np.asarray(fn(STAT_SEEDS[1] ^ (1 << 40), 64, n, defect="ignore_key_hi")),
                              np.asarray(fn(STAT_SEEDS[1], 64, n, defect="ignore_key_hi")))


# ---- statistics --------------------------------------------------------------------------------------------------------------
def _streams(seed):
    return dict(coarse=pr.u_coarse(seed, ROWS, COLS).astype(np.float64), fill=pr.u_fill(seed, ROWS, COLS).astype(np.float64),
                gauss=pr.n_gauss64(seed, ROWS, COLS))


_stream_cache = {}


def streams(seed):
    if seed not in _stream_cache:
        _stream_cache[seed] = _streams(seed)
    return _stream_cache[seed]


@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_uniform_streams_mean_and_variance(seed):
    for name in ("coarse", "fill"):
        u = streams(seed)[name]
        assert u.size == N >= 100000 and u.min() >= 0 and u.max() < 1
        assert abs(u.mean() - 0.5) <= 5 * math.sqrt(1 / 12 / N), name
        assert abs(u.var() - 1 / 12) <= 5 * math.sqrt((1 / 80 - 1 / 144) / N), name


@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_gaussian_stream_moments_and_kolmogorov_distance(seed):
    n = streams(seed)["gauss"]
    assert n.size == N and np.isfinite(n).all()
    assert abs(n.mean()) <= 5 * math.sqrt(1 / N)
    assert abs(n.var() - 1) <= 5 * math.sqrt(2 / N)
    assert abs((n ** 4).mean() - 3) <= 5 * math.sqrt(96 / N)
    x = np.sort(n.ravel())
    cdf = 0.5 * (1 + torch.erf(torch.from_numpy(x / math.sqrt(2))).numpy())
    k = np.arange(1, N + 1)
    D = max(float((k / N - cdf).max()), float((cdf - (k - 1) / N).max()))
    bound = math.sqrt(math.log(2 / KS_LEVEL) / (2 * N))
    print(f"seed {seed:#x}: Kolmogorov distance {D:.3e}, bound {bound:.3e}")
    assert abs(bound - 8.58e-3) < 1e-5 and D <= bound
    # float32 evaluation of the same draws: the error the gaussian bound of the GPU test is built from
    err = np.abs(pr.n_gauss32(seed, ROWS, COLS).astype(np.float64) - n).max()
    print(f"seed {seed:#x}: max |n_gauss32 - n_gauss64| = {err:.2e}")
    assert err <= 5e-6


def _corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1]), a.size


@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_lag_one_correlations(seed):
    s = streams(seed)
    pairs = {}
    for name, a in s.items():
        pairs[f"{name}: inside a row"] = _corr(a[:, :-1], a[:, 1:])
        pairs[f"{name}: rows gray and gray + 1"] = _corr(a[:-1], a[1:])
    # the three streams of one ray: the same counter word x (j = i = rank < 64), the stream word alone tells them apart
    pairs["coarse / gauss"] = _corr(s["coarse"], s["gauss"])
    pairs["coarse / fill"] = _corr(s["coarse"], s["fill"])
    pairs["gauss / fill"] = _corr(s["gauss"], s["fill"])
    u1, u2 = pr.gauss_uniforms(seed, ROWS, COLS)
    pairs["gauss: u1 / u2 of one slot"] = _corr(u1, u2)
    nxt = streams((seed + 1) & 0xFFFFFFFFFFFFFFFF)
    for name, a in s.items():
        pairs[f"{name}: call seeds k and k + 1"] = _corr(a, nxt[name])
    for what, (r, n) in pairs.items():
        assert n >= 100000 - ROWS - COLS
        assert abs(r) <= 5 / math.sqrt(n), (what, r, 5 / math.sqrt(n))


def test_a_reused_counter_would_show_in_these_statistics():
    """the statistics can fail: with the stream word ignored, candidates and fill-up of a ray are the same numbers"""
    seed = STAT_SEEDS[1]
    r, n = _corr(pr.u_coarse(seed, ROWS, 64, defect="ignore_stream"), pr.u_fill(seed, ROWS, 64, defect="ignore_stream"))
    assert r > 0.999
    a = pr.u_coarse(seed, ROWS, COLS, defect="always_x")       # 4 candidates of a lane share one draw
    assert _corr(a[:, :64], a[:, 64:128])[0] > 0.999


# ---- every comparison rejects the wrong variants -------------------------------------------------------------------------------
def cpu_stages(c, noise):
    """the oracle's stages on a SamplerCase with the dense noise given: -> likelihood [SB,NR,NC], z_cand, z_dg [SB,NR,K], z [SB,NR,K]"""
    from oracle.oracle import Oracle
    u_c, n_g, u_f = noise
    out = dict(L=[], z_cand=[], z_dg=[], z=[])
    for s, scene in enumerate(c.scenes):
        orc = Oracle(scene, None)
        zc = orc.sample_coarse(c.rays[s], c.NC, u_c[s])
        z_dg, L = orc.sample_depthguided(c.rays[s], zc, c.K, c.G, n_g[s], want_L=True)
        for k, v in (("L", L), ("z_cand", zc), ("z_dg", z_dg), ("z", orc.fill_up(c.rays[s], z_dg, u_f[s]))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


REJECT_CASES = [c for c in pr.PHILOX_CASES if c.id in ("NC200-K40-G15-SB2-seed3-call2", "NC1024-K256-G96-SB1-seed0-call1")]
_right = {}


def right(pc):
    if pc.id not in _right:
        c = pc.build()
        _right[pc.id] = cpu_stages(c, (c.u_coarse, c.n_gauss, c.u_fill))
    return _right[pc.id]


@pytest.mark.parametrize("pc", pr.PHILOX_CASES, ids=[c.id for c in pr.PHILOX_CASES])
def test_cases_keep_the_precondition(pc):
    c = pc.build()
    assert c.rays.shape[1] <= 400 and c.u_coarse.shape == (pc.SB, c.rays.shape[1], pc.NC)
    for s in range(pc.SB):
        assert c.surface[s].sum() >= 20 and (~c.surface[s]).sum() >= 5, (int(c.surface[s].sum()), int((~c.surface[s]).sum()))
    if pc.G:
        assert 0 < pc.n32_err <= 5e-6 and pc.dn == sr.MARGIN * pc.n32_err


def test_case_set_covers_the_issue():
    cs = pr.PHILOX_CASES
    assert {c.NC for c in cs} == {63, 200, 1024, 2048, 4096} and {c.SB for c in cs} == {1, 2}
    assert {(c.K, c.G) for c in cs} == {(16, 5), (40, 15), (128, 48), (256, 96), (12, 0), (12, 12)}
    assert {(c.seed, c.calls) for c in cs} == set(pr.SEEDS)
    assert len(REJECT_CASES) == 2 and REJECT_CASES[0].call_seed >> 32 != 0
    # rays with some slots kept and some empty (rank != slot index in the fill-up), K <= 64 and K > 64
    partial = {c.id: int(((c.build().orc_z_dg == 0).any(-1) & (c.base.orc_z_dg != 0).any(-1)).sum()) for c in cs}
    assert sum(n >= 20 for i, n in partial.items() if "-K16-" in i or "-K40-" in i or "-K12-G0" in i) >= 3, partial
    assert sum(n >= 20 for i, n in partial.items() if "-K128-" in i or "-K256-" in i) >= 3, partial
    assert all(partial[c.id] >= 20 for c in REJECT_CASES), partial


def test_float32_gaussian_passes_the_gaussian_comparison():
    """the right one passes: the oracle's stages on n_gauss32 against those on n_gauss64, within the bound built from their difference"""
    for pc in REJECT_CASES:
        c, ok = pc.build(), right(pc)
        n32 = pr.n_gauss32(pc.call_seed, pc.SB * c.rays.shape[1], pc.G).reshape(c.n_gauss.shape)
        got = cpu_stages(c, (c.u_coarse, n32, c.u_fill))
        keep = pc.K - pc.G
        for s in range(pc.SB):
            gstd = pr.gauss_std(ok["L"][s], ok["z_cand"][s], pc.K, pc.G)
            assert (gstd[c.surface[s]] > 0).sum() >= 20 and (gstd >= 0).all()
            assert pr.compare_bits(got["z_dg"][s][:, :keep], ok["z_dg"][s][:, :keep], "short-list") == []
            assert pr.compare_gauss(got["z_dg"][s][:, keep:], ok["z_dg"][s][:, keep:], gstd, pc.dn, "gaussian slots")[0] == []
            assert pr.compare_gauss(got["z"][s], ok["z"][s], gstd, pc.dn, "z")[0] == []


@pytest.mark.parametrize("defect", pr.DEFECTS)
def test_comparisons_reject(defect):
    """one stream at a time from the wrong restatement, the other two right, through the oracle's stages: the comparison that the GPU
    test makes for that stream must report it"""
    hits = {"candidates": ("always_x", "shift6", "ignore_key_hi"), "gaussian": ("ignore_stream", "ignore_key_hi"),
            "fill-up": ("ignore_stream", "ignore_key_hi", "rank_as_slot")}
    n = 0
    for pc in REJECT_CASES:
        if defect == "ignore_key_hi" and pc.call_seed >> 32 == 0:
            continue                                       # (key word 1 is zero there: nothing to ignore)
        c, ok = pc.build(), right(pc)
        SB, NR, K, G, keep = pc.SB, c.rays.shape[1], pc.K, pc.G, pc.K - pc.G
        bad = pr.noise(pc.call_seed, SB, NR, pc.NC, K, G, defect, z_dg=ok["z_dg"].reshape(SB * NR, K))
        if defect in hits["candidates"]:
            got = cpu_stages(c, (bad[0], c.n_gauss, c.u_fill))
            for k in ("L", "z_dg", "z"):
                assert pr.compare_bits(got[k], ok[k], k), (defect, pc.id, k)
            n += 1
        if defect in hits["fill-up"]:
            got = cpu_stages(c, (c.u_coarse, c.n_gauss, bad[2]))
            assert pr.compare_bits(got["z_dg"], ok["z_dg"], "z_dg") == []
            assert pr.compare_bits(got["z"], ok["z"], "z"), (defect, pc.id)
            n += 1
        if defect in hits["gaussian"]:
            got = cpu_stages(c, (c.u_coarse, bad[1], c.u_fill))
            for s in range(SB):
                gstd = pr.gauss_std(ok["L"][s], ok["z_cand"][s], K, G)
                assert pr.compare_gauss(got["z_dg"][s][:, keep:], ok["z_dg"][s][:, keep:], gstd, pc.dn, "gaussian slots")[0], (defect, pc.id)
                assert pr.compare_gauss(got["z"][s], ok["z"][s], gstd, pc.dn, "z")[0], (defect, pc.id)
            n += 1
    assert n >= 1
