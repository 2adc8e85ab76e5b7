"""The host restatement of the NOVEL renderers' sampler (tests/novel_sampler_ref.py) proved on the CPU: it is the oracle on the true
rays when nothing is deformed, it meets what the unmodified reference renderer recorded (tests/golden/novel_sampler.npz, written by
tools/gen_novel_sampler_golden.py), and the offsets matter on every case the GPU tests run -- so a sampler that ignores them cannot
pass there.  And the C ABI of the new entry point: declared, exported, bound, and refusing bad arguments before any launch.
"""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from synthetic import synth
from tests import knn_ref
from tests import novel_sampler_ref as N
from tests import stage_refs as sr

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "novel_sampler.npz"
F32 = np.float32
IDS = [c.id for c in N.GRID]


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["index"]))


@pytest.mark.parametrize("case", N.GRID, ids=IDS)
def test_zero_offsets_are_the_oracle_on_the_true_rays(case):
    """pseudo-rays through the undeformed points: Oracle.likelihood of the rays, bit for bit"""
    c = case.refs()
    pts = knn_ref.ray_points(c.rays, c.z_cand).reshape(c.SB, c.NR, c.NC, 3)
    for s, sc in enumerate(c.scenes):
        got = N.likelihood(sc, c.rays[s], pts[s])
        assert np.array_equal(got.view(np.uint32), c.L_plain[s].view(np.uint32))
        assert (got > 0).any(-1).sum() >= 5


@pytest.mark.parametrize("case", N.GRID, ids=IDS)
def test_the_offsets_change_the_likelihood_of_a_quarter_of_the_rays(case):
    c = case.refs()
    for s in range(c.SB):
        share = float((c.L[s] != c.L_plain[s]).any(-1).mean())
        print(f"{c.id}[{s}]: the offsets change the likelihood on {share:.3f} of {c.NR} rays")
        assert share >= 0.25


@pytest.mark.parametrize("name", sorted(N.GOLDEN_CASES))
def test_restatement_meets_the_reference(name, golden):
    """on the reference's recorded run: the same candidates and vertex indices, its likelihood under compare_likelihood, its z_dg under
    compare_decisions of its own likelihood (gaussian bound: 4 x the float32 oracle's error on the same rays, undeformed, + 2e-6 -- the
    moments are the same sums over the same depths, so that error is the scale of any float32 evaluation's), its fill-up bit for bit"""
    from oracle.oracle import Oracle
    g, index = golden
    c = N.GOLDEN_CASES[name].refs()
    ix = index[name]
    assert (ix["NC"], ix["K"], ix["G"], ix["NV"], ix["V"], ix["NR"]) == (c.NC, c.K, c.G, c.NV, c.V, c.NR)
    rec = lambda k: g[f"{name}.{k}"]
    for k, mine in (("rays", c.rays), ("vertices", c.vertices), ("offsets_in", c.offsets), ("n_gauss", c.n_gauss), ("u_fill", c.u_fill)):
        assert np.array_equal(rec(k), mine), k
    # u_coarse is not stored: the seeded draw reproduces the recorded candidates through the oracle's sample_coarse
    assert np.array_equal(synth.make_noise(c.NR, c.NC, c.G, c.K, seed=ix["noise_seed"])[0], c.u_coarse[0])
    np.testing.assert_allclose(rec("z_cand"), c.z_cand, rtol=0, atol=2.5e-7 * float(c.rays[..., 7].max()))
    assert np.array_equal(rec("idx"), c.idx)
    K, G = c.K, c.G
    lik, z_dg, z = rec("likelihood")[0], rec("z_dg")[0], rec("z")[0]
    assert sr.compare_likelihood(lik, c.L[0].astype(np.float64)) == []
    assert (lik > 0).any(-1).sum() >= 20 and (lik == 0).all(-1).sum() >= 5
    orc_z, orc_L = Oracle(c.scenes[0], None).sample_depthguided(c.rays[0], c.z_cand[0], K, G, c.n_gauss[0], want_L=True)
    tol, cpu_err = sr.gauss_bound(orc_z, sr.select_rows(orc_L, c.z_cand[0], K, G, c.n_gauss[0])[0], K, G)
    own, hit = sr.select_rows(lik, rec("z_cand")[0], K, G, c.n_gauss[0])
    print(f"{name}: gaussian slots: oracle err {cpu_err:.2e} bound {tol:.2e} reference err {sr.gauss_error(z_dg, own, K, G):.2e}")
    assert sr.compare_decisions(z_dg, own, hit, K, G, tol) == []
    # ... and the restated likelihood decides hit / no-hit as the reference's does on every ray.  (Its short-list is NOT compared: the
    # two likelihoods differ by an ulp on 0.2 % of the values, which reorders candidates at a cut on some rays of both cases.)
    _, mine_hit = sr.select_rows(c.L[0], c.z_cand[0], K, G, c.n_gauss[0])
    assert np.array_equal(mine_hit, hit)
    assert np.array_equal(sr.fill_up_f32(z_dg, c.rays[0], c.u_fill[0]), z)
    # the stand-in model's compositing on the recorded z: float64 restatement within the project's 1e-4
    import torch
    pts = knn_ref.ray_points(c.rays, z[None])
    idx, _ = knn_ref.nearest_batch(pts, c.vertices)
    a, b = knn_ref.deform(pts, idx, c.offsets), knn_ref.deform(pts, idx, rec("offsets_gen"))
    dirs = np.repeat(c.rays[:, :, None, 3:6], K, 2).reshape(1, c.NR * K, 3)
    out = N.standin_model_np(a, b, dirs).reshape(c.NR, K, 4)
    w, rgb, depth = sr.composite_ref(torch.from_numpy(c.rays[0]), torch.from_numpy(z), torch.from_numpy(out), True)
    for got, want in ((w, rec("weights")[0]), (rgb, rec("rgb")[0]), (depth, rec("depth")[0])):
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-4)
    assert float(rec("weights").sum(-1).max()) > 0.5 and float(out[..., 3].max()) > 5


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
NAME = "diner_sample_depthguided_points"


def test_entry_point_is_declared_built_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    mk = (ROOT / "diner_amd" / "csrc" / "Makefile").read_text()
    assert "sampler_points.hip" in mk and "sampler_blocks.hpp" in mk
    m = re.search(rf"\b{NAME}\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m and m.group(1).count(",") + 1 == 13 == len(_lib.SYMBOLS[NAME][1])
    L = _lib.lib()
    assert getattr(L, NAME)
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 3 == L.diner_version()
    import diner_amd
    import diner_amd.novel as novel
    assert issubclass(novel.NeRFRendererDGS, diner_amd.NeRFRendererDGS) and novel.NeRFRendererDGS is not diner_amd.NeRFRendererDGS


def test_bad_arguments_return_codes_before_any_launch():
    from diner_amd import _lib
    L = _lib.lib()
    p = 64                                                              # a non-NULL dummy, never dereferenced
    err = lambda: L.diner_last_error()

    def scene(**kw):
        sc = _lib.DinerScene()
        sc.SB, sc.NV, sc.H, sc.W, sc.image_w, sc.image_h = 1, 2, 8, 8, 8.0, 8.0
        sc.poses = sc.focal = sc.c = sc.maps = p
        for k, v in kw.items():
            setattr(sc, k, v)
        return sc

    def cfg(NC=64, K=8, G=4):
        c = _lib.DinerSamplerCfg()
        c.n_candidates, c.n_samples, c.n_gaussian, c.depth_diff_max = NC, K, G, 0.05
        return c

    def call(sc=None, c=None, rays=p, z_cand=p, xyz=p, NR=5, z_out=p):
        sc, c = sc or scene(), c or cfg()
        return getattr(L, NAME)(C.byref(sc), rays, z_cand, xyz, NR, C.byref(c), None, None, 1, z_out, None, None, None)

    assert call(z_cand=None) == -1 and b"z_cand" in err()
    assert call(xyz=None) == -1 and b"xyz_cand" in err()
    assert call(rays=None) == -1 and call(z_out=None) == -1
    assert call(c=cfg(NC=4097)) == -3 and b"4096" in err()
    assert call(c=cfg(K=8, G=9)) == -1 and b"n_gaussian" in err()          # K < G
    assert call(c=cfg(NC=0)) == -1 and call(c=cfg(K=0)) == -1
    assert call(NR=-1) == -1
    assert call(sc=scene(maps=None)) == -1 and call(sc=scene(NV=0)) == -1
    assert getattr(L, NAME)(None, p, p, p, 5, C.byref(cfg()), None, None, 1, p, None, None, None) == -1
    assert getattr(L, NAME)(C.byref(scene()), p, p, p, 5, None, None, None, 1, p, None, None, None) == -1
    assert call(NR=0, rays=None, z_cand=None, xyz=None, z_out=None) == 0   # nothing to do, whatever the pointers
    assert call(sc=scene(SB=0), rays=None, z_cand=None, xyz=None, z_out=None) == 0
