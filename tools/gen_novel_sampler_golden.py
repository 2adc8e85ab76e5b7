"""Golden vectors of the NOVEL renderer's sampler and compositing (diner_amd/novel.py; diner_amd/csrc/sampler_points.hip).

FROM REFERENCE CODE: the UNMODIFIED ``src.models.novel.nerf_novel_renderer.NeRFRendererDGS`` runs on the CPU against the reference
``PixelNeRF`` holding a synthetic scene's maps and cameras (oracle/ref_harness.py: ``install_stubs``, ``build_model``, ``replay_noise``,
``capture_likelihoods``).  Its one dependency without a build here, ``pytorch3d.ops.knn.knn_points``, is stubbed in ``sys.modules`` by the
fp32 contract search of tests/knn_ref.py (``brute_f32``), so the recorded vertex indices are the ones the device must return.  Nothing
of the reference is copied into this repository.

Recorded per case (tests/novel_sampler_ref.py: GOLDEN_CASES, which also gives the scene, the rays, the mesh and the noise seeds): the
rays, vertices, both offset sets, n_gauss and u_fill, and from the reference z_cand, the vertex indices of the candidates, the likelihood
per candidate (the maximum over views of the captured per-view tensor), z_dg, the filled z, and ``composite`` on that z with the stand-in
model below: weights, rgb, depth.  u_coarse is not stored (random mantissas do not compress; with z_cand it would pass the size limit
of a committed file): it is ``synth.make_noise(NR, NC, G, K, seed=5)[0]``, and the host test holds z_cand to it.

The tool prints how the restatement of tests/novel_sampler_ref.py compares with what it records; tests/test_novel_sampler_host.py asserts it.
Runs only where the reference source tree exists; the tests read the committed ``tests/golden/novel_sampler.npz`` only.

    python tools/gen_novel_sampler_golden.py            # (re)writes tests/golden/novel_sampler.npz
"""
from __future__ import annotations

import json
import sys
import types
from collections import namedtuple
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle.ref_harness import build_model, capture_likelihoods, install_stubs, replay_noise  # noqa: E402
from synthetic import synth  # noqa: E402
from tests import knn_ref as R  # noqa: E402
from tests import novel_sampler_ref as N  # noqa: E402
from tests import stage_refs as sr  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "novel_sampler.npz"
_KNN = namedtuple("KNN", "dists idx knn")
_record = {}


def knn_points_f32(p1, p2, lengths1=None, lengths2=None, K=1, **kw):
    """the fp32 contract search, in pytorch3d's return layout"""
    assert K == 1 and lengths1 is None and lengths2 is None
    idx, d2 = R.nearest_batch(p1.numpy(), p2.numpy())
    _record["idx"] = idx
    return _KNN(torch.from_numpy(d2)[..., None], torch.from_numpy(idx.astype(np.int64))[..., None], None)


def reference_renderer(**kw):
    install_stubs()
    root, ops, knn = (types.ModuleType(n) for n in ("pytorch3d", "pytorch3d.ops", "pytorch3d.ops.knn"))
    knn.knn_points = knn_points_f32
    root.ops, ops.knn = ops, knn
    sys.modules.update({"pytorch3d": root, "pytorch3d.ops": ops, "pytorch3d.ops.knn": knn})
    import matplotlib
    matplotlib.use("Agg")
    from src.models.novel.nerf_novel_renderer import NeRFRendererDGS
    return NeRFRendererDGS(**kw)


def standin_model(in_pts, gen_pts, viewdirs):
    """An analytic point model: a smooth function of the two deformed points and the view direction -> [..,4] = rgb in (0,1) and a
    sigma of order 10 (negative in places: the relu of the compositing).  tests/novel_sampler_ref.py restates it."""
    a, b, d = in_pts, gen_pts, viewdirs
    rgb = 0.5 + 0.5 * torch.sin(3.0 * a + 2.0 * b[..., [1, 2, 0]] + d)
    r2 = (a * a).sum(-1) + 0.5 * (b * b).sum(-1)
    sigma = 12.0 * torch.exp(-4.0 * r2) * (1.2 + torch.cos(5.0 * b[..., 0] + d[..., 2])) - 1.0
    return torch.cat([rgb, sigma[..., None]], -1)


def run_case(c):
    c.build()
    assert c.SB == 1
    K, NC, G, NR = c.K, c.NC, c.G, c.NR
    sc = c.scenes[0]
    nerf = build_model(sc, synth.make_mlp_weights(1))           # (the sampler reads none of the weights)
    rend = reference_renderer(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=True)
    t = torch.from_numpy
    rays, verts, off_in = t(c.rays), t(c.vertices), t(c.offsets)
    off_gen = t((0.03 * np.random.default_rng(2).normal(size=c.offsets.shape)).astype(np.float32))
    u_coarse, n_gauss, u_fill = t(c.u_coarse[0]), t(c.n_gauss[0]), t(c.u_fill[0])
    with torch.no_grad():
        # pass A: which rays have any non-zero likelihood (decides the shape of the randn draw)
        with replay_noise(rand_queue=[u_coarse]):
            zA = rend.sample_depthguided(rays, nerf, K, NC, verts, off_in, n_gaussian=0)
        hit = zA[0, :, 0] != 0
        store = {}
        with replay_noise(rand_queue=[u_coarse], randn_queue=[n_gauss[hit]]), capture_likelihoods(store):
            z_dg = rend.sample_depthguided(rays, nerf, K, NC, verts, off_in, n_gaussian=G)
        idx = _record["idx"].astype(np.int32)                   # [1, NR*NC]: the candidates' vertices
        with replay_noise(rand_queue=[u_coarse]):
            z_cand = rend.sample_coarse(rays, n_coarse=NC)
        zs = z_dg.sort(dim=-1).values.view(-1, K)
        miss = zs == 0
        col_rank = torch.cumsum(miss.int(), dim=-1) - 1
        u_compact = u_fill[torch.where(miss)[0], col_rank[miss]]
        with replay_noise(rand_queue=[u_compact]):
            z_fill = rend.fill_up_uniform_samples(z_dg.clone(), rays)
        weights, rgb, depth = rend.composite(standin_model, rays, z_fill, verts, off_in, off_gen)
    lik = store["pt_likelihood_views"].max(dim=1).values.reshape(1, NR, NC).numpy()
    z_cand, z_dg, z_fill = z_cand.numpy(), z_dg.numpy(), z_fill.numpy()

    # how the restatement compares (asserted by tests/test_novel_sampler_host.py)
    c.refs()
    ng = c.n_gauss[0]
    own, own_hit = sr.select_rows(lik[0], z_cand[0], K, G, ng)
    tol, _ = sr.gauss_bound(z_dg[0].astype(np.float64), own, K, G)
    print(f"{c.id}: NR={NR}, rays with a non-zero likelihood {int((lik[0] > 0).any(-1).sum())}; z_cand bit-equal to the oracle's: "
          f"{np.array_equal(z_cand, c.z_cand)} (max diff {np.abs(z_cand - c.z_cand).max():.2e}); indices equal: {np.array_equal(idx, c.idx)}")
    print(f"  likelihood, reference against restatement: max diff {np.abs(lik[0].astype(np.float64) - c.L[0]).max():.2e}, bit-equal share "
          f"{(lik[0] == c.L[0]).mean():.4f}, findings {sr.compare_likelihood(lik[0], c.L[0].astype(np.float64))}")
    print(f"  decisions, reference z_dg against select_rows of its own likelihood: findings "
          f"{sr.compare_decisions(z_dg[0], own, own_hit, K, G, sr.MARGIN * 1e-6 + sr.FLOOR_GAUSS)}")
    print(f"  fill-up restated bit-equal: {np.array_equal(sr.fill_up_f32(z_dg[0], c.rays[0], c.u_fill[0]), z_fill[0])}; "
          f"rays the offsets change: {((c.L[0] != c.L_plain[0]).any(-1)).mean():.3f}")
    return dict(rays=c.rays, vertices=c.vertices, offsets_in=c.offsets, offsets_gen=off_gen.numpy(), n_gauss=c.n_gauss, u_fill=c.u_fill,
                z_cand=z_cand, idx=idx, likelihood=lik, z_dg=z_dg, z=z_fill, weights=weights.numpy(), rgb=rgb.numpy(), depth=depth.numpy())


def main():
    out, index = {}, {}
    for name, c in N.GOLDEN_CASES.items():
        for k, v in run_case(c).items():
            out[f"{name}.{k}"] = v
        index[name] = dict(NC=c.NC, K=c.K, G=c.G, NV=c.NV, V=c.V, NR=c.NR, noise_seed=5, white_bkgd=True)
    out["index"] = np.array(json.dumps(index))
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN.relative_to(ROOT)} ({GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
