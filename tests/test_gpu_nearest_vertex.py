"""The nearest-vertex search and the NOVEL renderers' deformation on the MI355X (diner_amd/csrc/nearest_vertex.hip; glue.nearest_vertex,
glue.deform_points, glue.deform_ray_points; diner_amd.compat.knn_points):

* both kernels bit-equal -- idx and d2, every point, no exclusions -- to the fp32 contract restated in tests/knn_ref.py and to each
  other, at the sizes where they can go wrong: V around the cluster size of 64 and beyond one LDS tile of either kernel, N around the
  workgroup size of 256, the point count from which the brute-force kernel holds 4 points per thread, one scene and two with
  different vertex sets; points inside the mesh's box, out to 2.0 from it and exactly on vertices (d2 = 0); degenerate vertex sets;
* the fused deformation bit-equal to the gather / add restatement and to the golden of the unmodified reference;
* two runs bit-equal, the cluster cache, non-contiguous input, the pytorch3d stand-in, the autograd rules.

The contract is IEEE fp32 without contraction: the device has no freedom, so every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import knn_ref as R

pytestmark = pytest.mark.gpu

N_SIZES = (1, 255, 257, 5000)            # NV_THREADS = 256 points per workgroup
V_SIZES = (1, 63, 64, 65, 1000, 4097)    # clusters of 64; 1024 vertices per LDS tile of the brute-force kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_refs = {}


def case(V, N=5000, reach=2.0):
    """two scenes with different vertex sets, N points each, and the contract's result: computed once per case and left unchanged"""
    if (V, N) not in _refs:
        verts = np.stack([R.sphere_mesh(V, seed=V), R.sphere_mesh(V, seed=V + 7, radius=0.11, centre=(-0.03, 0.02, 0.0))])
        pts = np.stack([R.points_around(verts[sb], N, seed=V + sb, reach=reach) for sb in range(2)])
        _refs[(V, N)] = (verts, pts, R.nearest_batch(pts, verts))
    return _refs[(V, N)]


def check_search(glue, dev, verts, pts, want, methods=("brute", "clusters", "auto")):
    v, p = T(verts, dev), T(pts, dev)
    for m in methods:
        idx, d2 = glue.nearest_vertex(p, v, method=m)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == pts.shape[:2]
        idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
        diff = int((idx != want[0]).sum()), int((bits(d2) != bits(want[1])).sum())
        assert diff == (0, 0), f"{m}: V={verts.shape[1]} N={pts.shape[1]} SB={pts.shape[0]}: idx / d2 differ at {diff} points"


@pytest.mark.parametrize("V", V_SIZES)
def test_both_kernels_are_bit_equal_to_the_contract(V, dev):
    from diner_amd import glue
    verts, pts, (widx, wd2) = case(V)
    on = (pts[0][:, None, :] == verts[0][None, :, :]).all(-1).any(1)
    assert on.sum() > 1000 and (wd2[0][on] == 0).all()                     # points exactly on vertices: d2 = 0
    for SB in (1, 2):
        for N in N_SIZES:
            check_search(glue, dev, verts[:SB], pts[:SB, :N], (widx[:SB, :N], wd2[:SB, :N]))
    assert not np.array_equal(verts[0], verts[1])                           # the scenes' vertex sets differ: a wrong stride shows
    # two runs give the same bits
    v, p = T(verts, dev), T(pts, dev)
    for m in ("brute", "clusters"):
        a, b = glue.nearest_vertex(p, v, method=m), glue.nearest_vertex(p, v, method=m)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_four_points_per_thread_and_tiled_boxes(dev):
    """the two paths the sizes above do not reach: the brute-force kernel with 4 points per thread (from 2 x 256 workgroups of 1024
    points on) and the pruned kernel with more clusters than one LDS tile of boxes holds (1024)"""
    from diner_amd import glue
    verts = R.sphere_mesh(63, seed=63)[None]
    N = 2 * 256 * 1024 + 3
    pts = R.points_around(verts[0], N, seed=1, reach=2.0)[None]
    check_search(glue, dev, verts, pts, R.nearest_batch(pts, verts, chunk=16384), methods=("brute", "clusters"))
    V = 1024 * 64 + 500                                                     # 1032 clusters: two tiles, the second ragged
    verts = np.stack([R.sphere_mesh(V, seed=2), R.sphere_mesh(V, seed=3, radius=0.2)])
    pts = np.stack([R.points_around(verts[sb], 257, seed=4 + sb, reach=2.0) for sb in range(2)])
    check_search(glue, dev, verts, pts, R.nearest_batch(pts, verts, chunk=64), methods=("brute", "clusters"))


@pytest.mark.parametrize("name", ("duplicated", "coplanar", "colinear", "identical"))
def test_degenerate_vertex_sets(name, dev):
    from diner_amd import glue
    verts = R.degenerate_sets()[name]
    pts = R.points_around(verts, 900, seed=21, reach=0.5)
    want = R.brute_f32(pts, verts)
    if name == "duplicated":
        assert (want[0] < verts.shape[0] // 2).all()
    check_search(glue, dev, verts[None], pts[None], (want[0][None], want[1][None]), methods=("brute", "clusters"))
    mv, mp = R.mirror_set()                                                  # a tie behind a bound that equals the best
    check_search(glue, dev, mv[None], mp[None], tuple(x[None] for x in R.brute_f32(mp, mv)), methods=("brute", "clusters"))


def golden():
    import json
    from pathlib import Path
    d = dict(np.load(Path(__file__).resolve().parent / "golden" / "deform_points.npz", allow_pickle=False))
    return json.loads(str(d.pop("index"))), d


@pytest.mark.parametrize("method", ("brute", "clusters"))
def test_deform_points_reproduces_the_reference_golden(method, dev):
    from diner_amd import glue
    index, d = golden()
    for name in index:
        p, v = T(d[f"{name}.points"], dev), T(d[f"{name}.vertices"], dev)
        o1, o2 = T(d[f"{name}.offsets"], dev), T(d[f"{name}.offsets2"], dev)
        one = glue.deform_points(p, v, o1, method=method)
        assert isinstance(one, torch.Tensor) and np.array_equal(bits(one.cpu().numpy()), bits(d[f"{name}.deformed"]))
        a, b = glue.deform_points(p, v, o1, o2, method=method)
        assert np.array_equal(bits(a.cpu().numpy()), bits(d[f"{name}.deformed"]))
        assert np.array_equal(bits(b.cpu().numpy()), bits(d[f"{name}.deformed2"]))
        idx, _ = glue.nearest_vertex(p, v, method=method)
        assert np.array_equal(idx.cpu().numpy(), d[f"{name}.idx"])


def test_deform_points_against_the_restatement(dev):
    from diner_amd import glue
    verts, pts, (widx, _) = case(4097)
    g = np.random.default_rng(8)
    o1, o2 = (0.02 * g.normal(size=(2,) + verts.shape)).astype(np.float32)
    for SB, N in ((1, 257), (2, 5000)):
        want1, want2 = R.deform(pts[:SB, :N], widx[:SB, :N], o1[:SB]), R.deform(pts[:SB, :N], widx[:SB, :N], o2[:SB])
        for m in ("brute", "clusters", "auto"):
            a, b = glue.deform_points(T(pts[:SB, :N], dev), T(verts[:SB], dev), T(o1[:SB], dev), T(o2[:SB], dev), method=m)
            assert np.array_equal(bits(a.cpu().numpy()), bits(want1)) and np.array_equal(bits(b.cpu().numpy()), bits(want2))
            one = glue.deform_points(T(pts[:SB, :N], dev), T(verts[:SB], dev), T(o2[:SB], dev), method=m)
            assert np.array_equal(bits(one.cpu().numpy()), bits(want2))


@pytest.mark.parametrize("K", (1, 40))
@pytest.mark.parametrize("B", (1, 65))
def test_deform_ray_points(B, K, dev):
    from diner_amd import glue
    V, SB = 1000, 2
    verts = case(V)[0]
    g = np.random.default_rng(B * 100 + K)
    rays = np.zeros((SB, B, 8), np.float32)
    rays[..., :3] = g.normal(size=(SB, B, 3)) * 0.05 + np.array([0.0, 0.0, -1.6])
    d = g.normal(size=(SB, B, 3)) * 0.06 + np.array([0.0, 0.0, 1.0])
    rays[..., 3:6] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays[..., 6], rays[..., 7] = 1.0, 2.5
    z = np.sort(g.uniform(1.0, 2.5, size=(SB, B, K)), -1).astype(np.float32)
    o1, o2 = (0.02 * g.normal(size=(2,) + verts.shape)).astype(np.float32)
    pts = R.ray_points(rays, z)
    widx, _ = R.nearest_batch(pts, verts)
    want1, want2 = R.deform(pts, widx, o1), R.deform(pts, widx, o2)
    for m in ("brute", "clusters"):
        a, b, p = glue.deform_ray_points(T(rays, dev), T(z, dev), T(verts, dev), T(o1, dev), T(o2, dev), return_points=True, method=m)
        assert a.shape == b.shape == p.shape == (SB, B * K, 3)
        assert np.array_equal(bits(p.cpu().numpy()), bits(pts))
        assert np.array_equal(bits(a.cpu().numpy()), bits(want1)) and np.array_equal(bits(b.cpu().numpy()), bits(want2))
        one = glue.deform_ray_points(T(rays, dev), T(z, dev), T(verts, dev), T(o1, dev), method=m)
        assert isinstance(one, torch.Tensor) and np.array_equal(bits(one.cpu().numpy()), bits(want1))
        pair = glue.deform_ray_points(T(rays, dev), T(z, dev), T(verts, dev), T(o1, dev), return_points=True, method=m)
        assert len(pair) == 2 and torch.equal(pair[1], p)


def test_cluster_cache_rebuilds_after_an_in_place_edit(dev):
    from diner_amd import deform, glue
    verts, pts, want = case(1000)
    v, p = T(verts, dev), T(pts[:, :257], dev)
    deform.clear_cache()
    n0 = deform.cluster_builds
    glue.nearest_vertex(p, v, method="clusters")
    glue.nearest_vertex(p, v, method="clusters")
    glue.deform_points(p, v, torch.zeros_like(v), method="clusters")
    assert deform.cluster_builds == n0 + 1                                   # one structure serves them all
    v.mul_(-1.0)                                                             # an in-place edit: another mesh at the same address
    idx, d2 = glue.nearest_vertex(p, v, method="clusters")
    assert deform.cluster_builds == n0 + 2
    widx, wd2 = R.nearest_batch(pts[:, :257], -verts)
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(bits(d2.cpu().numpy()), bits(wd2))
    assert not np.array_equal(widx, want[0][:, :257])
    glue.nearest_vertex(p, v.clone(), method="clusters")                     # another tensor: another structure
    assert deform.cluster_builds == n0 + 3
    deform.clear_cache()


def test_non_contiguous_and_non_fp32_inputs(dev):
    from diner_amd import glue
    verts, pts, (widx, wd2) = case(1000)
    wide = torch.zeros((2, 257, 5), dtype=torch.float32, device=dev)
    wide[..., 1:4] = T(pts[:, :257], dev)
    view = wide[..., 1:4]
    assert not view.is_contiguous()
    for m in ("brute", "clusters"):
        idx, d2 = glue.nearest_vertex(view, T(verts, dev), method=m)
        assert np.array_equal(idx.cpu().numpy(), widx[:, :257]) and np.array_equal(bits(d2.cpu().numpy()), bits(wd2[:, :257]))
        idx, _ = glue.nearest_vertex(view.double(), T(verts, dev).double().transpose(0, 1).contiguous().transpose(0, 1), method=m)
        assert np.array_equal(idx.cpu().numpy(), widx[:, :257])
    empty = glue.nearest_vertex(torch.zeros((2, 0, 3), device=dev), T(verts, dev))
    assert empty[0].shape == (2, 0) and empty[1].shape == (2, 0)


def test_compat_knn_points_returns_pytorch3d_shapes(dev):
    from diner_amd import compat
    verts, pts, (widx, wd2) = case(1000)
    p, v = T(pts[:, :257], dev), T(verts, dev)
    res = compat.knn_points(p, v, K=1)
    dists, idx, nn = res
    assert res._fields == ("dists", "idx", "knn") and nn is None
    assert dists.shape == (2, 257, 1) and dists.dtype == torch.float32 and idx.shape == (2, 257, 1) and idx.dtype == torch.int64
    assert np.array_equal(idx[..., 0].cpu().numpy(), widx[:, :257]) and np.array_equal(bits(dists[..., 0].cpu().numpy()), bits(wd2[:, :257]))
    nn = compat.knn_points(p, v, return_nn=True).knn
    assert nn.shape == (2, 257, 1, 3)
    assert np.array_equal(nn[:, :, 0].cpu().numpy(), np.stack([verts[sb][widx[sb, :257]] for sb in range(2)]))
    # the reference's own lines (src/models/novel/nerf_novel_renderer.py:47-49) on the stand-in's result
    off = torch.randn_like(v)
    closest = off[torch.arange(2).unsqueeze(1), idx.squeeze(), :]
    from diner_amd import glue
    assert torch.equal(p + closest, glue.deform_points(p, v, off))


def test_autograd_rules(dev):
    from diner_amd import glue
    verts, pts, _ = case(1000)
    v, o1, o2 = T(verts, dev), T(verts * 0.1, dev), T(verts * -0.2, dev)
    p = T(pts[:, :257], dev).requires_grad_(True)
    for m in ("brute", "clusters"):
        a, b = glue.deform_points(p, v, o1, o2, method=m)
        ga, gb = torch.randn_like(a), torch.randn_like(b)
        (g,) = torch.autograd.grad([a, b], [p], [ga, gb])
        assert torch.equal(g, ga + gb)                                       # identity to the points, from both outputs
        one = glue.deform_points(p, v, o1, method=m)
        (g,) = torch.autograd.grad(one, p, ga)
        assert torch.equal(g, ga)
        with torch.no_grad():
            assert torch.equal(glue.deform_points(p, v, o1, method=m), one.detach())
    for kw in (dict(offsets=o1.clone().requires_grad_(True)), dict(offsets=o1, offsets2=o2.clone().requires_grad_(True)),
               dict(offsets=o1, target_vertices=v.clone().requires_grad_(True))):
        args = dict(target_vertices=v, offsets2=None)
        args.update(kw)
        with pytest.raises(NotImplementedError, match="requires grad"):
            glue.deform_points(p.detach(), **args)
    rays, z = torch.zeros((2, 3, 8), device=dev), torch.ones((2, 3, 4), device=dev)
    for name in ("rays", "z_samp", "target_vertices", "offsets"):
        args = dict(rays=rays, z_samp=z, target_vertices=v, offsets=o1)
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match="requires grad"):
            glue.deform_ray_points(**args)
        with torch.no_grad():
            assert glue.deform_ray_points(**args).shape == (2, 12, 3)        # data under no_grad
