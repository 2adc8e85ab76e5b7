"""The nearest-vertex search and the NOVEL renderers' deformation (diner_amd/csrc/nearest_vertex.hip; glue.nearest_vertex,
glue.deform_points, glue.deform_ray_points; diner_amd.compat) as far as they go without a GPU: the golden of the UNMODIFIED reference
``deform_points`` (tools/gen_deform_golden.py) against the restatements of tests/knn_ref.py, the fp32 contract against float64, the
host emulation of the pruned search against the contract bit for bit, the same comparisons rejecting deliberately wrong forms, and the
new entry points' declarations, bindings and refusals before any launch."""
import inspect
import json
import re
import sys
import types
from pathlib import Path

import numpy as np
import pytest

from tests import knn_ref as R

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("diner_nearest_vertex_workspace_floats", "diner_nearest_vertex_keys", "diner_nearest_vertex_build", "diner_nearest_vertex",
               "diner_deform_points", "diner_deform_ray_points")
REL = 1e-6              # the chosen vertex is never farther than the optimum by more than this, relative, in float64
AMBIGUOUS_CAP = 0.002   # share of points whose best and second-best float64 distances are within REL of each other
_fixture = {}


def fixture():
    if not _fixture:
        d = dict(np.load(ROOT / "tests" / "golden" / "deform_points.npz", allow_pickle=False))
        _fixture["index"] = json.loads(str(d.pop("index")))
        _fixture["data"] = d
    return _fixture["index"], _fixture["data"]


# ---- the golden ------------------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases():
    index, d = fixture()
    assert tuple(index) == ("sb1", "sb2")
    assert [index[n]["SB"] for n in index] == [1, 2]
    for name, c in index.items():
        assert 290 <= c["B"] <= 310 and 125 <= c["V"] <= 135
        assert d[f"{name}.points"].shape == (c["SB"], c["B"], 3) and d[f"{name}.vertices"].shape == (c["SB"], c["V"], 3)
        assert d[f"{name}.offsets"].shape == d[f"{name}.offsets2"].shape == (c["SB"], c["V"], 3)
        assert d[f"{name}.idx"].shape == (c["SB"], c["B"]) and d[f"{name}.idx"].dtype == np.int32
        assert d[f"{name}.deformed"].shape == d[f"{name}.deformed2"].shape == (c["SB"], c["B"], 3)
        assert all(d[f"{name}.{k}"].dtype == np.float32 for k in ("points", "vertices", "offsets", "offsets2", "deformed", "deformed2"))
    assert not np.array_equal(d["sb2.vertices"][0], d["sb2.vertices"][1])         # every scene its own vertex set
    assert (ROOT / "tests" / "golden" / "deform_points.npz").stat().st_size < 100_000


@pytest.mark.parametrize("name", ("sb1", "sb2"))
def test_deform_restatement_reproduces_the_reference_bit_for_bit(name):
    _, d = fixture()
    pts, idx = d[f"{name}.points"], d[f"{name}.idx"]
    assert np.array_equal(R.deform(pts, idx, d[f"{name}.offsets"]), d[f"{name}.deformed"])
    assert np.array_equal(R.deform(pts, idx, d[f"{name}.offsets2"]), d[f"{name}.deformed2"])
    # the recorded indices are the float64 search's, and the fp32 contract finds the same vertices on these inputs
    for sb in range(pts.shape[0]):
        assert np.array_equal(R.brute_f64(pts[sb], d[f"{name}.vertices"][sb])[0], idx[sb])
    assert np.array_equal(R.nearest_batch(pts, d[f"{name}.vertices"])[0], idx)
    # a gather through another scene's offsets, or a shifted index, does not pass
    if pts.shape[0] == 2:
        assert not np.array_equal(R.deform(pts, idx, d[f"{name}.offsets"][::-1]), d[f"{name}.deformed"])
    assert not np.array_equal(R.deform(pts, (idx + 1) % d[f"{name}.vertices"].shape[1], d[f"{name}.offsets"]), d[f"{name}.deformed"])


def test_ray_points_are_a_multiplication_then_an_addition():
    g = np.random.default_rng(3)
    rays = g.normal(size=(2, 5, 8)).astype(np.float32)
    z = g.uniform(1.0, 2.5, size=(2, 5, 7)).astype(np.float32)
    p = R.ray_points(rays, z)
    assert p.shape == (2, 35, 3) and p.dtype == np.float32
    b, k = 3, 4
    want = rays[1, b, :3] + np.float32(z[1, b, k]) * rays[1, b, 3:6]
    assert np.array_equal(p[1, b * 7 + k], want)
    fused = (rays[:, :, None, :3].astype(np.float64) + z[..., None].astype(np.float64) * rays[:, :, None, 3:6]).astype(np.float32)
    assert not np.array_equal(p, fused.reshape(2, 35, 3))           # a fused multiply-add would differ


# ---- (b) against (a) ---------------------------------------------------------------------------------------------------------------------
def compare_to_f64(idx, points, vertices, ref):
    """the failures of a search result against the float64 search `ref` = brute_f64(points, vertices)"""
    ridx, best, second = ref
    bad = []
    chosen = R.dist_f64(points, vertices, idx)
    far = chosen > best * (1.0 + REL)
    if far.any():
        bad.append(f"{int(far.sum())} points got a vertex farther than the optimum by more than {REL:g} relative")
    ambiguous = (second - best) <= REL * best
    if ambiguous.mean() > AMBIGUOUS_CAP:
        bad.append(f"ambiguous share {ambiguous.mean():.3%} above {AMBIGUOUS_CAP:.1%}")
    off = (idx != ridx) & ~ambiguous
    if off.any():
        bad.append(f"{int(off.sum())} indices differ from float64 outside the ambiguous set")
    return bad, float(ambiguous.mean())


_cases = {}


def f64_case(V, reach):
    """(points, vertices, the float64 search, the contract's search), computed once per case"""
    if (V, reach) not in _cases:
        g = np.random.default_rng(V + int(reach * 10))
        verts = R.sphere_mesh(V, seed=V, centre=(0.0, 0.0, 0.0))
        d = g.normal(size=(5000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts = (d * reach * g.uniform(size=(5000, 1)) ** (1 / 3)).astype(np.float32)       # uniform in the ball of radius `reach`
        _cases[(V, reach)] = (pts, verts, R.brute_f64(pts, verts), R.brute_f32(pts, verts))
    return _cases[(V, reach)]


@pytest.mark.parametrize("reach", (0.2, 2.0))
@pytest.mark.parametrize("V", (65, 1000, 4097))
def test_fp32_contract_against_float64(V, reach):
    pts, verts, ref, (idx, d2) = f64_case(V, reach)
    bad, share = compare_to_f64(idx, pts, verts, ref)
    print(f"V={V} reach={reach}: ambiguous share {share:.3%}, index differences {int((idx != ref[0]).sum())}")
    assert bad == []
    assert np.allclose(d2, ref[1], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("variant", ("second_nearest",))
def test_float64_comparison_rejects_wrong_forms(variant):
    pts, verts, ref, _ = f64_case(1000, 0.2)
    idx, _ = R.brute_f32(pts, verts, variant=variant)
    assert (idx != ref[0]).mean() >= 0.009                             # 1 % of the points
    bad, _ = compare_to_f64(idx, pts, verts, ref)
    assert bad, f"{variant} passes the comparison"


# ---- (c) against (b), bit for bit ----------------------------------------------------------------------------------------------------------
def bit_equal(a, b):
    """idx and d2 of two searches, bit for bit"""
    return np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[1], np.float32).view(np.uint32), np.asarray(b[1], np.float32).view(np.uint32))


def _pruned_case(verts, pts, order=None):
    cl = R.build_clusters(verts, order=order)
    assert R.bound_violations(pts, cl) == 0
    return R.pruned_f32(pts, cl), R.brute_f32(pts, verts)


@pytest.mark.parametrize("V", (1, 63, 64, 65, 1000, 4097))
def test_pruned_search_equals_the_contract_on_random_inputs(V):
    verts = R.sphere_mesh(V, seed=V)
    pts = R.points_around(verts, 1500, seed=V + 1)
    cl = R.build_clusters(verts)
    assert cl["C"] == (V + 63) // 64 and sorted(cl["index"][:V].tolist()) == list(range(V))
    assert np.isnan(cl["sorted"][V:]).all() and (cl["index"][V:] == 0).all()
    assert R.bound_violations(pts, cl) == 0
    idx, d2, work = R.pruned_f32(pts, cl, return_work=True)
    want = R.brute_f32(pts, verts)
    assert bit_equal((idx, d2), want)
    on = (pts[:, None, :] == verts[None, :, :]).all(-1).any(1)
    assert on.sum() >= 400 and (d2[on] == 0).all()                   # a point exactly on a vertex
    if V >= 1000:
        print(f"V={V}: clusters scanned per point {work.mean():.1f} of {cl['C']}")
        assert work.mean() < 0.5 * cl["C"]                             # the bound prunes
    # any vertex order gives the same results (the order decides the time only)
    g = np.random.default_rng(V)
    assert bit_equal(R.pruned_f32(pts, R.build_clusters(verts, order=g.permutation(V))), want)


@pytest.mark.parametrize("name", ("duplicated", "coplanar", "colinear", "identical"))
def test_pruned_search_on_degenerate_vertex_sets(name):
    verts = R.degenerate_sets()[name]
    pts = R.points_around(verts, 900, seed=21, reach=0.5)
    got, want = _pruned_case(verts, pts)
    assert bit_equal(got, want)
    if name == "duplicated":
        assert (want[0] < verts.shape[0] // 2).all()                 # the lower index of every pair wins
        assert bit_equal(_pruned_case(verts, pts, order=np.argsort(R.morton_keys(verts), kind="stable")[::-1])[0], want)
    if name == "identical":
        assert (want[0] == 0).all()
    keys = R.morton_keys(verts)
    assert (keys >= 0).all() and (keys < 2 ** 30).all()
    if name == "coplanar":
        assert (keys & 0x09249249 == 0).all()                          # the z bits: a zero-extent axis contributes 0
    if name == "identical":
        assert (keys == 0).all()


def test_non_finite_points_and_vertices():
    verts = R.sphere_mesh(200, seed=4)
    pts = R.points_around(verts, 64, seed=5)
    pts[0] = (np.nan, 0.0, 0.0)
    pts[1] = (np.inf, 0.0, 0.0)
    pts[2] = (-np.inf, np.inf, 0.0)
    pts[3] = (0.0, np.nan, np.inf)
    pts[4] = (3e38, -3e38, 3e38)                                       # finite, every d2 overflows to +inf
    got, want = _pruned_case(verts, pts)
    assert bit_equal(got, want)
    assert (want[0][:5] == 0).all() and np.isinf(want[1][:5]).all()     # no vertex with d2 < +inf: index 0, d2 = +inf
    bad = verts.copy()
    bad[0] = (np.nan, 0.0, 0.0)                                         # vertex 0 can never win
    bad[7] = (np.inf, -np.inf, 0.0)
    bad[100] = (0.0, np.nan, np.nan)
    keys = R.morton_keys(bad)
    assert (keys >= 0).all() and (keys < 2 ** 30).all()                 # a non-finite vertex cannot produce an out-of-range key
    got, want = _pruned_case(bad, pts)
    assert bit_equal(got, want)
    assert not np.isin(want[0][5:], (0, 7, 100)).any()
    allnan = np.full((70, 3), np.nan, np.float32)
    got, want = _pruned_case(allnan, pts)
    assert bit_equal(got, want) and (want[0] == 0).all() and np.isinf(want[1]).all()


def test_bit_comparison_rejects_wrong_forms():
    dup = R.degenerate_sets()["duplicated"]
    pts = R.points_around(dup, 900, seed=21, reach=0.5)
    want = R.brute_f32(pts, dup)
    # ties broken to the highest index
    assert not bit_equal(R.brute_f32(pts, dup, variant="highest_index"), want)
    # d2 summed in another order: the same vertices almost everywhere, other bits
    verts = R.sphere_mesh(1000, seed=1000)
    p2 = R.points_around(verts, 1500, seed=1001)
    right, other = R.brute_f32(p2, verts), R.brute_f32(p2, verts, variant="other_order")
    assert not bit_equal(other, right) and (other[0] == right[0]).mean() > 0.99
    # second-nearest for 1 % of the points
    assert not bit_equal(R.brute_f32(p2, verts, variant="second_nearest"), right)
    # pruning with a strict bound (scan iff lb < best) loses the tie with a lower index in a cluster whose bound EQUALS the best:
    # on the duplicate set once the higher index of a pair sits in the earlier cluster (the reversed order, shifted by one so that
    # cluster boundaries fall inside pairs) ...
    rev = np.roll(np.argsort(R.morton_keys(dup), kind="stable")[::-1], 1)
    on = dup[: dup.shape[0] // 2]                                      # points exactly on the vertices: d2 = lb = 0
    cl = R.build_clusters(dup, order=rev)
    assert bit_equal(R.pruned_f32(on, cl), R.brute_f32(on, dup))
    assert not bit_equal(R.pruned_f32(on, cl, variant="strict_prune"), R.brute_f32(on, dup))
    # ... and under the stable Morton order on the mirror set
    mv, mp = R.mirror_set()
    cl = R.build_clusters(mv)
    assert R.brute_f32(mp, mv)[0].tolist() == [0]
    assert bit_equal(R.pruned_f32(mp, cl), R.brute_f32(mp, mv))
    assert R.pruned_f32(mp, cl, variant="strict_prune")[0].tolist() == [1]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_built_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert "nearest_vertex.hip" in (ROOT / "diner_amd" / "csrc" / "Makefile").read_text()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
        assert m, name
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
        assert getattr(L, name)
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 3 == L.diner_version()


def test_bad_arguments_return_codes_before_any_launch():
    from diner_amd import _lib
    L = _lib.lib()
    p = 64                                                              # a non-NULL dummy, never dereferenced
    err = lambda: L.diner_last_error()
    nv = lambda pts, v, ws, SB, N, V, idx, d2: L.diner_nearest_vertex(pts, v, ws, SB, N, V, idx, d2, None)
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert nv(args[0], args[1], None, 1, 5, 7, args[2], args[3]) == -1 and b"NULL pointer" in err()
    assert nv(p, p, None, 1, 5, 0, p, p) == -1 and b"non-positive V" in err()
    assert nv(p, p, None, 1, 5, -3, p, p) == -1
    assert nv(p, p, None, -1, 5, 7, p, p) == -1 and b"negative" in err()
    assert nv(p, p, None, 1, -5, 7, p, p) == -1
    assert nv(p, p, None, 1, 5, 2 ** 24 + 1, p, p) == -3 and b"2^24" in err()
    assert nv(p, p, None, 1, 2 ** 31, 7, p, p) == -3 and b"2^31" in err()
    assert nv(p, p, None, 65536, 5, 7, p, p) == -3 and b"65535" in err()
    assert nv(p, p, 72, 1, 5, 7, p, p) == -1 and b"aligned" in err()      # a misaligned cluster structure
    assert nv(None, None, None, 1, 0, 7, None, None) == 0                 # N == 0: nothing to do, whatever the pointers
    assert nv(None, None, None, 0, 5, 7, None, None) == 0
    assert nv(None, None, None, 1, 0, 0, None, None) == -1                # ... but V <= 0 is refused first

    dp = lambda pts, v, o1, o2, SB, N, V, out, out2: L.diner_deform_points(pts, v, None, o1, o2, SB, N, V, out, out2, None)
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert dp(args[0], args[1], args[2], None, 1, 5, 7, args[3], None) == -1 and b"NULL pointer" in err()
    assert dp(p, p, p, p, 1, 5, 7, p, None) == -1 and b"together" in err()
    assert dp(p, p, p, None, 1, 5, 7, p, p) == -1
    assert dp(p, p, p, None, 1, 5, 0, p, None) == -1
    assert dp(p, p, p, None, 1, 5, 2 ** 24 + 1, p, None) == -3
    assert dp(None, None, None, None, 1, 0, 7, None, None) == 0

    rp = lambda r, z, v, o1, SB, B, K, V, out: L.diner_deform_ray_points(r, z, v, None, o1, None, SB, B, K, V, out, None, None, None)
    for hole in range(5):
        args = [p, p, p, p, p]
        args[hole] = None
        assert rp(args[0], args[1], args[2], args[3], 1, 5, 4, 7, args[4]) == -1 and b"NULL pointer" in err()
    assert rp(p, p, p, p, 1, -5, 4, 7, p) == -1 and rp(p, p, p, p, 1, 5, -4, 7, p) == -1
    assert rp(p, p, p, p, 1, 5, 4, 0, p) == -1
    assert rp(p, p, p, p, 1, 2 ** 29, 4, 7, p) == -3 and b"2^31" in err()
    assert rp(None, None, None, None, 1, 5, 0, 7, None) == 0 and rp(None, None, None, None, 1, 0, 4, 7, None) == 0

    assert L.diner_nearest_vertex_keys(None, 1, 7, p, None) == -1 and L.diner_nearest_vertex_keys(p, 1, 7, None, None) == -1
    assert L.diner_nearest_vertex_keys(p, 1, 0, p, None) == -1 and L.diner_nearest_vertex_keys(p, 1, 2 ** 24 + 1, p, None) == -3
    assert L.diner_nearest_vertex_keys(None, 0, 7, None, None) == 0
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert L.diner_nearest_vertex_build(*args[:2], 1, 7, args[2], None) == -1 and b"NULL pointer" in err()
    assert L.diner_nearest_vertex_build(p, p, 1, 7, 72, None) == -1 and b"aligned" in err()
    assert L.diner_nearest_vertex_build(p, p, 1, 0, p, None) == -1 and L.diner_nearest_vertex_build(p, p, 65536, 7, p, None) == -3
    # per scene and cluster of 64: 64 x (x, y, z, index) + 6 AABB floats
    ws = L.diner_nearest_vertex_workspace_floats
    assert ws(1, 1) == ws(1, 64) == 262 and ws(1, 65) == 524 and ws(3, 26317) == 3 * 412 * 262
    assert ws(0, 5) == 0 and ws(1, 0) == -1 and ws(-1, 5) == -1 and ws(1, 2 ** 24 + 1) == -1 and ws(65536, 5) == -1
    assert ws(1, 2 ** 24) == 2 ** 18 * 262


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_glue_surface_and_refusals_need_no_gpu():
    import torch

    from diner_amd import deform, glue
    assert glue.nearest_vertex is deform.nearest_vertex and glue.deform_points is deform.deform_points
    assert glue.deform_ray_points is deform.deform_ray_points
    sig = inspect.signature(glue.deform_points).parameters
    assert list(sig)[:3] == ["points", "target_vertices", "offsets"]                    # the reference's signature (:40)
    assert sig["offsets2"].default is None and sig["method"].default == "auto"
    sig = inspect.signature(glue.deform_ray_points).parameters
    assert list(sig)[:6] == ["rays", "z_samp", "target_vertices", "offsets", "offsets2", "return_points"]
    assert sig["return_points"].default is False
    assert inspect.signature(glue.nearest_vertex).parameters["method"].default == "auto"
    p, v = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.nearest_vertex(p, v)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.deform_points(p, v, v)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.deform_ray_points(torch.zeros(1, 4, 8), torch.zeros(1, 4, 2), v, v)
    with pytest.raises(ValueError, match="method"):
        glue.nearest_vertex(p, v, method="kdtree")
    assert deform.AUTO_CLUSTERS_MIN_V >= 64


def test_compat_knn_points_signature_and_refusals():
    import torch

    from diner_amd import compat
    from diner_amd.compat import pytorch3d_knn
    assert compat.knn_points is pytorch3d_knn.knn_points
    sig = inspect.signature(compat.knn_points).parameters
    assert list(sig) == ["p1", "p2", "lengths1", "lengths2", "K", "version", "return_nn", "return_sorted"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, None, 1, -1, False, True]
    p, v = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    with pytest.raises(NotImplementedError, match="K=1"):
        compat.knn_points(p, v, K=2)
    with pytest.raises(NotImplementedError, match="lengths"):
        compat.knn_points(p, v, lengths1=torch.tensor([4]))
    with pytest.raises(NotImplementedError, match="lengths"):
        compat.knn_points(p, v, lengths2=torch.tensor([5]))


def test_install_registers_stand_ins_only_without_a_real_pytorch3d():
    from diner_amd.compat import pytorch3d_knn as K
    names = K.MODULES
    saved = {n: sys.modules.pop(n) for n in names if n in sys.modules}
    try:
        # nothing is registered by importing the package
        assert not any(n in sys.modules for n in names)
        real = types.ModuleType("pytorch3d")                             # a "real" package: anything that is not our stand-in
        sys.modules["pytorch3d"] = real
        assert K.install() is False
        assert sys.modules["pytorch3d"] is real and "pytorch3d.ops" not in sys.modules and "pytorch3d.ops.knn" not in sys.modules
        del sys.modules["pytorch3d"]
        import importlib.util
        if importlib.util.find_spec("pytorch3d") is None:
            assert K.install() is True
            from pytorch3d.ops.knn import knn_points                     # the NOVEL renderers' import line
            import pytorch3d.ops
            assert knn_points is K.knn_points and pytorch3d.ops.knn_points is K.knn_points
            first = sys.modules["pytorch3d"]
            assert K.install() is True and sys.modules["pytorch3d"] is first      # a second call changes nothing
    finally:
        for n in names:
            sys.modules.pop(n, None)
        sys.modules.update(saved)
