"""Golden vectors of the NOVEL renderers' point deformation (diner_amd/csrc/nearest_vertex.hip; glue.deform_points).

FROM REFERENCE CODE: the UNMODIFIED ``NeRFRendererDGS.deform_points`` (reference src/models/novel/nerf_novel_renderer.py:40-50) runs on
the CPU.  Its one dependency without a build here, ``pytorch3d.ops.knn.knn_points``, is stubbed in ``sys.modules`` by the float64
brute-force restatement of tests/knn_ref.py (pytorch3d has CUDA kernels only): the search itself has no runnable reference and is
pinned to the contract of include/diner_hip.h; what this fixture pins to the reference is everything around it -- the gather
``offsets[arange(SB)[:, None], idx.squeeze()]``, the batch indexing, the add and the shapes.  Nothing of the reference is copied into
this repository.  Recorded per case: points, vertices, two offset sets, the restated indices and the reference's outputs for both sets.

Runs only where the reference source tree exists; the tests read the committed ``tests/golden/deform_points.npz`` only.

    python tools/gen_deform_golden.py            # (re)writes tests/golden/deform_points.npz
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

from oracle.ref_harness import install_stubs  # noqa: E402
from tests import knn_ref as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "deform_points.npz"
CASES = {"sb1": dict(SB=1, B=301, V=131, seed=11), "sb2": dict(SB=2, B=297, V=129, seed=12)}
_KNN = namedtuple("KNN", "dists idx knn")
_record = {}


def knn_points_f64(p1, p2, lengths1=None, lengths2=None, K=1, **kw):
    """the float64 restatement, in pytorch3d's return layout"""
    assert K == 1 and lengths1 is None and lengths2 is None
    idx, best = [], []
    for sb in range(p1.shape[0]):
        i, b, _ = R.brute_f64(p1[sb].numpy(), p2[sb].numpy())
        idx.append(i)
        best.append(b)
    _record["idx"] = np.stack(idx)
    return _KNN(torch.from_numpy(np.stack(best)).to(p1.dtype)[..., None], torch.from_numpy(np.stack(idx))[..., None], None)


def reference_renderer():
    install_stubs()
    root, ops, knn = (types.ModuleType(n) for n in ("pytorch3d", "pytorch3d.ops", "pytorch3d.ops.knn"))
    knn.knn_points = knn_points_f64
    root.ops, ops.knn = ops, knn
    sys.modules.update({"pytorch3d": root, "pytorch3d.ops": ops, "pytorch3d.ops.knn": knn})
    import matplotlib
    matplotlib.use("Agg")
    from src.models.novel.nerf_novel_renderer import NeRFRendererDGS
    return NeRFRendererDGS()


def main():
    rend = reference_renderer()
    out, index = {}, {}
    for name, c in CASES.items():
        g = np.random.default_rng(c["seed"])
        verts = np.stack([R.sphere_mesh(c["V"], c["seed"] + 100 * sb) for sb in range(c["SB"])])
        pts = np.stack([R.points_around(verts[sb], c["B"], c["seed"] + 7 * sb, reach=0.5) for sb in range(c["SB"])])
        off1 = (0.02 * g.normal(size=verts.shape)).astype(np.float32)
        off2 = (0.02 * g.normal(size=verts.shape)).astype(np.float32)
        t = torch.from_numpy
        with torch.no_grad():
            d1 = rend.deform_points(t(pts), t(verts), t(off1)).numpy()
            idx = _record["idx"].astype(np.int32)
            d2 = rend.deform_points(t(pts), t(verts), t(off2)).numpy()
        assert d1.shape == pts.shape and d1.dtype == np.float32
        mine, _ = R.nearest_batch(pts, verts)
        print(f"{name}: SB={c['SB']} B={c['B']} V={c['V']}: fp32 contract indices differ from float64 at {int((mine != idx).sum())} points; "
              f"deform restatement bit-equal: {np.array_equal(R.deform(pts, idx, off1), d1) and np.array_equal(R.deform(pts, idx, off2), d2)}")
        out.update({f"{name}.points": pts, f"{name}.vertices": verts, f"{name}.offsets": off1, f"{name}.offsets2": off2,
                    f"{name}.idx": idx, f"{name}.deformed": d1, f"{name}.deformed2": d2})
        index[name] = c
    out["index"] = np.array(json.dumps(index))
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN.relative_to(ROOT)} ({GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
