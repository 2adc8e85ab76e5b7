"""``pytorch3d.ops.knn.knn_points`` for ``K = 1`` on :func:`diner_amd.glue.nearest_vertex` -- the one pytorch3d function the fork's NOVEL /
NOVEL_PE renderers call (reference ``src/models/novel/nerf_novel_renderer.py:8, :47``).  pytorch3d ships CUDA kernels only and has no
ROCm build; :func:`install` registers stand-in modules ``pytorch3d``, ``pytorch3d.ops`` and ``pytorch3d.ops.knn`` so that the
unmodified renderers import.  It acts only when called, and only when the real package cannot be imported."""
from __future__ import annotations

import importlib
import importlib.util
import sys
import types
from collections import namedtuple

_KNN = namedtuple("KNN", "dists idx knn")
MODULES = ("pytorch3d", "pytorch3d.ops", "pytorch3d.ops.knn")


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True):
    """pytorch3d's signature.  p1 [N,P1,3], p2 [N,P2,3] -> the named tuple ``(dists [N,P1,1] fp32 squared distances, idx [N,P1,1] int64,
    knn [N,P1,1,3] or None)``.  ``K != 1`` and ragged batches (``lengths1`` / ``lengths2``) raise ``NotImplementedError``; ``version``
    and ``return_sorted`` have no meaning at K = 1.  The distances carry no gradient (the reference discards them)."""
    import torch

    from ..deform import nearest_vertex
    if K != 1:
        raise NotImplementedError(f"diner_amd.compat.knn_points serves K=1 only (the NOVEL renderers' use), not K={K}")
    if lengths1 is not None or lengths2 is not None:
        raise NotImplementedError("diner_amd.compat.knn_points does not serve ragged batches (lengths1 / lengths2)")
    idx32, d2 = nearest_vertex(p1, p2)
    idx = idx32.to(torch.int64).unsqueeze(-1)
    nn = None
    if return_nn:
        nn = torch.gather(p2, 1, idx.expand(-1, -1, 3)).unsqueeze(2)
    return _KNN(dists=d2.unsqueeze(-1), idx=idx, knn=nn)


def _real_pytorch3d_available():
    if "pytorch3d" in sys.modules:
        return not getattr(sys.modules["pytorch3d"], "__diner_amd_stand_in__", False)
    try:
        return importlib.util.find_spec("pytorch3d") is not None
    except (ImportError, ValueError):
        return False


def install():
    """Register the stand-ins in ``sys.modules``.  -> True when they are in place (now or from an earlier call), False when a real
    pytorch3d is importable and nothing was touched."""
    if _real_pytorch3d_available():
        return False
    if getattr(sys.modules.get("pytorch3d"), "__diner_amd_stand_in__", False):
        return True
    root, ops, knn = (types.ModuleType(n) for n in MODULES)
    for m in (root, ops, knn):
        m.__diner_amd_stand_in__ = True
    root.__path__, ops.__path__ = [], []          # packages: `import pytorch3d.ops.knn` walks them
    root.ops, ops.knn = ops, knn
    knn.knn_points = ops.knn_points = knn_points
    for n, m in zip(MODULES, (root, ops, knn)):
        sys.modules[n] = m
    return True
