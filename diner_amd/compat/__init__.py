"""Stand-ins for third-party packages the fork's code imports and that have no ROCm build.  Nothing here acts at import time:
call :func:`install` before importing the code that needs them."""
from .pytorch3d_knn import install, knn_points  # noqa: F401

__all__ = ["install", "knn_points"]
