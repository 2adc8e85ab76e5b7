"""Golden vectors of the ray / bounding-box intersection (diner_amd/csrc/ray_box.hip; glue.ray_box, glue.box_rays).

FROM REFERENCE CODE: the UNMODIFIED ``FacescapeDataSet.get_near_far`` (reference src/data/facescape.py:152-185) runs on the CPU, on the
project's rays -- gen_rays' pixel-centre, unit-direction rays of tests/ray_box_ref.py, rounded to float32 as ``get_mask_at_box`` rounds
its own (:131-132).  The function's source is cut out of the reference file and executed as it stands with numpy in scope (the module
around it imports the data-loading stack); nothing of it is copied into this repository.  Recorded per camera: the inputs (extrinsics,
intrinsics, size, bounds, offset), and the reference's ``near``, ``far`` (scattered to [H,W], 0 at a miss) and ``mask_at_box``.

Three cameras outside the box [[-0.12,-0.16,-0.10],[0.11,0.15,0.13]], all looking at the origin; for each the tool prints the hit
share, the share of the ambiguous set (tests/ray_box_ref.py) and the mask mismatches of the float64 restatement outside that set.

Runs only where the reference source tree exists; the tests read the committed ``tests/golden/ray_box.npz`` only (data, no program
text).

    python tools/gen_ray_box_golden.py            # (re)writes tests/golden/ray_box.npz
"""
from __future__ import annotations

import ast
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle.ref_harness import REFERENCE_ROOT  # noqa: E402
from tests import ray_box_ref as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "ray_box.npz"
BOUNDS = np.array([[-0.12, -0.16, -0.10], [0.11, 0.15, 0.13]], np.float32)
CAMERAS = {   # name -> (H, W, focal, eye)
    "48x64": (48, 64, 150.0, (0.3, -0.2, -1.8)),
    "37x53": (37, 53, 110.0, (1.2, 0.4, -1.0)),
    "32x32": (32, 32, 70.0, (0.0, 0.0, -1.5)),
}


def reference_get_near_far():
    """the reference's get_near_far, compiled from its own source text"""
    path = Path(REFERENCE_ROOT) / "src" / "data" / "facescape.py"
    text = path.read_text()
    for node in ast.walk(ast.parse(text)):
        if isinstance(node, ast.FunctionDef) and node.name == "get_near_far":
            node.decorator_list = []                                   # a @staticmethod of the dataset class
            scope = {"np": np}
            exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), scope)
            return scope["get_near_far"]
    raise RuntimeError(f"get_near_far not found in {path}")


def main():
    get_near_far = reference_get_near_far()
    out, index = {"bounds": BOUNDS, "box_offset": np.array(R.BOX_OFFSET, np.float64)}, {}
    for name, (H, W, f, eye) in CAMERAS.items():
        E, K = R.look_at(eye).astype(np.float32), R.intrinsics(f, H, W).astype(np.float32)
        o, d = R.gen_rays_ref(E, K, H, W)
        ray_o, ray_d = o.reshape(-1, 3).astype(np.float32), d.reshape(-1, 3).astype(np.float32)
        near_c, far_c, mask = get_near_far(BOUNDS, ray_o.copy(), ray_d.copy())   # (it edits ray_d in place)
        near, far = np.zeros(H * W), np.zeros(H * W)
        near[mask], far[mask] = near_c, far_c
        out.update({f"{name}.extrinsics": E, f"{name}.intrinsics": K, f"{name}.near": near.reshape(H, W), f"{name}.far": far.reshape(H, W),
                    f"{name}.mask": mask.reshape(H, W)})
        index[name] = dict(H=H, W=W, focal=f, eye=list(eye), z_near=0.1, z_far=10.0)
        mine = R.ray_box_ref(E, K, H, W, 0.1, 10.0, BOUNDS)
        want = dict(near=near.reshape(H, W), far=far.reshape(H, W), mask=mask.reshape(H, W))
        off = (mine["mask"] != want["mask"]) & ~mine["ambiguous"]
        print(f"{name}: hit share {mask.mean():.2%}, ambiguous {mine['ambiguous'].mean():.2%}, mask mismatches outside it {int(off.sum())}, "
              f"compare: {R.compare(mine, want, mine['ambiguous']) or 'passes'}")
    out["index"] = np.array(json.dumps(index))
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN.relative_to(ROOT)} ({GOLDEN.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
