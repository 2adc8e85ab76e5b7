"""Golden vectors of the image wire format and of Multiface's depth planes (diner_amd/csrc/image_wire.hip; diner_amd/wire.py).

FROM REFERENCE CODE: the UNMODIFIED readers of the reference's datasets run on the CPU, on PNGs this tool writes with PIL into a
temporary directory: ``FacescapeDataSet.read_rgba`` (src/data/facescape.py:59-66), ``DTUDataSet.read_rgb`` (src/data/dtu.py:72-88, with
its resize off: the caller resizes the bytes), ``MultiFaceDataset.read_img`` / ``read_alpha`` / ``read_depth`` (src/data/multiface.py:
65-109), and the statements of ``MultiFaceDataset.__getitem__`` that finish a sample: the depth std (:305-311) and the white fill
(:322-323).  The readers are imported from the reference's files through the stubs of oracle/ref_harness.py (``pil_to_tensor`` is a
pure dtype / layout conversion there); the statements of ``__getitem__`` are cut out of the reference file by line and executed as they
stand with their variables in scope.  Nothing of the reference's text is copied into this repository.

Stored in tests/golden/wire_images.npz: the inputs (bytes), the readers' outputs, and for the gamma cases the mask of entries where this
torch build's ``x ** 0.5`` is not the correctly rounded root of its operand (tests/wire_images_ref.py explains the bars).  The tool
prints how the restatement compares on every output.

Runs only where the reference source tree exists; the tests read the committed fixture only (data, no program text).

    python tools/gen_wire_images_golden.py            # (re)writes tests/golden/wire_images.npz
"""
from __future__ import annotations

import ast
import json
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch
from PIL import Image

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import ref_harness as rh  # noqa: E402
from tests import wire_images_ref as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "wire_images.npz"
ALPHA_EDGES = np.array([0, 127, 128, 254, 255], np.uint8)     # both sides of the two thresholds


def image_inputs():
    """name -> uint8 [N,H,W,4] (the fourth channel is the alpha; the RGB readers get the first three)"""
    rs = np.random.RandomState(51)
    i = np.arange(256, dtype=np.uint8).reshape(16, 16)
    out = {"ramp": np.stack([i, i, i, i], -1)[None], "ramp_rev": np.stack([i, i, i, 255 - i], -1)[None]}
    for name, (N, H, W) in (("rand5x7", (3, 5, 7)), ("rand33x64", (3, 33, 64)), ("one", (1, 1, 1))):
        px = rs.randint(0, 256, (N, H, W, 4)).astype(np.uint8)
        edge = rs.rand(N, H, W) < 0.6                                # random alphas rarely sit on a threshold
        px[..., 3] = np.where(edge, ALPHA_EDGES[rs.randint(0, 5, (N, H, W))], px[..., 3])
        out[name] = px
    return out


def depth_inputs():
    """2 x 48 x 48 uint16 planes, 40 % zeros in the depth; confidences in [0, 1] x 1e4, and up to 2 x 1e4 so that the clip acts"""
    rs = np.random.RandomState(52)
    d = rs.randint(4000, 16000, (2, 48, 48)).astype(np.uint16)
    d[rs.rand(2, 48, 48) < 0.4] = 0
    return dict(depth=d, conf=rs.randint(0, 10001, d.shape).astype(np.uint16), conf_high=rs.randint(9000, 20001, d.shape).astype(np.uint16))


def getitem_statements(first_lines):
    """the statements of MultiFaceDataset.__getitem__ that begin on the given lines, compiled from the reference's own text"""
    path = Path(rh.REFERENCE_ROOT) / "src" / "data" / "multiface.py"
    tree = ast.parse(path.read_text())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "__getitem__")
    body = sorted((n for n in ast.walk(fn) if isinstance(n, ast.stmt) and n.lineno in first_lines), key=lambda n: n.lineno)
    assert [n.lineno for n in body] == sorted(first_lines), f"{path} is not the file the line numbers were taken from"
    return compile(ast.Module(body=body, type_ignores=[]), str(path), "exec")


def main():
    rh.install_stubs()
    import matplotlib
    matplotlib.use("Agg")
    from src.data.dtu import DTUDataSet
    from src.data.facescape import FacescapeDataSet
    from src.data.multiface import MultiFaceDataset
    std_code = getitem_statements((305, 306, 311))     # read_depth; the constant / conf2std + clip branch; std[depth == 0] = 0
    fill_code = getitem_statements((322,))             # src_rgbs[alpha < 1] = 1
    fx, report = {}, []

    def put(key, ref, mine, mask=None):
        fx[key] = ref
        report.append((key, R.compare(mine, ref, mask)))

    with tempfile.TemporaryDirectory() as td:
        for name, px in image_inputs().items():
            fx[f"{name}/pixels"] = px
            N = px.shape[0]
            for n in range(N):
                Image.fromarray(px[n]).save(f"{td}/rgba{n}.png")
                Image.fromarray(np.ascontiguousarray(px[n, ..., :3])).save(f"{td}/rgb{n}.png")
                Image.fromarray(np.ascontiguousarray(px[n, ..., 3])).save(f"{td}/a{n}.png")
            # the root's operand is the same for every variant of a case: one mask per case
            t = torch.from_numpy(R.gamma_pre_root(np.ascontiguousarray(px[..., :3].transpose(0, 3, 1, 2)).astype(R.F) / R.F(255)))
            mask = (t ** (1.0 / 2.0)).numpy().view(np.uint32) != np.sqrt(t.numpy()).view(np.uint32)
            fx[f"{name}/multiface/sqrt_mask"] = mask
            for sym in (False, True):
                for bg in (1.0, 0.0):
                    out = [FacescapeDataSet.read_rgba(f"{td}/rgba{n}.png", symmetric_range=sym, bg=bg) for n in range(N)]
                    mine = R.decode_image(px, None, "below_half", bg, False, sym)
                    put(f"{name}/facescape/sym{int(sym)}/bg{int(bg)}/rgb", torch.stack([o[0] for o in out]).numpy(), mine[0])
                    put(f"{name}/facescape/sym{int(sym)}/bg{int(bg)}/alpha", torch.stack([o[1] for o in out]).numpy(), mine[1])
                out = [DTUDataSet.read_rgb(NS(downsample=None), f"{td}/rgb{n}.png", symmetric_range=sym) for n in range(N)]
                put(f"{name}/dtu/sym{int(sym)}/rgb", torch.stack(out).numpy(), R.decode_image(px[..., :3], None, "none", 1.0, False, sym)[0])
                scope = dict(src_rgbs=torch.stack([MultiFaceDataset.read_img(f"{td}/rgb{n}.png", symmetric_range=sym) for n in range(N)]),
                             src_alphas=torch.stack([MultiFaceDataset.read_alpha(f"{td}/a{n}.png") for n in range(N)]))
                exec(fill_code, scope)
                mine = R.decode_image(px[..., :3], px[..., 3], "below_one", 1.0, True, sym)
                put(f"{name}/multiface/sym{int(sym)}/rgb", scope["src_rgbs"].numpy(), mine[0], mask)
                put(f"{name}/multiface/sym{int(sym)}/alpha", scope["src_alphas"].numpy(), mine[1])

        dep = depth_inputs()
        for k, v in dep.items():
            fx[f"depth/{k}"] = v
        N = dep["depth"].shape[0]
        for case, conf in (("const", None), ("conf", "conf"), ("conf_high", "conf_high")):
            ds, ss = [], []
            for n in range(N):
                Image.fromarray(dep["depth"][n]).save(f"{td}/d{n}.png")
                if conf:
                    Image.fromarray(dep[conf][n]).save(f"{td}/c{n}.png")
                scope = dict(self=NS(read_depth=MultiFaceDataset.read_depth, depth_std_suffix=".png" if conf else None), torch=torch,
                             src_depth_path=f"{td}/d{n}.png", src_depth_std_path=f"{td}/c{n}.png")
                exec(std_code, scope)
                ds.append(scope["src_depth"]), ss.append(scope["src_depth_std"])
            mine = R.decode_multiface_depth(dep["depth"], dep[conf] if conf else None)
            put(f"depth/{case}/depth", torch.stack(ds).numpy(), mine[0])
            put(f"depth/{case}/std", torch.stack(ss).numpy(), mine[1])
        clipped = (fx["depth/conf_high/std"] == 0) & (fx["depth/conf_high/depth"] != 0)
        assert clipped.mean() > 0.2, "the high confidences must make the clip act"

    masks = [fx[k] for k in fx if k.endswith("sqrt_mask")]
    bad = [(k, why) for k, why in report if why]
    print(f"{len(report)} outputs; the restatement " + ("meets the bars on all of them" if not bad else f"MISSES on {bad}"))
    print(f"root masks: {sum(int(m.sum()) for m in masks)} of {sum(m.size for m in masks)} entries; per case " +
          ", ".join(f"{k.split('/')[0]} {fx[k].mean():.2%}" for k in fx if k.endswith("sqrt_mask")))
    fx["index"] = np.array(json.dumps(dict(torch=torch.__version__, cases=sorted({k.split("/")[0] for k in fx}))))
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLDEN, **fx)
    print(f"wrote {GOLDEN.relative_to(ROOT)} ({GOLDEN.stat().st_size} bytes)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
