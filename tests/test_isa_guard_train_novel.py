"""Compile-time guard of the NOVEL training path's kernels (diner_amd/csrc/train_novel.hip), cross-compiled for gfx950 (no GPU): no FLAT
instruction in the code object (tests/test_isa_guard.py's rule), and both kernels present."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "train_novel.hip"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_train_novel") / "train_novel.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(SRC)], check=True, capture_output=True, timeout=900)
    return asm.read_text()


def test_no_flat_instructions(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_both_kernels_present(isa):
    for k in ("point_inputs_novel_kernel", "novel_gen_scatter_kernel"):
        assert re.search(rf"^_ZN5diner11train_novel\d+{k}\S*:", isa, re.M), k
