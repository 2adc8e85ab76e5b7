"""Compile-time guard of the shape-general point/MLP kernel (diner_amd/csrc/points_mlp_gen.hip), cross-compiled for gfx950 (no
GPU): the rule of tests/test_isa_guard.py -- no FLAT instruction in the code object -- and the three instantiations the launcher
selects by d_hidden, all on exact fp32 MFMA."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "points_mlp_gen.hip"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_gen") / "points_mlp_gen.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(SRC)], check=True, capture_output=True, timeout=900)
    return asm.read_text()


def test_no_flat_instructions(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_three_instantiations_on_fp32_mfma(isa):
    names = set(re.findall(r"^(_ZN5diner3gen21points_mlp_gen_kernelINS0_7DefaultELi(\d)ELi(\d)EE\S*):", isa, re.M))
    assert {(rb, ct) for _, rb, ct in names} == {("1", "1"), ("2", "1"), ("2", "2")}
    for name, _, _ in names:
        body = isa[isa.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "v_mfma_f32_32x32x2_f32" in body, name
        assert not re.search(r"v_mfma_\w+_(f16|bf16)", body), name       # no reduced-precision operands on this path
    # 512 threads, the LDS A image (128 KiB) + the taps
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.max_flat_workgroup_size:\s+(\d+).*?\.name:\s+(\S+)", isa, flags=re.S)
    kern = [(int(g), int(w)) for g, w, n in meta if "points_mlp_gen_kernel" in n]
    assert len(kern) == 3 and all(g == 128 * 1024 + 64 * 32 and w == 512 for g, w in kern), kern
