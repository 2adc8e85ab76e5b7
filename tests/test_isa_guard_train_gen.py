"""Compile-time guard of the shape-general training kernels (diner_amd/csrc/train_gen.hip), cross-compiled for gfx950 (no GPU): no FLAT
instruction in the code object (tests/test_isa_guard.py's rule), and the GEMM kernels on exact fp32 MFMA with no spills."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "train_gen.hip"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_train_gen") / "train_gen.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(SRC)], check=True, capture_output=True, timeout=900)
    return asm.read_text()


def _gemm_kernels(isa):
    return sorted(set(re.findall(r"^(_ZN5diner9train_gen15gemm_act_kernelILb[01]ELb[01]EEEvNS0_8GemmArgsE):", isa, re.M)))


def test_no_flat_instructions(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_point_input_kernels_present(isa):
    for k in ("point_inputs_gen_kernel", "point_inputs_bwd_gen_kernel", "camg_ray_reduce_kernel", "camg_view_partial_kernel",
              "camg_view_final_kernel"):
        assert re.search(rf"^_ZN5diner9train_gen\d+{k}\S*:", isa, re.M), k


def test_gemm_kernels_on_fp32_mfma(isa):
    names = _gemm_kernels(isa)
    assert len(names) == 4, names                       # A along k / m  x  B along n / k
    for name in names:
        body = isa[isa.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "v_mfma_f32_32x32x2_f32" in body, name
        assert not re.search(r"v_mfma_\w+_(f16|bf16)", body), name       # exact fp32 only on this path


def test_gemm_kernels_do_not_spill(isa):
    for name in _gemm_kernels(isa):
        m = re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel", isa, re.S)
        assert m, name
        seg = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(1)).group(1))
        assert seg == 0, (name, seg)
