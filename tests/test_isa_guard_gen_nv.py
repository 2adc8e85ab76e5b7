"""Compile-time guard of the NOVEL point model's kernels (diner_amd/csrc/points_mlp_gen_nv.hip and points_mlp_gen_f16_nv.hip),
cross-compiled for gfx950 (no GPU), on the pattern of tests/test_isa_guard_gen.py: no FLAT instruction in either code object, the
three <RB,CT> instantiations the launchers select by d_hidden, exact fp32 MFMA only in the fp32 unit (split-fp16 MFMA only in the
other), 512 threads, and an LDS footprint (the 128-KiB A image + two tap records per point) within the 160 KiB of a CU."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "diner_amd" / "csrc"
UNITS = {"fp32": ("points_mlp_gen_nv.hip", "points_mlp_gen_nv_kernel"), "f16x3": ("points_mlp_gen_f16_nv.hip", "points_mlp_gen_f16_nv_kernel")}


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request, tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    src, kernel = UNITS[request.param]
    asm = tmp_path_factory.mktemp("isa_gen_nv") / (src + ".s")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(CSRC / src)], check=True, capture_output=True, timeout=900)
    return request.param, kernel, asm.read_text()


def test_no_flat_instructions(unit):
    _, _, isa = unit
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_three_instantiations_on_the_units_own_mfma(unit):
    prec, kernel, isa = unit
    names = set(re.findall(rf"^(_ZN5diner\d+\w*?\d+{kernel}ILi(\d)ELi(\d)EE\S*):", isa, re.M))
    assert {(rb, ct) for _, rb, ct in names} == {("1", "1"), ("2", "1"), ("2", "2")}, names
    for name, _, _ in names:
        body = isa[isa.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        mfma = set(re.findall(r"\b(v_mfma_\w+)", body))
        if prec == "fp32":
            assert mfma == {"v_mfma_f32_32x32x2_f32"}, (name, mfma)     # no reduced-precision operands on this path
        else:
            assert mfma == {"v_mfma_f32_32x32x16_f16"}, (name, mfma)    # the split-fp16 products; lin_out runs on the VALU
    # 512 threads; the LDS A image (128 KiB) + the encoder's and the general Tap per point
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.max_flat_workgroup_size:\s+(\d+).*?\.name:\s+(\S+)", isa, flags=re.S)
    kern = [(int(g), int(w)) for g, w, n in meta if kernel in n]
    assert len(kern) == 3 and all(g == 128 * 1024 + 2 * 64 * 32 and g <= 160 * 1024 and w == 512 for g, w in kern), kern


def test_the_parent_units_instantiate_no_novel_kernel():
    """the novel kernels live in translation units of their own: the parents' code objects (pinned by tests/test_isa_guard_gen*.py) hold none"""
    for src in ("points_mlp_gen.hip", "points_mlp_gen_f16.hip", "points_mlp_gen_kernel.hpp", "points_mlp_gen_f16_kernel.hpp"):
        assert "_nv_kernel" not in (CSRC / src).read_text(), src
