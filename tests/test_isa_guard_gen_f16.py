"""Compile-time guard of the shape-general f16x3 point/MLP kernel (diner_amd/csrc/points_mlp_gen_f16.hip and its lookup-mode twin
points_mlp_gen_f16_ix.hip), cross-compiled for gfx950 (no GPU): the rule of tests/test_isa_guard.py -- no FLAT instruction in either
code object -- and the three instantiations of each on fp16 MFMA, with no fp32 MFMA anywhere (lin_out runs on the VALU), inside the
LDS budget, on 512 threads."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "diner_amd" / "csrc"
# unit -> its instantiations of the kernel template (points_mlp_gen_f16_kernel.hpp): the mangled kernel name with the mode
KERNEL = "points_mlp_gen_f16_kernel"
UNITS = {"points_mlp_gen_f16": f"{KERNEL}INS0_7DefaultE", "points_mlp_gen_f16_ix": f"{KERNEL}INS0_2IxE"}


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request, tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_gen_f16") / f"{request.param}.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(CSRC / f"{request.param}.hip")], check=True, capture_output=True, timeout=900)
    return UNITS[request.param], asm.read_text()


def test_no_flat_instructions(unit):
    _, isa = unit
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_three_instantiations_on_fp16_mfma(unit):
    kernel, isa = unit
    names = set(re.findall(rf"^(_ZN5diner6genf16\d+{kernel}Li(\d)ELi(\d)EE\S*):", isa, re.M))
    assert {(rb, ct) for _, rb, ct in names} == {("1", "1"), ("2", "1"), ("2", "2")}
    for name, _, _ in names:
        body = isa[isa.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "v_mfma_f32_32x32x16_f16" in body, name
        assert "v_mfma_f32_32x32x2_f32" not in body and not re.search(r"v_mfma_\w+_f32\b", body), name   # lin_out is VALU fp32
        assert "v_permlane32_swap" in body and "ds_write_b128" in body and "ds_read_b128" in body, name  # the operand image's path


def test_resources(unit):
    """512 threads, the LDS A image (128 KiB) + the taps within the 160-KiB budget; the spill size is reported, not bounded"""
    kernel, isa = unit
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.max_flat_workgroup_size:\s+(\d+).*?\.name:\s+(\S+).*?"
                      r"\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", isa, flags=re.S)
    kern = [(n, int(g), int(w), int(p), int(v), int(s)) for g, w, n, p, v, s in meta if kernel in n]
    report = "; ".join(f"{n.split(kernel)[1][:11]}: LDS {g} B, {w} threads, {v} VGPRs, private segment {p} B ({s} VGPRs spilled)"
                       for n, g, w, p, v, s in kern)
    assert len(kern) == 3, report
    assert all(g == 128 * 1024 + 64 * 32 and g <= 160 * 1024 and w == 512 for _, g, w, _, _, _ in kern), report
    assert all(v <= 256 for _, _, _, _, v, _ in kern), report
