"""Compile-time guard of the frame-output and score kernels (diner_amd/csrc/frame_out.hip), cross-compiled for gfx950 (no GPU): no FLAT
instruction in the code object (tests/test_isa_guard.py's rule), no spills, the 16-byte / 12-byte accesses of the wide paths, and the
score kernel's LDS inside the 64 KiB a workgroup gets without asking."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "frame_out.hip"
KERNELS = ("depth_range_partial_kernel", "depth_range_final_kernel", "depth_cmap_kernel", "frames_u8_kernel", "image_scores_partial_kernel",
           "image_scores_final_kernel")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_frame_out") / "frame_out.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(SRC)], check=True, capture_output=True, timeout=900)
    return asm.read_text()


def bodies(isa, kernel):
    """{mangled name: instructions} of every instantiation of a kernel"""
    out = {}
    for name in sorted(set(re.findall(rf"^(_ZN5diner\S*{kernel}\S*):", isa, re.M))):
        body = isa[isa.index(name + ":"):]
        out[name] = body[:body.index("s_endpgm")]
    return out


def test_no_flat_instructions(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_kernels_present_without_spills(isa):
    for k in KERNELS:
        names = bodies(isa, k)
        assert names, k
        for name in names:
            m = re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel", isa, re.S)
            assert m, name
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(1)).group(1)) == 0, name


def test_wide_paths_use_wide_accesses(isa):
    frames = bodies(isa, "frames_u8_kernel")
    assert len(frames) == 4                                            # {4 pixels, 1 pixel} x {save_image, video}
    wide = {n: b for n, b in frames.items() if "ILi4E" in n}
    assert len(wide) == 2
    for name, body in wide.items():
        assert "global_load_dwordx4" in body and "global_store_dwordx3" in body, name
        assert "global_store_byte" not in body, name
    for name, body in bodies(isa, "depth_range_partial_kernel").items():
        assert ("global_load_dwordx4" in body) == ("ILi4E" in name), name
    for name, body in bodies(isa, "depth_cmap_kernel").items():
        assert ("global_store_dwordx4" in body) == ("ILi2E" in name), name


def test_no_float_contraction_in_the_quantisation(isa):
    # save_image's multiply and add are two fp32 roundings: no fused multiply-add on floats in the frame kernels
    for name, body in bodies(isa, "frames_u8_kernel").items():
        assert not re.search(r"v_(fma|fmac|mad|mac)_f32", body), name


def test_score_kernel_lds(isa):
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+)", isa, flags=re.S)
    lds = {name: int(size) for size, name in meta if "image_scores_partial_kernel" in name}
    assert len(lds) == 1 and 0 < list(lds.values())[0] <= 65536, lds
