"""Compile-time guard of the image wire kernels (diner_amd/csrc/image_wire.hip), cross-compiled for gfx950 (no GPU), a sibling of
tests/test_isa_guard_frame_out.py: no FLAT instruction in the code object (tests/test_isa_guard.py's rule), no scratch and no LDS, the
16-byte / 12-byte / 4-byte loads and 16-byte stores of the four-pixel path, and the arithmetic the bit-exactness rests on: true
divisions (v_div_scale / v_div_fixup sequences, never a bare reciprocal) and the root's refinement after v_sqrt_f32.  The divisions', the
root's and the 64-bit index arithmetic's own expansions are made of fused multiply-adds, so the absence of a contracted multiply-add in the
decode is not something the instruction list can show; it is pinned by value (tests/test_gpu_wire_images.py, bit for bit)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "image_wire.hip"
KERNELS = {"decode_image_kernel": 2, "encoder_input_kernel": 2, "decode_depth_mf_kernel": 1}     # instantiations of each


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_image_wire") / "image_wire.s"
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


def test_kernels_present_without_scratch_or_lds(isa):
    for k, count in KERNELS.items():
        names = bodies(isa, k)
        assert len(names) == count, (k, sorted(names))
        for name, body in names.items():
            m = re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel", isa, re.S)
            assert m, name
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(1)).group(1)) == 0, name
            assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", m.group(1)).group(1)) == 0, name
            assert not re.search(r"^\s+(ds_|scratch_|buffer_atomic|global_atomic)", body, re.M), name


def test_four_pixel_path_uses_wide_accesses(isa):
    wide = {n: b for n, b in bodies(isa, "decode_image_kernel").items() if "ILi4E" in n}
    assert len(wide) == 1
    for name, body in wide.items():
        for op in ("global_load_dwordx4", "global_load_dwordx3", "global_load_dword ", "global_store_dwordx4"):     # RGBA, RGB, the plane
            assert op in body, (name, op)
        assert "global_load_ubyte" not in body and "global_store_dword " not in body, name
    for name, body in bodies(isa, "encoder_input_kernel").items():
        if "ILi4E" in name:
            assert "global_store_dwordx4" in body and "global_store_dword " not in body, name


def test_divisions_and_root_are_the_ieee_ones(isa):
    for k in ("decode_image_kernel", "encoder_input_kernel"):
        for name, body in bodies(isa, k).items():
            scales, fixups, rcps = (len(re.findall(rf"^\s+{op}", body, re.M)) for op in ("v_div_scale_f32", "v_div_fixup_f32", "v_rcp_f32"))
            roots = len(re.findall(r"^\s+v_sqrt_f32", body, re.M))
            assert fixups >= 7 and scales == 2 * fixups, (name, scales, fixups)       # / 255 x 4, / 1.1 x 3 per pixel at the least
            assert rcps <= fixups + roots, (name, rcps, fixups, roots)               # one per division, a few for the integer index arithmetic: none stands in for a division
            assert roots >= 3, name
            assert not re.search(r"^\s+v_rsq_f32", body, re.M), name

