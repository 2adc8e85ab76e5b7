"""Compile-time guard of the bounding-box kernels (diner_amd/csrc/ray_box.hip), cross-compiled for gfx950 (no GPU): no FLAT instruction in
the code object (tests/test_isa_guard.py's rule), no spills, and every kernel present."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "ray_box.hip"
KERNELS = ("ray_box_mark_kernel", "ray_box_scan_kernel", "ray_box_compact_kernel", "gen_rays_box_kernel", "frame_from_hits_kernel")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_ray_box") / "ray_box.s"
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
