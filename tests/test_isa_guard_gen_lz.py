"""Compile-time guard of the lin_z-map forms of the shape-general point/MLP kernels and of the builder of their maps
(diner_amd/csrc/points_mlp_gen_lz.hip, points_mlp_gen_lz_bc.hip, points_mlp_gen_f16_lz.hip, points_mlp_gen_f16_lz_bc.hip,
linz_maps_gen.hip), cross-compiled for gfx950 (no GPU): the rule of tests/test_isa_guard.py -- no FLAT instruction in any of the code
objects."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "diner_amd" / "csrc"
# unit -> the mangled kernel name up to its <RB, CT>: the template's name and, for the point/MLP kernels, the mode
UNITS = {"points_mlp_gen_lz": "points_mlp_gen_kernelINS0_2LzE", "points_mlp_gen_lz_bc": "points_mlp_gen_kernelINS0_4LzBcE",
         "points_mlp_gen_f16_lz": "points_mlp_gen_f16_kernelINS0_2LzE", "points_mlp_gen_f16_lz_bc": "points_mlp_gen_f16_kernelINS0_4LzBcE",
         "linz_maps_gen": "linz_maps_gen_kernelI"}


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request, tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_gen_lz") / f"{request.param}.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(CSRC / f"{request.param}.hip")], check=True, capture_output=True, timeout=900)
    return UNITS[request.param], asm.read_text()


def test_no_flat_instructions(unit):
    kernel, isa = unit
    assert len(set(re.findall(rf"^(_ZN5diner\w*?\d+{kernel}Li\dELi\dEE\S*):", isa, re.M))) == 3, "the three <RB, CT> instantiations"
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))
