"""Compile-time guard of the NOVEL_PE point model's kernels (diner_amd/csrc/points_mlp_gen_nvpe.hip and points_mlp_gen_f16_nvpe.hip)
and of the builder of their deformation map (novel_pe_map.hip), cross-compiled for gfx950 (no GPU), on the pattern of
tests/test_isa_guard_gen_nv.py: no FLAT instruction and no atomic in any code object, the three <RB,CT> instantiations the launchers
select by d_hidden, exact fp32 MFMA only in the fp32 unit and the map builder (split-fp16 MFMA only in the f16x3 unit), 512 threads,
and an LDS footprint -- the 128-KiB A image + two tap records + 8 floats per point -- equal to what the kernel declares and within
the 160 KiB of a CU."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "diner_amd" / "csrc"
UNITS = {"fp32": ("points_mlp_gen_nvpe.hip", "points_mlp_gen_nvpe_kernel"), "f16x3": ("points_mlp_gen_f16_nvpe.hip", "points_mlp_gen_f16_nvpe_kernel")}
MAP_UNIT = ("novel_pe_map.hip", "novel_pe_map_kernel")
LDS = 128 * 1024 + 2 * 64 * 32 + 64 * 8 * 4      # A image + the encoder's and the general Tap + src_pe | tgt_pe | 0 0 per point


def _isa(src, tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_gen_nvpe") / (src + ".s")
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(CSRC / src)], check=True, capture_output=True, timeout=900)
    return asm.read_text()


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request, tmp_path_factory):
    src, kernel = UNITS[request.param]
    return request.param, kernel, _isa(src, tmp_path_factory)


@pytest.fixture(scope="module")
def map_unit(tmp_path_factory):
    return MAP_UNIT[1], _isa(MAP_UNIT[0], tmp_path_factory)


def _kernels(isa, kernel):
    """(symbol, LDS bytes, max workgroup size) of every kernel of the code object whose name holds ``kernel``"""
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.max_flat_workgroup_size:\s+(\d+).*?\.name:\s+(\S+)", isa, flags=re.S)
    return [(n, int(g), int(w)) for g, w, n in meta if kernel in n]


def _no_flat_no_atomics(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))
    atomics = re.findall(r"^\s+(\w*atomic\w*)", isa, re.M)
    assert not atomics, sorted(set(atomics))


def test_no_flat_instructions_and_no_atomics(unit):
    _no_flat_no_atomics(unit[2])


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
    kern = _kernels(isa, kernel)
    assert len(kern) == 3 and all(g == LDS and g <= 160 * 1024 and w == 512 for _, g, w in kern), kern
    # ... which is the size the kernel declares: the constant its __shared__ array is sized by, in 16-byte entries
    src = (CSRC / UNITS[prec][0]).read_text()
    decl = re.search(r"constexpr int (NVPE_LDS_\w+) = (A_\w+) \+ 2 \* TILE_P \* \(int\)\(sizeof\(Tap\) / sizeof\(\w+\)\) \+ 2 \* TILE_P;", src)
    assert decl and f"lds[{decl.group(1)}]" in src
    assert (8192 + 2 * 64 * 2 + 2 * 64) * 16 == LDS                    # A_F4 = A_H8 = 8192, a Tap is two 16-byte entries


def test_the_map_builder_is_one_exact_fp32_kernel(map_unit):
    kernel, isa = map_unit
    _no_flat_no_atomics(isa)
    assert set(re.findall(r"\b(v_mfma_\w+)", isa)) == {"v_mfma_f32_32x32x2_f32"}
    kern = _kernels(isa, kernel)
    assert len(kern) == 1 and kern[0][1] == 128 * 1024 and kern[0][2] == 512, kern


def test_the_parent_and_novel_units_instantiate_no_pe_kernel():
    """the novel_pe kernels live in translation units of their own: the parents' and the NOVEL units' code objects (pinned by
    tests/test_isa_guard_gen*.py) hold none, and include nothing of theirs"""
    for src in ("points_mlp_gen.hip", "points_mlp_gen_f16.hip", "points_mlp_gen_kernel.hpp", "points_mlp_gen_f16_kernel.hpp",
                "points_mlp_gen_nv.hip", "points_mlp_gen_f16_nv.hip", "linz_maps_gen.hip"):
        text = (CSRC / src).read_text()
        assert "nvpe" not in text and "novel_pe" not in text and "NovelPe" not in text, src
