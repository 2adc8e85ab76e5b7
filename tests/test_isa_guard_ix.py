"""Compile-time guard of the any-lookup-mode twins of the default point/MLP kernel (diner_amd/csrc/points_mlp_f16_ix.hip:
points_mlp_f16_kernel<LINZ, false, VIT, int, int>), cross-compiled for gfx950 (no GPU).  They run the same generated assembly core as
the default kernels, so they carry the register contract tests/test_isa_guard.py checks on points_mlp_f16.hip: the core owns
v[CAP:255] and every AGPR, the compiler's code stays below CAP, no MFMA outside the core, the weight ring never drains inside a GEMM
block, no FLAT instruction, 256 registers per lane and no AGPR in the metadata."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "diner_amd" / "csrc"
TWIN = re.compile(r"^_ZN5diner5f16x321points_mlp_f16_kernelILb[01]ELb0ELb[01]EJiiEE\S+:")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-C", str(CSRC), "f16_core16.inc", "f16_core16_trace.inc"], check=True, capture_output=True)
    asm = tmp_path_factory.mktemp("isa_f16_ix") / "points_mlp_f16_ix.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fno-unroll-loops", "-Wno-inline-asm", "-S",
                    "--cuda-device-only", "-o", str(asm), str(CSRC / "points_mlp_f16_ix.hip")], check=True, capture_output=True, timeout=900)
    return asm.read_text()


def _cap():
    return int(re.search(r"constexpr int F16_VGPR_CAP = (\d+);", (CSRC / "f16_core16.inc").read_text()).group(1))


def test_four_twins_and_nothing_else(isa):
    starts = [l for l in isa.split("\n") if TWIN.match(l)]
    assert len(starts) == 4, "expected <lin_z maps | per-point lin_z GEMMs> x <view-sequential | views-in-tile>, any lookup mode"
    names = set(re.findall(r"^(_Z\S+):\s*(?:;.*)?$", isa, re.M))
    assert all("points_mlp_f16_kernel" in n and "EJiiEE" in n for n in names), sorted(names)   # no default kernel, no pack kernel


def test_compiler_stays_out_of_the_core_registers(isa):
    cap = _cap()
    lines = isa.split("\n")
    starts = [i for i, l in enumerate(lines) if TWIN.match(l)]
    for s0 in starts:
        end = next(i for i in range(s0, len(lines)) if "s_endpgm" in lines[i])
        in_asm, core_mfma, core_loads, stmt = False, 0, 0, []
        for i in range(s0, end):
            l = lines[i].split(";")[0] if not lines[i].lstrip().startswith(";;") else lines[i]
            if "#ASMSTART" in lines[i]:
                in_asm, stmt = True, []
                continue
            if "#ASMEND" in lines[i]:
                in_asm = False
                if any("v_mfma" in x for x in stmt):
                    assert not any("vmcnt(0)" in x for x in stmt), f"asm statement ending at line {i}: vmcnt(0) inside a GEMM block"
                continue
            if in_asm:
                stmt.append(l)
                core_mfma += "v_mfma" in l
                core_loads += "global_load_dwordx4" in l
                continue
            assert "v_accvgpr" not in l and not re.search(r"\ba\[?\d", l), f"line {i}: compiler-generated AGPR use: {l}"
            assert "v_mfma" not in l, f"line {i}: MFMA outside the generated core: {l}"
            for m in re.finditer(r"\bv\[?(\d+)(?::(\d+))?\]?", l):
                hi = int(m.group(2) or m.group(1))
                assert hi < cap, f"line {i}: compiler code touches v{hi} >= {cap} (the core's registers): {l}"
        assert core_mfma >= 400 and core_loads >= 100


def test_no_flat_instructions(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_register_budget(isa):
    meta = re.findall(r"\.agpr_count:\s+(\d+)\n\s+\.args:.*?\.name:\s+(\S+).*?\.vgpr_count:\s+(\d+)", isa, flags=re.S)
    kern = [(int(a), n, int(v)) for a, n, v in meta if "points_mlp_f16_kernel" in n]
    assert len(kern) == 4
    for agpr, name, vgpr in kern:
        assert agpr == 0 and vgpr <= 256, (name, agpr, vgpr)
