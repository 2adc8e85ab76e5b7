"""Compile-time guard of the shape-general f16x3 training kernels (diner_amd/csrc/train_gen_f16.hip), cross-compiled for gfx950 (no GPU):
no FLAT instruction in the code object (tests/test_isa_guard.py's rule), the GEMM kernels on fp16 MFMA only, no scratch spill, and a VGPR
count within what each kernel's launch bound leaves a wave."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = ROOT / "diner_amd" / "csrc" / "train_gen_f16.hip"
KERNEL = r"_ZN5diner13train_gen_f1621gemm_act_f16x3_kernelILb([01])ELb([01])ELb([01])ELb([01])EEEvNS0_8GemmArgsE"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa_train_gen_f16") / "train_gen_f16.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", str(asm),
                    str(SRC)], check=True, capture_output=True, timeout=900)
    return asm.read_text()


def _gemm_kernels(isa):
    return sorted(set(m.group(0) for m in re.finditer(rf"^{KERNEL}(?=:)", isa, re.M)))


def _descriptor(isa, name):
    m = re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel", isa, re.S)
    assert m, name
    return m.group(1)


def test_no_flat_instructions(isa):
    flat = re.findall(r"^\s+(flat_\w+)", isa, re.M)
    assert not flat, sorted(set(flat))


def test_kernels_present(isa):
    names = _gemm_kernels(isa)
    # A along k x B along k / n, A along m x B along k / n, A along k x pre-split B; each with and without the Softplus staging
    assert len(names) == 10, names
    assert re.search(r"^_ZN5diner13train_gen_f1619split_weight_kernel\S*:", isa, re.M)


def test_gemm_kernels_on_fp16_mfma_only(isa):
    for name in _gemm_kernels(isa):
        body = isa[isa.index(name + ":"):]
        body = body[:body.index("s_endpgm")]
        mfma = set(re.findall(r"\b(v_mfma_\w+)", body))
        assert mfma == {"v_mfma_f32_32x32x16_f16"}, (name, mfma)


def test_gemm_kernels_do_not_spill_and_fit_their_launch_bound(isa):
    for name in _gemm_kernels(isa):
        d = _descriptor(isa, name)
        seg = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", d).group(1))
        assert seg == 0, (name, seg)
        ak, bnc, pre, _ = (int(x) for x in re.match(KERNEL, name).groups())
        # 256-thread workgroups: two per CU (k-staged operands, the step's hot forms) leave a wave 256 of the SIMD's 512 registers
        # (VGPRs + AGPRs), one per CU all 512
        budget = 256 if (ak and not bnc) else 512
        total = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", d).group(1))
        assert total <= budget, (name, total, budget)
    # the hot forms are the two-per-CU ones
    for pre in (0, 1):
        assert any(re.match(KERNEL, n).groups()[:3] == ("1", "0", str(pre)) for n in _gemm_kernels(isa))
