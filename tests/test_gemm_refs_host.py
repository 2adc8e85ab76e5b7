"""CPU checks of tests/gemm_refs.py (no GPU): the float64 restatement equals torch's float64 ``linear`` and its autograd for each product
form and activation; both float32 CPU evaluations stay inside the fp32 bound and the numpy emulation of the f16x3 arithmetic inside the
f16x3 bound on every case; the allowance never exceeds its rigorous cap; every comparison rejects its mutant (one of the three passes
dropped, the last contraction element of the smallest-magnitude row dropped, Softplus(0) in the padding of a ragged tile, the bias added
once per split, the old C ignored under ``accumulate``, two rows of a 16-row block exchanged, a k-step multiplied twice); and the entry
points refuse what they must before any device work (diner_train_gemm now as diner_train_gemm_act).

Largest figure / bound on the CPU side over all cases: the float32 evaluations below 0.25 by construction (the allowance is 4 x their own
error + 2^-24), 0.27 where the rigorous cap replaces it (the 4 x 4 x 4 products and a 31-row dW with Softplus); the emulation 0.58 (a 33-row
dW with Softplus(3) on an operand, whose float32 Softplus error the emulation carries), 0.51 on the 4 x 4 x 4 forward.
A mutant that a bound does not reject is a finding about the case, never a reason to move the bound: the cases give the element the
dropped-element mutant removes a path to C[m_small, 0] (positive operand, positive S)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_refs as gr
from tests.gemm_refs import ACT_CASES, ALL_CASES, ACT_RELU, ACT_SOFTPLUS

IDS = lambda cases: [c.id for c in cases]
SMALL = [c for c in ALL_CASES if c.M * c.N * c.K <= 1 << 25]


def t_act(x, code, beta):
    if code == ACT_RELU:
        return torch.relu(x)
    if code == ACT_SOFTPLUS:
        return F.softplus(x, beta=beta, threshold=20.0)
    return x


@pytest.mark.parametrize("case", SMALL, ids=IDS(SMALL))
def test_restatement_equals_torch_float64(case):
    """forward: F.linear; dX: the input gradient of act_s followed by F.linear; dW: the weight gradient of F.linear; the epilogue factor:
    autograd's derivative of the activation"""
    d = case.build()
    A, B = (torch.from_numpy(d[k].astype(np.float64)) for k in ("A", "B"))
    bias = None if d["bias"] is None else torch.from_numpy(d["bias"].astype(np.float64))
    a, b = t_act(A, case.act_a, case.beta), t_act(B, case.act_b, case.beta)
    if case.form in ("fwd", "nn"):
        acc = F.linear(a, b.T.contiguous(), bias)                          # B^T is the layer's weight [N, K]
    elif case.form == "dx":
        x = torch.zeros(case.M, case.N, dtype=torch.float64, requires_grad=True)
        F.linear(x, b).backward(a)                                         # b [K, N]: a layer N -> K, a its output gradient
        acc = x.grad if bias is None else x.grad + bias
    else:
        w = torch.zeros(case.M, case.N, dtype=torch.float64, requires_grad=True)
        F.linear(b, w).backward(a.T.contiguous())                          # b = X [rows, N], a^T = dY [rows, M]: w.grad = dY^T X
        acc = w.grad if bias is None else w.grad + bias
    if d["S"] is not None:
        s = torch.from_numpy(d["S"].astype(np.float64)).requires_grad_(True)
        t_act(s, case.act_s, case.beta).backward(acc.detach().clone())     # autograd's act_bwd: acc * act'(s)
        acc = s.grad
    if d["C0"] is not None:
        acc = acc + torch.from_numpy(d["C0"].astype(np.float64))
    ref, absr = gr.ref64(case)
    err = np.abs(acc.detach().numpy() - ref)
    assert (err <= 64 * 2.0 ** -53 * case.K * absr + 1e-300).all(), float((err / np.where(absr > 0, absr, 1)).max())


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS(ALL_CASES))
def test_float32_evaluations_and_emulation_are_inside_their_bounds(case):
    for prec in ("fp32", "f16x3"):
        a = gr.allowance(case, prec)
        assert 2.0 ** -24 <= a <= gr.cap(case)
        r_mm, r_seq = gr.worst(gr.eval_matmul32(case), case, prec), gr.worst(gr.eval_seq32(case, gr.DEPTH[prec]), case, prec)
        assert r_mm <= 1.0 and r_seq <= 1.0, (prec, r_mm, r_seq, gr.cpu_side(case, prec), gr.cap(case))
    r = gr.worst(gr.emulate_f16x3(case), case, "f16x3")
    print(f"FIG {case.id} emulation / bound {r:.3f} cpu32 {max(gr.cpu_side(case, 'f16x3')):.3e} allowance {gr.allowance(case, 'f16x3'):.3e}")
    assert r <= 1.0, r
    assert np.isfinite(gr.bound(case, "f16x3")).all() and (gr.bound(case, "f16x3") >= 0).all()


def rejected(got, case, prec):
    return gr.worst(got, case, prec) > 1.0


NOT_DW512 = [c for c in ALL_CASES if c.K < 8192]   # the 8192-row products add nothing to a mutant's shape coverage


@pytest.mark.parametrize("case", NOT_DW512, ids=IDS(NOT_DW512))
def test_mutants_every_case(case):
    for which in ("hh", "hl", "lh"):
        assert rejected(gr.mutant_pass_dropped(case, which), case, "f16x3"), which
    for prec in ("fp32", "f16x3"):
        assert rejected(gr.mutant_drop_element(case, prec), case, prec), ("element dropped", prec)
        assert rejected(gr.mutant_step_twice(case, prec), case, prec), ("k-step twice", prec)
        if case.M >= 2:
            assert rejected(gr.mutant_rows_exchanged(case, prec), case, prec), ("rows exchanged", prec)


BOTH_SP = [c for c in ACT_CASES if c.act_a == ACT_SOFTPLUS and c.act_b == ACT_SOFTPLUS]
BIAS_SPLIT = [c for c in ALL_CASES if c.bias and c.splits > 1]
WITH_C0 = [c for c in ALL_CASES if c.c0 and c.K < 8192]


def test_mutant_case_sets_are_not_empty():
    assert len([c for c in BOTH_SP if c.K % 32]) >= 3 and {c.form for c in BOTH_SP} >= {"fwd", "dx", "dw", "nn"}
    assert len(BIAS_SPLIT) >= 2 and {c.form for c in BIAS_SPLIT} >= {"fwd", "dw"}
    assert any(c.accumulate and not c.atomic for c in WITH_C0) and any(c.atomic for c in WITH_C0)
    assert any(c.pad_c and c.pad_s and c.pad_a for c in ACT_CASES)


@pytest.mark.parametrize("case", BOTH_SP, ids=IDS(BOTH_SP))
def test_mutant_softplus_in_the_padding(case):
    for prec in ("fp32", "f16x3"):
        if case.K % gr.TILE_K[prec]:
            assert rejected(gr.mutant_softplus_padding(case, prec), case, prec), prec


@pytest.mark.parametrize("case", BIAS_SPLIT, ids=IDS(BIAS_SPLIT))
def test_mutant_bias_once_per_split(case):
    assert rejected(gr.mutant_bias_per_split(case, "fp32"), case, "fp32")
    assert rejected(gr.mutant_bias_per_split(case, "fp32"), case, "f16x3")


@pytest.mark.parametrize("case", WITH_C0, ids=IDS(WITH_C0))
def test_mutant_old_c_ignored(case):
    assert rejected(gr.mutant_ignore_c0(case, "fp32"), case, "fp32")
    assert rejected(gr.mutant_ignore_c0(case, "fp32"), case, "f16x3")


def test_cap_alone_would_not_reject_a_dropped_pass():
    """why the allowance is taken from the float32 evaluations: at K = 1024 the rigorous cap is wider than a dropped lo*hi pass"""
    case = next(c for c in ACT_CASES if c.id == "fwd-128x4x1024")
    ref, absr = gr.ref64(case)
    err = np.abs(gr.mutant_pass_dropped(case, "lh") - ref)
    assert (err <= gr.model_term(case) + gr.cap(case) * absr).all()
    assert rejected(gr.mutant_pass_dropped(case, "lh"), case, "f16x3")


def test_scale_from_amax_and_split():
    assert gr.scale_from_amax(np.float32(1.0)) == 2.0 ** 13 and gr.scale_from_amax(np.float32(0.0)) == 1.0
    assert gr.scale_from_amax(np.float32(3e-12)) * 3e-12 >= 2.0 ** 13 and gr.scale_from_amax(np.float32(3e-12)) * 3e-12 < 2.0 ** 14
    assert gr.scale_from_amax(np.float32(1e-38)) == 2.0 ** 100
    x = np.array([1.0 + 2.0 ** -12, 3.0e-7, -65504.0 / 16], np.float32)
    hi, lo = gr.split16(x, 16.0)
    assert hi[0] == 16.0 and lo[0] == 2.0 ** -8
    assert abs((hi[1] + lo[1]) / 16.0 - x[1]) <= 2.0 ** -24 / 16.0          # the fp16 subnormal floor of the lo half
    assert hi[2] == -65504.0 and lo[2] == 0.0


# ---- refusals: return code only, before any device work (every pointer is fake) -----------------------------------------------------
@pytest.mark.parametrize("entry,kw,what", gr.REFUSALS, ids=[f"{e}-{i}" for i, (e, _, _) in enumerate(gr.REFUSALS)])
def test_refusals(entry, kw, what):
    from diner_amd import _lib
    fake = C.c_void_p(1 << 20)
    assert gr.refusal_call(_lib.lib(), entry, fake, None, **kw) == -1, (entry, kw)
    assert what in _lib.lib().diner_last_error().decode(), (_lib.lib().diner_last_error(), what)


@pytest.mark.parametrize("entry", ["act", "f16x3", "std_fp32", "std_f16x3"])
def test_refusal_base_call_is_accepted(entry):
    from diner_amd import _lib
    assert gr.refusal_call(_lib.lib(), entry, C.c_void_p(1 << 20), None, M=0) == 0   # M = 0: valid, nothing to launch
