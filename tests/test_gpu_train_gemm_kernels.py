"""The training GEMM kernels, one by one on the GPU through the C ABI, element by element against float64: ``gemm_kernel``,
``gemm_f16x3_kernel``, ``dw512_kernel`` (diner_train_gemm, both precisions), ``gemm_panel_kernel``, ``gemm_core_kernel``, ``gemm_act_kernel``
(diner_train_gemm_act), ``gemm_act_f16x3_kernel`` streamed and pre-split (diner_train_gemm_act_f16x3, _f16x3_w) and the splitters
``split_panel_kernel``, ``pack_core_kernel``, ``split_weight_kernel``.  Restatement, case table and bounds are those of tests/gemm_refs.py
(CPU values only; tests/test_gemm_refs_host.py proves them and that every comparison rejects its mutant).  Every output is filled with NaN
before the call; padding columns (ldc > N) and spare rows must keep their NaN bits.

Bounds: per element, relative to absr = |act_s'| (|actA(A)| @ |actB(B)| + |bias|) + |old C|: fp32 kernels allowance x absr, f16x3 kernels
the model term of the fp16 hi/lo split + allowance x absr; allowance = min(4 x the worse of two float32 CPU evaluations + 2^-24,
(K + splits + 2) x 2^-24); Softplus terms as gemm_refs.py derives them.  None is tuned to the figures below.

Largest errors observed over all cases of a family (in units of absr; CPU side: the float32 evaluation the allowance is taken from; GPU
side: MI355X) and the largest GPU error / bound of any element:

    family                                   CPU float32 side   GPU        largest GPU / bound
    gemm_act_kernel (fp32)                   8.05e-07           9.85e-07   0.33   (fwd 128 x 4 x 1024)
    gemm_act_f16x3_kernel, streamed          6.23e-07           3.48e-06   0.63   (fwd 4 x 4 x 4: the model term, not the accumulation)
    gemm_act_f16x3_kernel, pre-split         6.23e-07           5.73e-07   0.34   (fwd 128 x 4 x 1024)
    gemm_kernel (fp32)                       2.86e-07           2.86e-07   0.35   (dX 132 x 512 x 512)
    gemm_f16x3_kernel                        2.86e-07           4.71e-07   0.28   (nn 128 x 512 x 56)
    gemm_kernel (fp32), dW 512 x 512         2.92e-07           3.61e-07   0.31   (8200 rows; atomics: 3.51e-07, 0.30 in a second run)
    dw512_kernel                             1.19e-07           1.00e-07   0.14   (8192 / 8200 rows; atomics: 9.41e-08 in a second run)
    gemm_panel_kernel                        2.36e-07           2.22e-07   0.32   (forward, M = 1, K = 56)
    gemm_core_kernel                         1.58e-07           2.68e-07   0.30   (forward, M = 65)

The device's Softplus, measured through a one-hot B on the fp32 kernel against float64: 1.9 x 2^-24 of the result at beta 1, 17 x 2^-24 at
beta 3 (where x beta is itself rounded), 0.42 of its bound, (|x beta| + 4) x 2^-23, at most.
One-hot B (C = actA(A) selected): the fp32 kernels return it bit for bit in all four stride forms and at every ragged M, N and K of the
table; the f16x3 kernels within the model term.  Pre-split, panel and core results lie within the sum of the bounds of the streamed f16x3
kernel's; every splitter's planes equal the emulation's hi and lo bit for bit; sentinels intact; the core's max|C| word exact.
No kernel was found wrong.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_refs as gr
from tests.gemm_refs import ACT_CASES, ACT_RELU, ACT_SOFTPLUS, CORE_CASES, DW512_CASES, FORMS, ONEHOT_CASES, ONEHOT_SOFTPLUS, PANEL_CASES, STD_CASES

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NAN = float("nan")
SPARE = 3                                     # rows allocated past M in every output
IDS = lambda cases: [c.id for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)     # a copy: the cases' arrays are read-only


def P_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def call(name, *args):
    from diner_amd import _lib
    rc = getattr(_lib.lib(), name)(*args)
    assert rc == 0, (name, rc, _lib.lib().diner_last_error())
    torch.cuda.synchronize()


def fig(family, case, cpu, gpu, ratio):
    """one line per comparison for the table in the module docstring"""
    print(f"FIG {family} | {case.id} cpu {cpu:.3e} gpu {gpu:.3e} ratio {ratio:.3f}")


def padded(mat, pad, dev, spare=0):
    """a [rows + spare, cols + pad] device matrix of NaN holding `mat` in its upper left"""
    rows, cols = mat.shape
    buf = torch.full((rows + spare, cols + pad), NAN, device=dev)
    buf[:rows, :cols] = T(mat, dev)
    return buf


class Operands:
    """a case's operands on the device, as its form stores them"""

    def __init__(self, case, dev):
        self.c, self.dev = case, dev
        d = self.d = case.build()
        st = gr.stored(case, d)
        (a, self.sam, self.sak), (b, self.sbk, self.sbn) = st["A"], st["B"]
        self.A, self.B = T(a, dev), T(b, dev)
        self.bias = None if d["bias"] is None else T(d["bias"], dev)
        self.S = None if d["S"] is None else padded(d["S"], case.pad_s, dev)
        self.lds = 0 if self.S is None else self.S.stride(0)
        self.amax = None
        if d["amax"] is not None:
            flat = T(d["A"], dev)
            self.amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
            call("diner_train_amax", P_(flat), flat.numel(), P_(self.amax), ST(dev))
            assert self.amax.cpu().numpy().view(F32)[0] == d["amax"]

    def out(self, preset):
        """the NaN-filled output (ldc = N + pad_c, SPARE rows more); preset: old C, zeros (atomic onto nothing) or None"""
        c = self.c
        buf = torch.full((c.M + SPARE, c.N + c.pad_c), NAN, device=self.dev)
        if preset is not None:
            buf[:c.M, :c.N] = T(preset, self.dev)
        return buf

    def result(self, buf):
        """the [M, N] result; everything else of the buffer must still hold its NaN bits"""
        c = self.c
        bits = buf.view(torch.int32)
        nanbits = torch.full((1,), NAN, device=self.dev).view(torch.int32)[0]
        assert (bits[c.M:] == nanbits).all(), "a spare row was written"
        assert (bits[:, c.N:] == nanbits).all(), "a padding column was written"
        return buf[:c.M, :c.N].cpu().numpy()

    def preset(self):
        c, d = self.c, self.d
        if d["C0"] is not None:
            return d["C0"]
        return np.zeros((c.M, c.N), F32) if c.atomic else None

    def gemm_args(self, buf):
        c = self.c
        return (P_(self.A), P_(self.B), P_(self.bias), P_(self.S), P_(buf), c.M, c.N, c.K, self.sam, self.sak, self.sbk, self.sbn, buf.stride(0),
                self.lds)

    # ---- the entries ---------------------------------------------------------------------------------------------------------------
    def act_fp32(self):
        c, buf = self.c, self.out(self.preset())
        call("diner_train_gemm_act", *self.gemm_args(buf), c.act_a, c.act_b, c.act_s, c.beta, c.accumulate, c.atomic, c.k_chunk, ST(self.dev))
        return self.result(buf)

    def act_f16x3(self, accumulate=None):
        c, d = self.c, self.d
        buf = self.out(self.preset())
        call("diner_train_gemm_act_f16x3", *self.gemm_args(buf), c.act_a, c.act_b, c.act_s, c.beta,
             c.accumulate if accumulate is None else accumulate, c.atomic, c.k_chunk, P_(self.amax), None, d["exp_a"], d["exp_b"], ST(self.dev))
        return self.result(buf)

    def can_presplit(self):
        c = self.c
        return FORMS[c.form][0] and c.act_b == 0 and not c.atomic and c.k_chunk == 0

    def split_weight(self):
        """planes of diner_train_split_weight for the stored B: [N, K] (fwd) or [K, N] (dx: transpose)"""
        from diner_amd import _lib
        c = self.c
        halfs = int(_lib.lib().diner_train_split_weight_halfs(c.N, c.K))
        hi, lo = (torch.full((halfs,), NAN, dtype=torch.float16, device=self.dev) for _ in range(2))
        call("diner_train_split_weight", P_(self.B), c.N, c.K, self.B.stride(0), int(FORMS[c.form][1]), self.d["exp_b"], P_(hi), P_(lo), ST(self.dev))
        return hi, lo

    def act_f16x3_w(self):
        c, d = self.c, self.d
        hi, lo = self.split_weight()
        buf = self.out(self.preset())
        call("diner_train_gemm_act_f16x3_w", P_(self.A), self.sam, P_(hi), P_(lo), P_(self.bias), P_(self.S), self.lds, P_(buf), buf.stride(0), c.M,
             c.N, c.K, c.act_a, c.act_s, c.beta, c.accumulate, P_(self.amax), d["exp_a"], d["exp_b"], ST(self.dev))
        return self.result(buf)

    def std(self, precision):
        c, d = self.c, self.d
        assert c.act_s in (0, ACT_RELU) and ACT_SOFTPLUS not in (c.act_a, c.act_b)
        buf = self.out(self.preset())
        call("diner_train_gemm", *self.gemm_args(buf), int(c.act_a == ACT_RELU), int(c.act_b == ACT_RELU), c.accumulate, c.atomic, c.k_chunk,
             precision, P_(self.amax), None, d["exp_a"], d["exp_b"], ST(self.dev))
        return self.result(buf)

    def weight(self):
        """the panel / core entries' weight matrix and its transpose flag: [512, K] as stored, or its transpose [K, 512] for the dX cases"""
        if self.c.S:
            return self.B.t().contiguous(), 1
        return self.B, 0

    def addend(self):
        return None if self.d["C0"] is None else padded(self.d["C0"], 4 if self.c.pad_c else 0, self.dev)

    def panel(self):
        c, d = self.c, self.d
        W, tr = self.weight()
        kpad = (c.K + 31) // 32 * 32
        hi, lo = (torch.full((512 * kpad,), NAN, dtype=torch.float16, device=self.dev) for _ in range(2))
        call("diner_train_split_panel", P_(W), c.K, W.stride(0), tr, d["exp_b"], P_(hi), P_(lo), ST(self.dev))
        add, buf = self.addend(), self.out(None)
        call("diner_train_gemm_panel", P_(self.A), self.sam, P_(hi), P_(lo), P_(self.bias), P_(self.S), self.lds, P_(add),
             0 if add is None else add.stride(0), P_(buf), buf.stride(0), c.M, c.K, int(c.act_a == ACT_RELU), P_(self.amax), d["exp_a"], d["exp_b"],
             ST(self.dev))
        planes = [p.view(kpad // 32, 512, 32).permute(1, 0, 2).reshape(512, kpad) for p in (hi, lo)]     # [k/32][512][32] -> [n][k]
        return self.result(buf), planes

    def core(self, in_place=False, reductions=False):
        c, d = self.c, self.d
        W, tr = self.weight()
        pack = torch.full((2 * 512 * 512,), NAN, dtype=torch.float16, device=self.dev)
        call("diner_train_pack_core", P_(W), W.stride(0), tr, d["exp_b"], P_(pack), ST(self.dev))
        buf = self.out(d["C0"] if in_place else None)
        add = buf if in_place else self.addend()
        colsum = torch.zeros(512, device=self.dev) if reductions else None
        word = torch.zeros(1, dtype=torch.int32, device=self.dev) if reductions else None
        call("diner_train_gemm_core", P_(self.A), self.sam, P_(pack), P_(self.bias), P_(self.S), self.lds, P_(add), 0 if add is None else add.stride(0),
             P_(buf), buf.stride(0), c.M, int(c.act_a == ACT_RELU), P_(self.amax), d["exp_a"], d["exp_b"], P_(colsum), P_(word), ST(self.dev))
        # [col_tile][kb][part][lane = 32 h + c][8]: B[32 tile + c][16 kb + 8 h + j]  ->  [part][n][k]
        planes = pack.view(16, 32, 2, 2, 32, 8).permute(2, 0, 4, 1, 3, 5).reshape(2, 512, 512)
        return self.result(buf), planes, colsum, word


def check(family, case, got, precision):
    """every element within the case's bound; a FIG line"""
    assert np.isfinite(got).all(), (family, case.id, "non-finite result")
    ratio = gr.worst(got, case, precision)
    fig(family, case, max(gr.cpu_side(case, precision)), gr.worst_abs(got, case), ratio)
    assert ratio <= 1.0, (family, case.id, ratio)


def check_pair(what, case, x, y):
    """two f16x3 routes of the same product: within the sum of their bounds"""
    b = 2.0 * gr.bound(case, "f16x3")
    err = np.abs(x.astype(F64) - y.astype(F64))
    assert (err <= b).all(), (what, case.id, float((err / np.where(b > 0, b, 1)).max()))


def check_planes(case, hi, lo):
    """[n][k] planes (already cut to N x K) against the emulation's split of B * 2^exp_b, bit for bit"""
    (_, _), (bh, bl) = gr.split_case(case)
    assert np.array_equal(hi.cpu().numpy().astype(F64), bh.T), (case.id, "hi plane")
    assert np.array_equal(lo.cpu().numpy().astype(F64), bl.T), (case.id, "lo plane")


# ---- the shape-general entries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACT_CASES, ids=IDS(ACT_CASES))
def test_gemm_act_kernels(case, dev):
    op = Operands(case, dev)
    check("gemm_act_kernel (fp32)", case, op.act_fp32(), "fp32")
    streamed = op.act_f16x3()
    check("gemm_act_f16x3_kernel, streamed", case, streamed, "f16x3")
    if op.can_presplit():
        pre = op.act_f16x3_w()
        check("gemm_act_f16x3_kernel, pre-split", case, pre, "f16x3")
        check_pair("pre-split against streamed", case, pre, streamed)
        hi, lo = op.split_weight()
        npad, kpad = (case.N + 127) // 128 * 128, (case.K + 31) // 32 * 32
        hi, lo = hi.view(npad, kpad), lo.view(npad, kpad)
        check_planes(case, hi[:case.N, :case.K], lo[:case.N, :case.K])
        for p in (hi, lo):                                   # the zero padding the GEMM reads without bounds
            assert (p[case.N:] == 0).all() and (p[:, case.K:] == 0).all()


# ---- the standard entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STD_CASES, ids=IDS(STD_CASES))
def test_standard_gemm_kernels(case, dev):
    op = Operands(case, dev)
    check("gemm_kernel (fp32)", case, op.std(0), "fp32")
    f16 = op.std(1)
    check("gemm_f16x3_kernel", case, f16, "f16x3")
    check_pair("standard against shape-general f16x3", case, f16, op.act_f16x3())


@pytest.mark.parametrize("case", DW512_CASES, ids=IDS(DW512_CASES))
def test_dw512_kernel(case, dev):
    op = Operands(case, dev)
    check("gemm_kernel (fp32), dW 512 x 512", case, op.std(0), "fp32")
    check("dw512_kernel", case, op.std(1), "f16x3")


@pytest.mark.parametrize("case", PANEL_CASES, ids=IDS(PANEL_CASES))
def test_panel_kernel(case, dev):
    op = Operands(case, dev)
    got, (hi, lo) = op.panel()
    check("gemm_panel_kernel", case, got, "f16x3")
    check_planes(case, hi[:, :case.K], lo[:, :case.K])
    assert (hi[:, case.K:] == 0).all() and (lo[:, case.K:] == 0).all()
    # the streamed shape-general kernel on the same data: the addend as the old C of an accumulating call
    if case.K % 4 == 0:
        check_pair("panel against streamed", case, got, op.act_f16x3(accumulate=int(case.c0)))


@pytest.mark.parametrize("case", CORE_CASES, ids=IDS(CORE_CASES))
def test_core_kernel(case, dev):
    op = Operands(case, dev)
    got, planes, colsum, word = op.core(reductions=True)
    check("gemm_core_kernel", case, got, "f16x3")
    check_planes(case, planes[0], planes[1])
    check_pair("core against streamed", case, got, op.act_f16x3(accumulate=int(case.c0)))
    # the folded reductions are taken over the stored result: max|C| exactly, the column sums within (M + 8) roundings of sum |C|
    assert word.cpu().numpy().view(F32)[0] == np.abs(got).max()
    cs, g64 = colsum.cpu().numpy().astype(F64), got.astype(F64)
    assert (np.abs(cs - g64.sum(0)) <= (case.M + 8) * gr.U * np.abs(g64).sum(0)).all()
    if case.c0:                                              # the addend aliasing the output, as the residual stream uses it
        again, _, _, _ = op.core(in_place=True)
        assert np.array_equal(again, got)


# ---- one-hot B: the kernel returns a selection of actA(A) ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONEHOT_CASES, ids=IDS(ONEHOT_CASES))
def test_one_hot_selection(case, dev):
    d = case.build()
    want = gr.operands32(case, d)[0][:, d["sel"]]
    op = Operands(case, dev)
    assert np.array_equal(op.act_fp32(), want), "gemm_act_kernel"
    assert np.array_equal(op.std(0), want), "gemm_kernel"
    mt = gr.model_term(case)
    for name, got in (("gemm_act_f16x3_kernel", op.act_f16x3()), ("gemm_f16x3_kernel", op.std(1))):
        err = np.abs(got.astype(F64) - want.astype(F64))
        assert (err <= mt).all(), (name, float(err.max()), float(mt.max()))


@pytest.mark.parametrize("case", ONEHOT_SOFTPLUS, ids=IDS(ONEHOT_SOFTPLUS))
def test_one_hot_measures_the_device_softplus(case, dev):
    """C = Softplus(A) selected: the device's log1pf(expf(x beta)) / beta against float64.  Bound (reasoning, not tuned): x beta is rounded
    once, which moves exp by |x beta| ulp at most and the result by no more (d log1p(e) / d log e <= 1); expf, log1pf and the division add
    one ulp each, one more for the product: (|x beta| + 4) x 2^-23 of the result."""
    d = case.build()
    x = d["A"][:, d["sel"]].astype(F64)
    want = gr.act(x, ACT_SOFTPLUS, case.beta)
    op = Operands(case, dev)
    got = op.act_fp32().astype(F64)
    rel = np.abs(got - want) / want
    lim = (np.abs(x * case.beta) + 4.0) * 2.0 ** -23
    print(f"FIG device softplus | {case.id} largest relative error {rel.max():.3e} = {rel.max() / 2.0 ** -24:.2f} x 2^-24, largest error / bound "
          f"{(rel / lim).max():.3f}")
    assert (rel <= lim).all()
    got16 = op.act_f16x3().astype(F64)
    assert (np.abs(got16 - want) <= gr.model_term(case) + lim * want).all()


# ---- refused calls: return code only; the operands are real buffers and the output keeps its NaN ------------------------------------------
def test_refusals_launch_nothing(dev):
    from diner_amd import _lib
    buf = torch.zeros(1 << 14, device=dev)
    for entry, kw, what in gr.REFUSALS:
        out = torch.full((1 << 14,), NAN, device=dev)
        over = dict(kw)                                      # A, B -> the zeros, C -> the NaN buffer
        over.setdefault("C", P_(out))
        assert gr.refusal_call(_lib.lib(), entry, P_(buf), ST(dev), **over) == -1, (entry, kw)
        assert what in _lib.lib().diner_last_error().decode(), (entry, kw)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), (entry, kw)
