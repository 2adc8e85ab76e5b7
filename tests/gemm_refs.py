"""Float64 restatements, cases and bounds of the training GEMM kernels (train.hip: gemm_kernel, gemm_f16x3_kernel, gemm_panel_kernel,
dw512_kernel; train_core.hip: gemm_core_kernel; train_gen.hip: gemm_act_kernel; train_gen_f16.hip: gemm_act_f16x3_kernel; and the
splitters split_panel_kernel, pack_core_kernel, split_weight_kernel).  CPU values only; tests/test_gemm_refs_host.py proves the
restatement, the bounds and the rejection of every mutant, tests/test_gpu_train_gemm_kernels.py runs the kernels against it.

One product, every entry point:   C[m,n] = (old C[m,n] +) act_s'(S[m,n]) * ( sum_k actA(A[m,k]) actB(B[k,n]) + bias[n] )
with the logical A [M,K], B [K,N]; the four stride forms (``form``) only say how the two are stored:
    fwd  A k-contiguous, B k-contiguous (a weight [N,K])      nn  A m-contiguous, B k-contiguous (never issued by the step)
    dx   A k-contiguous, B n-contiguous (a weight [K,N])      dw  A m-contiguous (dY [K,M]), B n-contiguous (X [K,N])
The panel and core entries (addend + (sum + bias) * [S > 0]) are the same formula with the addend as the old C.

Bounds, every one per element and relative to the sum of absolute terms
    absr = |act_s'(S)| * ( |actA(A)| @ |actB(B)| + |bias| ) + |old C|:
  * allowance(case, precision) = min( 4 x the larger error, in units of absr, of two float32 CPU evaluations (numpy's float32 matmul;
    a strictly k-sequential float32 accumulation in steps of the kernel's MFMA depth, chunk by chunk under split-K) + 2^-24,
    (K + splits + 2) x 2^-24 ).  The cap is the textbook bound of a K-term float32 dot product plus one rounding per split added and two for
    the epilogue; the allowance never exceeds it.
  * Softplus on an operand adds 4 x |float32 numpy softplus - float64 softplus| per operand element, propagated through |.| @ |.|.
  * Softplus as the epilogue derivative (not set by the issue; reasoning): the kernel evaluates g * z / (z + 1) with z = expf(beta s):
    a float32 evaluation of the factor differs from float64 by the exponential's argument rounding and last ulp, one addition and one
    division, so the bound grows by (4 x the largest relative error of numpy's float32 factor over the case + 2 x 2^-24) x absr.
    ReLU's factor [s > 0] is exact.
  * fp32 kernels: allowance x absr (+ the Softplus terms).
  * f16x3 kernels: the model term |A - A^| @ |B| + |A^| @ |B - B^| + |A_lo| @ |B_lo| (A, B the float32-activated operands, A^ = hi + lo
    unscaled; everything the scheme loses before accumulation, the fp16 subnormal floor included), times |act_s'|, + the fp32 form.
"""
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Optional

import numpy as np

F32, F64, F16 = np.float32, np.float64, np.float16
U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_SOFTPLUS = 0, 1, 2
EXP_ACT, EXP_W = -4, 4                      # diner_amd/training.py: the static scales of activations and weights
DEPTH = {"fp32": 2, "f16x3": 16}            # contraction depth of v_mfma_f32_32x32x2_f32 / v_mfma_f32_32x32x16_f16
TILE_K = {"fp32": 16, "f16x3": 32}          # k-step of the fp32 / f16x3 block tiles
FORMS = {"fwd": (True, False), "dx": (True, True), "dw": (False, True), "nn": (False, False)}   # (AK, BNC)


# ---- activations as train_blocks.hpp states them (dtype-preserving: float32 in, float32 arithmetic) ----------------------------------
def act(x, code, beta):
    if code == ACT_RELU:
        return np.where(x < 0, x.dtype.type(0), x)
    if code == ACT_SOFTPLUS:
        b = x.dtype.type(beta)
        xb = x * b
        return np.where(xb > 20, x, np.log1p(np.exp(np.minimum(xb, x.dtype.type(20)))) / b)
    return x


def dact(s, code, beta):
    """the factor act_bwd multiplies the gradient by: ReLU [s > 0]; Softplus z / (z + 1), z = exp(beta s), 1 where beta s > 20"""
    if code == ACT_RELU:
        return (s > 0).astype(s.dtype)
    if code == ACT_SOFTPLUS:
        b = s.dtype.type(beta)
        xb = s * b
        z = np.exp(np.minimum(xb, s.dtype.type(20)))
        return np.where(xb > 20, s.dtype.type(1), z / (z + s.dtype.type(1)))
    return np.ones_like(s)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    id: str
    form: str                      # fwd dx dw nn
    M: int
    N: int
    K: int
    act_a: int = ACT_NONE
    act_b: int = ACT_NONE
    act_s: int = ACT_NONE          # with S
    beta: float = 1.0
    bias: bool = False
    S: bool = False
    gscale: Optional[float] = None  # A is a gradient: rows of magnitude 1e-3 .. 1 times gscale, scaled by its measured maximum
    accumulate: int = 0
    atomic: int = 0
    k_chunk: int = 0
    c0: bool = False               # a non-zero old C (accumulate / atomic / addend)
    pad_c: int = 0                 # ldc - N
    pad_s: int = 0                 # lds - N
    pad_a: int = 0                 # row stride of A minus its row length
    onehot: bool = False           # B selects columns of A (0 / 1)
    entry: str = "act"             # act (diner_train_gemm_act + _f16x3 (+ _w)) | std (diner_train_gemm) | panel | core
    seed: int = 0

    @property
    def splits(self):
        return 1 if self.k_chunk <= 0 else -(-self.K // self.k_chunk)

    def build(self):
        return _build(self)


def _spikes(x, rng, beta):
    """Softplus inputs on both sides of x * beta = 20 (and on it)"""
    flat = x.reshape(-1)
    vals = np.array([25.0, -25.0, 20.0, 19.9, 20.1, 30.0], F64) / beta
    pos = rng.choice(flat.size, size=min(flat.size // 2, 2 * len(vals)), replace=False)
    flat[pos] = np.resize(vals, pos.size).astype(F32)


@lru_cache(maxsize=None)
def _build(c):
    rng = np.random.default_rng(1000 + c.seed)
    M, N, K = c.M, c.N, c.K
    d = {}
    if c.gscale is not None:
        rowmag = 10.0 ** rng.integers(-3, 1, size=(K, 1) if c.form == "dw" else (M, 1))       # rows of the STORED gradient matrix
        g = rng.standard_normal((K, M) if c.form == "dw" else (M, K)) * rowmag * c.gscale
        A = (g.T if c.form == "dw" else g).astype(F32)
    else:
        A = (rng.standard_normal((M, K)) * 2.0).astype(F32)
    if c.onehot:
        sel = (7 * np.arange(N) + 3) % K
        sel[0], sel[-1] = K - 1, 0
        B = np.zeros((K, N), F32)
        B[sel, np.arange(N)] = 1.0
        d["sel"] = sel
    elif c.form == "dw":
        B = (rng.standard_normal((K, N)) * 2.0).astype(F32)                                   # an activation matrix
    else:
        B = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(F32)                            # a weight
    A = np.ascontiguousarray(A)
    if c.act_a == ACT_SOFTPLUS:
        _spikes(A, rng, c.beta)
    if c.act_b == ACT_SOFTPLUS and not c.onehot:
        _spikes(B, rng, c.beta)
    # the element the dropped-element mutant removes must reach C[m_small, 0]: keep it away from a ReLU's zero
    m_small = int(np.argmin(np.abs(A).max(axis=1)))
    if not c.onehot:
        A[m_small, K - 1] = abs(A[m_small, K - 1]) + F32(1e-3) * np.abs(A[m_small]).max()
        B[K - 1, 0] = abs(B[K - 1, 0]) + F32(1e-2)
    d.update(A=A, B=B, m_small=m_small)
    d["bias"] = rng.standard_normal(N).astype(F32) if c.bias else None
    if c.S:
        S = (rng.standard_normal((M, N)) * 2.0).astype(F32)
        if c.act_s == ACT_SOFTPLUS:
            _spikes(S, rng, c.beta)
        S[m_small, 0] = abs(S[m_small, 0]) + F32(0.5)
        d["S"] = S
    else:
        d["S"] = None
    scale_c = np.abs(A).max() * np.abs(B).max()
    d["C0"] = (rng.standard_normal((M, N)) * scale_c).astype(F32) if c.c0 else None
    # the scales of the f16x3 split (scale_of): 2^exp, or the power of two that maps max|A| into [2^13, 2^14)
    d["exp_a"], d["exp_b"] = EXP_ACT, (EXP_ACT if c.form == "dw" else EXP_W)
    if c.gscale is not None:
        amax = np.abs(A).max().astype(F32)
        d["exp_a"] = 0
        d["amax"] = amax
        d["scale_a"] = scale_from_amax(amax)
    else:
        d["amax"] = None
        d["scale_a"] = 2.0 ** d["exp_a"]
    d["scale_b"] = 2.0 ** d["exp_b"]
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def scale_from_amax(amax):
    """scale_of with a device word: e = 13 - exponent(max|x|), clamped to +-100 (0 for an all-zero operand)"""
    bits = int(np.asarray(amax, F32).view(np.uint32))
    e = 0 if bits == 0 else 13 - (((bits >> 23) & 0xFF) - 127)
    return 2.0 ** max(-100, min(100, e))


# ---- storage: how the logical operands lie in memory for each form -------------------------------------------------------------------
def stored(c, d):
    """-> dict(A=(buffer [rows, ld], sam, sak), B=(buffer, sbk, sbn)): buffers hold NaN in the padding columns"""
    ak, bnc = FORMS[c.form]
    A, B = d["A"], d["B"]

    def rows(mat, pad):
        buf = np.full((mat.shape[0], mat.shape[1] + pad), np.nan, F32)
        buf[:, :mat.shape[1]] = mat
        return buf
    if ak:
        ba = rows(A, c.pad_a)
        sa = (ba.shape[1], 1)
    else:
        ba = rows(A.T, c.pad_a)
        sa = (1, ba.shape[1])
    if bnc:
        bb = rows(B, 0)
        sb = (bb.shape[1], 1)
    else:
        bb = rows(B.T, 0)
        sb = (1, bb.shape[1])
    return dict(A=(ba, *sa), B=(bb, *sb))


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------
def epilogue64(c, d, acc, absacc):
    """(+ bias) * act_s'(S) (+ old C) on a float64 accumulation and on its sum of absolute terms -> ref, absr, factor"""
    f = dact(d["S"].astype(F64), c.act_s, c.beta) if d["S"] is not None else np.ones((c.M, c.N))
    if d["bias"] is not None:
        acc = acc + d["bias"].astype(F64)
        absacc = absacc + np.abs(d["bias"].astype(F64))
    ref, absr = acc * f, absacc * np.abs(f)
    if d["C0"] is not None:
        ref = ref + d["C0"].astype(F64)
        absr = absr + np.abs(d["C0"].astype(F64))
    return ref, absr, f


@lru_cache(maxsize=None)
def ref64(c):
    """-> ref, absr (float64 [M,N])"""
    d = c.build()
    a, b = act(d["A"].astype(F64), c.act_a, c.beta), act(d["B"].astype(F64), c.act_b, c.beta)
    ref, absr, _ = epilogue64(c, d, a @ b, np.abs(a) @ np.abs(b))
    return ref, absr


# ---- the two float32 CPU evaluations -------------------------------------------------------------------------------------------------
def epilogue32(c, d, acc_chunks, mutate=None):
    """the kernels' float32 epilogue on per-split float32 accumulations: bias where the split index is 0, the derivative, old C / atomics"""
    mutate = mutate or {}
    out = None if d["C0"] is None or mutate.get("ignore_c0") else d["C0"].copy()
    f = dact(d["S"], c.act_s, c.beta) if d["S"] is not None else None
    for z, acc in enumerate(acc_chunks):
        v = acc
        if d["bias"] is not None and (z == 0 or mutate.get("bias_per_split")):
            v = v + d["bias"]
        if f is not None:
            v = v * f
        out = v if out is None else out + v
    return out.astype(F32)


def chunks_of(c):
    kc = c.k_chunk if c.k_chunk > 0 else c.K
    return [(k, min(k + kc, c.K)) for k in range(0, c.K, kc)]


def operands32(c, d):
    return act(d["A"], c.act_a, c.beta).astype(F32), act(d["B"], c.act_b, c.beta).astype(F32)


def eval_matmul32(c, mutate=None):
    d = c.build()
    a, b = operands32(c, d)
    return epilogue32(c, d, [a[:, k0:k1] @ b[k0:k1] for k0, k1 in chunks_of(c)], mutate)


def eval_seq32(c, depth):
    """strictly k-sequential float32 accumulation, `depth` products at a time (each group summed exactly, rounded once, added)"""
    d = c.build()
    a, b = operands32(c, d)
    a64, b64 = a.astype(F64), b.astype(F64)
    accs = []
    for k0, k1 in chunks_of(c):
        acc = np.zeros((c.M, c.N), F32)
        for n0 in range(0, c.N, 128):            # column blocks: the running sum stays in cache over a long contraction
            blk, bb = np.zeros((c.M, min(128, c.N - n0)), F32), np.ascontiguousarray(b64[:, n0:n0 + 128])
            for k in range(k0, k1, depth):
                e = min(k + depth, k1)
                blk += (a64[:, k:e] @ bb[k:e]).astype(F32)
            acc[:, n0:n0 + 128] = blk
        accs.append(acc)
    return epilogue32(c, d, accs)


# ---- the f16x3 arithmetic ----------------------------------------------------------------------------------------------------------------
def split16(x32, scale):
    """float32 (activated) -> hi, lo as float64, still scaled: hi = fp16(t), lo = fp16(t - float(hi)), t = x * scale"""
    t = (x32 * F32(scale)).astype(F32)
    hi = t.astype(F16)
    lo = (t - hi.astype(F32)).astype(F16)
    return hi.astype(F64), lo.astype(F64)


@lru_cache(maxsize=2)                       # (the 8192-row cases' halves are 130 MB each)
def split_case(c):
    d = c.build()
    a, b = operands32(c, d)
    return split16(a, d["scale_a"]), split16(b, d["scale_b"])


def emulate_f16x3(c, passes=("hh", "hl", "lh")):
    """hi*hi + hi*lo + lo*hi in float64, unscaled, epilogue in float64 (everything lost BEFORE accumulation and nothing else)"""
    d = c.build()
    (ah, al), (bh, bl) = split_case(c)
    inv = 1.0 / (d["scale_a"] * d["scale_b"])
    acc = np.zeros((c.M, c.N))
    if "hh" in passes:
        acc += ah @ bh
    if "hl" in passes:
        acc += ah @ bl
    if "lh" in passes:
        acc += al @ bh
    return epilogue64(c, d, acc * inv, np.zeros((c.M, c.N)))[0]


def model_term(c):
    """|A - A^| @ |B| + |A^| @ |B - B^| + |A_lo| @ |B_lo| (before the epilogue factor)"""
    d = c.build()
    a, b = (x.astype(F64) for x in operands32(c, d))
    (ah, al), (bh, bl) = split_case(c)
    sa, sb = d["scale_a"], d["scale_b"]
    ahat, bhat = (ah + al) / sa, (bh + bl) / sb
    return np.abs(a - ahat) @ np.abs(b) + np.abs(ahat) @ np.abs(b - bhat) + (np.abs(al) @ np.abs(bl)) / (sa * sb)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cpu_side(c, precision):
    """-> (error of numpy's float32 matmul, error of the sequential float32 evaluation), each the case's max of |c32 - ref| / absr"""
    ref, absr = ref64(c)
    safe = np.where(absr > 0, absr, 1.0)
    return tuple(float((np.abs(e.astype(F64) - ref) / safe).max()) for e in (eval_matmul32(c), eval_seq32(c, DEPTH[precision])))


def cap(c):
    return (c.K + c.splits + 2) * U


def allowance(c, precision):
    return min(4.0 * max(cpu_side(c, precision)) + U, cap(c))


@lru_cache(maxsize=None)
def softplus_terms(c):
    """the Softplus allowances (see the module docstring), already times the epilogue factor; 0 without Softplus"""
    d = c.build()
    _, absr = ref64(c)
    out = np.zeros((c.M, c.N))
    if ACT_SOFTPLUS in (c.act_a, c.act_b):
        a64, b64 = act(d["A"].astype(F64), c.act_a, c.beta), act(d["B"].astype(F64), c.act_b, c.beta)
        a32, b32 = operands32(c, d)
        da = 4.0 * np.abs(a32.astype(F64) - a64) if c.act_a == ACT_SOFTPLUS else np.zeros_like(a64)
        db = 4.0 * np.abs(b32.astype(F64) - b64) if c.act_b == ACT_SOFTPLUS else np.zeros_like(b64)
        f = np.abs(dact(d["S"].astype(F64), c.act_s, c.beta)) if d["S"] is not None else 1.0
        out += (da @ np.abs(b64) + np.abs(a64) @ db) * f
    if c.act_s == ACT_SOFTPLUS and d["S"] is not None:
        f64, f32 = dact(d["S"].astype(F64), c.act_s, c.beta), dact(d["S"], c.act_s, c.beta).astype(F64)
        rel = float((np.abs(f32 - f64) / f64).max())
        out += (4.0 * rel + 2.0 * U) * absr
    return out


@lru_cache(maxsize=None)
def bound(c, precision):
    """per-element bound [M,N] of an fp32 ("fp32") or an f16x3 ("f16x3") kernel on this case"""
    d = c.build()
    _, absr = ref64(c)
    b = allowance(c, precision) * absr + softplus_terms(c)
    if precision == "f16x3":
        f = np.abs(dact(d["S"].astype(F64), c.act_s, c.beta)) if d["S"] is not None else 1.0
        b = b + model_term(c) * f
    return b


def worst(got, c, precision):
    """largest |got - ref| / bound over the elements (elements with a zero bound must be exact: inf otherwise)"""
    ref, _ = ref64(c)
    b = bound(c, precision)
    err = np.abs(np.asarray(got, F64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def worst_abs(got, c):
    """largest |got - ref| / absr (the unit the table speaks in)"""
    ref, absr = ref64(c)
    return float((np.abs(np.asarray(got, F64) - ref) / np.where(absr > 0, absr, 1.0)).max())


# ---- the case table ------------------------------------------------------------------------------------------------------------------
SP1, SP3 = (ACT_SOFTPLUS, 1.0), (ACT_SOFTPLUS, 3.0)
CODES = [(ACT_NONE, 1.0), (ACT_RELU, 1.0), SP1, SP3]
GSCALES = [1.0, 1e-12, 1e9]
# (M, N, K): k-contiguous contraction in {4, 32, 36, 68, 100, 1024} = 1, 1, 2, 3, 4, 32 k-steps of the f16x3 pipeline, four of them ragged;
# M in {4, 124, 128, 132, 1028}, N in {4, 124, 128, 132, 260}; 1028 x 260 = 9 row tiles x 3 column blocks (tile_of's mixed branch)
KC_SHAPES = [(4, 4, 4), (124, 132, 32), (128, 128, 36), (132, 124, 68), (4, 260, 100), (1028, 260, 36), (128, 4, 1024), (132, 132, 100)]
# dW: contraction over rows in {1, 31, 33, 255, 257, 1000}, k_chunk in {0, 32, 256}
DW_SHAPES = [(4, 4, 1, 0), (124, 132, 31, 32), (128, 128, 33, 32), (132, 124, 255, 256), (260, 128, 257, 256), (128, 260, 1000, 256),
             (132, 132, 1000, 32), (1028, 260, 33, 0), (4, 128, 257, 0)]


def _general_cases():
    out = []
    for i, (M, N, K) in enumerate(KC_SHAPES):
        ragged = K % 32 != 0
        # Softplus sits on the ragged-K cases (a padding staged as Softplus(0) shows only where BOTH operands carry it)
        ca, beta = (SP1 if i % 2 == 0 else SP3) if ragged else CODES[i % 2]
        out.append(GemmCase(f"fwd-{M}x{N}x{K}", "fwd", M, N, K, act_a=ca, act_b=ca if ragged and i % 4 == 0 else ACT_NONE, beta=beta,
                            bias=True, seed=10 + i))
        cs, beta = (SP3 if i % 2 == 0 else SP1) if ragged else CODES[(i + 1) % 2]
        out.append(GemmCase(f"dx-{M}x{N}x{K}", "dx", M, N, K, act_s=cs, beta=beta, S=True, gscale=GSCALES[i % 3], seed=30 + i))
        ca, beta = CODES[(i + 1) % 4]
        cb = ca if ragged and ca == ACT_SOFTPLUS else CODES[(i + 2) % 4][0] if CODES[(i + 2) % 4][1] == beta else ACT_RELU
        out.append(GemmCase(f"nn-{M}x{N}x{K}", "nn", M, N, K, act_a=ca, act_b=cb, beta=beta, bias=i % 2 == 0, seed=50 + i))
    for i, (M, N, K, kc) in enumerate(DW_SHAPES):
        cb, beta = CODES[(i + 1) % 4]
        out.append(GemmCase(f"dw-{M}x{N}x{K}-kc{kc}", "dw", M, N, K, act_b=cb, beta=beta, gscale=GSCALES[i % 3], atomic=1, k_chunk=kc,
                            seed=70 + i))
    # Softplus on both operands of a ragged dW contraction, and a k-contiguous B under a dX-like epilogue with an operand code on B
    out.append(GemmCase("dw-128x132x33-sp-both", "dw", 128, 132, 33, act_a=ACT_SOFTPLUS, act_b=ACT_SOFTPLUS, beta=1.0, atomic=1, k_chunk=32,
                        seed=90))
    out.append(GemmCase("dx-132x128x36-sp-both", "dx", 132, 128, 36, act_a=ACT_SOFTPLUS, act_b=ACT_SOFTPLUS, act_s=ACT_RELU, beta=3.0, S=True,
                        seed=91))
    return out


GENERAL_CASES = _general_cases()

# argument modes, one small shape each
MODE_CASES = [
    GemmCase("mode-bias-splitk", "dw", 132, 124, 100, bias=True, atomic=1, k_chunk=32, gscale=1.0, seed=100),
    GemmCase("mode-bias-splitk-kcontig", "fwd", 124, 132, 100, act_a=ACT_RELU, bias=True, atomic=1, k_chunk=32, seed=101),
    GemmCase("mode-accumulate", "fwd", 132, 124, 36, act_a=ACT_RELU, bias=True, accumulate=1, c0=True, seed=102),
    GemmCase("mode-accumulate-dx", "dx", 124, 132, 68, act_s=ACT_RELU, S=True, gscale=1.0, accumulate=1, c0=True, seed=103),
    GemmCase("mode-atomic-c0", "dw", 124, 132, 257, act_b=ACT_RELU, gscale=1e-12, atomic=1, k_chunk=256, c0=True, seed=104),
    GemmCase("mode-strides", "dx", 132, 124, 36, act_s=ACT_SOFTPLUS, beta=1.0, S=True, gscale=1e9, pad_c=8, pad_s=4, pad_a=4, seed=105),
    GemmCase("mode-strides-fwd", "fwd", 124, 132, 68, act_a=ACT_SOFTPLUS, beta=3.0, bias=True, pad_c=8, pad_a=4, seed=106),
]
ACT_CASES = GENERAL_CASES + MODE_CASES


def _onehot_cases():
    out = []
    shapes = {"fwd": [(4, 4, 4), (124, 132, 36), (132, 124, 100), (128, 128, 68), (1028, 260, 32)],
              "dx": [(4, 4, 4), (124, 260, 68), (132, 124, 36), (1028, 132, 100)],
              "nn": [(4, 4, 4), (124, 132, 100), (132, 260, 68), (1028, 124, 36)],
              "dw": [(4, 4, 1), (124, 132, 31), (132, 124, 33), (128, 260, 255), (260, 128, 257), (1028, 4, 1000)]}
    i = 0
    for form, ss in shapes.items():
        for (M, N, K) in ss:
            out.append(GemmCase(f"onehot-{form}-{M}x{N}x{K}", form, M, N, K, act_a=(ACT_NONE, ACT_RELU)[i % 2], onehot=True,
                                k_chunk=32 if form == "dw" and K > 32 else 0, atomic=int(form == "dw"), seed=200 + i))
            i += 1
    return out


ONEHOT_CASES = _onehot_cases()
ONEHOT_SOFTPLUS = [GemmCase(f"onehot-softplus-{form}", form, 132, 124, 36 if form != "dw" else 33, act_a=ACT_SOFTPLUS, beta=b, onehot=True,
                            atomic=int(form == "dw"), seed=230 + i) for i, (form, b) in enumerate([("fwd", 1.0), ("dx", 3.0), ("dw", 1.0), ("nn", 3.0)])]


# the standard entries at their fixed widths (relu flags = code ReLU; S = the ReLU mask)
def _std_cases():
    out = []
    for i, (M, K) in enumerate([(132, 56), (1028, 512)]):
        out.append(GemmCase(f"std-fwd-{M}x512x{K}", "fwd", M, 512, K, act_a=ACT_RELU, bias=True, accumulate=i, c0=bool(i), entry="std",
                            seed=300 + i))
    out.append(GemmCase("std-dx-132x512x512", "dx", 132, 512, 512, act_s=ACT_RELU, S=True, gscale=1e-12, entry="std", seed=303))
    out.append(GemmCase("std-dx-124x56x512", "dx", 124, 56, 512, gscale=1e9, entry="std", seed=304))
    out.append(GemmCase("std-dx-124x4x512-relu_a", "dx", 124, 4, 512, act_a=ACT_RELU, entry="std", seed=305))
    out.append(GemmCase("std-dw-512x56x1000", "dw", 512, 56, 1000, act_b=ACT_RELU, gscale=1.0, atomic=1, k_chunk=256, c0=True, entry="std",
                        seed=306))
    out.append(GemmCase("std-dw-4x512x257", "dw", 4, 512, 257, gscale=1e-12, atomic=1, k_chunk=32, entry="std", seed=307))
    out.append(GemmCase("std-nn-128x512x56", "nn", 128, 512, 56, act_a=ACT_RELU, act_b=ACT_RELU, bias=True, entry="std", seed=308))
    return out


STD_CASES = _std_cases()
# dw512_kernel: 512 x 512 over rows >= 8192 (launch_gemm's threshold; 8200: 51 chunks of 160 rows, one of 40, twelve empty), onto a
# non-zero dW, k_chunk as training.py passes it
DW512_CASES = [GemmCase(f"dw512-{rows}-relu{r}", "dw", 512, 512, rows, act_b=ACT_RELU if r else ACT_NONE, gscale=(1.0, 1e-12)[r],
                        atomic=1, k_chunk=4096, c0=True, entry="std", seed=320 + i)
               for i, (rows, r) in enumerate([(8192, 0), (8192, 1), (8200, 0), (8200, 1)])]

PANEL_M = [1, 63, 64, 65, 64 * 9 + 17]


def _panel_cases():
    out = []
    for i, M in enumerate(PANEL_M):
        K = (56, 512)[i % 2]
        # forward: relu(X) W^T + b + addend;  dX: addend + (dY W) * [S > 0]
        out.append(GemmCase(f"panel-fwd-{M}x512x{K}", "fwd", M, 512, K, act_a=ACT_RELU, bias=True, c0=i % 2 == 0, entry="panel", seed=400 + i))
        K = (512, 56)[i % 2]
        out.append(GemmCase(f"panel-dx-{M}x512x{K}", "fwd", M, 512, K, act_s=ACT_RELU, S=True, gscale=GSCALES[i % 3], c0=i % 2 == 1,
                            pad_c=8 * (i % 2), pad_s=4 * (i % 2), pad_a=4 * (i % 2), entry="panel", seed=410 + i))
    return out


def _core_cases():
    out = []
    for i, M in enumerate(PANEL_M):
        out.append(GemmCase(f"core-fwd-{M}", "fwd", M, 512, 512, act_a=ACT_RELU, bias=True, c0=i % 2 == 1, entry="core", seed=420 + i))
        out.append(GemmCase(f"core-dx-{M}", "fwd", M, 512, 512, act_s=ACT_RELU, S=True, gscale=GSCALES[i % 3], c0=i % 2 == 0,
                            pad_c=8 * (i % 2), pad_s=4 * (i % 2), pad_a=4 * (i % 2), entry="core", seed=430 + i))
    return out


PANEL_CASES, CORE_CASES = _panel_cases(), _core_cases()
ALL_CASES = ACT_CASES + STD_CASES + DW512_CASES + PANEL_CASES + CORE_CASES
assert len({c.id for c in ALL_CASES + ONEHOT_CASES + ONEHOT_SOFTPLUS}) == len(ALL_CASES + ONEHOT_CASES + ONEHOT_SOFTPLUS)


# ---- mutants: what a subtly wrong kernel would return, on the CPU --------------------------------------------------------------------
def mutant_drop_element(c, precision):
    """the last contraction element of the smallest-magnitude row dropped"""
    d = c.build()
    A = d["A"].copy()
    A[d["m_small"], c.K - 1] = 0
    return _evaluate(c, precision, {**d, "A": A})


def _evaluate(c, precision, d):
    """the case's float32 matmul evaluation / f16x3 emulation on modified operands"""
    a, b = act(d["A"], c.act_a, c.beta).astype(F32), act(d["B"], c.act_b, c.beta).astype(F32)
    if precision == "fp32":
        return epilogue32(c, d, [a[:, k0:k1] @ b[k0:k1] for k0, k1 in chunks_of(c)])
    (ah, al), (bh, bl) = split16(a, d["scale_a"]), split16(b, d["scale_b"])
    acc = (ah @ bh + ah @ bl + al @ bh) / (d["scale_a"] * d["scale_b"])
    return epilogue64(c, d, acc, np.zeros_like(acc))[0]


def mutant_softplus_padding(c, precision):
    """every k of the ragged last k-step staged as act(0) on both operands instead of 0"""
    d = c.build()
    pad = -c.K % TILE_K[precision]
    A = np.concatenate([d["A"], np.zeros((c.M, pad), F32)], axis=1)
    B = np.concatenate([d["B"], np.zeros((pad, c.N), F32)], axis=0)
    return _evaluate(replace(c, K=c.K + pad, k_chunk=0), precision, {**d, "A": A, "B": B})


def mutant_bias_per_split(c, precision):
    assert precision == "fp32"
    return eval_matmul32(c, {"bias_per_split": True})


def mutant_ignore_c0(c, precision):
    assert precision == "fp32"
    return eval_matmul32(c, {"ignore_c0": True})


def mutant_rows_exchanged(c, precision):
    """rows 1 and 4 of the first 16-row block exchanged (slot16(1) = 4): the permutation of a transposing store not undone"""
    out = np.array(eval_matmul32(c) if precision == "fp32" else emulate_f16x3(c))
    r = 4 if c.M > 4 else c.M - 1
    out[[1, r]] = out[[r, 1]]
    return out


def mutant_step_twice(c, precision):
    """the last k-step multiplied twice"""
    d = c.build()
    k0 = (c.K - 1) // TILE_K[precision] * TILE_K[precision]
    A = np.concatenate([d["A"], d["A"][:, k0:]], axis=1)
    B = np.concatenate([d["B"], d["B"][k0:]], axis=0)
    return _evaluate(replace(c, K=A.shape[1], k_chunk=0), precision, {**d, "A": A, "B": B})


def mutant_pass_dropped(c, which):
    return emulate_f16x3(c, passes=tuple(p for p in ("hh", "hl", "lh") if p != which))


# ---- refused calls: (entry, overrides of the valid base call, a piece of the error text) ---------------------------------------------------
_STRIDES = [(dict(N=62), "N % 4"), (dict(k_chunk=48), "k_chunk"), (dict(sak=2, sam=2), "contiguous"), (dict(sbn=2, sbk=2), "contiguous"),
            (dict(K=62), "multiples of 4"), (dict(sam=66), "multiples of 4"), (dict(sam=1, sak=64, M=6), "multiples of 4"),
            (dict(sam=1, sak=66), "multiples of 4"), (dict(sbn=1, sbk=66), "multiples of 4"), (dict(sbk=1, sbn=66), "multiples of 4"),
            (dict(A=None), "NULL")]
_CODES = [(dict(act_a=3), "activation"), (dict(act_b=-1), "activation"), (dict(act_s=7), "activation"), (dict(act_a=2, beta=0.0), "beta"),
          (dict(act_s=2, beta=-1.0), "beta"), (dict(act_b=2, beta=float("nan")), "beta")]
REFUSALS = ([("act", kw, what) for kw, what in _STRIDES + _CODES] + [("f16x3", kw, what) for kw, what in _STRIDES + _CODES]
            + [("f16x3", dict(k_chunk=32), "atomic")]
            + [(e, kw, what) for e in ("std_fp32", "std_f16x3") for kw, what in _STRIDES] + [("std_fp32", dict(precision=7), "precision")])


def refusal_call(lib, entry, ptr, stream, **kw):
    """the entry's call on an 8 x 64 x 64 forward product whose pointers are all `ptr`, with overrides"""
    a = dict(A=ptr, B=ptr, bias=None, S=None, C=ptr, M=8, N=64, K=64, sam=64, sak=1, sbk=1, sbn=64, ldc=64, lds=0, act_a=0, act_b=0, act_s=0,
             beta=1.0, accumulate=0, atomic=0, k_chunk=0, precision={"std_f16x3": 1}.get(entry, 0))
    a.update(kw)
    g = lambda *names: [a[n] for n in names]
    head = g("A", "B", "bias", "S", "C", "M", "N", "K", "sam", "sak", "sbk", "sbn", "ldc", "lds")
    if entry == "act":
        return lib.diner_train_gemm_act(*head, *g("act_a", "act_b", "act_s", "beta", "accumulate", "atomic", "k_chunk"), stream)
    if entry == "f16x3":
        return lib.diner_train_gemm_act_f16x3(*head, *g("act_a", "act_b", "act_s", "beta", "accumulate", "atomic", "k_chunk"), None, None,
                                              EXP_ACT, EXP_W, stream)
    return lib.diner_train_gemm(*head, *g("act_a", "act_b", "accumulate", "atomic", "k_chunk", "precision"), None, None, EXP_ACT, EXP_W, stream)
