"""Host-side checks (no GPU) of the shape-general f16x3 training path: the renderer's third switch and its routing predicate, the new C
entry points (declared, exported, bound) and their argument validation, which returns codes before any launch."""
import ctypes as C
import itertools
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ("diner_train_gemm_act_f16x3", "diner_train_gemm_act_f16x3_w", "diner_train_split_weight", "diner_train_split_weight_halfs")
D = 64  # a non-NULL, 16-byte aligned dummy pointer, never dereferenced


def test_constructor_accepts_the_switch_and_keeps_it_a_plain_attribute():
    from diner_amd import NeRFRendererDGS
    assert NeRFRendererDGS().train_f16x3_any_shape is False
    r = NeRFRendererDGS(train_any_shape=True, train_f16x3_any_shape=True)
    assert r.train_f16x3_any_shape is True and r.train_any_shape is True and r.f16x3_any_shape is False
    r.train_f16x3_any_shape = False
    assert "train_f16x3_any_shape" in vars(r)


@pytest.mark.parametrize("standard", [True, False])
def test_routing_predicate_in_all_switch_and_precision_combinations(standard):
    from diner_amd import NeRFRendererDGS
    from diner_amd.renderer import STANDARD_SHAPE, MlpShape
    shape = STANDARD_SHAPE if standard else MlpShape(55, 256, 64, 2, 1, 6, 50.0)
    assert shape.standard == standard
    for any_shape, f16_switch, prec in itertools.product((False, True), (False, True), ("fp32", "f16x3")):
        r = NeRFRendererDGS(train_any_shape=any_shape, train_f16x3_any_shape=f16_switch)
        r.precision = prec
        want = (not standard) and any_shape and f16_switch and prec == "f16x3"
        assert r._use_gen_train_f16(shape) == want, (standard, any_shape, f16_switch, prec)
        assert r._use_gen_train(shape) == ((not standard) and any_shape)       # the fp32 switch's own predicate is what it was
        r._force_gen_train = True                                              # test-only: the standard shape on the path as well
        assert r._use_gen_train_f16(shape) == (f16_switch and prec == "f16x3")


def test_inference_switch_does_not_send_training_to_f16x3():
    from diner_amd import NeRFRendererDGS
    from diner_amd.renderer import MlpShape
    r = NeRFRendererDGS(train_any_shape=True, f16x3_any_shape=True)
    assert not r._use_gen_train_f16(MlpShape(55, 256, 64, 2, 1, 6, 50.0))


def test_new_symbols_are_declared_exported_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # new entry points only: the ABI version stays


def test_split_weight_sizes():
    from diner_amd import _lib
    lib = _lib.lib()
    assert lib.diner_train_split_weight_halfs(96, 40) == 128 * 64
    assert lib.diner_train_split_weight_halfs(512, 512) == 512 * 512
    assert lib.diner_train_split_weight_halfs(4, 128) == 128 * 128
    assert lib.diner_train_split_weight_halfs(0, 128) == 0


def _gemm(lib, **kw):
    a = dict(A=D, B=D, bias=None, S=None, C=D, M=0, N=128, K=128, sam=128, sak=1, sbk=1, sbn=128, ldc=128, lds=0, act_a=0, act_b=0, act_s=0,
             beta=1.0, accumulate=0, atomic=0, k_chunk=0, amax_a=None, amax_b=None, exp_a=-4, exp_b=4)
    a.update(kw)
    return lib.diner_train_gemm_act_f16x3(a["A"], a["B"], a["bias"], a["S"], a["C"], a["M"], a["N"], a["K"], a["sam"], a["sak"], a["sbk"],
                                          a["sbn"], a["ldc"], a["lds"], a["act_a"], a["act_b"], a["act_s"], a["beta"], a["accumulate"],
                                          a["atomic"], a["k_chunk"], a["amax_a"], a["amax_b"], a["exp_a"], a["exp_b"], None)


def test_gemm_accepts_valid_arguments_without_work():
    from diner_amd import _lib
    assert _gemm(_lib.lib()) == 0          # M == 0: validated, nothing launched
    assert _gemm(_lib.lib(), k_chunk=64, atomic=1) == 0 and _gemm(_lib.lib(), k_chunk=128) == 0      # split-K with atomics; one chunk


@pytest.mark.parametrize("kw,what", [(dict(A=None), b"NULL"), (dict(act_a=3), b"activation"), (dict(act_s=2, beta=0.0), b"beta"),
                                      (dict(N=6), b"size"), (dict(k_chunk=48), b"size"), (dict(k_chunk=64), b"atomic"), (dict(sam=3, sak=5), b"contiguous"),
                                      (dict(sbk=2, sbn=2), b"contiguous"), (dict(K=126), b"multiples of 4"), (dict(A=68), b"aligned"),
                                      (dict(exp_a=61), b"exponent")])
def test_gemm_rejects_bad_arguments(kw, what):
    from diner_amd import _lib
    lib = _lib.lib()
    assert _gemm(lib, **kw) == -1
    assert what in lib.diner_last_error()


def test_pre_split_entry_points_reject_bad_arguments():
    from diner_amd import _lib
    lib = _lib.lib()
    w = lambda **kw: lib.diner_train_gemm_act_f16x3_w(*[{**dict(A=D, sam=128, Bhi=D, Blo=D, bias=None, S=None, lds=0, C=D, ldc=128, M=0, N=128, K=128,
                                                                 act_a=0, act_s=0, beta=1.0, accumulate=0, amax_a=None, exp_a=-4, exp_b=4,
                                                                 stream=None), **kw}[k]
                                                        for k in ("A", "sam", "Bhi", "Blo", "bias", "S", "lds", "C", "ldc", "M", "N", "K", "act_a",
                                                                  "act_s", "beta", "accumulate", "amax_a", "exp_a", "exp_b", "stream")])
    assert w() == 0
    for kw, what in ((dict(Blo=None), b"NULL"), (dict(act_a=7), b"activation"), (dict(act_a=2, beta=float("inf")), b"beta"),
                     (dict(K=130), b"size"), (dict(Bhi=72), b"aligned"), (dict(exp_b=-61), b"exponent")):
        assert w(**kw) == -1
        assert what in lib.diner_last_error(), kw
    s = lib.diner_train_split_weight
    assert s(None, 128, 128, 128, 0, 4, D, D, None) == -1
    assert s(D, 128, 128, 64, 0, 4, D, D, None) == -1 and b"ld" in lib.diner_last_error()
    assert s(D, 128, 128, 128, 0, 99, D, D, None) == -1 and b"exponent" in lib.diner_last_error()
    assert s(D, 128, 128, 128, 0, 4, D, 8, None) == -1 and b"aligned" in lib.diner_last_error()
    with pytest.raises(ValueError):
        _lib.check(_gemm(lib, A=None), "diner_train_gemm_act_f16x3")
