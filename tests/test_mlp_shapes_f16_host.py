"""Host-side checks of the shape-general f16x3 inference path (no GPU): the C ABI's *_gen_f16 entry points and their envelope, and the
renderer's choice of route (``f16x3_any_shape`` x precision x standard / non-standard model x grad mode) on stub models, without
launching anything."""
import ctypes as C
import re
import warnings
from pathlib import Path

import pytest
import torch

from tests.test_mlp_shapes_host import _shape, _stub

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["diner_mlp_gen_f16_packed_floats", "diner_pack_mlp_gen_f16", "diner_render_points_gen_f16", "diner_render_gen_f16",
               "diner_render_image_gen_f16", "diner_render_points_gen_f16_ix", "diner_render_gen_f16_ix", "diner_render_image_gen_f16_ix"]


def test_new_symbols_are_declared_and_exported():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        # the argument list of the fp32 twin
        twin = name.replace("_gen_f16", "_gen")
        assert _lib.SYMBOLS[name][0] is _lib.SYMBOLS[twin][0] and _lib.SYMBOLS[name][1] == _lib.SYMBOLS[twin][1], name
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # new entry points only: the ABI version stays


def test_packed_size_follows_the_shape():
    from diner_amd import _lib
    lib = _lib.lib()
    # case (a), d_hidden 128, d_in 55, d_latent 512: 1024 halfs per (feature tile, k-block of 16): lin_in 4 tiles x 4 k-blocks, 3 lin_z
    # 4 x 32, 10 block layers 4 x 8; then fp32: biases 14 x 128 + 32, lin_out 4 x 128
    want = 1024 * (4 * 4 + 3 * 4 * 32 + 10 * 4 * 8) // 2 + 14 * 128 + 32 + 4 * 128
    assert lib.diner_mlp_gen_f16_packed_floats(C.byref(_shape())) == want
    # d_latent 24 and d_in 87 (num_freqs 10) pad their last k-block; no lin_z layer beyond combine_layer
    sh = _shape(d_latent=24, d_in=87, num_freqs=10, d_hidden=64, n_blocks=2, combine_layer=1)
    want = 1024 * (2 * 6 + 1 * 2 * 2 + 4 * 2 * 4) // 2 + (1 + 1 + 4) * 64 + 32 + 4 * 64
    assert lib.diner_mlp_gen_f16_packed_floats(C.byref(sh)) == want


@pytest.mark.parametrize("kw, what", [
    (dict(d_hidden=48), "d_hidden=48"), (dict(d_hidden=544), "d_hidden=544"), (dict(combine_type=1), "combine_type"),
    (dict(d_out=5), "d_out=5"), (dict(d_latent=12), "d_latent=12"), (dict(d_latent=1032), "d_latent=1032"),
    (dict(n_blocks=0), "n_blocks=0"), (dict(combine_layer=-1), "combine_layer=-1"), (dict(num_freqs=0, d_in=7), "num_freqs=0"),
    (dict(d_in=56), "d_in=56"), (dict(beta=-1.0), "beta"),
])
def test_out_of_envelope_shapes_are_unsupported_with_a_reason(kw, what):
    from diner_amd import _lib
    lib = _lib.lib()
    sh = _shape(**kw)
    assert lib.diner_mlp_gen_f16_packed_floats(C.byref(sh)) == -3          # DINER_E_UNSUPPORTED
    assert what in lib.diner_last_error().decode()
    with pytest.raises(NotImplementedError, match=re.escape(what)):
        _lib.check(lib.diner_render_points_gen_f16(None, C.byref(sh), None, None, None, 0, 1, None, None), "diner_render_points_gen_f16")


def test_null_arguments_are_invalid_not_a_crash():
    from diner_amd import _lib
    lib = _lib.lib()
    assert lib.diner_mlp_gen_f16_packed_floats(None) == -1
    assert lib.diner_pack_mlp_gen_f16(C.byref(_shape()), None, None, None) == -1
    assert lib.diner_render_points_gen_f16(None, None, None, None, None, 0, 1, None, None) == -1
    assert "shape is NULL" in lib.diner_last_error().decode()


# ---- route selection ------------------------------------------------------------------------------------------------------------
NONSTD = dict(d_hidden=64, n_blocks=2, combine_layer=1, beta=10.0)


def _renderer(switch, precision):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(f16x3_any_shape=switch)
    r.precision = precision
    return r


def test_the_switch_is_a_constructor_keyword_and_a_plain_attribute():
    from diner_amd import NeRFRendererDGS
    assert NeRFRendererDGS().f16x3_any_shape is False
    assert NeRFRendererDGS(f16x3_any_shape=True).f16x3_any_shape is True
    assert NeRFRendererDGS(n_samples=8, f16x3_any_shape=1).f16x3_any_shape is True
    r = NeRFRendererDGS()
    r.f16x3_any_shape = True
    assert r._use_gen_f16(NeRFRendererDGS._validate_model(_stub(NONSTD)))
    assert r.memory_report()["cached"]["mlp_gen_f16_packed"] == 0


def test_switch_on_non_standard_f16x3_takes_the_f16_route_without_a_warning():
    r = _renderer(True, "f16x3")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        shape = r._route(_stub(NONSTD))
    assert r._use_gen(shape) and r._use_gen_f16(shape)
    assert r.effective_precision == "f16x3" and r.precision == "f16x3"
    fn, name = r._gen_entry("render_points_gen_ix", True)
    assert name == "diner_render_points_gen_f16_ix" and fn is not None
    assert r._gen_entry("mlp_gen_packed_floats", True)[1] == "diner_mlp_gen_f16_packed_floats"
    assert r._gen_entry("render_image_gen", False)[1] == "diner_render_image_gen"


def test_switch_on_precision_fp32_keeps_the_fp32_route():
    r = _renderer(True, "fp32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        shape = r._route(_stub(NONSTD))
    assert r._use_gen(shape) and not r._use_gen_f16(shape) and r.effective_precision == "fp32"


def test_switch_off_warns_and_runs_fp32_as_before():
    r = _renderer(False, "f16x3")
    with pytest.warns(UserWarning, match="fp32"):
        shape = r._route(_stub(NONSTD))
    assert r._use_gen(shape) and not r._use_gen_f16(shape) and r.effective_precision == "fp32"


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_the_standard_model_keeps_its_kernels(switch, precision):
    r = _renderer(switch, precision)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        shape = r._route(_stub({}))
    assert shape.standard and not r._use_gen(shape) and not r._use_gen_f16(shape) and r.effective_precision == precision


def test_an_autograd_frame_is_not_sent_to_the_f16_route():
    """render_image's launch under autograd (``saved``) settles for the training path's exact fp32 and says so"""
    r = _renderer(True, "f16x3")
    with pytest.warns(UserWarning, match="fp32"):
        r._route(_stub(NONSTD), f16_ok=False)
    assert r.effective_precision == "fp32"


def test_training_stays_exact_fp32_and_says_so():
    """with both switches on, a model whose parameters require grad goes to the fp32 training path (which would warn and set
    effective_precision 'fp32'); without train_any_shape it raises as before -- decided before any launch"""
    from diner_amd import NeRFRendererDGS
    m = _stub(dict(d_hidden=64, n_blocks=2, combine_layer=1))
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1, f16x3_any_shape=True)
    shape = NeRFRendererDGS._validate_model(m)
    assert r._wants_grad(m, None) and not r._use_gen_train(shape)
    with pytest.raises(NotImplementedError, match="inference"):
        r(m, torch.zeros(1, 4, 8))
    r.train_any_shape = True
    assert r._use_gen_train(shape)
    with pytest.warns(UserWarning, match="fp32"):
        r._settle_fp32(shape)
    assert r.effective_precision == "fp32"
    with torch.no_grad():
        assert not r._wants_grad(m, None) and r._use_gen_f16(shape)     # the same model under no_grad is inference again
