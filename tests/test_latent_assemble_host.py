"""The latent assembly (diner_assemble_latent / _backward, glue.assemble_latent) as far as it goes without a GPU: the two entry points are
declared, exported and bound; every invalid argument comes back as its error code with a message before any launch; the layout predicate
and the mode check of the Python side."""
import ctypes as C
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("diner_assemble_latent", "diner_assemble_latent_backward")
INVALID, UNSUPPORTED = -1, -3
PTR = 4096    # a non-NULL dummy device pointer: never dereferenced, every call below is refused before a launch


def _levels(specs):
    from diner_amd import _lib
    lv = _lib.DinerLatentLevels()
    for i, (ptr, c, h, w) in enumerate(specs):
        lv.level[i].data, lv.level[i].C, lv.level[i].h, lv.level[i].w = ptr, c, h, w
    return lv


def _both(specs, n_levels=None, N=2, h=4, w=4, levels_null=False, other=PTR):
    """(rc, message) of the forward and of the backward entry point for the same arguments"""
    from diner_amd import _lib
    lib = _lib.lib()
    lv = None if levels_null else C.byref(_levels(specs))
    n = len(specs) if n_levels is None else n_levels
    out = []
    rc = lib.diner_assemble_latent(lv, n, N, h, w, other, None)
    out.append((rc, lib.diner_last_error().decode()))
    rc = lib.diner_assemble_latent_backward(other, n, N, h, w, lv, None)
    out.append((rc, lib.diner_last_error().decode()))
    return out


def test_symbols_are_declared_exported_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "image_encoder.py:262-272" in header
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # additions only
    assert _lib.LATENT_MAX_LEVELS == 5 and C.sizeof(_lib.DinerLatentLevel) == 24 and C.sizeof(_lib.DinerLatentLevels) == 120


GOOD = [(PTR, 8, 4, 4), (PTR, 16, 2, 2)]


@pytest.mark.parametrize("kw, code, word", [
    (dict(specs=GOOD, levels_null=True), INVALID, "NULL"),
    (dict(specs=GOOD, other=None), INVALID, "NULL"),                               # out_nhwc / d_out_nhwc
    (dict(specs=[(PTR, 8, 4, 4), (None, 16, 2, 2)]), INVALID, "NULL"),             # a level's data
    (dict(specs=GOOD, n_levels=0), INVALID, "n_levels"),
    (dict(specs=GOOD, n_levels=6), INVALID, "n_levels"),
    (dict(specs=GOOD, n_levels=-1), INVALID, "n_levels"),
    (dict(specs=GOOD, N=0), INVALID, "non-positive"),
    (dict(specs=GOOD, N=-3), INVALID, "non-positive"),
    (dict(specs=GOOD, h=0), INVALID, "non-positive"),
    (dict(specs=GOOD, w=-1), INVALID, "non-positive"),
    (dict(specs=[(PTR, 8, 4, 4), (PTR, 16, 0, 2)]), INVALID, "non-positive"),
    (dict(specs=[(PTR, 8, 4, 4), (PTR, 16, 2, -2)]), INVALID, "non-positive"),
    (dict(specs=[(PTR, 0, 4, 4)]), INVALID, "non-positive"),
    (dict(specs=[(PTR, 8, 4, 4), (PTR, 12, 2, 2)]), UNSUPPORTED, "multiple of 8"),  # a level's C not a multiple of 8
    (dict(specs=[(PTR, 4, 4, 4)]), UNSUPPORTED, "multiple of 8"),
    (dict(specs=[(PTR, 512, 4, 4), (PTR, 512, 2, 2), (PTR, 8, 1, 1)]), UNSUPPORTED, "C=1032"),   # the sum beyond 1024
    (dict(specs=[(PTR, 1032, 4, 4)]), UNSUPPORTED, "1032"),
])
def test_invalid_arguments_return_their_code_before_any_launch(kw, code, word):
    for rc, msg in _both(**kw):
        assert rc == code, (rc, msg)
        assert word in msg, msg
        assert msg.startswith("assemble_latent"), msg


def test_error_codes_raise_through_check():
    from diner_amd import _lib
    lib = _lib.lib()
    with pytest.raises(ValueError, match="n_levels"):
        _lib.check(lib.diner_assemble_latent(C.byref(_levels(GOOD)), 9, 2, 4, 4, PTR, None), "diner_assemble_latent")
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        _lib.check(lib.diner_assemble_latent_backward(PTR, 1, 2, 4, 4, C.byref(_levels([(PTR, 20, 4, 4)])), None),
                   "diner_assemble_latent_backward")


def test_layout_predicate():
    """latent_is_packed = the NHWC-strided fp32 layout AND a CUDA tensor; without a GPU the layout half is what can be shown (the CUDA
    half: tests/test_gpu_latent_assemble.py)"""
    from diner_amd import glue
    buf = torch.zeros(2, 3, 5, 7, 16)                       # [SB, NV, h, w, C]
    packed, nchw = buf.permute(0, 1, 4, 2, 3), torch.zeros(2, 3, 16, 5, 7)
    assert packed.shape == nchw.shape
    assert glue.nhwc_strided(packed) and not glue.nhwc_strided(nchw)
    assert not glue.nhwc_strided(packed.double()) and not glue.nhwc_strided(packed.contiguous())
    assert not glue.nhwc_strided(buf[..., :8].permute(0, 1, 4, 2, 3))     # a channel slice of a wider buffer is not one contiguous pack
    assert not glue.nhwc_strided(packed[0]) and not glue.nhwc_strided(None)
    assert not glue.latent_is_packed(nchw)
    assert glue.latent_is_packed(packed) == packed.is_cuda     # (a CPU tensor is never "packed": the kernels read device memory)


def test_mode_check_raises_naming_the_mode():
    from diner_amd import glue
    lv = [torch.zeros(2, 8, 4, 4)]
    for mode in ("nearest", "bicubic", "nearest "):
        with pytest.raises(NotImplementedError, match=repr(mode)):
            glue.assemble_latent(lv, 1, 2, mode=mode)
    with pytest.raises(RuntimeError, match="GPU only"):        # the default mode passes the check and goes on to the device test
        glue.assemble_latent(lv, 1, 2)
    with pytest.raises(ValueError, match="levels"):
        glue.assemble_latent([], 1, 2)
