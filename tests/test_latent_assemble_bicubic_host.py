"""The bicubic latent assembly (diner_assemble_latent_bicubic / _backward, glue.assemble_latent_bicubic) as far as it goes without a GPU:
the two entry points are declared, exported and bound; every invalid argument comes back as its error code with a message that starts with
"assemble_latent_bicubic", before any launch; the Python side's checks; and the proof of the numpy restatement the GPU tests use
(tests/latent_bicubic_ref.py) against CPU torch, on every case of tests/test_gpu_latent_assemble_bicubic.py:

* torch's fp32 F.interpolate(mode="bicubic", align_corners=True) lies within the forward bound (C_F * 2^-23 * max|level|, derived in
  latent_bicubic_ref.py) of the float64 restatement, and a same-size level is bit-equal;
* align_corners=False, mode="bilinear" and the restatement with A = -0.5 each lie OUTSIDE that bound wherever a level is resampled and has
  more than one texel: the comparison rejects a wrong implementation;
* the float64 autograd gradient of torch's bicubic lies within 1e-5 of the largest element of Wy^T d Wx (the gap is fp32 against double
  tap placement: torch's float64 kernel places its taps in double);
* the kernels' arithmetic restated in fp32, operation by operation (factored coefficients in fp32, the adjoint's sum in the kernel's
  order), lies within the forward and the backward bound of the float64 restatement: the bounds are ones that arithmetic meets."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import latent_bicubic_ref as R

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("diner_assemble_latent_bicubic", "diner_assemble_latent_bicubic_backward")
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
    rc = lib.diner_assemble_latent_bicubic(lv, n, N, h, w, other, None)
    out.append((rc, lib.diner_last_error().decode()))
    rc = lib.diner_assemble_latent_bicubic_backward(other, n, N, h, w, lv, None)
    out.append((rc, lib.diner_last_error().decode()))
    return out


def test_symbols_are_declared_exported_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "image_encoder.py:262-272" in header and 'mode="bicubic", align_corners=True' in header
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # additions only


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
    (dict(specs=GOOD, N=65536), UNSUPPORTED, "65535"),
])
def test_invalid_arguments_return_their_code_before_any_launch(kw, code, word):
    for rc, msg in _both(**kw):
        assert rc == code, (rc, msg)
        assert word in msg, msg
        assert msg.startswith("assemble_latent_bicubic"), msg


def test_error_codes_raise_through_check():
    from diner_amd import _lib
    lib = _lib.lib()
    with pytest.raises(ValueError, match="assemble_latent_bicubic: n_levels"):
        _lib.check(lib.diner_assemble_latent_bicubic(C.byref(_levels(GOOD)), 9, 2, 4, 4, PTR, None), "diner_assemble_latent_bicubic")
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        _lib.check(lib.diner_assemble_latent_bicubic_backward(PTR, 1, 2, 4, 4, C.byref(_levels([(PTR, 20, 4, 4)])), None),
                   "diner_assemble_latent_bicubic_backward")


def test_python_side_checks():
    from diner_amd import glue
    lv = [torch.zeros(2, 8, 4, 4)]
    with pytest.raises(NotImplementedError, match="'bicubic'"):      # the bilinear function keeps refusing the mode
        glue.assemble_latent(lv, 1, 2, mode="bicubic")
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.assemble_latent_bicubic(lv, 1, 2)
    with pytest.raises(ValueError, match="levels"):
        glue.assemble_latent_bicubic([], 1, 2)


def test_encode_keeps_refusing_other_modes_before_any_device_work():
    from types import SimpleNamespace as NS

    from diner_amd import glue
    for mode in ("nearest", "nearest ", "area", "bilinear "):
        with pytest.raises(NotImplementedError, match=repr(mode)):
            glue.encode(NS(encoder=NS(upsample_interp=mode)), *[None] * 5)


# ---- the restatement against CPU torch ------------------------------------------------------------------------------------------------
def test_weights_at_the_grid_points_are_exact():
    """t = 0 gives (0, 1, 0, 0) exactly in fp32: an identity resample is the identity matrix, bit for bit"""
    for n in (1, 2, 5, 13):
        for factored in (False, True):
            assert np.array_equal(R.weights_1d(n, n, np.float32, factored=factored), np.eye(n, dtype=np.float32))
    assert np.array_equal(R.weights_1d(3, 1), [[1, 0, 0]]) and np.array_equal(R.weights_1d(1, 4), np.ones((4, 1)))


def _upcat(levels, size, **kw):
    return torch.cat([F.interpolate(t, size=size, **kw) for t in levels], 1)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_forward_against_torch(name):
    r = R.ref(name)
    assert R.C_F <= 64
    lv = [t.numpy() for t in r.levels]
    wrong = {"align_corners=False": _upcat(r.levels, r.size, mode="bicubic", align_corners=False).double(),
             "bilinear": _upcat(r.levels, r.size, mode="bilinear", align_corners=True).double(),
             "A=-0.5": torch.from_numpy(R.upcat_bicubic(lv, r.size, A=-0.5))}
    own32 = torch.from_numpy(R.upcat_bicubic(lv, r.size, dtype=np.float32, factored=True)).double()     # the kernels' coefficients, in fp32
    off = 0
    for t, spec in zip(r.levels, r.specs):
        c = spec[0]
        sl = slice(off, off + c)
        bound = R.C_F * R.ULP * float(t.abs().max())
        err = float((r.out[:, sl].double() - r.out64[:, sl]).abs().max())
        err32 = float((own32[:, sl] - r.out64[:, sl]).abs().max())
        print(f"{name} level {spec}: torch fp32 - float64 restatement: {err / (R.ULP * float(t.abs().max())):.2f} units "
              f"(fp32 restatement: {err32 / (R.ULP * float(t.abs().max())):.2f}), c_f = {R.C_F:.2f}")
        assert err <= bound and err32 <= bound, (name, spec, err, err32, bound)
        if spec[1:] == tuple(r.size):
            assert torch.equal(r.out[:, sl], t), "torch's identity resample is bit-equal"
            assert torch.equal(own32[:, sl].float(), t)
        if r.resampled(spec):
            for what, other in wrong.items():
                # (an output of 1 x 1 is the level's corner texel, t = 0, in every align_corners=True variant: only the
                # align_corners=False one, which reads the level's centre, can differ there)
                if tuple(r.size) != (1, 1) or what == "align_corners=False":
                    assert float((other[:, sl] - r.out64[:, sl]).abs().max()) > bound, (name, spec, what)
        off += c


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_backward_against_torch_autograd(name):
    r = R.ref(name)
    lv64 = [t.double().requires_grad_(True) for t in r.levels]
    grads = torch.autograd.grad(_upcat(lv64, r.size, mode="bicubic", align_corners=True), lv64, r.d_out.double())
    for g, want, spec in zip(grads, r.grads, r.specs):
        err, scale = float((g - want).abs().max()), float(want.abs().max())
        print(f"{name} level {spec}: float64 autograd - Wy^T d Wx: {err:.3e} on a scale of {scale:.3e}")
        assert err <= 1e-5 * scale, (name, spec, err, scale)


def _adjoint_fp32_in_kernel_order(d_out, spec, off, size):
    """assemble_latent_bc_bwd_kernel in numpy fp32: acc = acc + (wy * wx) * d over the fine rows (outside) and columns (inside), ascending;
    a term whose weight is 0 adds an exact 0, so walking every fine pixel gives the kernel's sum"""
    c, hl, wl = spec
    Wy, Wx = R.weights_1d(hl, size[0], np.float32, factored=True), R.weights_1d(wl, size[1], np.float32, factored=True)
    d = d_out[:, off:off + c]
    acc = np.zeros((d.shape[0], c, hl, wl), dtype=np.float32)
    for y in range(size[0]):
        for x in range(size[1]):
            wgt = Wy[y][:, None] * Wx[x][None, :]
            acc = acc + wgt[None, None] * d[:, :, y, x][:, :, None, None]
    return acc


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_bound_holds_for_the_stated_arithmetic(name):
    r = R.ref(name)
    assert R.C_B <= 16
    off = 0
    for want, A, n, spec in zip(r.grads, r.A, r.n, r.specs):
        got = _adjoint_fp32_in_kernel_order(r.d_out.numpy(), spec, off, r.size)
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want.numpy())
        bound = (n + R.C_B) * R.ULP * A.numpy()
        print(f"{name} level {spec}: n = {n}, max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (name, spec)
        if spec[1:] == tuple(r.size):
            assert np.array_equal(got, r.d_out.numpy()[:, off:off + spec[0]])
        off += spec[0]
