"""conv1's input (diner_encoder_input / _backward, glue.encoder_input, glue.encode) as far as it goes without a GPU: the torch
restatement of tests/encoder_input_ref.py reproduces the reference's captured conv1 input (tests/golden/encoder_input_*.npz, written by
tools/gen_encoder_input_golden.py) -- image channels bit for bit, the encoding within tol_pe -- and the same comparison rejects four
deliberately broken forms; the adjoint restatement equals float64 autograd through the forward restatement; the two entry points are
declared, exported and bound with the header's argument counts, and refuse bad arguments before any launch."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import encoder_input_ref as R

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NAMES = ("encoder_input_p4_f4", "encoder_input_p2_f0", "encoder_input_p6_nope", "encoder_input_p0")
NEW_SYMBOLS = ("diner_encoder_input", "diner_encoder_input_backward")
PTR = 4096    # a non-NULL dummy device pointer: never dereferenced, every call below is refused before a launch


def load(name):
    d = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
    cfg = json.loads(str(d["config"]))
    return d, cfg


def mismatch(got, want, pad, F):
    """None when ``got`` [N, 3 + Cpe, Hp, Wp] passes against ``want``, else what fails: image channels bit-equal, the encoding within
    tol_pe and exactly 0 on the image's own pixels, the same for every image"""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not torch.equal(got[:, :3], want[:, :3].to(got.dtype)):
        return "image channels are not bit-equal"
    if got.shape[1] > 3:
        err = float((got[:, 3:].double() - want[:, 3:].double()).abs().max())
        if not err <= R.tol_pe(F):
            return f"encoding off by {err:.3e} > tol_pe {R.tol_pe(F):.3e}"
        Hp, Wp = got.shape[-2:]
        if float(got[:, 3:, pad:Hp - pad, pad:Wp - pad].abs().max()) != 0.0:
            return "the encoding is not 0 on the image's own pixels"
        if not torch.equal(got[:, 3:], got[:1, 3:].expand_as(got[:, 3:])):
            return "the encoding differs between images"
    return None


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    d, cfg = load(name)
    pad, F = cfg["image_padding"], cfg["padding_pe"]
    want = torch.from_numpy(d["conv1_input"])
    N = cfg["SB"] * cfg["NV"]
    assert want.shape == (N, 3 + R.pe_channels(pad, F), cfg["H"] + 2 * pad, cfg["W"] + 2 * pad)
    assert np.array_equal(d["mean"], np.float32(R.IMAGENET_MEAN)) and np.array_equal(d["std"], np.float32(R.IMAGENET_STD))
    images = torch.from_numpy(d["images"]).flatten(0, 1)
    got = R.encoder_input_ref(images, pad, F, d["mean"].tolist(), d["std"].tolist())
    assert got.dtype == torch.float32
    assert mismatch(got, want, pad, F) is None
    got64 = R.encoder_input_ref(images, pad, F, dtype=torch.float64)
    assert float((got64[:, :3] - want[:, :3].double()).abs().max()) <= 2.0 ** -23 * float(want[:, :3].abs().max())
    if got.shape[1] > 3:
        assert float((got64[:, 3:] - want[:, 3:].double()).abs().max()) <= R.tol_pe(F)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_comparison_rejects_a_broken_restatement(variant):
    d, cfg = load("encoder_input_p4_f4")
    pad, F = cfg["image_padding"], cfg["padding_pe"]
    images = torch.from_numpy(d["images"]).flatten(0, 1)
    bad = R.encoder_input_ref(images, pad, F, variant=variant)
    why = mismatch(bad, d["conv1_input"], pad, F)
    print(variant, "->", why)
    assert why is not None
    assert ("image channels" in why) == (variant == "clamp_short")


def test_tol_pe_is_the_stated_bound():
    assert R.tol_pe(4) == pytest.approx(2.0 ** -21 * (np.pi * 8 + 2)) and 1.2e-5 < R.tol_pe(4) < 1.4e-5
    assert R.tol_pe(0) == R.tol_pe(-1) == 2.0 ** -20


@pytest.mark.parametrize("N, H, W, pad, F", [(1, 3, 5, 2, 1), (2, 4, 4, 6, 2), (2, 9, 6, 0, 4), (1, 1, 1, 3, 0), (2, 1, 7, 2, -1)])
def test_adjoint_restatement_equals_float64_autograd(N, H, W, pad, F):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.rand((N, 3, H, W), generator=g, dtype=torch.float64).requires_grad_(True)
    out = R.encoder_input_ref(x, pad, F, dtype=torch.float64)
    d_out = torch.randn(out.shape, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(out, x, d_out)
    got, abs_sum, n_terms = R.encoder_input_adjoint_ref(d_out, pad, F)
    assert got.shape == x.shape and n_terms.shape == (H, W) and int(n_terms.sum()) == (H + 2 * pad) * (W + 2 * pad)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert bool((abs_sum >= got.abs() - 1e-12).all())
    ny, nx = (2 * pad + 1 if H == 1 else pad + 1), (2 * pad + 1 if W == 1 else pad + 1)
    assert int(n_terms[0, 0]) == ny * nx        # a corner pixel


def _params(decl):
    return [p for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",") if p.strip()]


def test_symbols_are_declared_exported_and_bound_with_the_headers_argument_counts():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        m = re.search(rf"^int {name}\([^;]*\);", header, re.M)
        assert m, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        assert len(args) == len(_params(m.group(0))), name
    assert "image_encoder.py:222-232" in header and "pixelnerf.py:44" in header
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # additions only


def _fwd(images=PTR, N=2, H=4, W=5, pad=2, F=4, xs=PTR, ys=PTR, std=(0.229, 0.224, 0.225), out=PTR):
    from diner_amd import _lib
    lib = _lib.lib()
    rc = lib.diner_encoder_input(images, N, H, W, pad, F, xs, ys, 0.485, 0.456, 0.406, *std, out, None)
    return rc, lib.diner_last_error().decode()


def _bwd(d_out=PTR, N=2, H=4, W=5, pad=2, F=4, std=(0.229, 0.224, 0.225), d_images=PTR):
    from diner_amd import _lib
    lib = _lib.lib()
    rc = lib.diner_encoder_input_backward(d_out, N, H, W, pad, F, *std, d_images, None)
    return rc, lib.diner_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(pad=-1), -1, "pad"),
    (dict(H=1, W=5, pad=0), -1, "below 2"),
    (dict(H=4, W=1, pad=0), -1, "below 2"),
    (dict(N=0), -1, "non-positive"),
    (dict(H=0), -1, "non-positive"),
    (dict(W=-2), -1, "non-positive"),
    (dict(F=-2), -1, "pe_freqs"),
    (dict(std=(0.229, 0.0, 0.225)), -1, "std"),
    (dict(F=31), -3, "pe_freqs"),
])
def test_bad_sizes_return_their_code_before_any_launch(kw, code, word):
    for rc, msg in (_fwd(**kw), _bwd(**kw)):
        assert rc == code, (rc, msg)
        assert word in msg and msg.startswith("encoder_input"), msg


def test_null_pointers_are_refused():
    for kw in (dict(images=None), dict(out=None), dict(xs=None), dict(ys=None)):
        rc, msg = _fwd(**kw)
        assert rc == -1 and "NULL" in msg, (kw, rc, msg)
    for kw in (dict(d_out=None), dict(d_images=None)):
        rc, msg = _bwd(**kw)
        assert rc == -1 and "NULL" in msg, (kw, rc, msg)
    rc, msg = _fwd(N=70000)
    assert rc == -3 and "65535" in msg


def test_the_pad_limit_is_the_backwards_alone():
    """only the backward holds 2 (pad + 1) column sums in LDS; the forward refuses nothing about pad but a padded size of 2^30"""
    rc, msg = _bwd(pad=4096)
    assert rc == -3 and "pad=4096" in msg and msg.startswith("encoder_input_backward"), (rc, msg)
    rc, msg = _fwd(pad=2 ** 29)
    assert rc == -3 and msg.startswith("encoder_input:"), (rc, msg)


def test_python_side_refuses_before_the_device():
    from types import SimpleNamespace as NS

    from diner_amd import glue
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.encoder_input(torch.zeros(2, 3, 4, 5), 2, 4)
    with pytest.raises(ValueError, match=r"\[\.\.\., 3, H, W\]"):
        glue.encoder_input(torch.zeros(2, 4, 4, 5), 2, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.encoder_input_backward(torch.zeros(2, 21, 8, 9), 2, 4)
    model = NS(encoder=NS(upsample_interp="nearest"))
    with pytest.raises(NotImplementedError, match="'nearest'"):
        glue.encode(model, *[None] * 5)
    assert glue.IMAGENET_MEAN == R.IMAGENET_MEAN and glue.IMAGENET_STD == R.IMAGENET_STD
