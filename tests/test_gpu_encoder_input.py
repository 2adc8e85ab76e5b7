"""GPU tests of conv1's input (glue.encoder_input: diner_encoder_input / _backward).

Forward: against the reference's captured conv1 input (tests/golden/encoder_input_*.npz) and against the torch restatement of
tests/encoder_input_ref.py on the kernel's own coordinates.  Image channels bit-equal; the encoding within tol_pe = 2^-21 (f_max + 2)
(coordinate rounding <= 2^-23 scaled by f_max = pi 2^(F-1), one ulp of an argument <= f_max + pi/2 for FMA against multiply-add, 5e-7 per
sine implementation, margin 2), exactly 0 on the image's own pixels and bit-equal between the images.  Every shape also runs with
padding_pe = -1 and 0.
Backward: against the float64 restatement, per element |err| <= n_terms 2^-24 sum|terms| / std[c] (the bound of an n-term fp32 sum in any
order, n - 1 additions and the division); two runs bit-equal; <A x, g> = <x, A^T g> to that bound weighted by |x| and summed; the autograd function's
forward equals the no-grad call bit for bit; no backward launch without a needed gradient."""
import json
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import encoder_input_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
GOLDEN_NAMES = ("encoder_input_p4_f4", "encoder_input_p2_f0", "encoder_input_p6_nope", "encoder_input_p0")
# name -> (N, H, W, pad, F)
SHAPES = {
    "scalar_path": (1, 3, 5, 2, 1),          # Wp = 9: no 16-byte stores
    "vector_path": (3, 8, 12, 2, 4),         # Wp = 16
    "pad_above_size": (2, 4, 4, 6, 2),       # Wp = 16
    "product_pad": (2, 16, 16, 64, 4),       # 144 x 144: several blocks, 16-byte stores
    "pad_0": (2, 9, 6, 0, 3),                # the encoding is off whatever F says
}
PE_MODES = ("own", "none", "f0")             # the case's own padding_pe, -1, 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _F(F, mode):
    return {"own": F, "none": -1, "f0": 0}[mode]


_images = {}


def images_of(name):
    """seeded CPU inputs of a shape, made once and left unchanged"""
    if name not in _images:
        N, H, W, _, _ = SHAPES[name]
        g = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 40)
        _images[name] = torch.rand((N, 3, H, W), generator=g)
    return _images[name]


def check_forward(got, images, pad, F, dev, golden=None):
    from diner_amd import glue
    N, _, H, W = images.shape
    Hp, Wp, Cpe = H + 2 * pad, W + 2 * pad, R.pe_channels(pad, F)
    assert got.shape == (N, 3 + Cpe, Hp, Wp) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu()
    xs, ys = glue._coords(Hp, Wp, dev) if Cpe else (None, None)
    refs = [("restatement fp32", R.encoder_input_ref(images, pad, F, xs=xs, ys=ys)),
            ("restatement float64", R.encoder_input_ref(images, pad, F, xs=xs, ys=ys, dtype=torch.float64))]
    if golden is not None:
        refs.append(("reference", torch.from_numpy(golden)))
    for what, ref in refs:
        if ref.dtype == torch.float32:
            assert torch.equal(got[:, :3], ref[:, :3]), f"image channels differ from the {what}"
        if Cpe:
            err = float((got[:, 3:].double() - ref[:, 3:].double()).abs().max())
            print(f"N={N} {H}x{W} pad={pad} F={F}: encoding max err vs {what} {err:.3e}, tol_pe {R.tol_pe(F):.3e}")
            assert err <= R.tol_pe(F), (what, err)
    if Cpe:
        assert float(got[:, 3:, pad:Hp - pad, pad:Wp - pad].abs().max()) == 0.0
        assert torch.equal(got[:, 3:], got[:1, 3:].expand(N, -1, -1, -1)), "the encoding differs between images"
        assert float(got[0, 3:].abs().amax((1, 2)).min()) > 0.1       # every encoding channel has content on the padding


@pytest.mark.parametrize("mode", PE_MODES)
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_forward_against_the_reference(name, mode, dev):
    from diner_amd import glue
    d = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
    cfg = json.loads(str(d["config"]))
    pad, F = cfg["image_padding"], _F(cfg["padding_pe"], mode)
    images = torch.from_numpy(d["images"])                     # [SB, NV, 3, H, W]: the leading dimensions are flattened
    got = glue.encoder_input(images.to(dev), pad, F, d["mean"].tolist(), d["std"].tolist())
    same = F == cfg["padding_pe"] or R.pe_channels(pad, F) == R.pe_channels(pad, cfg["padding_pe"]) == 0
    check_forward(got, images.flatten(0, 1), pad, F, dev, golden=d["conv1_input"] if same else None)
    if not same:   # another F: the image channels are still the reference's
        assert torch.equal(got[:, :3].cpu(), torch.from_numpy(d["conv1_input"][:, :3]))


@pytest.mark.parametrize("mode", PE_MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_forward_against_the_restatement(name, mode, dev):
    from diner_amd import glue
    N, H, W, pad, F = SHAPES[name]
    F = _F(F, mode)
    images = images_of(name)
    got = glue.encoder_input(images.to(dev), pad, F)
    check_forward(got, images, pad, F, dev)
    again = glue.encoder_input(images.to(dev), pad, F)
    assert torch.equal(got, again)


def test_other_constants_and_dtypes(dev):
    """mean / std as tensors, half images, extra leading dimensions"""
    from diner_amd import glue
    N, H, W, pad, F = SHAPES["vector_path"]
    images = images_of("vector_path").half().float()
    mean, std = torch.tensor([0.1, -0.2, 0.3]).view(3, 1, 1), torch.tensor([0.5, 2.0, 1.25]).view(3, 1, 1)
    got = glue.encoder_input(images.half().to(dev).reshape(1, N, 3, H, W), pad, F, mean, std)
    want = R.encoder_input_ref(images, pad, F, mean, std)
    assert got.shape == want.shape and torch.equal(got[:, :3].cpu(), want[:, :3])


@pytest.mark.parametrize("name", ["scalar_path", "vector_path"])
def test_misaligned_input(name, dev):
    """images that start 4 bytes into a larger buffer (no 16-byte alignment) give the same result"""
    from diner_amd import glue
    N, H, W, pad, F = SHAPES[name]
    images = images_of(name).to(dev)
    buf = torch.zeros(images.numel() + 1, device=dev)
    buf[1:] = images.reshape(-1)
    view = buf[1:].view(N, 3, H, W)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert torch.equal(glue.encoder_input(view, pad, F), glue.encoder_input(images, pad, F))
    g = torch.ones((N, 3 + R.pe_channels(pad, F), H + 2 * pad, W + 2 * pad), device=dev)
    gbuf = torch.zeros(g.numel() + 1, device=dev)
    gbuf[1:] = g.reshape(-1)
    assert torch.equal(glue.encoder_input_backward(gbuf[1:].view(g.shape), pad, F), glue.encoder_input_backward(g, pad, F))


_cot = {}


def cotangent_of(name, F):
    """d_out and its float64 adjoint (gradient, sum of |terms| / std, number of terms), made once"""
    key = (name, F)
    if key not in _cot:
        N, H, W, pad, _ = SHAPES[name]
        g = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 70)
        d_out = torch.randn((N, 3 + R.pe_channels(pad, F), H + 2 * pad, W + 2 * pad), generator=g)
        _cot[key] = (d_out, *R.encoder_input_adjoint_ref(d_out, pad, F))
    return _cot[key]


@pytest.mark.parametrize("mode", PE_MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_backward_against_float64(name, mode, dev):
    from diner_amd import glue
    N, H, W, pad, F = SHAPES[name]
    F = _F(F, mode)
    d_out, want, abs_sum, n_terms = cotangent_of(name, F)
    got = glue.encoder_input_backward(d_out.to(dev), pad, F)
    again = glue.encoder_input_backward(d_out.to(dev), pad, F)
    assert got.shape == (N, 3, H, W) and got.dtype == torch.float32
    assert torch.equal(got, again), "two backward calls must be bit-identical"
    err = (got.cpu().double() - want).abs()
    bound = n_terms.double() * 2.0 ** -24 * abs_sum
    print(f"{name} F={F}: terms up to {int(n_terms.max())}, max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (name, float((err - bound).max()))
    if min(H, W) > 1:
        assert int(n_terms.max()) == (pad + 1) ** 2      # a corner pixel


@pytest.mark.parametrize("name", ["vector_path", "pad_above_size", "scalar_path"])
def test_adjoint_identity(name, dev):
    """<encoder_input(x) - encoder_input(0), g> = <x, backward(g)>: the encoding and the mean drop out of the difference"""
    from diner_amd import glue
    N, H, W, pad, F = SHAPES[name]
    x = images_of(name)
    d_out, _, abs_sum, n_terms = cotangent_of(name, F)
    Ax = (glue.encoder_input(x.to(dev), pad, F).double() - glue.encoder_input(torch.zeros_like(x).to(dev), pad, F).double()).cpu()
    Atg = glue.encoder_input_backward(d_out.to(dev), pad, F).cpu().double()
    if Ax.shape[1] > 3:
        assert float(Ax[:, 3:].abs().max()) == 0.0
    lhs, rhs = float((Ax * d_out.double()).sum()), float((x.double() * Atg).sum())
    # the backward's bound, n_terms 2^-24 sum|terms| / std per element of A^T g, weighted by |x|: nothing is added for the forward's roundings
    bound = float((x.double().abs() * n_terms.double() * 2.0 ** -24 * abs_sum).sum())
    print(f"{name}: <Ax, g> = {lhs:.10e}, <x, A^T g> = {rhs:.10e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_autograd_function(dev):
    from diner_amd import glue
    N, H, W, pad, F = SHAPES["vector_path"]
    d_out, want, abs_sum, n_terms = cotangent_of("vector_path", F)
    x = images_of("vector_path").to(dev).reshape(1, N, 3, H, W).requires_grad_(True)
    out = glue.encoder_input(x, pad, F)
    assert out.requires_grad
    with torch.no_grad():
        assert torch.equal(glue.encoder_input(x, pad, F), out)        # the no-grad call's values, bit for bit
    assert torch.equal(glue.encoder_input(x.detach(), pad, F), out)
    (out * d_out.to(dev)).sum().backward()
    assert x.grad.shape == x.shape and torch.equal(x.grad.reshape(N, 3, H, W), glue.encoder_input_backward(d_out.to(dev), pad, F))
    assert bool(((x.grad.reshape(N, 3, H, W).cpu().double() - want).abs() <= n_terms.double() * 2.0 ** -24 * abs_sum).all())
    h = images_of("vector_path").half().to(dev).requires_grad_(True)   # a gradient comes back in the images' dtype
    glue.encoder_input(h, pad, F).sum().backward()
    assert h.grad.dtype == torch.float16 and h.grad.shape == h.shape


def test_no_backward_launch_without_a_needed_gradient(dev, monkeypatch):
    from diner_amd import glue
    N, H, W, pad, F = SHAPES["vector_path"]

    def boom(*a, **k):
        raise AssertionError("the backward kernel was launched")

    monkeypatch.setattr(glue, "encoder_input_backward", boom)
    ctx = NS(needs_input_grad=(False, False, False, False, False), pad=pad, F=F, std=list(R.IMAGENET_STD), shape=(N, 3, H, W),
             dtype=torch.float32)
    d_out = cotangent_of("vector_path", F)[0].to(dev)
    assert glue._EncoderInputFn.backward(ctx, d_out) == (None,) * 5
    ctx.needs_input_grad = (True, False, False, False, False)
    with pytest.raises(AssertionError, match="launched"):
        glue._EncoderInputFn.backward(ctx, d_out)
    out = glue.encoder_input(images_of("vector_path").to(dev), pad, F)     # nothing requires grad: no autograd node at all
    assert out.grad_fn is None and not out.requires_grad


def test_bad_arguments(dev):
    from diner_amd import _lib, glue
    lib = _lib.lib()
    x = images_of("vector_path").to(dev)
    N, _, H, W = x.shape
    out = torch.empty((N, 21, H + 4, W + 4), device=dev)
    xs, ys = glue._coords(H + 4, W + 4, dev)
    c = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    st = glue._st(dev)
    for args, word in (((x.data_ptr(), N, H, W, -1, 4, xs.data_ptr(), ys.data_ptr(), *c, out.data_ptr(), st), "pad"),
                       ((x.data_ptr(), N, 1, W, 0, 4, xs.data_ptr(), ys.data_ptr(), *c, out.data_ptr(), st), "below 2"),
                       ((x.data_ptr(), N, H, W, 2, 4, None, ys.data_ptr(), *c, out.data_ptr(), st), "NULL")):
        rc = lib.diner_encoder_input(*args)
        msg = lib.diner_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.encoder_input(x.cpu(), 2, 4)
    with pytest.raises(ValueError):
        glue.encoder_input(x, -1, 4)
    # NULL xs / ys are fine with the encoding off
    assert lib.diner_encoder_input(x.data_ptr(), N, H, W, 2, -1, None, None, *c, out.data_ptr(), st) == 0
    torch.cuda.synchronize()
