"""The NOVEL and NOVEL_PE render kernels across their latent-width envelope on the GPU (csrc/points_mlp_gen_nv.hip,
points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nv.hip, points_mlp_gen_f16_nvpe.hip, novel_pe_map.hip), through
diner_amd.novel.NeRFRendererDGS.render_points_novel / render_points_novel_pe:
(i)  every case of tests/novel_shape_cases.py in fp32 and f16x3 against the float64 restatement of the same seeded inputs, every point
     compared at the project's bars (tests/novel_point_ref.rgbsigma_errors: rgb 1e-4 abs, sigma 1e-4 relative to max(1, sigma/12)); a
     second run and a fresh renderer (packs and a map of its own) bit-equal.  Each case prints ``e_gpu``, ``e32`` (the error of the CPU
     float32 restatement against the same float64 result) and their ratio; the ratio is recorded in DESIGN.md, not asserted.
(ii) C = 520 with the eight channels past 512 disconnected is the C = 512 model of the first 512 channels: bit for bit in fp32 (every
     extra term is an exact zero added in the same k order; NOVEL_PE's pe tail moves from columns 0 .. 7 to columns 8 .. 15 of piece 2),
     at the bars in f16x3.
tests/test_novel_shapes_host.py proves on the CPU that every case is a sound yardstick: it rejects the wrong forms these shapes exist
to catch by 10 bars or more, and its float32 restatement needs no more than a quarter of a bar."""
import numpy as np
import pytest
import torch

from tests import novel_pe_point_ref as RPE
from tests import novel_point_ref as RN
from tests import novel_shape_cases as S

pytestmark = pytest.mark.gpu
BOUND = 1e-4
ROUTE = {("novel", "fp32"): "novel_points_gen", ("novel", "f16x3"): "novel_points_gen_f16",
         ("novel_pe", "fp32"): "novel_pe_points_gen", ("novel_pe", "f16x3"): "novel_pe_points_gen_f16"}
POINTS = {"novel": ("xyz_in", "xyz_gen", "viewdirs"), "novel_pe": ("xyz_in", "xyz_gen", "xyz_tgt", "viewdirs")}
ALL = [(kind, name) for kind, table in S.TABLES.items() for name in table]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def renderer(precision):
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(f16x3_any_shape=precision == "f16x3")
    r.precision = precision
    return r


def build(kind, inp, dev):
    return (RPE if kind == "novel_pe" else RN).model_from_inputs(inp, device=dev)


def render(kind, precision, model, inp, dev, r=None):
    """-> (rgb-sigma on the device, the renderer), the route and the effective precision asserted, the model never called"""
    r = r or renderer(precision)
    fn = r.render_points_novel_pe if kind == "novel_pe" else r.render_points_novel
    out = fn(model, *[T(inp[k], dev) for k in POINTS[kind]])
    assert r.last_route == ROUTE[kind, precision] and r.last_binding == "ctypes" and r.effective_precision == precision
    assert model.calls == 0 and out.shape == inp["xyz_in"].shape[:2] + (4,)
    return out, r


_models = {}


def model(kind, name, dev):
    if (kind, name) not in _models:
        _models[kind, name] = build(kind, S.case(kind, name)[0], dev)
    return _models[kind, name]


# ---- (i) every shape against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("kind, name", ALL, ids=[n for _, n in ALL])
def test_shape_meets_float64(kind, name, precision, dev):
    inp, r64, r32 = S.case(kind, name)
    m = model(kind, name, dev)
    out, r = render(kind, precision, m, inp, dev)
    got = out.cpu().numpy()
    e_gpu, e32 = RN.rgbsigma_errors(got, r64), RN.rgbsigma_errors(r32, r64)
    ratio = [g / c if c > 0 else float("inf") for g, c in zip(e_gpu, e32)]
    print(f"{name} {precision}: e_gpu rgb {e_gpu[0]:.2e} sigma {e_gpu[1]:.2e} | e32 rgb {e32[0]:.2e} sigma {e32[1]:.2e} | "
          f"ratio rgb {ratio[0]:.2f} sigma {ratio[1]:.2f}")
    assert np.isfinite(got).all()
    assert e_gpu[0] <= BOUND and e_gpu[1] <= BOUND
    assert torch.equal(out, render(kind, precision, m, inp, dev, r)[0])          # a second run
    assert torch.equal(out, render(kind, precision, m, inp, dev)[0])             # a fresh renderer: packs and a map of its own


# ---- (ii) C = 520 with its last eight channels disconnected is C = 512 ------------------------------------------------------------------------------
def _pair(kind):
    """(the C = 520 case with the channels 512 .. 519 disconnected, the C = 512 model of its first 512 channels): the same function"""
    name = "pe_c520" if kind == "novel_pe" else "nv_c520"
    inp, _, _ = S.case(kind, name)
    C, K = 520, 512
    lz = S.lin_z_keys(inp)
    wide = dict(inp, weights={k: v.copy() for k, v in inp["weights"].items()})
    for k in lz:
        wide["weights"][k][:, K:C] = 0
    cut = lambda w: np.ascontiguousarray(np.concatenate([w[:, :K], w[:, C:]], 1))     # the latent columns 0 .. 511 (+ the six pe columns)
    narrow = dict(wide, weights={k: cut(v) if k in lz else v for k, v in wide["weights"].items()},
                  latent=np.ascontiguousarray(inp["latent"][:, :, :K]), gen_latent=np.ascontiguousarray(inp["gen_latent"][:K]),
                  cfg=dict(inp["cfg"], scene=dict(inp["cfg"]["scene"], C=K)))
    if kind == "novel_pe":
        wide["deform_w"] = inp["deform_w"].copy()
        wide["deform_w"][:K, K:C] = 0          # the map's first 512 channels no longer read the latent's last eight
        narrow["deform_w"] = cut(wide["deform_w"][:K])
        narrow["deform_b"] = np.ascontiguousarray(inp["deform_b"][:K])
        narrow["dims"] = dict(inp["dims"], d_latent=K + 6)
    else:
        narrow["dims"] = dict(inp["dims"], d_latent=K)
    return wide, narrow


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("kind", ["novel_pe", "novel"])
def test_c520_with_a_disconnected_tail_is_c512(kind, precision, dev):
    """fp32: bit for bit.  The GEMM runs its k-blocks in order and piece by piece into one accumulator, so the wide model adds, after
    piece 1, products with exact zero weights (NOVEL: 8; NOVEL_PE: 8, then the pe columns, which the narrow model has as the first 8
    columns of its piece 2), and the map builder's second piece adds 8 zero products to channels 0 .. 511.  f16x3 splits its operands
    per 16-wide k-block the same way, but is held at the bars only."""
    wide, narrow = _pair(kind)
    r64 = S.restate(kind, narrow)
    assert np.abs(S.restate(kind, wide) - r64).max() <= 1e-12 and float((r64[..., 3] > 0).mean()) >= 1 / 3
    got_w, rw = render(kind, precision, build(kind, wide, dev), wide, dev)
    got_n, rn = render(kind, precision, build(kind, narrow, dev), narrow, dev)
    if kind == "novel_pe":
        assert rw._pe_map_pack.shape[-1] == 520 and rn._pe_map_pack.shape[-1] == 512
        assert torch.equal(rw._pe_map_pack[..., :512], rn._pe_map_pack)        # (one builder serves both precisions)
    print(f"{kind} {precision}: max |wide - narrow| = {float((got_w - got_n).abs().max()):.2e}")
    for which, got in (("C = 520", got_w), ("C = 512", got_n)):
        e = RN.rgbsigma_errors(got.cpu().numpy(), r64)
        print(f"{kind} {precision} {which}: |rgb| {e[0]:.2e}, |sigma| {e[1]:.2e}")
        assert e[0] <= BOUND and e[1] <= BOUND
    if precision == "fp32":
        assert torch.equal(got_w, got_n), float((got_w - got_n).abs().max())
