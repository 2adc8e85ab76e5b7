"""The NOVEL_PE point model on the GPU (diner_amd.novel.NeRFRendererDGS.render_points_novel_pe; csrc/points_mlp_gen_nvpe.hip,
points_mlp_gen_f16_nvpe.hip and novel_pe_map.hip through diner_render_points_novel_pe / diner_pack_novel_pe_map):
(i)   every ``novel_pe_point_*`` fixture -- the unmodified reference's NOVEL_PE PixelNeRF on the CPU (tools/gen_novel_pe_point_golden.py)
      -- in fp32 and f16x3 at the bars of tests/novel_point_ref.rgbsigma_errors (rgb 1e-4 abs, sigma 1e-4 relative to max(1, sigma/12)),
      every point compared, and a second run bit-equal;
(ii)  with deformation_layer = [I | 0], bias 0 and zero pe columns in every lin_z, fp32 ``render_points_novel_pe`` is
      ``render_points_novel`` of the NOVEL model with the same latent columns bit for bit: every extra term is an exact zero and the
      identity GEMM of the map builder is exact;
(iii) the deformation map follows an in-place change of ``deformation_layer.weight`` and of ``encoder.latent``;
(iv)  ``composite()`` with ``hip_point_model`` and ``pass_points`` against the PyTorch route on the restated model
      (tests/novel_pe_point_ref.py), on the geometry of tests/golden/novel_sampler.npz, and ``last_route`` in every routing case.
tests/test_novel_pe_point_host.py proves the restatement against the same fixtures on the CPU."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from synthetic import synth
from tests import novel_pe_point_ref as R
from tests import novel_point_ref as RN
from tests import novel_sampler_ref as N
from tools.gen_novel_pe_point_golden import CASES, case_inputs, input_digests

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
BOUND = 1e-4
POINTS = ("xyz_in", "xyz_gen", "xyz_tgt", "viewdirs")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


_cases = {}


def case(name, dev):
    """(inputs rebuilt from seeds and digest-checked, the stand-in model on the device, the reference's rgb-sigma): built once"""
    if name not in _cases:
        inp, g = case_inputs(CASES[name]), np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
        assert json.loads(str(g["digests"])) == input_digests(inp)
        _cases[name] = (inp, R.model_from_inputs(inp, device=dev), g["rgbsigma"])
    return _cases[name]


def renderer(precision="fp32", **kw):
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(f16x3_any_shape=precision == "f16x3", **kw)
    r.precision = precision
    return r


ROUTE = {"fp32": "novel_pe_points_gen", "f16x3": "novel_pe_points_gen_f16"}


# ---- (i) golden parity, determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_points_novel_pe_meets_the_reference(name, precision, dev):
    inp, m, ref = case(name, dev)
    r = renderer(precision)
    args = [T(inp[k], dev) for k in POINTS]
    out = r.render_points_novel_pe(m, *args)
    assert r.last_route == ROUTE[precision] and r.last_binding == "ctypes" and r.effective_precision == precision
    assert out.shape == ref.shape and m.calls == 0
    e_rgb, e_sigma = R.rgbsigma_errors(out.cpu().numpy(), ref)
    print(f"{name} {precision}: |rgb| {e_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {e_sigma:.2e}")
    assert e_rgb <= BOUND and e_sigma <= BOUND
    again = renderer(precision).render_points_novel_pe(m, *args)           # another renderer: packs and a map of its own
    assert torch.equal(out, again) and torch.equal(out, r.render_points_novel_pe(m, *args))


def test_no_points(dev):
    inp, m, _ = case("novel_pe_point_b", dev)
    e = torch.empty((1, 0, 3), device=dev)
    assert renderer().render_points_novel_pe(m, e, e, e, e).shape == (1, 0, 4)


# ---- (ii) against the NOVEL kernel ------------------------------------------------------------------------------------------------------------------
def test_identity_deformation_is_the_novel_kernel_bit_for_bit(dev):
    """case (a): C = 512, so the pe tail is a gather piece of its own behind the 512 latent columns"""
    inp, _, _ = case("novel_pe_point_a", dev)
    Cc = inp["cfg"]["scene"]["C"]
    ident = dict(inp)
    ident["deform_w"] = np.concatenate([np.eye(Cc, dtype=np.float32), np.zeros((Cc, 6), np.float32)], 1)
    ident["deform_b"] = np.zeros(Cc, np.float32)
    ident["weights"] = {k: v.copy() for k, v in inp["weights"].items()}
    lz = [k for k in ident["weights"] if k.startswith("lin_z.") and k.endswith(".weight")]
    assert len(lz) == 3
    for k in lz:
        ident["weights"][k][:, Cc:] = 0
    pe_model = R.model_from_inputs(ident, device=dev)
    novel = dict(ident, dims=dict(ident["dims"], d_latent=Cc))
    novel["weights"] = {k: np.ascontiguousarray(v[:, :Cc]) if k in lz else v for k, v in ident["weights"].items()}
    novel_model = RN.model_from_inputs(novel, device=dev)
    xi, xg, xt, vd = [T(inp[k], dev) for k in POINTS]
    want = renderer("fp32").render_points_novel(novel_model, xi, xg, vd)
    r = renderer("fp32")
    got = r.render_points_novel_pe(pe_model, xi, xg, xt, vd)
    assert torch.equal(r._pe_map_pack, r._latent_pack)                      # the identity GEMM is exact: the map is the packed latent
    assert torch.isfinite(want).all() and float(want[..., 3].max()) > 0
    assert torch.equal(got, want), float((got - want).abs().max())


# ---- (iii) the caches -------------------------------------------------------------------------------------------------------------------------
def test_deformation_map_follows_in_place_changes(dev):
    inp, m, ref = case("novel_pe_point_c", dev)
    r = renderer()
    args = [T(inp[k], dev) for k in POINTS]
    a = r.render_points_novel_pe(m, *args)
    dmap, pos = r._pe_map_pack, r._pe_pos_pack
    assert r.render_points_novel_pe(m, *args) is not a and r._pe_map_pack is dmap and r._pe_pos_pack is pos     # unchanged: the same packs
    rep = r.memory_report(m)["cached"]
    assert rep["novel_pe_map"] == inp["latent"].size * 4 == rep["latent_nhwc"]                                   # the latent's byte size
    assert rep["novel_pe_pos_encodings"] == (inp["pos_encodings"].size + inp["tgt_pos_encoding"].size) // 3 * 4 * 4
    assert rep["total"] == sum(v for k, v in rep.items() if k != "total")
    for tensor in (m.deformation_layer.weight, m.encoder.latent):
        keep, before = tensor.detach().clone(), r._pe_map_pack
        try:
            with torch.no_grad():
                tensor.mul_(0.5)                                                                             # what an optimizer step does
            b = r.render_points_novel_pe(m, *args)
            assert r._pe_map_pack is not before and not torch.equal(a, b)
            assert torch.equal(b, renderer().render_points_novel_pe(m, *args))
        finally:
            with torch.no_grad():
                tensor.copy_(keep)                    # (in place on the tensor itself: its version counter moves)
        assert max(R.rgbsigma_errors(r.render_points_novel_pe(m, *args).cpu().numpy(), ref)) <= BOUND
    # the head table, the pos-encoding maps and the target cameras are read again after an in-place write
    for tensor in (m.deformation_layer.bias, m.pos_encodings, m.tgt_pos_encoding, m.tgt_c, m.mlp_fine.lin_z[0].weight):
        keep = tensor.detach().clone()
        with torch.no_grad():
            tensor.add_(0.25)
            try:
                assert not torch.equal(r.render_points_novel_pe(m, *args), a)
            finally:
                tensor.copy_(keep)
    assert torch.equal(r.render_points_novel_pe(m, *args), a)                                               # every source restored exactly


# ---- (iv) composite() and the routing ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler_case(dev):
    """the nc64 case of tests/golden/novel_sampler.npz (its rays, filled z, vertices and both offset sets) with a NOVEL_PE stand-in
    model on its scene: a 64-channel latent (72 padded columns), a 128-wide MLP"""
    g = np.load(GOLDEN / "novel_sampler.npz")
    c = N.GOLDEN_CASES["nc64"].build()
    rec = {k: g[f"nc64.{k}"] for k in ("rays", "z", "vertices", "offsets_in", "offsets_gen")}
    assert np.array_equal(rec["rays"], c.rays) and np.array_equal(rec["vertices"], c.vertices)
    sc = c.batched_scene()
    rs = np.random.RandomState(41)
    Cc, fp = 64, 4
    dims = dict(d_latent=Cc + 6, d_hidden=128, n_blocks=3, combine_layer=2, beta=0.0)
    inp = {k: getattr(sc, k) for k in ("poses", "focal", "c", "image_shape", "depths", "depths_std", "normals")}
    inp["latent"] = rs.standard_normal((1, c.NV, Cc, 12 + 2 * fp, 12 + 2 * fp)).astype(np.float32)
    inp["weights"] = synth.make_mlp_weights(42, bias_scale=0.1, d_in=55, **{k: v for k, v in dims.items() if k != "beta"})
    inp["gen_latent"] = rs.standard_normal((Cc, 28, 20)).astype(np.float32)
    inp["deform_w"] = np.concatenate([rs.uniform(-1, 1, (Cc, Cc)) / np.sqrt(Cc + 6), rs.uniform(-1, 1, (Cc, 6))], 1).astype(np.float32)
    inp["deform_b"] = rs.uniform(-0.1, 0.1, Cc).astype(np.float32)
    inp["pos_encodings"] = rs.uniform(-1, 1, (1, c.NV, 3, 36, 30)).astype(np.float32)
    inp["tgt_pos_encoding"] = rs.uniform(-1, 1, (1, 1, 3, 26, 34)).astype(np.float32)
    inp["gen_poses"] = synth.look_at_origin_w2c(0.7, 1.7)[None, None]
    inp["gen_focal"], inp["gen_c"] = np.array([[[60.0, 63.0]]], np.float32), np.array([[[21.5, 26.0]]], np.float32)
    inp["gen_image_shape"] = np.array([40, 56], np.float32)
    inp["tgt_poses"] = synth.look_at_origin_w2c(-0.4, 1.8)[None, None]
    inp["tgt_focal"], inp["tgt_c"] = np.array([[[70.0, 73.5]]], np.float32), np.array([[[22.75, 32.5]]], np.float32)
    inp["tgt_image_shape"] = np.array([48, 60], np.float32)
    inp["cfg"] = dict(scene=dict(feature_padding=fp, C=Cc), num_freqs=6, index_interp="bilinear", index_padding="border")
    inp["dims"] = dims
    return c, {k: T(v, dev) for k, v in rec.items()}, R.model_from_inputs(inp, device=dev)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_composite_matches_the_torch_route(sampler_case, precision, dev):
    c, rec, m = sampler_case
    geo = (rec["vertices"], rec["offsets_in"], rec["offsets_gen"])
    kw = dict(n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G, pass_points=True)
    on, off = renderer(precision, hip_point_model=True, **kw), renderer("fp32", **kw)
    m.calls = 0
    with torch.no_grad():
        want = off.composite(m, rec["rays"], rec["z"], *geo)
        assert off.last_route == "torch" and m.calls == 1
        got = on.composite(m, rec["rays"], rec["z"], *geo)
        assert on.last_route == ROUTE[precision] and on.effective_precision == precision and m.calls == 1
        on.check_finite()
        for k, a, b in zip(("weights", "rgb", "depth"), got, want):
            err = float((a - b).abs().max())
            print(f"composite {precision}: max |d {k}| = {err:.2e}")
            assert err <= BOUND, k
        assert float(want[0].sum(-1).max()) > 0.5 and float(want[1].std()) > 1e-2                   # (a frame with content)


def test_routing_cases(sampler_case, dev):
    from diner_amd.novel import NeRFRendererDGS
    c, rec, m = sampler_case
    call = lambda r, model=m: r.composite(model, rec["rays"], rec["z"], rec["vertices"], rec["offsets_in"], rec["offsets_gen"])
    kw = dict(n_samples=c.K, n_depth_candidates=c.NC, n_gaussian=c.G)
    r = renderer("fp32", hip_point_model=True, pass_points=True, **kw)
    m.calls = 0
    call(r)                                                                     # grad mode on, no parameter requires grad: the kernel
    assert r.last_route == "novel_pe_points_gen" and m.calls == 0
    m.deformation_layer.weight.requires_grad_(True)                             # training: PyTorch, with a graph to the parameter
    try:
        w, rgb, depth = call(r)
        assert r.last_route == "torch" and m.calls == 1 and rgb.requires_grad
        g, = torch.autograd.grad(rgb.sum(), m.deformation_layer.weight)
        assert float(g.abs().max()) > 0
        with torch.no_grad():
            call(r)
        assert r.last_route == "novel_pe_points_gen" and m.calls == 1
    finally:
        m.deformation_layer.weight.requires_grad_(False)
    with torch.no_grad():
        r.hip_point_model = False                                               # a plain attribute
        call(r)
        assert r.last_route == "torch" and m.calls == 2
        r.hip_point_model = True
        m.encoder.index_interp = "bicubic"
        try:
            call(r)
            assert r.last_route == "torch" and m.calls == 3
        finally:
            m.encoder.index_interp = "bilinear"
        m.encoder.index_padding = "zeros"                                       # a served mode: the kernel, like the PyTorch route
        try:
            got = call(r)
            assert r.last_route == "novel_pe_points_gen" and m.calls == 3
            want = call(renderer("fp32", pass_points=True, **kw))
            assert float((got[1] - want[1]).abs().max()) <= BOUND and m.calls == 4
        finally:
            m.encoder.index_padding = "border"
        # the pinned fallbacks: a deformation_layer with pass_points False (the model is then called with two point sets) ...
        seen = []
        two = lambda a, b, viewdirs=None: seen.append(2) or m(a, b, a, viewdirs=viewdirs)
        two.deformation_layer = m.deformation_layer
        rn = NeRFRendererDGS(hip_point_model=True, **kw)
        call(rn, two)
        assert rn.last_route == "torch" and seen == [2]
        # ... pass_points with a model that has no deformation_layer, and any other callable
        fn = lambda a, b, p, viewdirs=None: seen.append(3) or m(a, b, p, viewdirs=viewdirs)
        call(r, fn)
        assert r.last_route == "torch" and seen == [2, 3]
