"""Host-side checks of the shape-general inference path (no GPU): the C ABI's new entry points and their shape envelope, the
renderer's classification of models (``_validate_model``), and the seeded inputs of the ``shape_*`` fixtures."""
import ctypes as C
import json
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
SHAPE_FIXTURES = sorted(p.stem for p in GOLDEN.glob("shape_*.npz"))
NEW_SYMBOLS = ["diner_mlp_gen_packed_floats", "diner_pack_mlp_gen", "diner_render_points_gen", "diner_render_gen",
               "diner_render_image_gen"]


def _shape(**kw):
    from diner_amd import _lib
    d = dict(d_in=55, d_latent=512, d_hidden=128, n_blocks=5, combine_layer=3, num_freqs=6, beta=0.0, d_out=4, combine_type=0)
    d.update(kw)
    return _lib.DinerMlpShape(*[d[f] for f, _ in _lib.DinerMlpShape._fields_])


def test_new_symbols_are_declared_and_exported():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert lib.diner_version() == _lib.ABI_VERSION == 3


def test_packed_size_follows_the_shape():
    from diner_amd import _lib
    lib = _lib.lib()
    # case (a): lin_in 4 tiles x 7 k-blocks, 3 lin_z 4 x 64, 10 block layers 4 x 16, lin_out 1 x 16 (256 floats per tile and
    # k-block), biases 14 x 128 + 32
    want = 256 * (4 * 7 + 3 * 4 * 64 + 10 * 4 * 16 + 16) + 14 * 128 + 32
    assert lib.diner_mlp_gen_packed_floats(C.byref(_shape())) == want
    # the standard shape has the fp32 image of diner_pack_mlp (points_mlp.hip)
    std = 16 * 7 * 256 + 13 * 16 * 64 * 256 + 64 * 256 + 14 * 512 + 32
    assert lib.diner_mlp_gen_packed_floats(C.byref(_shape(d_hidden=512))) == std


@pytest.mark.parametrize("kw, what", [
    (dict(d_hidden=48), "d_hidden=48"), (dict(d_hidden=544), "d_hidden=544"), (dict(d_hidden=0), "d_hidden=0"),
    (dict(combine_type=1), "combine_type"), (dict(d_out=5), "d_out=5"), (dict(d_latent=12), "d_latent=12"),
    (dict(d_latent=1032), "d_latent=1032"), (dict(n_blocks=0), "n_blocks=0"), (dict(combine_layer=-1), "combine_layer=-1"),
    (dict(num_freqs=0, d_in=7), "num_freqs=0"), (dict(d_in=56), "d_in=56"), (dict(beta=-1.0), "beta"),
    (dict(beta=float("nan")), "beta"),
])
def test_out_of_envelope_shapes_return_not_implemented(kw, what):
    from diner_amd import _lib
    lib = _lib.lib()
    sh = _shape(**kw)
    assert lib.diner_mlp_gen_packed_floats(C.byref(sh)) == -3
    assert what.encode() in lib.diner_last_error()
    raw = _lib.DinerMlpGenRaw()
    assert lib.diner_pack_mlp_gen(C.byref(sh), C.byref(raw), C.c_void_p(8), None) == -3
    assert lib.diner_render_points_gen(None, C.byref(sh), None, None, None, 0, 1, None, None) in (-1, -3)


def test_no_mean_over_views_needs_one_view():
    """combine_layer >= n_blocks: the reference reshapes (SB, NV, B, 4) to (SB, B, 4) (pixelnerf.py:137), which works for NV = 1 only"""
    from diner_amd import _lib
    lib = _lib.lib()
    sc = _lib.DinerScene()
    sc.SB, sc.NV, sc.H, sc.W, sc.h, sc.w, sc.C, sc.num_freqs = 1, 2, 2, 2, 2, 2, 512, 6
    sc.image_w = sc.image_h = 2.0
    sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 8   # non-NULL dummies, never dereferenced (NR = 0)
    sh = _shape(combine_layer=1000)
    assert lib.diner_render_points_gen(C.byref(sc), C.byref(sh), C.c_void_p(8), None, None, 0, 4, None, None) == -3
    assert b"pixelnerf.py:137" in lib.diner_last_error()
    sc.NV = 1
    assert lib.diner_render_points_gen(C.byref(sc), C.byref(sh), C.c_void_p(8), None, None, 0, 4, None, None) == 0


def test_pack_mlp_gen_rejects_null_pointers():
    from diner_amd import _lib
    lib = _lib.lib()
    raw = _lib.DinerMlpGenRaw()
    assert lib.diner_pack_mlp_gen(C.byref(_shape()), C.byref(raw), C.c_void_p(8), None) == -1
    assert b"NULL" in lib.diner_last_error()


def _stub(cfg_or_dims, NV=1, C_lat=512):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(8, 8, NV, seed=0, feature_padding=2, C=C_lat)
    dims = dict(cfg_or_dims)
    F = dims.pop("num_freqs", 6)
    d = {k: v for k, v in dims.items() if k != "beta"}
    w = synth.make_mlp_weights(1, d_in=7 + 8 * F, d_latent=C_lat, **d)
    return model_from_scene(sc, w, device="cpu", num_freqs=F, d_latent=C_lat, **dims)


def test_standard_model_is_classified_standard():
    from diner_amd import NeRFRendererDGS
    from diner_amd.renderer import STANDARD_SHAPE
    shape = NeRFRendererDGS._validate_model(_stub({}))
    assert shape == STANDARD_SHAPE and shape.standard


@pytest.mark.parametrize("name", SHAPE_FIXTURES)
def test_validate_model_classifies_the_fixture_configs(name):
    from diner_amd import NeRFRendererDGS
    from tools.gen_shape_golden import CASES, mlp_dims
    cfg = CASES[name]
    d = mlp_dims(cfg)
    ctor = {k: v for k, v in d.items() if k not in ("d_in", "d_latent")}   # the ResnetFC constructor's defaults filled in
    m = _stub(dict(ctor, num_freqs=cfg["num_freqs"]), NV=cfg["scene"]["NV"], C_lat=cfg["scene"]["C"])
    shape = NeRFRendererDGS._validate_model(m)
    assert not shape.standard
    assert tuple(shape) == (d["d_in"], d["d_latent"], d["d_hidden"], d["n_blocks"], d["combine_layer"], cfg["num_freqs"], d["beta"])


@pytest.mark.parametrize("dims, what", [
    (dict(d_hidden=48), "d_hidden=48"), (dict(d_hidden=1024), "d_hidden=1024"), (dict(n_blocks=0, combine_layer=0), "n_blocks=0"),
])
def test_validate_model_rejects_shapes_outside_the_envelope(dims, what):
    from diner_amd import NeRFRendererDGS
    with pytest.raises(NotImplementedError, match=what):
        NeRFRendererDGS._validate_model(_stub(dims))


def test_validate_model_rejects_other_combine_types_and_heads():
    from diner_amd import NeRFRendererDGS
    m = _stub(dict(d_hidden=128))
    m.mlp_fine.combine_type = "max"
    with pytest.raises(NotImplementedError, match="combine_type"):
        NeRFRendererDGS._validate_model(m)
    m = _stub(dict(d_hidden=128))
    m.mlp_fine.d_out = 5
    with pytest.raises(NotImplementedError, match="d_out=5"):
        NeRFRendererDGS._validate_model(m)
    m = _stub(dict(d_hidden=128))
    m.mlp_fine.activation = torch.nn.Tanh()
    with pytest.raises(NotImplementedError, match="activation"):
        NeRFRendererDGS._validate_model(m)


def test_non_standard_model_runs_fp32_and_says_so_once():
    from diner_amd import NeRFRendererDGS
    m = _stub(dict(d_hidden=64, n_blocks=2, combine_layer=1, beta=10.0))
    r = NeRFRendererDGS()
    assert r.precision == "f16x3"
    with pytest.warns(UserWarning, match="fp32"):
        shape = r._route(m)
    assert r.effective_precision == "fp32" and shape.beta == 10.0 and r.precision == "f16x3"
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*precision=")
        r._route(m)                               # once per renderer
    r2 = NeRFRendererDGS()
    r2.precision = "fp32"
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*precision=")
        r2._route(m)
    assert r2.effective_precision == "fp32"
    r3 = NeRFRendererDGS()
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*precision=")
        r3._route(_stub({}))                      # the standard model: no warning, its precision stays
    assert r3.effective_precision == "f16x3"


def test_training_a_non_standard_model_raises_and_names_inference():
    from diner_amd import NeRFRendererDGS
    m = _stub(dict(d_hidden=64, n_blocks=2, combine_layer=1))
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1)
    with pytest.raises(NotImplementedError, match="inference"):
        r(m, torch.zeros(1, 2, 8))               # raised before any device work


def test_memory_report_counts_the_generic_pack():
    from diner_amd import NeRFRendererDGS
    rep = NeRFRendererDGS().memory_report()
    assert rep["cached"]["mlp_gen_packed"] == 0 and "mlp_packed" in rep["cached"]


@pytest.mark.parametrize("name", SHAPE_FIXTURES)
def test_fixture_digests_match_the_generator(name):
    from tools.gen_shape_golden import CASES, case_inputs, input_digests
    data = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    cfg = json.loads(str(data["config"]))
    assert cfg == json.loads(json.dumps(CASES[name]))
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    assert np.array_equal(rays, data["rays"])
    NR, K = rays.shape[1], cfg["K"]
    assert data["z_fill"].shape == (NR, K) and data["rgbsigma"].shape == (NR, K, 4) and data["rgb"].shape == (NR, 3)
    assert data["rgbsigma"][..., 3].max() > 1.0     # the case composites something: not an empty scene


def test_five_fixture_cases_and_none_named_like_the_parametrised_goldens():
    assert len(SHAPE_FIXTURES) >= 5
    assert not list(GOLDEN.glob("shape_*.npz")) or not any(p.name[0] == "g" for p in GOLDEN.glob("shape_*.npz"))
    assert sum(p.stat().st_size for p in GOLDEN.glob("shape_*.npz")) < 4e6
