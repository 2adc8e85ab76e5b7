"""Host-side checks of the shape-general training path (no GPU): the C ABI's new entry points and their argument validation (which
returns before any device work), the renderer's opt-in switch ``train_any_shape`` and its dispatch to diner_amd/training_gen.py, and
the seeded inputs of the ``trainshape_*`` fixtures."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
TRAINSHAPE_FIXTURES = ["trainshape_a_h128_nv2", "trainshape_b_h256_softplus_nv4", "trainshape_c_h96_f4_dtu",
                       "trainshape_d_lat256_h64_nearest_zeros", "trainshape_e_defaults_nv1", "trainshape_f_combine0_nv3"]
NEW_SYMBOLS = ["diner_train_gemm_act", "diner_train_point_inputs_gen", "diner_train_point_inputs_backward_gen"]
FAKE = C.c_void_p(1 << 20)   # a non-NULL pointer that no call below may dereference: every call fails validation or has no work


def test_new_symbols_are_declared_exported_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    for name, val in (("DINER_ACT_NONE", _lib.ACT_NONE), ("DINER_ACT_RELU", _lib.ACT_RELU), ("DINER_ACT_SOFTPLUS", _lib.ACT_SOFTPLUS)):
        assert re.search(rf"#define {name} {val}\b", header), name
    assert lib.diner_version() == _lib.ABI_VERSION == 3


def _gemm(**kw):
    from diner_amd import _lib
    a = dict(A=FAKE, B=FAKE, bias=None, S=None, C=FAKE, M=0, N=64, K=64, sam=64, sak=1, sbk=1, sbn=64, ldc=64, lds=0, act_a=0, act_b=0,
             act_s=0, beta=1.0, accumulate=0, atomic=0, k_chunk=0)
    a.update(kw)
    return _lib.lib().diner_train_gemm_act(*a.values(), None)


def test_gemm_act_accepts_valid_arguments_without_work():
    assert _gemm() == 0                                    # M = 0: nothing to launch
    assert _gemm(act_a=2, act_s=2, beta=100.0) == 0


@pytest.mark.parametrize("kw, what", [
    (dict(act_a=3), "activation"), (dict(act_b=-1), "activation"), (dict(act_s=7), "activation"),
    (dict(act_a=2, beta=0.0), "beta"), (dict(act_s=2, beta=-1.0), "beta"), (dict(act_b=2, beta=float("nan")), "beta"),
    (dict(N=62), "N % 4"), (dict(k_chunk=48), "k_chunk"), (dict(A=None), "NULL"),
    (dict(sak=2, sam=2), "contiguous"), (dict(K=62), "multiples of 4"),
])
def test_gemm_act_rejects_bad_arguments(kw, what):
    from diner_amd import _lib
    assert _gemm(**kw) == -1
    assert what in _lib.lib().diner_last_error().decode()


def _scene(**kw):
    from diner_amd import _lib
    s = _lib.DinerScene()
    s.SB, s.NV, s.H, s.W, s.h, s.w, s.C, s.num_freqs = 1, 2, 8, 8, 4, 4, 256, 4
    s.image_w, s.image_h, s.feature_padding, s.freq_factor = 8.0, 8.0, 0.0, 6.28
    s.poses = s.focal = s.c = s.maps = s.latent = FAKE.value
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _inputs(fn, sc, ld_in, index=None, NR=0):
    from diner_amd import _lib
    lib = _lib.lib()
    ix = C.byref(index) if index is not None else None
    if fn == "forward":
        return lib.diner_train_point_inputs_gen(C.byref(sc), ix, FAKE, FAKE, FAKE, NR, 4, 0, FAKE, ld_in, FAKE, FAKE, None)
    return lib.diner_train_point_inputs_backward_gen(C.byref(sc), ix, FAKE, FAKE, FAKE, NR, 4, 0, FAKE, ld_in, FAKE, None, FAKE, None, None,
                                                     None, None, None, None, None)


@pytest.mark.parametrize("fn", ["forward", "backward"])
def test_point_inputs_validation(fn):
    from diner_amd import _lib
    lib = _lib.lib()
    assert _inputs(fn, _scene(), 40) == 0                   # F = 4: 39 inputs in 40 columns; NR = 0: no work
    assert _inputs(fn, _scene(num_freqs=63), 512) == 0
    assert _inputs(fn, _scene(), 36) == -1 and "ld_in" in lib.diner_last_error().decode()
    assert _inputs(fn, _scene(), 42) == -1                  # not a multiple of 4
    assert _inputs(fn, _scene(num_freqs=0), 40) == -3 and "num_freqs" in lib.diner_last_error().decode()
    assert _inputs(fn, _scene(num_freqs=64), 1024) == -3
    for C_ in (12, 1032, 0):
        assert _inputs(fn, _scene(C=C_), 40) == -3 and "latent width" in lib.diner_last_error().decode()
    assert _inputs(fn, _scene(), 40, index=_lib.DinerLatentIndex(2, 0)) == -1
    assert _inputs(fn, _scene(), 40, index=_lib.DinerLatentIndex(1, 1)) == 0
    assert _inputs(fn, _scene(SB=1), 40, NR=-1) == -1


def _stub(dims, NV=1, C_lat=512, grad=True):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(8, 8, NV, seed=0, feature_padding=2, C=C_lat)
    dims = dict(dims)
    F = dims.pop("num_freqs", 6)
    d = {k: v for k, v in dims.items() if k != "beta"}
    w = synth.make_mlp_weights(1, d_in=7 + 8 * F, d_latent=C_lat, **d)
    m = model_from_scene(sc, w, device="cpu", num_freqs=F, d_latent=C_lat, **dims)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(grad)
    return m


def test_switch_is_off_by_default_and_the_raise_names_it():
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1)
    assert r.train_any_shape is False
    m = _stub(dict(d_hidden=64, n_blocks=2, combine_layer=1))
    with pytest.raises(NotImplementedError, match="inference") as e:
        r(m, torch.zeros(1, 2, 8))
    assert "train_any_shape" in str(e.value)
    assert NeRFRendererDGS(train_any_shape=True).train_any_shape is True


@pytest.fixture
def recorded(monkeypatch):
    """the renderer with its device work replaced: CPU rays pass, _scene returns a bare scene, training_gen.render_with_grad records
    its call"""
    from diner_amd import NeRFRendererDGS, _lib, training_gen
    calls = []

    def scene(self, model, need_latent=True, packed_mlp=None):
        sc = _lib.DinerScene()
        sc.SB, sc.NV = model.encoder.latent.shape[:2]
        return sc, ()

    def render(renderer, model, rays, z, scene, shape, keep=None):
        calls.append(dict(shape=shape, C=scene.C, z=z))
        SB, NR, K = z.shape
        g = rays.sum() * 0 if rays.requires_grad else torch.zeros(())
        return torch.zeros(SB, NR, 3) + g, torch.zeros(SB, NR) + g, torch.zeros(SB, NR, K) + g

    monkeypatch.setattr(NeRFRendererDGS, "_check_rays", staticmethod(lambda rays: rays))
    monkeypatch.setattr(NeRFRendererDGS, "_scene", scene)
    monkeypatch.setattr(training_gen, "render_with_grad", render)
    return calls


def test_switch_on_dispatches_forward_and_composite_to_training_gen(recorded):
    from diner_amd import NeRFRendererDGS
    from diner_amd.renderer import MlpShape
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1, train_any_shape=True)
    r.precision = "fp32"
    m = _stub(dict(d_hidden=64, n_blocks=2, combine_layer=1, beta=50.0), C_lat=256)
    z = torch.linspace(1.0, 2.0, 4).expand(1, 2, 4).contiguous()
    out = r(m, torch.zeros(1, 2, 8), want_weights=True, z_samples=z)
    assert r.last_route == "train_gen" and r.effective_precision == "fp32"
    assert out.fine.rgb.shape == (1, 2, 3) and out.fine.weights.shape == (1, 2, 4)
    assert recorded[-1]["shape"] == MlpShape(55, 256, 64, 2, 1, 6, 50.0) and recorded[-1]["C"] == 256
    r.last_route = None
    w_, rgb, depth = r.composite(m, torch.zeros(1, 2, 8), z)
    assert len(recorded) == 2 and r.last_route == "train_gen"
    # the standard model keeps the standard path unless forced (test-only switch)
    std = _stub({})
    r._force_gen_train = True
    r(std, torch.zeros(1, 2, 8), z_samples=z)
    assert len(recorded) == 3 and recorded[-1]["shape"].standard


def test_switch_on_f16x3_warns_once_and_settles_on_fp32(recorded):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1, train_any_shape=True)
    assert r.precision == "f16x3"
    m = _stub(dict(d_hidden=64, n_blocks=2, combine_layer=1))
    z = torch.linspace(1.0, 2.0, 4).expand(1, 2, 4).contiguous()
    with pytest.warns(UserWarning, match="precision="):
        r(m, torch.zeros(1, 2, 8), z_samples=z)
    assert r.effective_precision == "fp32"


def test_switch_on_out_of_envelope_shapes_still_raise(recorded):
    from diner_amd import NeRFRendererDGS
    r = NeRFRendererDGS(n_samples=4, n_depth_candidates=8, n_gaussian=1, train_any_shape=True)
    for dims in (dict(d_hidden=48, n_blocks=2, combine_layer=1), dict(d_hidden=64, n_blocks=65, combine_layer=1)):
        with pytest.raises(NotImplementedError, match="outside"):
            r(_stub(dims), torch.zeros(1, 2, 8), z_samples=torch.ones(1, 2, 4))
    assert not recorded


def test_no_mean_over_several_views_raises_before_device_work():
    from diner_amd import _lib, training_gen
    from diner_amd.renderer import MlpShape, NeRFRendererDGS
    sc = _lib.DinerScene()
    sc.SB, sc.NV = 1, 2
    with pytest.raises(NotImplementedError, match="pixelnerf.py:137"):
        training_gen.render_with_grad(NeRFRendererDGS(), None, None, None, sc, MlpShape(55, 512, 128, 5, 1000, 6))


def test_parameter_order_follows_the_model():
    from diner_amd import training_gen
    from diner_amd.renderer import NeRFRendererDGS
    for dims in (dict(d_hidden=64, n_blocks=3, combine_layer=1), dict(d_hidden=64, n_blocks=2, combine_layer=0),
                 dict(d_hidden=64, n_blocks=2, combine_layer=1000)):
        m = _stub(dims)
        ps = training_gen.mlp_params(m.mlp_fine)
        assert {id(p) for p in ps} == {id(p) for p in m.mlp_fine.parameters()} and len(ps) == len(list(m.mlp_fine.parameters()))
        lay = training_gen._Layout(NeRFRendererDGS._validate_model(m))
        assert ps[lay.out] is m.mlp_fine.lin_out.weight and len(ps) == lay.out + 2
        assert ps[lay.blk(1)] is m.mlp_fine.blocks[1].fc_0.weight
        if lay.nlz:
            assert ps[lay.lz(lay.nlz - 1)] is m.mlp_fine.lin_z[lay.nlz - 1].weight


@pytest.mark.parametrize("name", TRAINSHAPE_FIXTURES)
def test_fixture_digests_match_the_generator(name):
    from tools.gen_trainshape_golden import CASES, case_inputs, input_digests
    path = GOLDEN / f"{name}.npz"
    assert path.stat().st_size <= 300_000
    data = np.load(path, allow_pickle=False)
    cfg = json.loads(str(data["config"]))
    assert cfg == json.loads(json.dumps(CASES[name]))
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    NR, K = rays.shape[1], cfg["K"]
    assert data["z_fill"].shape == (1, NR, K) and data["rgb"].shape == (1, NR, 3)
    assert all(f"g_norm/{k}" in data.files for k in w)
    assert ("grad/rays" in data.files) == cfg["leaves"]


SHARED_SCAFFOLDING = ["_p", "_st", "prepare_latent", "remember_versions", "check_versions", "composite_backward", "camera_grad_buffers",
                      "latent_grad_out", "camera_grads_out", "camera_leaves", "camera_inputs"]


def test_both_autograd_functions_share_one_scaffolding():
    """training_gen takes the pieces around the layer schedule from training (the same function objects): no second copy to keep in step."""
    from diner_amd import training, training_gen
    for name in SHARED_SCAFFOLDING:
        assert getattr(training_gen, name) is getattr(training, name), name
