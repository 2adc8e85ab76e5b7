"""Host-side checks of the NOVEL point model's training path (no GPU): the two new entry points and what they refuse before any launch,
the ``novel_train_*`` fixtures (the unmodified reference's autograd, tools/gen_novel_train_golden.py) against the torch restatement of
tests/novel_train_ref.py in float64 and float32 at the bars the GPU tests use -- and that they reject a wrong restatement --, and the
routing of ``composite()`` with the two new constructor keywords."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import novel_point_ref as R
from tests import novel_train_ref as TR
from tools.gen_novel_train_golden import CASES, GEN_GRAD_WHOLE_BYTES, cotangent

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
POINTS, SCATTER = "diner_train_point_inputs_novel", "diner_train_novel_gen_scatter"


def _reads_latents(cfg):
    return min(cfg["mlp"].get("combine_layer", 1000), cfg["mlp"]["n_blocks"]) > 0


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name, nargs in ((POINTS, 15), (SCATTER, 9)):
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m and hasattr(lib, name) and name in _lib.SYMBOLS, name
        assert m.group(1).count(",") + 1 == nargs == len(_lib.SYMBOLS[name][1]), name
    assert lib.diner_version() == _lib.ABI_VERSION == 3
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3


# ---- refusals, without a device ------------------------------------------------------------------------------------------------------------
def _scene_and_gen(C_scene=64, C_gen=64, NV=2, h_g=28, w_g=20):
    from diner_amd import _lib
    sc = _lib.DinerScene()
    sc.SB, sc.NV, sc.H, sc.W, sc.h, sc.w, sc.C, sc.num_freqs = 2, NV, 2, 2, 2, 2, C_scene, 6
    sc.image_w = sc.image_h = 2.0
    sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 16   # non-NULL dummies, never dereferenced (P = 0 or refused earlier)
    g = _lib.DinerNovelGen()
    g.latent = g.poses = g.focal = g.c = 16
    g.h, g.w, g.C, g.image_w, g.image_h = h_g, w_g, C_gen, 40.0, 56.0
    return sc, g


def _points(sc, g, ix=None, P=0, sb=1, ld_in=56, null=(), gen=True):
    from diner_amd import _lib
    lib = _lib.lib()
    a = {k: (None if k in null else C.c_void_p(16)) for k in ("latent", "xyz_in", "xyz_gen", "viewdirs", "in_out", "zlat", "taps", "gen_taps")}
    rc = lib.diner_train_point_inputs_novel(C.byref(sc), None if ix is None else C.byref(ix), a["latent"], C.byref(g) if gen else None,
                                            a["xyz_in"], a["xyz_gen"], a["viewdirs"], P, sb, a["in_out"], ld_in, a["zlat"], a["taps"],
                                            a["gen_taps"], None)
    return rc, lib.diner_last_error().decode()


def test_no_points_is_ok_without_a_launch():
    from diner_amd import _lib
    sc, g = _scene_and_gen()
    assert _points(sc, g)[0] == 0
    for interp, pad in ((0, 0), (1, 1), (0, 2), (1, 2)):                          # every 4-tap mode
        assert _points(sc, g, ix=_lib.DinerLatentIndex(interp, pad))[0] == 0
    assert _points(sc, g, null=("zlat", "taps", "gen_taps", "latent"))[0] == 0     # combine_layer 0: no latent is read


def test_point_inputs_refusals():
    from diner_amd import _lib
    sc, g = _scene_and_gen()
    rc, msg = _points(sc, g, gen=False)
    assert rc == -1 and "gen is NULL" in msg
    for k in ("xyz_in", "xyz_gen", "viewdirs", "in_out"):
        rc, msg = _points(sc, g, null=(k,))
        assert rc == -1 and "NULL" in msg, k
    for k in ("latent", "taps", "gen_taps"):                                     # needed as soon as zlat is written
        rc, msg = _points(sc, g, null=(k,))
        assert rc == -1 and "NULL" in msg, k
    rc, msg = _points(sc, g, P=-1)
    assert rc == -1 and "bad P" in msg
    rc, msg = _points(sc, g, ix=_lib.DinerLatentIndex(3, 0))
    assert rc == -1 and "interp=3" in msg
    rc, msg = _points(sc, g, ix=_lib.DinerLatentIndex(0, 3))
    assert rc == -1 and "padding=3" in msg
    rc, msg = _points(sc, g, ix=_lib.DinerLatentIndex(2, 0))                      # where bicubic would sit: not served
    assert rc == -3 and "bicubic" in msg
    rc, msg = _points(sc, g, sb=2)
    assert rc == -1 and "sb 2" in msg
    rc, msg = _points(sc, g, ld_in=52)
    assert rc == -1 and "ld_in" in msg
    sc, g = _scene_and_gen(C_gen=128)
    rc, msg = _points(sc, g)
    assert rc == -1 and "general latent channels C=128 != latent channels C=64" in msg
    for kw in (dict(h_g=0), dict(w_g=0)):
        sc, g = _scene_and_gen(**kw)
        rc, msg = _points(sc, g)
        assert rc == -1 and "general latent size" in msg


def test_gen_scatter_refusals():
    from diner_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(16)
    assert lib.diner_train_novel_gen_scatter(p, p, 0, 64, 28, 20, 3, p, None) == 0          # no points: nothing is launched
    for args in ((None, p, 0, 64, 28, 20, 3, p), (p, None, 0, 64, 28, 20, 3, p), (p, p, 0, 64, 28, 20, 3, None), (p, p, -1, 64, 28, 20, 3, p),
                 (p, p, 0, 0, 28, 20, 3, p), (p, p, 0, 64, 0, 20, 3, p), (p, p, 0, 64, 28, 0, 3, p), (p, p, 0, 64, 28, 20, 0, p)):
        assert lib.diner_train_novel_gen_scatter(*args, None) == -1, args
        assert "train_novel_gen_scatter" in lib.diner_last_error().decode()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_grid():
    grid = {n: (c["scene"]["NV"], c["scene"]["C"], c["SB"], c["mlp"]["d_hidden"], c["mlp"]["n_blocks"], c["mlp"]["combine_layer"],
                c["index_interp"], c["index_padding"], c["P"]) for n, c in CASES.items()}
    assert grid == {"novel_train_a": (4, 64, 2, 128, 3, 2, "bilinear", "border", 70), "novel_train_b": (2, 128, 1, 64, 2, 1, "nearest", "zeros", 33),
                    "novel_train_c": (3, 64, 1, 96, 3, 2, "bilinear", "reflection", 64), "novel_train_d": (1, 1024, 1, 64, 2, 1000, "bilinear", "border", 5),
                    "novel_train_e": (3, 256, 1, 96, 2, 0, "bilinear", "border", 1), "novel_train_std": (4, 512, 1, 512, 5, 3, "bilinear", "border", 40)}
    assert CASES["novel_train_b"]["mlp"]["beta"] == 100.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_matches_the_seeded_inputs(name):
    inp, data = TR.load(name)                                                     # (config and digests are checked there)
    cfg = CASES[name]
    assert (GOLDEN / f"{name}.npz").stat().st_size < 1_000_000
    assert data["rgbsigma"].shape == (cfg["SB"], cfg["P"], 4) and data["rgbsigma"].dtype == np.float32
    whole = inp["gen_latent"].nbytes <= GEN_GRAD_WHOLE_BYTES
    assert ("gen_grad" in data) == whole
    if whole:
        assert data["gen_grad"].shape == inp["gen_latent"].shape
        assert abs(float(np.abs(data["gen_grad"]).max()) - float(data["gen_grad_max"])) <= 1e-6 * float(data["gen_grad_max"])
    if _reads_latents(cfg):
        assert float(data["latent_grad_norm"]) > 0 and float(data["gen_grad_norm"]) > 0
    else:
        assert float(data["latent_grad_norm"]) == 0 and float(data["gen_grad_norm"]) == 0
    assert float(data["rgbsigma"][..., 3].max()) > 0                              # the relu gate of sigma is open somewhere
    assert cotangent(cfg).shape == data["rgbsigma"].shape
    if cfg["SB"] > 1:
        assert not np.array_equal(inp["gen_poses"][0], inp["gen_poses"][1])


# ---- restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_gradients(name, dtype):
    inp, data = TR.load(name)
    TR.check_fixture(TR.reference_grads(inp, dtype), data, CASES[name], label=f"{name} {dtype}")


def test_restated_forward_is_the_point_model_restatement():
    inp, _ = TR.load("novel_train_c")
    m = R.model_from_inputs(inp, device="cpu")
    t = lambda k: torch.from_numpy(inp[k])
    with torch.no_grad():
        want = m(t("xyz_in"), t("xyz_gen"), viewdirs=t("viewdirs")).numpy()
    assert np.array_equal(TR.reference_grads(inp, torch.float32)["rgbsigma"], want)


@pytest.mark.parametrize("variant", TR.WRONG_VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_wrong_restatement_is_rejected(name, variant):
    """the view sum left out of gen_latent's gradient (the forward is right: only that gradient is wrong, wherever there is more than one
    view); the general lookup's feature_padding scaled by the encoder map's size: each is rejected wherever the model reads the latents"""
    inp, data = TR.load(name)
    cfg = CASES[name]
    matters = _reads_latents(cfg) and (variant != "gen_grad_one_view" or cfg["scene"]["NV"] > 1)
    got = TR.reference_grads(inp, torch.float64, variant)
    if not matters:
        return TR.check_fixture(got, data, cfg, label=f"{name} {variant}")
    with pytest.raises(AssertionError) as e:
        TR.check_fixture(got, data, cfg, label=f"{name} {variant}")
    assert "gen grad" in str(e.value)
    if variant == "gen_grad_one_view":                                           # nothing but gen_latent's gradient is wrong
        assert all(what.startswith("gen grad") for what, _, _ in e.value.args[0])


# ---- the shared layer schedule -------------------------------------------------------------------------------------------------------------
def test_both_autograd_functions_call_the_lifted_schedule():
    from diner_amd import training_gen, training_novel
    for fn in (training_gen._RenderGenFn, training_novel._RenderNovelFn):
        src = inspect.getsource(fn)
        assert "schedule_forward(" in src and "schedule_backward(" in src and "range(lay.nb)" not in src, fn


# ---- routing -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_composite(monkeypatch):
    """composite() with its device steps replaced (tests/test_novel_point_host.py's stubs): the point kernels record their calls"""
    from diner_amd import novel

    def run(r, model, grad=False):
        SB, B, K = 1, 3, 2
        calls = dict(infer=0, train=0)
        monkeypatch.setattr(r, "_check_rays", lambda rays: rays)
        monkeypatch.setattr(r, "_poll_status", lambda *a, **k: None)
        monkeypatch.setattr(r, "_status_word", lambda dev: None)
        monkeypatch.setattr(r, "_after_launch", lambda *a, **k: None)
        monkeypatch.setattr(novel.deform, "deform_ray_points",
                            lambda rays, z, *a, return_points=False, **k: tuple(torch.zeros(SB, B * K, 3) for _ in range(3 if return_points else 2)))
        monkeypatch.setattr(novel._CompositeFn, "apply", staticmethod(lambda out, *a: (out, None, None)))

        def infer(m, a, b, d):
            calls["infer"] += 1
            return torch.zeros(SB, B * K, 4)

        def train(r_, m, a, b, d, shape, f16=False):
            calls["train"] += 1
            calls["f16"] = f16
            return torch.zeros(SB, B * K, 4)
        monkeypatch.setattr(r, "render_points_novel", infer)
        from diner_amd import training_novel
        monkeypatch.setattr(training_novel, "render_points_with_grad", train)
        with torch.enable_grad() if grad else torch.no_grad():
            r.composite(model, torch.zeros(SB, B, 8), torch.zeros(SB, B, K), None, None, None)
        return calls
    return run


class _Fake(R.NovelPointModel):
    def forward(self, *pts, viewdirs=None):
        self.calls += 1
        return torch.zeros(*pts[0].shape[:2], 4)


def _fake(grad=("gen_latent",)):
    m = R.model_from_inputs(TR.load("novel_train_e")[0], device="cpu")
    m.__class__ = _Fake
    if "gen_latent" in grad:
        m.gen_latent.requires_grad_(True)
    if "mlp" in grad:
        m.mlp_fine.lin_out.bias.requires_grad_(True)
    if "latent" in grad:
        m.encoder.latent = m.encoder.latent.clone().requires_grad_(True)
    return m


def test_the_keywords_exist_and_default_off():
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS()
    assert r.train_hip_point_model is False and r.train_f16x3_any_shape is False
    r = NeRFRendererDGS(train_hip_point_model=True, train_f16x3_any_shape=True)
    assert r.train_hip_point_model is True and r.train_f16x3_any_shape is True and r.hip_point_model is False


def test_routing_of_composite_under_autograd(host_composite):
    from diner_amd.novel import NeRFRendererDGS
    on = lambda **kw: NeRFRendererDGS(hip_point_model=True, train_hip_point_model=True, **kw)
    # each of the three kinds of trainable tensor takes the new route
    for grad in (("gen_latent",), ("mlp",), ("latent",)):
        r, m = on(), _fake(grad)
        r.precision = "fp32"
        c = host_composite(r, m, grad=True)
        assert c["train"] == 1 and c["infer"] == 0 and m.calls == 0 and c["f16"] is False, grad
        assert r.last_route == "novel_train_gen" and r.effective_precision == "fp32" and r.last_binding == "ctypes"
    # f16x3 needs the precision and the plain renderer's switch
    r, m = on(train_f16x3_any_shape=True), _fake()
    assert r.precision == "f16x3"
    c = host_composite(r, m, grad=True)
    assert c["train"] == 1 and c["f16"] is True and r.last_route == "novel_train_gen_f16" and r.effective_precision == "f16x3"
    r = on()
    with pytest.warns(UserWarning, match="train_f16x3_any_shape"):
        c = host_composite(r, m, grad=True)
    assert c["f16"] is False and r.last_route == "novel_train_gen" and r.effective_precision == "fp32"
    # under no_grad, or with nothing that requires grad: the inference kernel, as before
    c = host_composite(r, m)
    assert c["infer"] == 1 and c["train"] == 0 and m.calls == 0
    c = host_composite(r, _fake(grad=()), grad=True)
    assert c["infer"] == 1 and c["train"] == 0


def test_every_pinned_route_stays(host_composite):
    from diner_amd.novel import NeRFRendererDGS
    torch_route = lambda r, m, **kw: (host_composite(r, m, **kw), r.last_route)
    # train_hip_point_model off (the default): a model that requires grad goes to PyTorch
    r, m = NeRFRendererDGS(hip_point_model=True), _fake()
    assert torch_route(r, m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 1
    # train_hip_point_model without hip_point_model: PyTorch
    r, m = NeRFRendererDGS(train_hip_point_model=True), _fake()
    assert torch_route(r, m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 1
    on = lambda **kw: NeRFRendererDGS(hip_point_model=True, train_hip_point_model=True, **kw)
    # a bicubic encoder, with and without the plain renderer's bicubic switch
    m = _fake()
    m.encoder.index_interp = "bicubic"
    r = on()
    assert torch_route(r, m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 1
    r.bicubic_index = True
    assert torch_route(r, m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 2
    # another callable
    seen = []
    fn = lambda a, b, viewdirs=None: seen.append(1) or torch.zeros(*a.shape[:2], 4)
    assert torch_route(on(), fn, grad=True) == (dict(infer=0, train=0), "torch") and seen == [1]
    # pass_points (NOVEL_PE's renderer), and NOVEL_PE's model
    m = _fake()
    assert torch_route(on(pass_points=True), m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 1
    m = _fake()
    m.deformation_layer = torch.nn.Linear(3, 3)
    assert torch_route(on(), m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 1
    # a fusion MLP outside the envelope
    m = _fake()
    m.mlp_fine.d_hidden = 48
    assert torch_route(on(), m, grad=True) == (dict(infer=0, train=0), "torch") and m.calls == 1


def test_data_that_requires_grad_is_still_refused():
    from diner_amd.novel import NeRFRendererDGS
    r, m = NeRFRendererDGS(hip_point_model=True, train_hip_point_model=True), _fake()
    z = torch.zeros(1, 3, 2)
    for kw in (dict(rays=torch.zeros(1, 3, 8, requires_grad=True)), dict(z=z.clone().requires_grad_(True)),
               dict(v=torch.zeros(1, 4, 3, requires_grad=True)), dict(oi=torch.zeros(1, 4, 3, requires_grad=True)),
               dict(og=torch.zeros(1, 4, 3, requires_grad=True))):
        a = dict(rays=torch.zeros(1, 3, 8), z=z, v=None, oi=None, og=None)
        a.update(kw)
        with pytest.raises(NotImplementedError, match="requires grad"):
            r.composite(m, a["rays"], a["z"], a["v"], a["oi"], a["og"])
