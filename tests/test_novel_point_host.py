"""Host-side checks of the NOVEL point model on the shape-general kernels (no GPU): the new entry point and what it refuses before any
launch, the seeded inputs of the ``novel_point_*`` fixtures, the torch restatement of tests/novel_point_ref.py against what the
unmodified reference recorded (and that the fixtures reject a wrong restatement), and the routing of ``composite()``."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import novel_point_ref as R
from tools.gen_novel_point_golden import CASES, case_inputs, input_digests, outside_fraction

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NAME = "diner_render_points_novel"
BOUND = 1e-4      # rgb abs; sigma relative to max(1, sigma / 12): the bars of tests/test_gpu_mlp_shapes*.py

_inputs = {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = case_inputs(CASES[name])
    return _inputs[name]


def restate(inp, dtype, variant=None):
    cfg, d = inp["cfg"], inp["dims"]
    keys = ("poses", "focal", "c", "image_shape", "depths", "latent", "gen_latent", "gen_poses", "gen_focal", "gen_c", "gen_image_shape", "weights")
    return R.novel_point_forward(torch.from_numpy(inp["xyz_in"]).to(dtype), inp["xyz_gen"], inp["viewdirs"], **{k: inp[k] for k in keys},
                                 n_blocks=d["n_blocks"], combine_layer=d["combine_layer"], beta=d["beta"], num_freqs=cfg["num_freqs"],
                                 freq_factor=6.28, feature_padding=cfg["scene"]["feature_padding"], index_interp=cfg["index_interp"],
                                 index_padding=cfg["index_padding"], variant=variant).numpy()


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound_and_the_abi_is_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    m = re.search(rf"\bint {NAME}\(([^;]*)\);", header)
    lib = _lib.lib()
    assert m and hasattr(lib, NAME) and NAME in _lib.SYMBOLS
    assert m.group(1).count(",") + 1 == 12 == len(_lib.SYMBOLS[NAME][1])
    assert "typedef struct DinerNovelGen" in header and C.sizeof(_lib.DinerNovelGen) == 56
    assert lib.diner_version() == _lib.ABI_VERSION == 3
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3


# ---- refusals, without a device ------------------------------------------------------------------------------------------------------------
def _shape(**kw):
    from diner_amd import _lib
    d = dict(d_in=55, d_latent=512, d_hidden=128, n_blocks=5, combine_layer=3, num_freqs=6, beta=0.0, d_out=4, combine_type=0)
    d.update(kw)
    return _lib.DinerMlpShape(*[d[f] for f, _ in _lib.DinerMlpShape._fields_])


def _scene_and_gen(C_scene=512, C_gen=512, NV=2, h_g=28, w_g=20):
    from diner_amd import _lib
    sc = _lib.DinerScene()
    sc.SB, sc.NV, sc.H, sc.W, sc.h, sc.w, sc.C, sc.num_freqs = 1, NV, 2, 2, 2, 2, C_scene, 6
    sc.image_w = sc.image_h = 2.0
    sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 16   # non-NULL dummies, never dereferenced (P = 0 or refused earlier)
    g = _lib.DinerNovelGen()
    g.latent = g.poses = g.focal = g.c = 16
    g.h, g.w, g.C, g.image_w, g.image_h = h_g, w_g, C_gen, 40.0, 56.0
    return sc, g


def _call(sc, g, sh, ix=None, P=0, precision=0):
    from diner_amd import _lib
    lib = _lib.lib()
    rc = lib.diner_render_points_novel(C.byref(sc), None if ix is None else C.byref(ix), C.byref(g), C.byref(sh), C.c_void_p(16), None, None,
                                       None, P, precision, None, None)
    return rc, lib.diner_last_error().decode()


def test_no_points_is_ok_without_a_launch():
    sc, g = _scene_and_gen()
    assert _call(sc, g, _shape())[0] == 0
    assert _call(sc, g, _shape(), precision=1)[0] == 0


def test_latent_channels_must_equal_d_latent():
    sc, g = _scene_and_gen(C_gen=256)
    rc, msg = _call(sc, g, _shape())
    assert rc == -1 and "general latent channels C=256 != d_latent=512" in msg
    sc, g = _scene_and_gen(C_scene=256)
    rc, msg = _call(sc, g, _shape())
    assert rc == -1 and "latent channels C=256 != d_latent=512" in msg


def test_general_latent_size_must_be_positive():
    for kw in (dict(h_g=0), dict(w_g=0)):
        sc, g = _scene_and_gen(**kw)
        rc, msg = _call(sc, g, _shape())
        assert rc == -1 and "general latent size" in msg


@pytest.mark.parametrize("kw, what", [(dict(d_hidden=48), "d_hidden=48"), (dict(d_hidden=544), "d_hidden=544"), (dict(d_latent=1032), "d_latent=1032"),
                                      (dict(d_out=5), "d_out=5")])
def test_out_of_envelope_shape_is_unsupported(kw, what):
    sc, g = _scene_and_gen()
    rc, msg = _call(sc, g, _shape(**kw))
    assert rc == -3 and what in msg


def test_no_mean_over_views_needs_one_view():
    sc, g = _scene_and_gen(NV=2)
    rc, msg = _call(sc, g, _shape(combine_layer=1000))
    assert rc == -3 and "novel_pixelnerf.py:234" in msg
    sc, g = _scene_and_gen(NV=1)
    assert _call(sc, g, _shape(combine_layer=1000))[0] == 0


def test_bicubic_index_and_unknown_precision_are_refused():
    """DinerLatentIndex carries the 4-tap modes only: a value past DINER_INDEX_NEAREST (where bicubic would sit) is refused"""
    from diner_amd import _lib
    sc, g = _scene_and_gen()
    rc, msg = _call(sc, g, _shape(), ix=_lib.DinerLatentIndex(2, 0))
    assert rc == -1 and "interp=2" in msg and "render_points_novel" in msg
    for interp, pad in ((0, 0), (1, 1), (0, 2)):
        assert _call(sc, g, _shape(), ix=_lib.DinerLatentIndex(interp, pad))[0] == 0
    rc, msg = _call(sc, g, _shape(), precision=2)
    assert rc == -1 and "precision=2" in msg
    # and the Python entry refuses a bicubic encoder by name, before it reads anything else
    from diner_amd.novel import NeRFRendererDGS
    m = R.model_from_inputs(inputs("novel_point_e"), device="cpu")
    m.encoder.index_interp = "bicubic"
    r = NeRFRendererDGS(hip_point_model=True)
    r.bicubic_index = True
    x = torch.zeros(1, 1, 3)
    with pytest.raises(NotImplementedError, match="bicubic"):
        r.render_points_novel(m, x, x, x)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_digests_match_the_seeded_inputs(name):
    inp, g = inputs(name), np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    cfg = CASES[name]
    assert sorted(g.files) == ["config", "digests", "rgbsigma"]                 # digests and the reference's output only
    assert json.loads(str(g["config"])) == json.loads(json.dumps(cfg))
    assert json.loads(str(g["digests"])) == input_digests(inp)
    assert g["rgbsigma"].shape == (cfg["SB"], cfg["P"], 4) and g["rgbsigma"].dtype == np.float32
    assert not np.array_equal(inp["xyz_in"], inp["xyz_gen"])
    assert inp["gen_latent"].shape[1:] != inp["latent"].shape[3:] and inp["gen_latent"].shape[1] != inp["gen_latent"].shape[2]
    if cfg["P"] >= 64:
        assert 0.05 <= outside_fraction(inp) <= 0.2                              # about a tenth of the general projections leave the map
    if cfg["SB"] > 1:
        assert not np.array_equal(inp["gen_poses"][0], inp["gen_poses"][1]) and not np.array_equal(inp["gen_focal"][0], inp["gen_focal"][1])


def test_the_cases_cover_the_grid():
    shapes = {n: (c["mlp"]["d_hidden"], c["index_interp"], c["index_padding"], c["SB"], c["scene"]["NV"], c["P"]) for n, c in CASES.items()}
    assert shapes == {"novel_point_a": (512, "bilinear", "border", 2, 4, 200), "novel_point_b": (128, "nearest", "zeros", 1, 2, 65),
                      "novel_point_c": (256, "bilinear", "reflection", 1, 3, 64), "novel_point_d": (64, "bilinear", "border", 1, 1, 130),
                      "novel_point_e": (96, "bilinear", "border", 1, 3, 1)}
    assert CASES["novel_point_d"]["scene"]["C"] == 1024 and CASES["novel_point_e"]["mlp"]["combine_layer"] == 0
    assert CASES["novel_point_c"]["mlp"]["beta"] > 0


# ---- restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name, dtype):
    ref = np.load(GOLDEN / f"{name}.npz")["rgbsigma"]
    e_rgb, e_sigma = R.rgbsigma_errors(restate(inputs(name), dtype), ref)
    print(f"{name} {dtype}: |rgb| {e_rgb:.2e}, |sigma| {e_sigma:.2e}")
    assert e_rgb <= BOUND and e_sigma <= BOUND
    assert float(ref[..., 3].max()) > 0


@pytest.mark.parametrize("variant", R.WRONG_VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_wrong_restatement_is_rejected(name, variant):
    """the gen lookup dropped, xyz_gen and xyz_in swapped, the gen latent added once instead of per view: each misses the bound by
    orders of magnitude wherever the model reads what the variant changes"""
    cfg = CASES[name]
    reads_latents = min(cfg["mlp"]["combine_layer"], cfg["mlp"]["n_blocks"]) > 0
    matters = variant == "swapped" or (reads_latents and (variant == "no_gen" or cfg["scene"]["NV"] > 1))
    ref = np.load(GOLDEN / f"{name}.npz")["rgbsigma"]
    e_rgb, e_sigma = R.rgbsigma_errors(restate(inputs(name), torch.float64, variant), ref)
    if matters:
        assert e_rgb > 1000 * BOUND, (e_rgb, e_sigma)
    else:
        assert e_rgb <= BOUND and e_sigma <= BOUND


def test_stand_in_model_is_the_restatement():
    inp = inputs("novel_point_c")
    m = R.model_from_inputs(inp, device="cpu")
    t = lambda k: torch.from_numpy(inp[k])
    with torch.no_grad():
        out = m(t("xyz_in"), t("xyz_gen"), viewdirs=t("viewdirs")).numpy()
    assert np.array_equal(out, restate(inp, torch.float32)) and m.calls == 1


# ---- routing -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_composite(monkeypatch):
    """composite() with its device steps replaced: the deformation returns the rays' own points twice, the compositing the model's
    output; the point kernel records its call instead of running"""
    from diner_amd import novel

    def run(r, model, grad=False):
        SB, B, K = 1, 3, 2
        kernel_calls = []
        monkeypatch.setattr(r, "_check_rays", lambda rays: rays)
        monkeypatch.setattr(r, "_poll_status", lambda *a, **k: None)
        monkeypatch.setattr(r, "_status_word", lambda dev: None)
        monkeypatch.setattr(r, "_after_launch", lambda *a, **k: None)
        monkeypatch.setattr(novel.deform, "deform_ray_points",
                            lambda rays, z, *a, return_points=False, **k: tuple(torch.zeros(SB, B * K, 3) for _ in range(3 if return_points else 2)))
        monkeypatch.setattr(novel._CompositeFn, "apply", staticmethod(lambda out, *a: (out, None, None)))
        monkeypatch.setattr(r, "render_points_novel", lambda m, a, b, d: kernel_calls.append(1) or torch.zeros(SB, B * K, 4))
        with torch.enable_grad() if grad else torch.no_grad():
            r.composite(model, torch.zeros(SB, B, 8), torch.zeros(SB, B, K), None, None, None)
        return len(kernel_calls)
    return run


class _Fake(R.NovelPointModel):
    def forward(self, *pts, viewdirs=None):
        self.calls += 1
        return torch.zeros(*pts[0].shape[:2], 4)


def _fake():
    m = R.model_from_inputs(inputs("novel_point_e"), device="cpu")
    m.__class__ = _Fake
    return m


def test_routing_of_composite(host_composite):
    from diner_amd.novel import NeRFRendererDGS
    # the switch on, inference, the NOVEL model: the kernel
    r, m = NeRFRendererDGS(hip_point_model=True), _fake()
    assert host_composite(r, m) == 1 and m.calls == 0
    # parameters that do not require grad: still the kernel with grad mode on
    assert host_composite(r, m, grad=True) == 1 and m.calls == 0
    # the switch off (the default): nothing changes
    r0 = NeRFRendererDGS()
    assert r0.hip_point_model is False
    assert host_composite(r0, m) == 0 and m.calls == 1 and r0.last_route == "torch"
    # training: a parameter requires grad under grad mode
    m = _fake()
    m.gen_latent.requires_grad_(True)
    assert host_composite(r, m, grad=True) == 0 and m.calls == 1 and r.last_route == "torch"
    assert host_composite(r, m) == 1 and m.calls == 1                            # ... and under no_grad the kernel again
    m = _fake()
    m.mlp_fine.lin_in.weight.requires_grad_(True)
    assert host_composite(r, m, grad=True) == 0 and m.calls == 1
    # pass_points (NOVEL_PE's renderer) and a deformation_layer (NOVEL_PE's model)
    m = _fake()
    assert host_composite(NeRFRendererDGS(hip_point_model=True, pass_points=True), m) == 0 and m.calls == 1
    m = _fake()
    m.deformation_layer = torch.nn.Linear(3, 3)
    assert host_composite(r, m) == 0 and m.calls == 1
    # a bicubic encoder, with and without the plain renderer's bicubic switch
    m = _fake()
    m.encoder.index_interp = "bicubic"
    assert host_composite(r, m) == 0 and m.calls == 1
    r.bicubic_index = True
    assert host_composite(r, m) == 0 and m.calls == 2 and r.last_route == "torch"
    r.bicubic_index = False
    # a callable that is not this model; a NOVEL model whose MLP lies outside the envelope
    calls = []
    fn = lambda a, b, viewdirs=None: calls.append(1) or torch.zeros(*a.shape[:2], 4)
    assert host_composite(r, fn) == 0 and calls == [1]
    m = _fake()
    m.mlp_fine.d_hidden = 48
    assert host_composite(r, m) == 0 and m.calls == 1


def test_memory_report_counts_the_general_latent():
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(hip_point_model=True)
    r._gen_latent_pack = torch.zeros(28, 20, 8)
    rep = r.memory_report()["cached"]
    assert rep["gen_latent_nhwc"] == 28 * 20 * 8 * 4
    assert rep["total"] == sum(v for k, v in rep.items() if k != "total") == rep["gen_latent_nhwc"]
