"""Host-side checks of the NOVEL_PE point model on the shape-general kernels (no GPU): the new entry points and what they refuse
before any launch, the seeded inputs of the ``novel_pe_point_*`` fixtures, the torch restatement of tests/novel_pe_point_ref.py against
what the unmodified reference recorded (and that the fixtures reject each wrong restatement), the hoisted form of the deformation
layer against the direct one, and the routing of ``composite()``."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import novel_pe_point_ref as R
from tools.gen_novel_pe_point_golden import CASES, case_inputs, input_digests, outside_fraction

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NAMES = {"diner_novel_pe_map_floats": 1, "diner_pack_novel_pe_map": 4, "diner_render_points_novel_pe": 14}
BOUND = 1e-4      # rgb abs; sigma relative to max(1, sigma / 12): the bars of tests/test_gpu_mlp_shapes*.py
KEYS = ("poses", "focal", "c", "image_shape", "depths", "latent", "pos_encodings", "gen_latent", "gen_poses", "gen_focal", "gen_c", "gen_image_shape",
        "tgt_pos_encoding", "tgt_poses", "tgt_focal", "tgt_c", "tgt_image_shape", "deform_w", "deform_b", "weights")

_inputs = {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = case_inputs(CASES[name])
    return _inputs[name]


def restate(inp, dtype, **kw):
    cfg, d = inp["cfg"], inp["dims"]
    kw = dict(dict(index_interp=cfg["index_interp"], index_padding=cfg["index_padding"]), **kw)
    return R.novel_pe_point_forward(torch.from_numpy(inp["xyz_in"]).to(dtype), inp["xyz_gen"], inp["xyz_tgt"], inp["viewdirs"],
                                    **{k: inp[k] for k in KEYS}, n_blocks=d["n_blocks"], combine_layer=d["combine_layer"], beta=d["beta"],
                                    num_freqs=cfg["num_freqs"], freq_factor=6.28, feature_padding=cfg["scene"]["feature_padding"], **kw).numpy()


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name, nargs in NAMES.items():
        m = re.search(rf"\bint(?:64_t)? {name}\(([^;]*)\);", header)
        assert m and hasattr(lib, name) and name in _lib.SYMBOLS, name
        assert m.group(1).count(",") + 1 == nargs == len(_lib.SYMBOLS[name][1]), name
    assert "typedef struct DinerNovelPe" in header and C.sizeof(_lib.DinerNovelPe) == 80
    assert C.sizeof(_lib.DinerNovelGen) == 56                                        # the NOVEL entry point's struct is untouched
    assert lib.diner_version() == _lib.ABI_VERSION == 3
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3


# ---- refusals, without a device ------------------------------------------------------------------------------------------------------------
def _shape(**kw):
    from diner_amd import _lib
    d = dict(d_in=55, d_latent=520, d_hidden=128, n_blocks=5, combine_layer=3, num_freqs=6, beta=0.0, d_out=4, combine_type=0)
    d.update(kw)
    return _lib.DinerMlpShape(*[d[f] for f, _ in _lib.DinerMlpShape._fields_])


def _structs(C_scene=512, C_gen=512, NV=2, **sizes):
    from diner_amd import _lib
    sc = _lib.DinerScene()
    sc.SB, sc.NV, sc.H, sc.W, sc.h, sc.w, sc.C, sc.num_freqs = 1, NV, 2, 2, sizes.get("h", 2), sizes.get("w", 2), C_scene, 6
    sc.image_w = sc.image_h = 2.0
    sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 16   # non-NULL dummies, never dereferenced (P = 0 or refused earlier)
    g = _lib.DinerNovelGen()
    g.latent = g.poses = g.focal = g.c = 16
    g.h, g.w, g.C, g.image_w, g.image_h = sizes.get("h_g", 28), sizes.get("w_g", 20), C_gen, 40.0, 56.0
    pe = _lib.DinerNovelPe()
    pe.map = pe.head = pe.src_pe = pe.tgt_pe = pe.poses = pe.focal = pe.c = 16
    pe.src_h, pe.src_w, pe.tgt_h, pe.tgt_w = (sizes.get(k, v) for k, v in (("src_h", 36), ("src_w", 30), ("tgt_h", 26), ("tgt_w", 34)))
    pe.image_w, pe.image_h = 48.0, 60.0
    return sc, g, pe


def _call(sc, g, pe, sh, ix=None, P=0, precision=0, packed=16):
    from diner_amd import _lib
    lib = _lib.lib()
    ref = lambda s: None if s is None else C.byref(s)
    rc = lib.diner_render_points_novel_pe(ref(sc), ref(ix), ref(g), ref(pe), ref(sh), C.c_void_p(packed), None, None, None, None, P, precision,
                                          None, None)
    return rc, lib.diner_last_error().decode()


def test_no_points_is_ok_without_a_launch():
    sc, g, pe = _structs()
    assert _call(sc, g, pe, _shape())[0] == 0
    assert _call(sc, g, pe, _shape(), precision=1)[0] == 0
    sc.SB = 0
    assert _call(sc, g, pe, _shape(), P=5)[0] == 0


def test_null_pointers_are_invalid():
    sc, g, pe = _structs()
    for args, what in (((None, g, pe, _shape()), "scene is NULL"), ((sc, None, pe, _shape()), "gen is NULL"), ((sc, g, None, _shape()), "pe is NULL"),
                       ((sc, g, pe, None), "shape is NULL")):
        rc, msg = _call(*args)
        assert rc == -1 and what in msg, msg
    rc, msg = _call(sc, g, pe, _shape(), packed=None)
    assert rc == -1 and "mlp_packed is NULL" in msg
    for field in ("map", "head", "src_pe", "tgt_pe"):
        sc, g, pe = _structs()
        setattr(pe, field, None)
        rc, msg = _call(sc, g, pe, _shape())
        assert rc == -1 and "NULL map / head / pos-encoding pointer" in msg, field
        assert _call(sc, g, pe, _shape(combine_layer=0))[0] == 0                    # ... which combine_layer 0 never reads
    sc, g, pe = _structs()
    pe.poses = None
    rc, msg = _call(sc, g, pe, _shape())
    assert rc == -1 and "NULL target camera pointer" in msg
    sc, g, pe = _structs()
    rc, msg = _call(sc, g, pe, _shape(), P=3)                                      # points / viewdirs / out are NULL in _call
    assert rc == -1 and "NULL points / viewdirs / out" in msg


def test_latent_channels_must_equal_d_latent_minus_8():
    sc, g, pe = _structs(C_gen=256)
    rc, msg = _call(sc, g, pe, _shape())
    assert rc == -1 and "general latent channels C=256 != d_latent - 8 = 512" in msg
    sc, g, pe = _structs(C_scene=520, C_gen=520)                                    # C = d_latent: the NOVEL kernel's convention, not this one's
    rc, msg = _call(sc, g, pe, _shape())
    assert rc == -1 and "latent channels C=520 != d_latent - 8 = 512" in msg


@pytest.mark.parametrize("key, what", [("h", "deformation map size"), ("w", "deformation map size"), ("h_g", "general latent size"),
                                       ("w_g", "general latent size"), ("src_h", "source pos-encoding size"), ("src_w", "source pos-encoding size"),
                                       ("tgt_h", "target pos-encoding size"), ("tgt_w", "target pos-encoding size")])
def test_map_sizes_must_be_positive(key, what):
    sc, g, pe = _structs(**{key: 0})
    rc, msg = _call(sc, g, pe, _shape())
    assert rc == -1 and what in msg


def test_negative_p_unknown_precision_and_index_are_invalid():
    from diner_amd import _lib
    sc, g, pe = _structs()
    rc, msg = _call(sc, g, pe, _shape(), P=-1)
    assert rc == -1 and "bad P" in msg
    rc, msg = _call(sc, g, pe, _shape(), precision=2)
    assert rc == -1 and "precision=2" in msg
    rc, msg = _call(sc, g, pe, _shape(), ix=_lib.DinerLatentIndex(2, 0))            # where bicubic would sit
    assert rc == -1 and "interp=2" in msg and "render_points_novel_pe" in msg
    rc, msg = _call(sc, g, pe, _shape(), ix=_lib.DinerLatentIndex(0, 3))
    assert rc == -1 and "padding=3" in msg
    for interp, pad in ((0, 0), (1, 1), (0, 2)):
        assert _call(sc, g, pe, _shape(), ix=_lib.DinerLatentIndex(interp, pad))[0] == 0


@pytest.mark.parametrize("kw, what", [(dict(d_hidden=48), "d_hidden=48"), (dict(d_hidden=544), "d_hidden=544"), (dict(d_latent=1032), "d_latent=1032"),
                                      (dict(d_latent=518), "d_latent=518"), (dict(d_out=5), "d_out=5")])
def test_out_of_envelope_shape_is_unsupported(kw, what):
    """C = 1024 would need d_latent = 1032; the unpadded C + 6 is refused like everywhere else"""
    sc, g, pe = _structs(C_scene=kw.get("d_latent", 520) - 8, C_gen=kw.get("d_latent", 520) - 8)
    rc, msg = _call(sc, g, pe, _shape(**kw))
    assert rc == -3 and what in msg


def test_no_mean_over_views_needs_one_view():
    sc, g, pe = _structs(NV=2)
    rc, msg = _call(sc, g, pe, _shape(combine_layer=1000))
    assert rc == -3 and "pe_novel_pixelnerf.py:284" in msg
    sc, g, pe = _structs(NV=1)
    assert _call(sc, g, pe, _shape(combine_layer=1000))[0] == 0


def test_map_builder_refusals():
    from diner_amd import _lib
    lib = _lib.lib()
    sc, _, _ = _structs()
    sc.h, sc.w = 24, 20
    assert lib.diner_novel_pe_map_floats(C.byref(sc)) == 1 * 2 * 24 * 20 * 512
    assert lib.diner_novel_pe_map_floats(None) == -1 and "scene is NULL" in lib.diner_last_error().decode()
    assert lib.diner_pack_novel_pe_map(C.byref(sc), None, C.c_void_p(16), None) == -1 and "NULL pointer" in lib.diner_last_error().decode()
    sc.C = 1024
    assert lib.diner_novel_pe_map_floats(C.byref(sc)) == -3 and "C=1024" in lib.diner_last_error().decode()
    assert lib.diner_pack_novel_pe_map(C.byref(sc), C.c_void_p(16), C.c_void_p(16), None) == -3
    sc.C = 20
    assert lib.diner_novel_pe_map_floats(C.byref(sc)) == -1 and "C=20" in lib.diner_last_error().decode()
    sc.C, sc.SB = 512, 0
    assert lib.diner_novel_pe_map_floats(C.byref(sc)) == 0
    assert lib.diner_pack_novel_pe_map(C.byref(sc), C.c_void_p(16), C.c_void_p(16), None) == 0      # no texel: nothing is launched


def test_python_entry_refuses_by_name():
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(hip_point_model=True, pass_points=True)
    x = torch.zeros(1, 1, 3)
    m = R.model_from_inputs(inputs("novel_pe_point_e"), device="cpu")
    m.encoder.index_interp = "bicubic"
    with pytest.raises(NotImplementedError, match="bicubic"):
        r.render_points_novel_pe(m, x, x, x, x)
    m = R.model_from_inputs(inputs("novel_pe_point_e"), device="cpu")
    m.tgt_poses = None
    with pytest.raises(TypeError, match="tgt_poses"):
        r.render_points_novel_pe(m, x, x, x, x)
    m = R.NovelPePointModel(1024, d_hidden=64, n_blocks=2, combine_layer=1)          # C = 1024: C + 8 leaves the envelope
    for k in r._PE_STATE:
        if getattr(m, k, None) is None:
            setattr(m, k, torch.zeros(1))
    with pytest.raises(NotImplementedError, match="d_latent=1032"):
        r.render_points_novel_pe(m, x, x, x, x)
    # the padding happens in this route only: every other route keeps refusing C + 6
    with pytest.raises(NotImplementedError, match="d_latent=262"):
        r._validate(R.model_from_inputs(inputs("novel_pe_point_e"), device="cpu"))
    assert r._validate_pe(R.model_from_inputs(inputs("novel_pe_point_e"), device="cpu")).d_latent == 264


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_digests_match_the_seeded_inputs(name):
    inp, g = inputs(name), np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    cfg = CASES[name]
    assert sorted(g.files) == ["config", "digests", "rgbsigma"]                 # digests and the reference's output only
    assert json.loads(str(g["config"])) == json.loads(json.dumps(cfg))
    assert json.loads(str(g["digests"])) == input_digests(inp)
    assert g["rgbsigma"].shape == (cfg["SB"], cfg["P"], 4) and g["rgbsigma"].dtype == np.float32
    pts = [inp[k] for k in ("xyz_in", "xyz_gen", "xyz_tgt")]
    assert all(not np.array_equal(a, b) for i, a in enumerate(pts) for b in pts[i + 1:])
    sizes = [inp["latent"].shape[3:], inp["gen_latent"].shape[1:], inp["pos_encodings"].shape[3:], inp["tgt_pos_encoding"].shape[3:]]
    assert len(set(sizes)) == 4 and all(h != w for h, w in sizes[1:])            # sizes of their own, the three new maps non-square
    assert inp["weights"]["lin_in.weight"].shape[1] == 55 and inp["deform_w"].shape == (cfg["scene"]["C"], cfg["scene"]["C"] + 6)
    if inp["dims"]["combine_layer"] > 0:
        assert inp["weights"]["lin_z.0.weight"].shape[1] == cfg["scene"]["C"] + 6
    if cfg["P"] >= 64:
        assert 0.05 <= outside_fraction(inp) <= 0.2                              # about a tenth of the target projections leave the map
    if cfg["SB"] > 1:
        assert not np.array_equal(inp["tgt_poses"][0], inp["tgt_poses"][1]) and not np.array_equal(inp["tgt_focal"][0], inp["tgt_focal"][1])


def test_the_cases_cover_the_grid():
    shapes = {n[-1]: (c["scene"]["C"], c["scene"]["NV"], c["SB"], c["P"], c["mlp"]["d_hidden"], c["index_interp"], c["index_padding"])
              for n, c in CASES.items()}
    assert shapes == {"a": (512, 4, 2, 200, 512, "bilinear", "border"), "b": (256, 2, 1, 65, 128, "nearest", "zeros"),
                      "c": (64, 3, 1, 64, 256, "bilinear", "reflection"), "d": (512, 1, 1, 130, 64, "bilinear", "border"),
                      "e": (256, 3, 1, 1, 96, "bilinear", "border")}
    assert CASES["novel_pe_point_d"]["mlp"]["combine_layer"] >= CASES["novel_pe_point_d"]["mlp"]["n_blocks"]
    assert CASES["novel_pe_point_e"]["mlp"]["combine_layer"] == 0 and CASES["novel_pe_point_c"]["mlp"]["beta"] > 0


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
def test_a_wrong_restatement_is_rejected(variant):
    """each deliberately wrong form misses the bar by orders of magnitude on every fixture that reads the latents (a .. d), and changes
    nothing where combine_layer is 0 (e)"""
    for name in sorted(CASES):
        cfg = CASES[name]
        ref = np.load(GOLDEN / f"{name}.npz")["rgbsigma"]
        e_rgb, e_sigma = R.rgbsigma_errors(restate(inputs(name), torch.float64, variant=variant), ref)
        if min(cfg["mlp"]["combine_layer"], cfg["mlp"]["n_blocks"]) > 0:
            assert e_rgb > 100 * BOUND, (name, e_rgb, e_sigma)
        else:
            assert e_rgb <= BOUND and e_sigma <= BOUND


@pytest.mark.parametrize("padding", ["border", "zeros", "reflection"])
@pytest.mark.parametrize("interp", ["bilinear", "nearest"])
def test_hoisted_deformation_layer_equals_the_direct_form(interp, padding):
    """map, then lookup, then head == lookup, then layer, in float64 to 1e-12, for every 4-tap lookup mode: zeros padding's missing taps
    included (the map carries no bias), on the case whose target and general projections leave their maps and with SB = 2"""
    inp = inputs("novel_pe_point_a")
    direct = restate(inp, torch.float64, index_interp=interp, index_padding=padding)
    hoisted = restate(inp, torch.float64, index_interp=interp, index_padding=padding, hoisted=True)
    assert np.abs(hoisted - direct).max() <= 1e-12 and float(direct[..., 3].max()) > 0


def test_stand_in_model_is_the_restatement():
    inp = inputs("novel_pe_point_c")
    m = R.model_from_inputs(inp, device="cpu")
    t = lambda k: torch.from_numpy(inp[k])
    with torch.no_grad():
        out = m(t("xyz_in"), t("xyz_gen"), t("xyz_tgt"), viewdirs=t("viewdirs")).numpy()
    assert np.array_equal(out, restate(inp, torch.float32)) and m.calls == 1


# ---- routing -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_composite(monkeypatch):
    """composite() with its device steps replaced: the deformation returns zero points, the compositing the model's output; both point
    kernels record their call instead of running"""
    from diner_amd import novel

    def run(r, model, grad=False):
        SB, B, K = 1, 3, 2
        calls = {"novel": 0, "novel_pe": 0}
        monkeypatch.setattr(r, "_check_rays", lambda rays: rays)
        monkeypatch.setattr(r, "_poll_status", lambda *a, **k: None)
        monkeypatch.setattr(r, "_status_word", lambda dev: None)
        monkeypatch.setattr(r, "_after_launch", lambda *a, **k: None)
        monkeypatch.setattr(novel.deform, "deform_ray_points",
                            lambda rays, z, *a, return_points=False, **k: tuple(torch.zeros(SB, B * K, 3) for _ in range(3 if return_points else 2)))
        monkeypatch.setattr(novel._CompositeFn, "apply", staticmethod(lambda out, *a: (out, None, None)))

        def count(which):
            def fn(m, *pts):
                calls[which] += 1
                return torch.zeros(SB, B * K, 4)
            return fn
        monkeypatch.setattr(r, "render_points_novel", count("novel"))
        monkeypatch.setattr(r, "render_points_novel_pe", count("novel_pe"))
        with torch.enable_grad() if grad else torch.no_grad():
            r.composite(model, torch.zeros(SB, B, 8), torch.zeros(SB, B, K), None, None, None)
        return calls["novel"], calls["novel_pe"]
    return run


class _Fake(R.NovelPePointModel):
    def forward(self, *pts, viewdirs=None):
        self.calls += 1
        return torch.zeros(*pts[0].shape[:2], 4)


def _fake():
    m = R.model_from_inputs(inputs("novel_pe_point_e"), device="cpu")
    m.__class__ = _Fake
    return m


def test_routing_of_composite(host_composite):
    from diner_amd.novel import NeRFRendererDGS
    from tests import novel_point_ref as RN
    from tools.gen_novel_point_golden import CASES as NCASES, case_inputs as ncase_inputs
    pe = lambda **kw: NeRFRendererDGS(hip_point_model=True, pass_points=True, **kw)
    # both switches on, inference, the NOVEL_PE model: the new kernel, with the third point set
    r, m = pe(), _fake()
    assert host_composite(r, m) == (0, 1) and m.calls == 0
    assert host_composite(r, m, grad=True) == (0, 1) and m.calls == 0              # no parameter requires grad
    # hip_point_model off (the default): nothing changes
    r0 = NeRFRendererDGS(pass_points=True)
    assert host_composite(r0, m) == (0, 0) and m.calls == 1 and r0.last_route == "torch"
    # a deformation_layer with pass_points False: PyTorch (the model would be called with two point sets)
    m = _fake()
    assert host_composite(NeRFRendererDGS(hip_point_model=True), m) == (0, 0) and m.calls == 1
    # pass_points with a model that has no deformation_layer (the NOVEL model): PyTorch
    n = RN.model_from_inputs(ncase_inputs(NCASES["novel_point_e"]), device="cpu")
    n.forward = lambda *pts, viewdirs=None: torch.zeros(*pts[0].shape[:2], 4)
    assert host_composite(r, n) == (0, 0) and r.last_route == "torch"
    # training: a parameter requires grad under grad mode
    for touch in (lambda m: m.deformation_layer.weight, lambda m: m.gen_latent, lambda m: m.mlp_fine.lin_in.weight):
        m = _fake()
        touch(m).requires_grad_(True)
        assert host_composite(r, m, grad=True) == (0, 0) and m.calls == 1 and r.last_route == "torch"
        assert host_composite(r, m) == (0, 1) and m.calls == 1                      # ... and under no_grad the kernel again
    # a deformation_layer of another shape; missing target state
    m = _fake()
    m.deformation_layer = torch.nn.Linear(3, 3)
    assert host_composite(r, m) == (0, 0) and m.calls == 1
    for k in ("tgt_poses", "tgt_pos_encoding", "pos_encodings", "gen_latent"):
        m = _fake()
        setattr(m, k, None)
        assert host_composite(r, m) == (0, 0) and m.calls == 1, k
    # a bicubic encoder, with and without the plain renderer's bicubic switch
    m = _fake()
    m.encoder.index_interp = "bicubic"
    assert host_composite(r, m) == (0, 0) and m.calls == 1
    r.bicubic_index = True
    assert host_composite(r, m) == (0, 0) and m.calls == 2 and r.last_route == "torch"
    r.bicubic_index = False
    # another callable; an MLP outside the envelope after padding
    calls = []
    fn = lambda a, b, p, viewdirs=None: calls.append(1) or torch.zeros(*a.shape[:2], 4)
    assert host_composite(r, fn) == (0, 0) and calls == [1]
    m = _fake()
    m.mlp_fine.d_hidden = 48
    assert host_composite(r, m) == (0, 0) and m.calls == 1


def test_memory_report_counts_the_new_packs_and_starts_at_zero():
    from diner_amd.novel import NeRFRendererDGS
    r = NeRFRendererDGS(hip_point_model=True, pass_points=True)
    rep = r.memory_report()["cached"]
    assert rep["novel_pe_map"] == 0 and rep["novel_pe_pos_encodings"] == 0 and rep["total"] == 0
    r._pe_map_pack = torch.zeros(1, 2, 24, 24, 8)
    r._pe_pos_pack = (torch.zeros(1, 2, 36, 30, 4), torch.zeros(1, 26, 34, 4))
    rep = r.memory_report()["cached"]
    assert rep["novel_pe_map"] == 2 * 24 * 24 * 8 * 4 and rep["novel_pe_pos_encodings"] == (2 * 36 * 30 + 26 * 34) * 4 * 4
    assert rep["total"] == sum(v for k, v in rep.items() if k != "total") == rep["novel_pe_map"] + rep["novel_pe_pos_encodings"]
