"""Host tests (no GPU) of the encoder's latent lookup modes (SpatialEncoder index_interp / index_padding, reference
src/models/image_encoder.py:24-25,119-125): model validation, the C ABI of the _ix entry points, and the index_* fixtures of
tools/gen_index_golden.py (seeded inputs, the out-of-map fraction that makes the padding matter, nearest firmness)."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
INDEX_FIXTURES = sorted(p.stem for p in GOLDEN.glob("index_*.npz"))
NEW_SYMBOLS = ["diner_linz_maps_floats", "diner_pack_linz_maps_ix", "diner_render_points_ix", "diner_render_ix", "diner_render_image_ix",
               "diner_render_points_gen_ix", "diner_render_gen_ix", "diner_render_image_gen_ix", "diner_train_point_inputs_ix"]
MODES = [(i, p) for i in ("bilinear", "nearest") for p in ("border", "zeros", "reflection")]


def _model(interp, padding, **dims):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(8, 8, 2, seed=1, feature_padding=2)
    d = dict(d_in=55, d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3)
    d.update(dims)
    w = synth.make_mlp_weights(2, d_in=d["d_in"], d_latent=d["d_latent"], d_hidden=d["d_hidden"], n_blocks=d["n_blocks"],
                               combine_layer=d["combine_layer"])
    return model_from_scene(sc, w, device="cpu", index_interp=interp, index_padding=padding,
                            **{k: v for k, v in d.items() if k != "d_in"})


@pytest.mark.parametrize("interp,padding", MODES)
def test_validate_model_accepts_the_six_modes(interp, padding):
    from diner_amd import NeRFRendererDGS, _lib
    from diner_amd.renderer import STANDARD_SHAPE
    m = _model(interp, padding)
    assert NeRFRendererDGS._validate_model(m) == STANDARD_SHAPE
    ix = NeRFRendererDGS._latent_index(m)
    if (interp, padding) == ("bilinear", "border"):
        assert ix is None                                     # the default keeps the entry points and torch ops it always used
    else:
        assert (ix.interp, ix.padding) == (_lib.INDEX_INTERP[interp], _lib.INDEX_PADDING[padding])


def test_validate_model_accepts_the_modes_on_other_shapes():
    from diner_amd import NeRFRendererDGS
    m = _model("nearest", "zeros", d_hidden=128, n_blocks=4, combine_layer=2)
    assert not NeRFRendererDGS._validate_model(m).standard


@pytest.mark.parametrize("interp,padding", [("bicubic", "border"), ("bilinear", "wrap"), ("nearest", "exponential"), ("area", "zeros")])
def test_validate_model_rejects_other_modes_and_names_the_supported_ones(interp, padding):
    from diner_amd import NeRFRendererDGS
    with pytest.raises(NotImplementedError) as e:
        NeRFRendererDGS._validate_model(_model(interp, padding))
    msg = str(e.value)
    for name in ("bilinear", "nearest", "border", "zeros", "reflection"):
        assert name in msg


def test_new_symbols_declared_exported_and_abi_still_3():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == 3 == _lib.ABI_VERSION
    assert "typedef struct DinerLatentIndex" in header
    for k, v in (("DINER_INDEX_BILINEAR", 0), ("DINER_INDEX_NEAREST", 1), ("DINER_INDEX_PAD_BORDER", 0), ("DINER_INDEX_PAD_ZEROS", 1),
                 ("DINER_INDEX_PAD_REFLECTION", 2)):
        assert int(re.search(rf"#define {k} (\d+)", header).group(1)) == v
    assert _lib.INDEX_INTERP == {"bilinear": 0, "nearest": 1} and _lib.INDEX_PADDING == {"border": 0, "zeros": 1, "reflection": 2}
    assert [f[0] for f in _lib.DinerLatentIndex._fields_] == ["interp", "padding"] and C.sizeof(_lib.DinerLatentIndex) == 8
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SYMBOLS, name
    so = ROOT / "diner_amd" / "lib" / "libdiner_hip.so"
    if not so.exists():
        pytest.skip("library not built")
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.diner_version() == 3


def test_unknown_mode_values_are_invalid_with_a_message():
    from diner_amd import _lib
    if not (ROOT / "diner_amd" / "lib" / "libdiner_hip.so").exists():
        pytest.skip("library not built")
    lib = _lib.lib()
    for bad in (_lib.DinerLatentIndex(2, 0), _lib.DinerLatentIndex(0, 3), _lib.DinerLatentIndex(-1, 1)):
        assert lib.diner_linz_maps_floats(1, 4, 4, C.byref(bad)) == -1
        assert b"latent index" in lib.diner_last_error()
        sc = _lib.DinerScene(SB=1, NV=1, H=4, W=4, h=4, w=4, C=512, num_freqs=6, image_w=4.0, image_h=4.0)
        sc.poses = sc.focal = sc.c = sc.maps = sc.latent = 16   # never dereferenced: the mode is rejected before any launch
        assert lib.diner_render_points_ix(C.byref(sc), C.byref(bad), 16, None, None, 0, 1, 0, None, None, None) == -1
        assert b"latent index" in lib.diner_last_error()


def test_ringed_linz_maps_size():
    from diner_amd import _lib
    if not (ROOT / "diner_amd" / "lib" / "libdiner_hip.so").exists():
        pytest.skip("library not built")
    lib = _lib.lib()
    assert lib.diner_linz_maps_floats(6, 10, 12, None) == 3 * 6 * 10 * 12 * 512
    for i in (0, 1):
        assert lib.diner_linz_maps_floats(6, 10, 12, C.byref(_lib.DinerLatentIndex(i, 1))) == 3 * 6 * 12 * 14 * 512
        assert lib.diner_linz_maps_floats(6, 10, 12, C.byref(_lib.DinerLatentIndex(i, 2))) == 3 * 6 * 10 * 12 * 512


def test_fixture_set():
    from tools.gen_index_golden import CASES, TRAIN_CASES
    assert INDEX_FIXTURES == sorted(list(CASES) + list(TRAIN_CASES))
    assert not any(re.match(r"g[0-9]", n) for n in INDEX_FIXTURES)      # tests/conftest.py parametrises over g[0-9]*.npz
    modes = {(c["interp"], c["padding"]) for c in CASES.values()}
    assert modes == set(MODES) - {("bilinear", "border")}                 # the five non-default modes
    assert any(c["padding"] == "zeros" and c["mlp"]["d_hidden"] != 512 for c in CASES.values())   # a non-standard shape with zeros
    # the mode after the feature_padding rescale (image_encoder.py:113-114), as in the shipped configs
    assert {c["padding"] for c in CASES.values() if c["scene"]["feature_padding"] > 0} >= {"zeros", "reflection"}
    assert {(c["interp"], c["padding"]) for c in TRAIN_CASES.values()} >= {("bilinear", "zeros")} and \
        any(c["interp"] == "nearest" for c in TRAIN_CASES.values())


@pytest.mark.parametrize("name", INDEX_FIXTURES)
def test_fixture_digests_and_padding_coverage(name):
    from tools.gen_index_golden import CASES, TRAIN_CASES, case_inputs, input_digests
    data = np.load(GOLDEN / f"{name}.npz", allow_pickle=False)
    cfg = json.loads(str(data["config"]))
    assert cfg == {**CASES, **TRAIN_CASES}[name]
    sc, w, rays, noise = case_inputs(cfg)
    assert json.loads(str(data["digests"])) == input_digests(sc, w, rays, noise)
    assert float(data["out_frac"]) >= 0.10, "the padding mode must decide a real share of the lookups"
    firm = data["firm"]
    assert firm.shape == data["z_fill"].shape[-2:] and firm.dtype == bool
    if cfg["interp"] == "nearest":
        assert firm.mean() >= 0.95, "most nearest lookups must be clear of a rounding boundary"
