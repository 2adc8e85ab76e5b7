"""Frame output and image scores (diner_amd/csrc/frame_out.hip; glue.torch_cmap, glue.frames_u8, glue.image_scores) as far as it goes
without a GPU: the numpy restatement of tests/frame_out_ref.py reproduces tests/golden/frame_out.npz (written by
tools/gen_golden_frame_out.py) -- every output of the UNMODIFIED reference ``torch_cmap`` bit for bit; the bytes of both quantisation
rules; the exact-integer scores to 1e-12 and the reference-form (float32, scipy uniform_filter) scores within the deviation the fixture
records for that form -- and the same comparisons reject deliberately wrong forms.  The byte rules and the scores are pinned by stated
arithmetic, not by running reference code (the fixture generator's docstring); ``torch_cmap`` is pinned by reference code.  Also: the
shipped viridis table, the new entry points' declarations and bindings, and the refusals before any launch."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import frame_out_ref as R

ROOT = Path(__file__).resolve().parents[1]
REL = 1e-12
NEW_SYMBOLS = ("diner_depth_range_workspace_floats", "diner_depth_range", "diner_depth_cmap", "diner_frames_u8",
               "diner_image_scores_workspace_floats", "diner_image_scores")
CMAP_CASES = ("flat_1x1", "one_7x7", "three_9x13_flat1", "two_33x70", "one_64x64", "ramp", "under_over", "vmin0", "given_vmin_only",
              "nan_inf", "extremes_ramp", "extremes_under_over")    # extremes_*: a table whose under / over / bad rows are no colour of it
SCORE_CASES = ("one_window_7x7", "small_8x9", "three_33x70", "tiles_75x141", "identical_20x24", "constant_12x15", "extremes_9x10")
NOISY_SCORE_CASES = ("one_window_7x7", "small_8x9", "three_33x70", "tiles_75x141")      # images with texture: every wrong form shows
SCORES = ("ssim", "psnr", "l2", "l1")
_fixture = {}


def fixture():
    """(index, {key: array}) of tests/golden/frame_out.npz, read once"""
    if not _fixture:
        d = dict(np.load(ROOT / "tests" / "golden" / "frame_out.npz", allow_pickle=False))
        _fixture["index"] = json.loads(str(d.pop("index")))
        _fixture["data"] = d
    return _fixture["index"], _fixture["data"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_fixture_holds_the_cases():
    index, d = fixture()
    assert tuple(index["cmap"]) == CMAP_CASES and tuple(index["frames"]) == CMAP_CASES and tuple(index["scores"]) == SCORE_CASES
    assert d["table"].shape == (259, 3) and d["table"].dtype == np.float64
    shapes = {(c["N"], c["H"], c["W"]) for c in index["cmap"].values()}
    assert {(1, 1, 1), (1, 7, 7), (3, 9, 13), (2, 33, 70), (1, 64, 64)} <= shapes
    assert (ROOT / "tests" / "golden" / "frame_out.npz").stat().st_size < 600_000


# ---- the colour map: pinned by the unmodified reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CMAP_CASES)
def test_restatement_reproduces_reference_torch_cmap_bit_for_bit(name):
    index, d = fixture()
    cfg = index["cmap"][name]
    got = R.torch_cmap_ref(d[f"cmap.{name}.depth"], d[cfg["table"]], cfg["vmin"], cfg["vmax"])
    want = d[f"cmap.{name}.out"]
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert np.array_equal(bits(got), bits(want))


def test_flat_image_is_black_and_zero_limit_counts_as_absent():
    index, d = fixture()
    assert (d["cmap.flat_1x1.out"] == 0).all()
    out = d["cmap.three_9x13_flat1.out"]
    assert (out[1] == 0).all() and (out[0].sum(axis=0) > 0).all() and (out[2].sum(axis=0) > 0).all()
    # vmin = 0 is the reference's "absent": the output is that of vmin = the image's minimum, and not that of a true 0
    dep = d["cmap.vmin0.depth"]
    assert index["cmap"]["vmin0"]["vmin"] == 0
    assert np.array_equal(d["cmap.vmin0.out"], R.torch_cmap_ref(dep, d["table"], float(dep.min()), 1.5))
    assert not np.array_equal(d["cmap.vmin0.out"], R.torch_cmap_ref(dep, d["table"], 1e-300, 1.5))
    # NaN pixel: the whole image bad (both limits NaN); +inf pixel: vmax = inf maps every finite pixel to the first colour
    out = d["cmap.nan_inf.out"]
    assert (out[0] == 0).all() and (out[1, :, 2, 7] == 0).all()
    rest = np.delete(out[1].reshape(3, -1), 2 * 13 + 7, axis=1)
    assert (rest == d["table"][0][:, None]).all()


@pytest.mark.parametrize("variant,name", [("round_index", "ramp"), ("round_index", "one_64x64"), ("no_eq_rule", "extremes_ramp"),
                                          ("swap_under_over", "extremes_under_over"), ("swap_under_over", "extremes_ramp")])
def test_wrong_colour_map_forms_are_rejected(variant, name):
    """(viridis' over row equals its last colour and its under row its first: the xa == N rule and the order of under and over show only
    with the extremes_* table)"""
    index, d = fixture()
    cfg = index["cmap"][name]
    wrong = R.torch_cmap_ref(d[f"cmap.{name}.depth"], d[cfg["table"]], cfg["vmin"], cfg["vmax"], variant=variant)
    assert not np.array_equal(bits(wrong), bits(d[f"cmap.{name}.out"]))


def test_shipped_table_is_the_fixtures_table():
    _, d = fixture()
    from diner_amd import glue
    key, shipped = glue._cmap_table("viridis")
    assert key == "viridis" and shipped.dtype == torch.float64 and np.array_equal(bits(shipped.numpy()), bits(d["table"]))
    assert (ROOT / "diner_amd" / "viridis_lut.py").stat().st_size < 20_000


def test_shipped_table_equals_matplotlibs_lut():
    matplotlib = pytest.importorskip("matplotlib")
    from diner_amd import glue
    cm = matplotlib.colormaps["viridis"]
    cm._init()
    assert np.array_equal(glue._cmap_table("viridis")[1].numpy(), cm._lut[:, :3])
    key, table = glue._cmap_table("magma")              # another name goes through matplotlib
    other = matplotlib.colormaps["magma"]
    other._init()
    assert key == "magma" and table.dtype == torch.float64 and np.array_equal(table.numpy(), other._lut[:, :3])


def test_other_colour_maps_need_matplotlib(monkeypatch):
    import sys

    from diner_amd import glue
    monkeypatch.setitem(sys.modules, "matplotlib", None)            # makes ``import matplotlib`` raise ImportError
    with pytest.raises(ImportError, match="matplotlib"):
        glue._cmap_table("magma")
    key, table = glue._cmap_table("viridis")                        # the shipped table needs none
    assert key == "viridis" and tuple(table.shape) == (259, 3)
    mine = torch.rand(12, 3, dtype=torch.float64)
    assert glue._cmap_table(mine)[1] is not None
    with pytest.raises(ValueError):
        glue._cmap_table(torch.rand(12, 3))                         # float32: not a table


# ---- the byte rules: pinned by stated arithmetic ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounding", R.ROUNDINGS)
def test_byte_ramp(rounding):
    _, d = fixture()
    v, want = d["bytes.values"], d[f"bytes.u8.{rounding}"]
    got = R.quantise_ref(v, rounding)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    other = R.quantise_ref(v, [r for r in R.ROUNDINGS if r != rounding][0])
    assert (other != want).sum() >= 256                             # the other rule: every (k + 0.5) / 255 differs
    # our definition where the cast is undefined
    assert got[np.isnan(v)].tolist() == [0] and (got[v < 0] == 0).all() and (got[v >= np.float32(256.0 / 255.0)] == 255).all()
    k = np.arange(256)
    assert np.array_equal(R.quantise_ref((k / 255.0).astype(np.float32), "save_image"), k.astype(np.uint8))


@pytest.mark.parametrize("rounding", R.ROUNDINGS)
@pytest.mark.parametrize("name", CMAP_CASES)
def test_frames_restatement(name, rounding):
    index, d = fixture()
    cfg = index["frames"][name]
    rgb, depth = d[f"frames.{name}.rgb"], d[f"cmap.{name}.depth"]
    table = d[cfg["table"]]
    c, dep = R.frames_u8_ref(rgb, depth, rounding, table=table, vmin=cfg["vmin"], vmax=cfg["vmax"])
    assert np.array_equal(c, d[f"frames.{name}.rgb_u8.{rounding}"])
    assert np.array_equal(dep, d[f"frames.{name}.depth_u8.{rounding}"])      # = the reference's float64 colours, quantised in double
    stacked = R.frames_u8_ref(rgb, depth, rounding, stacked=True, table=table, vmin=cfg["vmin"], vmax=cfg["vmax"])
    assert stacked.shape == (cfg["N"], 2 * cfg["H"], cfg["W"], 3)
    assert np.array_equal(stacked[:, :cfg["H"]], c) and np.array_equal(stacked[:, cfg["H"]:], dep)
    assert np.array_equal(R.frames_u8_ref(rgb, rounding=rounding), c)
    if cfg["H"] * cfg["W"] >= 49:                                            # the other rule changes at least one byte
        wrong, _ = R.frames_u8_ref(rgb, depth, rounding, table=table, vmin=cfg["vmin"], vmax=cfg["vmax"], variant="other_rounding")
        assert (wrong != c).any()


# ---- the scores: pinned by stated arithmetic ---------------------------------------------------------------------------------------------
def score_misses(name, variant=None):
    """{score: (|restatement - recorded reference form|, the recorded deviation of that form)} per image, worst image first"""
    _, d = fixture()
    got = R.image_scores_ref(d[f"scores.{name}.pred"], d[f"scores.{name}.gt"], variant=variant)
    out = {}
    for k in SCORES:
        ref, dev = d[f"scores.{name}.{k}_ref"], d[f"scores.{name}.{k}_dev"]
        with np.errstate(invalid="ignore"):
            miss = np.where(got[k] == ref, 0.0, np.abs(got[k] - ref))
        out[k] = (miss, dev)
    return got, out


@pytest.mark.parametrize("name", SCORE_CASES)
def test_scores_restatement(name):
    index, d = fixture()
    got, misses = score_misses(name)
    for k in SCORES:
        exact = d[f"scores.{name}.{k}_exact"]
        assert got[k].shape == (index["scores"][name]["N"],) and got[k].dtype == np.float64
        finite = np.isfinite(exact)
        assert np.array_equal(got[k][~finite], exact[~finite])
        assert (np.abs(got[k][finite] - exact[finite]) <= REL * np.abs(exact[finite])).all(), k
        miss, dev = misses[k]
        assert (miss <= dev + REL * np.maximum(1.0, np.abs(np.nan_to_num(exact, posinf=0.0)))).all(), (k, miss, dev)
        print(f"{name}: {k}: the float32 reference form deviates by {float(dev.max()):.3e}")


def test_special_pairs():
    _, d = fixture()
    got = R.image_scores_ref(d["scores.identical_20x24.pred"], d["scores.identical_20x24.gt"])
    assert (got["l1"][0], got["l2"][0], got["psnr"][0], got["ssim"][0]) == (0.0, 0.0, np.inf, 1.0)
    got = R.image_scores_ref(d["scores.extremes_9x10.pred"], d["scores.extremes_9x10.gt"])
    assert (got["l1"][0], got["l2"][0], got["psnr"][0]) == (1.0, 1.0, 0.0)
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    assert abs(got["ssim"][0] - c1 * c2 / ((1.0 + c1) * c2)) <= 1e-15         # mx = 0, my = 1, no variance
    got = R.image_scores_ref(d["scores.constant_12x15.pred"], d["scores.constant_12x15.gt"])
    mx, my = 100.0 / 255.0, 140.0 / 255.0
    assert abs(got["ssim"][0] - (2 * mx * my + c1) / (mx * mx + my * my + c1)) <= 1e-15
    for shape in ((1, 6, 20, 3), (1, 20, 6, 3)):
        with pytest.raises(ValueError):
            R.image_scores_ref(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))


@pytest.mark.parametrize("variant", ["no_cov_norm", "window_11", "no_crop"])
@pytest.mark.parametrize("name", NOISY_SCORE_CASES)
def test_wrong_ssim_forms_are_rejected(name, variant):
    index, _ = fixture()
    cfg = index["scores"][name]
    if variant == "window_11" and min(cfg["H"], cfg["W"]) < 11:
        with pytest.raises(ValueError):
            score_misses(name, variant)
        return
    _, misses = score_misses(name, variant)
    miss, dev = misses["ssim"]
    assert (dev > 0).all()
    assert (miss >= 100.0 * dev).all(), (miss, dev)


# ---- the C ABI and the Python surface ---------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_built_and_bound():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    assert "frame_out.hip" in (ROOT / "diner_amd" / "csrc" / "Makefile").read_text()
    for name in NEW_SYMBOLS:
        m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
        assert m, name
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1, name
    assert int(re.search(r"#define DINER_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 3
    for name, code in _lib.ROUNDINGS.items():
        assert re.search(rf"#define DINER_ROUND_{name.upper()} {code}\b", header)


def test_bad_arguments_return_codes_before_any_launch():
    from diner_amd import _lib
    L = _lib.lib()
    p = 64                                                            # a non-NULL dummy, never dereferenced
    for H, W in ((6, 20), (20, 6)):
        assert L.diner_image_scores(p, p, 1, H, W, p, p, None) == -1 and b"below 7" in L.diner_last_error()
        assert L.diner_image_scores_workspace_floats(1, H, W) == -1
    assert L.diner_image_scores(p, p, 1, 65536, 32768, p, p, None) == -3 and b"2^31" in L.diner_last_error()
    assert L.diner_image_scores(None, p, 1, 7, 7, p, p, None) == -1 and b"NULL" in L.diner_last_error()
    assert L.diner_image_scores(p, p, 0, 7, 7, p, p, None) == -1
    assert L.diner_image_scores(p, p, 1, 7, 7, p, 68, None) == -1 and b"aligned" in L.diner_last_error()
    # one partial set (5 doubles) per tile of 16 x 64 windows
    assert L.diner_image_scores_workspace_floats(1, 7, 7) == 10
    assert L.diner_image_scores_workspace_floats(3, 22, 70) == 3 * 10
    assert L.diner_image_scores_workspace_floats(1, 23, 71) == 4 * 10
    assert L.diner_image_scores_workspace_floats(2, 75, 141) == 2 * 5 * 3 * 10
    assert L.diner_depth_range_workspace_floats(3, 9, 13) == 3 * 2
    assert L.diner_depth_range_workspace_floats(1, 512, 512) == 64 * 2
    assert L.diner_depth_range_workspace_floats(1, 0, 5) == -1
    assert L.diner_depth_range(None, 1, 4, 4, p, p, None) == -1
    assert L.diner_depth_range(p, 1, 65536, 32768, p, p, None) == -3
    assert L.diner_depth_cmap(p, 1, 4, 4, None, 0.0, 1.0, 0, 1, p, 256, p, None) == -1 and b"range" in L.diner_last_error()
    assert L.diner_depth_cmap(p, 1, 4, 4, p, 0.0, 1.0, 0, 0, None, 256, p, None) == -1
    assert L.diner_depth_cmap(p, 1, 4, 4, p, 0.0, 1.0, 0, 0, p, 0, p, None) == -1
    assert L.diner_frames_u8(p, None, 1, 4, 4, 2, 0, None, 0.0, 0.0, 0, 0, None, 0, p, None, None) == -1 and b"rounding" in L.diner_last_error()
    assert L.diner_frames_u8(p, None, 1, 4, 4, 0, 1, None, 0.0, 0.0, 0, 0, None, 0, p, None, None) == -1 and b"stacked" in L.diner_last_error()
    assert L.diner_frames_u8(p, p, 1, 4, 4, 0, 0, p, 0.0, 0.0, 0, 0, p, 256, p, None, None) == -1 and b"depth_out" in L.diner_last_error()
    assert L.diner_frames_u8(None, None, 1, 4, 4, 0, 0, None, 0.0, 0.0, 0, 0, None, 0, p, None, None) == -1


def test_glue_refusals_need_no_gpu():
    from diner_amd import glue
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="frames_u8"):
        glue.image_scores(u8.float(), u8)
    with pytest.raises(TypeError, match="frames_u8"):
        glue.image_scores(u8, u8.to(torch.int32))
    with pytest.raises(ValueError, match="shapes differ"):
        glue.image_scores(u8, torch.zeros((1, 8, 9, 3), dtype=torch.uint8))
    for shape in ((1, 6, 20, 3), (20, 6, 3)):
        z = torch.zeros(shape, dtype=torch.uint8)
        with pytest.raises(ValueError, match="7 x 7"):
            glue.image_scores(z, z)
    with pytest.raises(ValueError):
        glue.image_scores(torch.zeros((8, 8, 4), dtype=torch.uint8), torch.zeros((8, 8, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.image_scores(u8, u8)
    with pytest.raises(TypeError):
        glue.torch_cmap(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(TypeError):
        glue.frames_u8(torch.zeros(3, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="rounding"):
        glue.frames_u8(torch.zeros(3, 4, 4), rounding="nearest")
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.torch_cmap(torch.zeros(4, 4))
    # the table quantised on the host by each rule, in double: the restatement's bytes
    _, d = fixture()
    table = torch.from_numpy(d["table"])
    for r in R.ROUNDINGS:
        assert np.array_equal(glue._quantise_table(table, r).numpy(), R.quantise_ref(d["table"], r))
    odd = torch.tensor([[-0.5, float("nan"), 2.0], [1.0, 0.999, 0.5]], dtype=torch.float64)
    for r in R.ROUNDINGS:
        assert np.array_equal(glue._quantise_table(odd, r).numpy(), R.quantise_ref(odd.numpy(), r))
