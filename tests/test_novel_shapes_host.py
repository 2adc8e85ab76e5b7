"""Host-side proof (no GPU) that every case of tests/novel_shape_cases.py is a sound yardstick for tests/test_gpu_novel_shapes.py:
its seeded inputs converge, the float32 restatement sits within a quarter of the bars of the float64 one (the room the GPU result
needs), at least a third of the sigmas are positive, between 5 % and 25 % of the general (and target) projections leave their map, the
hoisted and direct forms of the deformation layer agree, and the float64 result moves by 10 bars or more under each wrong form the
new shapes exist to catch.  The wrong forms are edits of the inputs fed to the same float64 restatement."""
import numpy as np
import pytest
import torch

from tests import novel_pe_point_ref as RPE
from tests import novel_point_ref as RN
from tests import novel_shape_cases as S
from tools import gen_novel_pe_point_golden as GPE
from tools import gen_novel_point_golden as GN

BOUND = 1e-4      # rgb abs; sigma relative to max(1, sigma / 12): the bars of tests/test_gpu_mlp_shapes*.py
KMAX = 512        # columns of a gather piece (csrc/points_mlp_gen_kernel.hpp)
ALL = [(kind, name) for kind, table in S.TABLES.items() for name in table]
IDS = [name for _, name in ALL]


# ---- the wrong forms: name -> edit(inp, C) of a private copy, or None where the form does not exist at this C ------------------------------
def _lz_cols(inp, cols, fn):
    for k in S.lin_z_keys(inp):
        w = inp["weights"][k] = inp["weights"][k].copy()
        fn(w, cols)


def _zero(w, cols):
    w[:, cols] = 0


def lz_tail8(inp, C):
    """the last 8 latent columns of every lin_z weight are zero: a dropped K tail, or a dropped piece-2 latent part"""
    _lz_cols(inp, slice(C - 8, C), _zero)


def latent_last(inp, C):
    """the encoder latent's channel C - 1 is zero: a dropped last channel of the gather (NOVEL) / of the builder's K (NOVEL_PE)"""
    inp["latent"] = inp["latent"].copy()
    inp["latent"][:, :, C - 1] = 0


def gen_last(inp, C):
    """gen_latent's channel C - 1 is zero: a dropped last channel of the gather's second lookup"""
    inp["gen_latent"] = inp["gen_latent"].copy()
    inp["gen_latent"][C - 1] = 0


def map_tail8(inp, C):
    """rows C - 8 .. C - 1 of deform_w[:, :C] are zero: the builder's last partial column tile left unwritten"""
    inp["deform_w"] = inp["deform_w"].copy()
    inp["deform_w"][C - 8:, :C] = 0


def lz_piece2(inp, C):
    """lin_z columns 512 .. C - 1 are zero: a skipped second piece"""
    _lz_cols(inp, slice(KMAX, C), _zero)


def pe_from_piece1(inp, C):
    """the pe columns C .. C + 5 trade places with piece 1's columns 0 .. 5: a tail indexed by 4 q where 4 qq is meant"""
    def swap(w, _):
        head, tail = w[:, :6].copy(), w[:, C:C + 6].copy()
        w[:, :6], w[:, C:C + 6] = tail, head
    _lz_cols(inp, None, swap)


EDITS = {"novel_pe": (lz_tail8, latent_last, gen_last, map_tail8, lz_piece2, pe_from_piece1), "novel": (lz_tail8, latent_last, gen_last, lz_piece2)}
VARIANTS = {"novel_pe": RPE.WRONG_VARIANTS, "novel": RN.WRONG_VARIANTS}


def mutants(kind, name):
    """(label, float64 result) of every wrong form that exists for this case"""
    inp, _, _ = S.case(kind, name)
    C, NV = inp["cfg"]["scene"]["C"], inp["cfg"]["scene"]["NV"]
    for edit in EDITS[kind]:
        if edit in (lz_piece2, pe_from_piece1) and C <= KMAX:
            continue
        m = dict(inp, weights=dict(inp["weights"]))
        edit(m, C)
        yield edit.__name__, S.restate(kind, m)
    for v in VARIANTS[kind]:
        if v == "gen_once" and NV == 1:      # "the general latent in view 0 only" is the model itself with one view
            continue
        yield v, S.restate(kind, inp, variant=v)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
def test_the_tables_cover_the_envelope():
    col = lambda table, f: [f(c) for c in table.values()]
    assert col(S.PE_CASES, lambda c: c["scene"]["C"]) == [8, 40, 248, 504, 520, 776, 1016, 520]
    assert col(S.NV_CASES, lambda c: c["scene"]["C"]) == [8, 40, 248, 520, 776, 1000]
    seeds = set()
    for table, fixtures in ((S.PE_CASES, GPE.CASES), (S.NV_CASES, GN.CASES)):
        hid = col(table, lambda c: c["mlp"]["d_hidden"])
        assert min(hid) <= 128 and any(128 < h <= 256 for h in hid) and max(hid) > 256          # <1,1>, <2,1>, <2,2>
        assert any(h & (h - 1) for h in hid)                                                     # one width that is no power of two
        assert set(col(table, lambda c: c["scene"]["NV"])) == {1, 2, 3, 4}
        assert set(col(table, lambda c: c["P"])) == {1, 63, 64, 65, 129} and max(col(table, lambda c: c["P"])) <= 130
        assert set(col(table, lambda c: c["index_interp"])) == {"bilinear", "nearest"}
        assert set(col(table, lambda c: c["index_padding"])) == {"border", "zeros", "reflection"}
        assert any(c["mlp"].get("beta", 0) == 100.0 for c in table.values()) and 2 in col(table, lambda c: c["SB"])
        for c in table.values():
            if c["mlp"]["combine_layer"] >= c["mlp"]["n_blocks"]:
                assert c["scene"]["NV"] == 1
            assert c["mlp"]["combine_layer"] > 0 and c["scene"]["C"] % 8 == 0                    # every case reads the latents
            assert {k: c["scene"][k] for k in GPE._SCENE} == GPE._SCENE                          # the generators' small maps
            mine = {c["scene"]["seed"] + 10 * sb for sb in range(c["SB"])} | {c["wseed"], c["pseed"]}
            assert not mine & seeds
            seeds |= mine
        assert any(c["mlp"]["combine_layer"] >= c["mlp"]["n_blocks"] for c in table.values())
        theirs = set()
        for c in fixtures.values():
            theirs |= {c["scene"]["seed"] + 10 * sb for sb in range(c["SB"])} | {c["wseed"], c["pseed"]}
        assert not theirs & seeds and max(theirs) < 300 <= min(seeds)
    assert all(c[k] == v for c in S.PE_CASES.values() for k, v in GPE._MAPS.items())
    assert all(c[k] == v for c in S.NV_CASES.values() for k, v in GN._GEN.items())


# ---- every case is a sound yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, name", ALL, ids=IDS)
def test_case_is_a_sound_yardstick(kind, name):
    inp, r64, r32 = S.case(kind, name)        # case_inputs asserts its re-draw converged and the nearest lookups' 1e-3-texel margin
    cfg = inp["cfg"]
    C, P = cfg["scene"]["C"], cfg["P"]
    assert r64.shape == (cfg["SB"], P, 4) and np.isfinite(r64).all() and r32.dtype == np.float32
    assert inp["latent"].shape[2:] == (C, 24, 24) and inp["gen_latent"].shape == (C, 28, 20)
    width = C + 6 if kind == "novel_pe" else C
    assert all(inp["weights"][k].shape == (inp["dims"]["d_hidden"], width) for k in S.lin_z_keys(inp)) and S.lin_z_keys(inp)
    e_rgb, e_sigma = RN.rgbsigma_errors(r32, r64)
    share = float((r64[..., 3] > 0).mean())
    out = [GPE.outside_fraction(inp, "tgt"), GPE.outside_fraction(inp, "gen")] if kind == "novel_pe" else [GN.outside_fraction(inp)]
    print(f"{name}: e32 rgb {e_rgb:.2e} sigma {e_sigma:.2e} (of the bar: {e_rgb / BOUND:.3f}, {e_sigma / BOUND:.3f}); sigma > 0: {share:.2f}, "
          f"max {r64[..., 3].max():.2f}; outside: {' '.join(f'{o:.2f}' for o in out)}")
    assert e_rgb <= BOUND / 4 and e_sigma <= BOUND / 4
    assert share >= 1 / 3
    if P > 1:         # (of a single point a fraction is 0 or 1: the two P = 1 cases only keep their point inside every map)
        assert all(0.05 <= o <= 0.25 for o in out), out
    else:
        assert out == [0.0] * len(out)
    if kind == "novel_pe":
        assert np.abs(S.restate(kind, inp, hoisted=True) - r64).max() <= 1e-12


@pytest.mark.parametrize("kind, name", ALL, ids=IDS)
def test_case_rejects_every_wrong_form(kind, name):
    _, r64, _ = S.case(kind, name)
    seen = []
    for label, got in mutants(kind, name):
        e_rgb, e_sigma = RN.rgbsigma_errors(got, r64)
        print(f"{name} {label}: |rgb| {e_rgb:.2e}, |sigma| {e_sigma:.2e}")
        assert max(e_rgb, e_sigma) >= 10 * BOUND, (label, e_rgb, e_sigma)
        seen.append(label)
    C = S.TABLES[kind][name]["scene"]["C"]
    assert len(seen) >= (4 if kind == "novel_pe" else 3) + len(VARIANTS[kind]) - 1 + (C > KMAX)


# ---- the renderer accepts every case, and picks the instantiation the table says -------------------------------------------------------------
@pytest.mark.parametrize("kind, name", ALL, ids=IDS)
def test_the_renderer_accepts_the_shape(kind, name):
    from diner_amd.novel import NeRFRendererDGS
    inp, _, _ = S.case(kind, name)
    C = inp["cfg"]["scene"]["C"]
    r = NeRFRendererDGS()
    if kind == "novel_pe":
        shape = r._validate_pe(RPE.model_from_inputs(inp, device="cpu"))
        assert shape.d_latent == C + 8
    else:
        shape = r._validate(RN.model_from_inputs(inp, device="cpu"))
        assert shape.d_latent == C
    assert shape.d_hidden == inp["dims"]["d_hidden"] and shape.combine_layer == inp["dims"]["combine_layer"]
