"""The NOVEL and NOVEL_PE render kernels across their latent-width envelope: the case tables of tests/test_novel_shapes_host.py (which
proves every case a sound yardstick on the CPU) and tests/test_gpu_novel_shapes.py (which runs the kernels against them).

The cfgs have the format of the generators' ``CASES`` and are consumed by their ``case_inputs``; no fixture belongs to them: every
expected value is the float64 restatement (tests/novel_point_ref.py, tests/novel_pe_point_ref.py; both proven against the unmodified
reference's fixtures by their host tests) of the seeded float32 inputs, computed at test time.  The seeds (300 and above) are disjoint
from the fixtures' (70 .. 93 and 170 .. 190).  ``C`` is the axis; the other axes are spread so that every kernel instantiation
(d_hidden <= 128: <1,1>, <= 256: <2,1>, above: <2,2>), a d_hidden that is no power of two, NV 1 .. 4, P in {1, 63, 64, 65, 129}, both
index_interp, all three index_padding, Softplus, SB = 2 and combine_layer >= n_blocks (NV = 1) each occur.  ``wseed`` / ``pseed`` were
chosen per case so that at least a third of the points have a positive float64 sigma (the relu hides nothing), every mutant of the
host test moves the result by 10 bars or more, and the float32 restatement's error is 1.5e-5 or less where the search ran (1, 8 and 16
threads, the direct and the hoisted form): it differs between CPUs by some tens of per cent, and the host test holds it to 2.5e-5.

NOVEL_PE: the GEMM's K is C + 8, a gather piece holds 512 columns, the f16x3 kernels' k-blocks 16, the map builder's column tiles 32:
    C = 8     K = 16: one full f16 k-block; four gathering lanes; the builder with 24 dead lanes
    C = 40    K = 48: the builder's partial second column tile
    C = 248   K = 256: the gather's q loop is exactly one full trip
    C = 504   K = 512: the pe tail in the last two quads of a full single piece
    C = 520   K = 528: piece 2 = 8 latent + 8 pe columns; the builder's second piece of 8
    C = 776   two pieces, C % 32 != 0 in both kernels
    C = 1016  K = 1024: two full pieces; the builder's second piece of 504
NOVEL: K = C; every C below is 8 (mod 16) and no multiple of 32, below 256, between 512 and 1024, and 520 = a second piece of 8.
"""
from __future__ import annotations

import functools

import torch

from tests import novel_pe_point_ref as RPE
from tests import novel_point_ref as RN
from tools import gen_novel_pe_point_golden as GPE
from tools import gen_novel_point_golden as GN

_S, _M, _G = GPE._SCENE, GPE._MAPS, GN._GEN


def _pe(C, NV, SB, P, mlp, interp, padding, seed, wseed, pseed):
    return dict(scene=dict(_S, NV=NV, seed=seed, C=C), SB=SB, num_freqs=6, mlp=mlp, P=P, index_interp=interp, index_padding=padding,
                wseed=wseed, pseed=pseed, **_M)


def _nv(C, NV, SB, P, mlp, interp, padding, seed, wseed, pseed):
    return dict(scene=dict(_S, NV=NV, seed=seed, C=C), SB=SB, num_freqs=6, mlp=mlp, P=P, index_interp=interp, index_padding=padding,
                wseed=wseed, pseed=pseed, **_G)


PE_CASES = {
    "pe_c8": _pe(8, 2, 1, 63, dict(d_hidden=96, n_blocks=3, combine_layer=2), "bilinear", "zeros", 300, 1063, 302),
    "pe_c40": _pe(40, 3, 1, 65, dict(d_hidden=128, n_blocks=3, combine_layer=2), "nearest", "border", 310, 1100, 312),
    "pe_c248": _pe(248, 4, 1, 64, dict(d_hidden=256, n_blocks=3, combine_layer=2, beta=100.0), "bilinear", "reflection", 320, 1256, 322),
    "pe_c504": _pe(504, 1, 1, 129, dict(d_hidden=64, n_blocks=2, combine_layer=1000), "bilinear", "border", 330, 1318, 2033),
    "pe_c520": _pe(520, 2, 2, 65, dict(d_hidden=160, n_blocks=3, combine_layer=2), "nearest", "reflection", 340, 1443, 2041),
    "pe_c776": _pe(776, 2, 1, 63, dict(d_hidden=512, n_blocks=3, combine_layer=2), "bilinear", "zeros", 360, 1509, 2052),
    "pe_c1016": _pe(1016, 2, 1, 64, dict(d_hidden=320, n_blocks=2, combine_layer=1), "nearest", "zeros", 370, 1603, 372),
    # a single point: four view sums, two pieces, Softplus in <2,2>
    "pe_c520_p1": _pe(520, 4, 1, 1, dict(d_hidden=512, n_blocks=2, combine_layer=1, beta=100.0), "bilinear", "border", 380, 381, 382),
}
NV_CASES = {
    "nv_c8": _nv(8, 3, 1, 65, dict(d_hidden=64, n_blocks=3, combine_layer=2), "bilinear", "reflection", 400, 1809, 402),
    "nv_c40": _nv(40, 1, 1, 129, dict(d_hidden=96, n_blocks=2, combine_layer=1000), "nearest", "zeros", 410, 1903, 2091),
    "nv_c248": _nv(248, 2, 2, 63, dict(d_hidden=160, n_blocks=2, combine_layer=1, beta=100.0), "bilinear", "zeros", 420, 2008, 2101),
    "nv_c520": _nv(520, 4, 1, 64, dict(d_hidden=128, n_blocks=3, combine_layer=2), "nearest", "border", 440, 441, 442),
    "nv_c776": _nv(776, 2, 1, 1, dict(d_hidden=512, n_blocks=2, combine_layer=1), "bilinear", "border", 450, 743, 452),
    "nv_c1000": _nv(1000, 3, 1, 65, dict(d_hidden=384, n_blocks=2, combine_layer=1), "nearest", "reflection", 460, 461, 462),
}
TABLES = {"novel_pe": PE_CASES, "novel": NV_CASES}

PE_KEYS = ("poses", "focal", "c", "image_shape", "depths", "latent", "pos_encodings", "gen_latent", "gen_poses", "gen_focal", "gen_c",
           "gen_image_shape", "tgt_pos_encoding", "tgt_poses", "tgt_focal", "tgt_c", "tgt_image_shape", "deform_w", "deform_b", "weights")
NV_KEYS = ("poses", "focal", "c", "image_shape", "depths", "latent", "gen_latent", "gen_poses", "gen_focal", "gen_c", "gen_image_shape", "weights")


def restate(kind, inp, dtype=torch.float64, **kw):
    """the restatement of ``kind`` ("novel" | "novel_pe") on one ``case_inputs`` dict (or an edited copy of one) -> rgb-sigma [SB,P,4]"""
    cfg, d = inp["cfg"], inp["dims"]
    common = dict(n_blocks=d["n_blocks"], combine_layer=d["combine_layer"], beta=d["beta"], num_freqs=cfg["num_freqs"], freq_factor=6.28,
                  feature_padding=cfg["scene"]["feature_padding"], index_interp=cfg["index_interp"], index_padding=cfg["index_padding"])
    x = torch.from_numpy(inp["xyz_in"]).to(dtype)
    with torch.no_grad():
        if kind == "novel_pe":
            return RPE.novel_pe_point_forward(x, inp["xyz_gen"], inp["xyz_tgt"], inp["viewdirs"], **{k: inp[k] for k in PE_KEYS},
                                              **dict(common, **kw)).numpy()
        return RN.novel_point_forward(x, inp["xyz_gen"], inp["viewdirs"], **{k: inp[k] for k in NV_KEYS}, **dict(common, **kw)).numpy()


@functools.lru_cache(maxsize=None)
def case(kind, name):
    """(inputs rebuilt from the seeds, the float64 restatement, the float32 restatement) of one case: built once, never written to"""
    inp = (GPE if kind == "novel_pe" else GN).case_inputs(TABLES[kind][name])
    r64, r32 = restate(kind, inp, torch.float64), restate(kind, inp, torch.float32)
    r64.setflags(write=False)
    r32.setflags(write=False)
    return inp, r64, r32


def lin_z_keys(inp):
    return sorted(k for k in inp["weights"] if k.startswith("lin_z.") and k.endswith(".weight"))
