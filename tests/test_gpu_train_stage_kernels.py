"""The training step's point, scatter and reduction kernels, one by one on the GPU through the C ABI: ``point_inputs_kernel`` (NCHW, NHWC
and the any-mode instantiations), ``point_inputs_gen_kernel``, ``bilinear_scatter_kernel``, ``nhwc_to_nchw_kernel``,
``point_inputs_bwd_kernel`` / ``point_inputs_bwd_gen_kernel`` with the ``camg_*`` reductions behind them, ``view_mean(_bwd)_kernel``,
``head(_bwd)_kernel``, ``amax_kernel``, ``colsum_kernel`` and ``colsum_amax_kernel``.  Expectations, case sets, comparison functions and
bounds are those of tests/train_stage_refs.py: float64 restatements and torch's float64 autograd.  tests/test_train_stage_refs_host.py
proves on the CPU that they reproduce the oracle, the reference's stored MLP inputs and grid_sample, that every point keeps 1e-3 texel
from every decision boundary (so no row is ever masked out of a comparison; rows exactly ON the boundaries come from ``BoundaryCase``,
whose arithmetic is exact), and that every comparison rejects a wrong implementation.  Outputs are filled with NaN before every call.

Bounds: 4 x the worse of two float32 CPU evaluations' error against float64 + a floor, from CPU values only -- elementwise outputs: one
float32 ulp of the family's magnitude (+ 4.2e-7, pe_sin's documented error, on the positional codes); reduced leaves: relative to the sum of
the absolute values of the element's per-row terms, floor (depth of the documented reduction) x 2^-24; depth texels: (rows of the texel) x
2^-24; the latent scatter: the forward's weight bound x sum |d_zlat| + (terms of the element) x 2^-24 x sum |d_zlat| |w|.
d_poses: rows 0..2 are written, row 3 is left untouched (camg_view_final_kernel writes 12 of the 16 elements; the caller zeroes it).

Largest errors observed over all cases (CPU side: the float32 evaluation the bound is taken from; GPU side: MI355X); reduced leaves and
depth texels in units of sum |terms|, the scatter in units of sum |d_zlat| (a weight's error):

    family                                  CPU float32 side   GPU        largest GPU / bound
    in: position                            3.23e-07           1.99e-07   0.15
    in: direction                           7.02e-08           7.20e-08   0.19
    in: depth distance                      3.23e-07           1.99e-07   0.23
    in: positional codes, octaves 0..2      9.85e-06           6.91e-06   0.25
    in: positional codes, octaves 3..5      6.52e-05           4.82e-05   0.25
    zlat                                    2.42e-06           2.39e-06   0.31
    tap weights                             1.26e-06           9.96e-07   0.30
    latent scatter (error / bound)          0.17               0.47       0.47
    d_rays                                  8.64e-06           3.38e-06   0.33
    d_poses (the lone point; else 3.6e-07)  4.22e-05           4.22e-05   0.25
    d_focal                                 5.63e-07           5.63e-07   0.20
    d_c                                     5.79e-07           4.98e-07   0.17
    d_image_shape                           3.41e-07           1.93e-07   0.14
    d_depths                                8.28e-06           9.11e-07   0.18
    head (sigmoid)                          8.43e-08           7.71e-08   0.18
    colsum                                  1.19e-07           1.21e-07   0.50
    colsum_amax, column sums                1.53e-07           2.77e-07   0.50

The largest GPU error / bound ratio of any case is 0.50 (a column sum over M = 1 row: the one rounding of db + x against a bound of two),
0.47 on the scatter, 0.33 at most elsewhere.  Bit for bit or exact: the tap indices, NCHW against NHWC, the _gen taps against the standard
entry's, a second run's rays and camera gradients, the layout change, amax, the head's relu and its gate, the column sums of whole numbers,
every element no row reaches.  The view mean is within its (NV + 1) ulp, its backward within 1 ulp.  No kernel was found wrong.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_stage_refs as ts
from tests.train_stage_refs import GEN_CASES, MODES, MODE_IDS, TRAIN_STAGE_CASES

pytestmark = pytest.mark.gpu
F32 = np.float32
IDS = lambda cases: [c.id for c in cases]
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def P_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def call(name, *args):
    from diner_amd import _lib
    rc = getattr(_lib.lib(), name)(*args)
    assert rc == 0, (name, rc, _lib.lib().diner_last_error())
    torch.cuda.synchronize()


def fig(family, cpu, gpu, bound):
    """one line per comparison for the table in the module docstring"""
    print(f"FIG {family} cpu {cpu:.3e} gpu {gpu:.3e} bound {bound:.3e} ratio {gpu / bound if bound > 0 else 0.0:.3f}")


def index_of(mode):
    from diner_amd import _lib
    return _lib.DinerLatentIndex(interp=_lib.INDEX_INTERP[mode[0]], padding=_lib.INDEX_PADDING[mode[1]])


class OnDevice:
    """a case's scenes as one DinerScene, built by hand as ``Stage`` of tests/test_gpu_bicubic.py builds it"""

    def __init__(self, case, dev):
        from diner_amd import _lib
        c = self.case = case.build()
        self.dev = dev
        sc = c.scenes
        maps = np.zeros((c.SB, c.NV, c.H, c.W, 8), F32)
        maps[..., 3] = np.stack([s.depths for s in sc])                               # nx ny nz depth | sigma 0 0 0 (pack.hip)
        lat = np.stack([s.latent for s in sc])                                        # [SB,NV,C,h,w]
        self.t = dict(poses=T(np.stack([s.poses for s in sc]), dev), focal=T(np.stack([s.focal for s in sc]), dev),
                      c=T(np.stack([s.c for s in sc]), dev), maps=T(maps, dev), lat_nchw=T(lat, dev),
                      lat_nhwc=T(lat.transpose(0, 1, 3, 4, 2), dev), rays=T(c.rays, dev), z=T(c.z, dev))
        s = _lib.DinerScene(SB=c.SB, NV=c.NV, H=c.H, W=c.W, h=c.h, w=c.w, C=c.C, num_freqs=c.F, image_w=float(sc[0].image_shape[0]),
                            image_h=float(sc[0].image_shape[1]), feature_padding=float(sc[0].feature_padding),
                            freq_factor=float(sc[0].freq_factor))
        s.poses, s.focal, s.c, s.maps = (self.t[k].data_ptr() for k in ("poses", "focal", "c", "maps"))
        s.latent = self.t["lat_nhwc"].data_ptr()
        self.scene = s
        self.R = c.NV * c.P

    def forward(self, entry, mode, sb=0, nhwc=1):
        """entry 'std' (diner_train_point_inputs / _ix) or 'gen' -> in [R, ld], zlat [R, C], idx [R, 4] int32, wt [R, 4] (numpy)"""
        c, t, dev = self.case, self.t, self.dev
        ld = 56 if entry == "std" else c.ld_in
        inp, zl, taps = (torch.full((self.R, n), NAN, device=dev) for n in (ld, c.C, 8))
        lat = t["lat_nhwc"] if nhwc else t["lat_nchw"]
        ix = index_of(mode)
        if entry == "std" and mode == MODES[0]:
            call("diner_train_point_inputs", C.byref(self.scene), P_(lat), nhwc, P_(t["rays"]), P_(t["z"]), c.NR, c.K, sb, P_(inp), P_(zl),
                 P_(taps), ST(dev))
        elif entry == "std":
            call("diner_train_point_inputs_ix", C.byref(self.scene), C.byref(ix), P_(lat), nhwc, P_(t["rays"]), P_(t["z"]), c.NR, c.K, sb,
                 P_(inp), P_(zl), P_(taps), ST(dev))
        else:
            assert nhwc
            call("diner_train_point_inputs_gen", C.byref(self.scene), None if mode == MODES[0] else C.byref(ix), P_(lat), P_(t["rays"]),
                 P_(t["z"]), c.NR, c.K, sb, P_(inp), ld, P_(zl), P_(taps), ST(dev))
        self.taps = taps
        tp = taps.cpu()
        return inp.cpu().numpy(), zl.cpu().numpy(), tp[:, :4].contiguous().view(torch.int32).numpy(), tp[:, 4:].numpy()

    def backward(self, entry, mode, sb=0, omit=(), with_far=True, start=None):
        """-> dict of the outputs (numpy; None where omitted).  Outputs start as NaN, except image_shape and depths (+=: ``start``'s
        values) and d_poses (a sentinel, to see which elements are written)."""
        from diner_amd import _lib
        c, t, dev = self.case, self.t, self.dev
        n = _lib.lib().diner_train_camera_workspace_floats(c.NR, c.K, c.NV)
        assert n == self.R * 24 + c.NV * 256 * 18
        ws = torch.full((n,), NAN, device=dev)
        out = dict(rays=torch.full((c.SB, c.NR, 8), NAN, device=dev), poses=torch.full((c.SB, c.NV, 4, 4), SENTINEL, device=dev),
                   focal=torch.full((c.SB, c.NV, 2), NAN, device=dev), c=torch.full((c.SB, c.NV, 2), NAN, device=dev),
                   image_shape=T(start["image_shape"], dev), depths=T(start["depths"], dev))
        for k in omit:
            out[k] = None
        d_in = T(c.d_in[sb] if entry == "gen" else c.d_in[sb][:, :56], dev)
        d_zl, d_far = T(c.d_zlat[sb], dev), T(np.broadcast_to(c.d_far[sb], (c.SB, c.NR)), dev) if with_far else None
        ix = index_of(mode)
        head = (C.byref(self.scene), C.byref(ix), P_(t["lat_nhwc"]), P_(t["rays"]), P_(t["z"]), c.NR, c.K, sb, P_(d_in))
        tail = (P_(d_zl), P_(d_far), P_(ws)) + tuple(P_(out[k]) for k in ts.LEAVES) + (ST(dev),)
        if entry == "std":
            call("diner_train_point_inputs_backward", *head, *tail)
        else:
            call("diner_train_point_inputs_backward_gen", *head, c.ld_in, *tail)
        return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


SENTINEL = -7.25
_dev_cases = {}


def on_device(case, dev):
    if case.id not in _dev_cases:
        _dev_cases[case.id] = OnDevice(case, dev)
    return _dev_cases[case.id]


# ---- (a) point inputs, forward ------------------------------------------------------------------------------------------------------------
def check_forward(c, r, inp, zl, idx, wt, tag):
    assert ts.compare_taps(idx, wt, r.idx, r.wt, r.bounds["wt"], c.h * c.w) == []
    assert ts.compare_inputs(inp, r.in55, r.bounds, c.F) == []
    assert ts.compare_abs("zlat", zl, r.zlat, r.bounds["zlat"]) == []
    n = 7 + 8 * c.F
    for name, cols in ts.in_families(c.F).items():
        fam = name if not name.startswith("code") else name[:-1] + ("_low" if int(name.rsplit("f", 1)[1]) < 3 else "_high")
        fig(f"{tag}:{fam}", r.cpu_err[name], float(np.abs(inp[:, cols] - r.in55[:, cols]).max()), r.bounds[name])
    fig(f"{tag}:zlat", r.cpu_err["zlat"], float(np.abs(zl - r.zlat).max()), r.bounds["zlat"])
    fig(f"{tag}:weights", r.cpu_err["wt"], float(np.abs(wt - r.wt).max()), r.bounds["wt"])
    assert inp.shape[1] >= n


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", TRAIN_STAGE_CASES + ts.BOUNDARY_CASES[1:], ids=IDS(TRAIN_STAGE_CASES + ts.BOUNDARY_CASES[1:]))
def test_point_inputs_forward(case, mode, dev):
    """diner_train_point_inputs (bilinear / border) and _ix (the five other modes), from the NCHW and the NHWC latent"""
    d = on_device(case, dev)
    r = d.case.refs(mode)
    nchw = d.forward("std", mode, nhwc=0)
    nhwc = d.forward("std", mode, nhwc=1)
    check_forward(d.case, r, *nhwc, "fwd")
    for a, b, name in zip(nchw, nhwc, ("in56", "zlat", "idx", "weights")):
        assert ts.compare_bits(name, a.view(F32) if a.dtype == np.int32 else a, b.view(F32) if b.dtype == np.int32 else b) == []


GEN_FWD = GEN_CASES + ts.BOUNDARY_CASES[:1]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", GEN_FWD, ids=IDS(GEN_FWD))
def test_point_inputs_gen_forward(case, mode, dev):
    d = on_device(case, dev)
    check_forward(d.case, d.case.refs(mode), *d.forward("gen", mode), "fwd_gen")


def test_gen_at_the_standard_shape_equals_the_standard_entry(dev):
    """(num_freqs, C) = (6, 512), bilinear / border: the taps bit for bit; in and zlat (sinf against pe_sin, the same lookup) within the
    float32 bound of the standard entry's"""
    d = on_device(GEN_CASES[2], dev)
    r = d.case.refs(MODES[0])
    s_in, s_zl, s_idx, s_wt = d.forward("std", MODES[0])
    g_in, g_zl, g_idx, g_wt = d.forward("gen", MODES[0])
    assert np.array_equal(s_idx, g_idx) and ts.compare_bits("weights", s_wt, g_wt) == []
    assert ts.compare_inputs(g_in, s_in.astype(np.float64)[:, :55], r.bounds, 6) == []
    assert ts.compare_abs("zlat", g_zl, s_zl.astype(np.float64), r.bounds["zlat"]) == []


@pytest.mark.parametrize("entry", ["std", "gen"])
def test_sb_1_reads_the_second_scene(entry, dev):
    d = on_device(ts.SB2_CASE, dev)
    for mode in (MODES[0], MODES[4]):
        r0, r1 = d.case.refs(mode, sb=0, backward=False), d.case.refs(mode, sb=1, backward=False)
        assert not np.array_equal(r0.idx, r1.idx) and np.abs(r0.zlat - r1.zlat).max() > 0.1      # other cameras, another latent
        check_forward(d.case, r1, *d.forward(entry, mode, sb=1), "fwd_sb1")
        check_forward(d.case, r0, *d.forward(entry, mode, sb=0), "fwd_sb0")


# ---- (b) latent scatter and the layout change ---------------------------------------------------------------------------------------------
def run_scatter(d, mode, rs):
    """the kernel's own taps of the _gen forward -> diner_train_bilinear_scatter into scene 1 of a non-zero [2, NV, h, w, C] target"""
    c, dev = d.case, d.dev
    r = c.refs(mode)
    _, _, idx, wt = d.forward("gen", mode)
    assert ts.compare_taps(idx, wt, r.idx, r.wt, r.bounds["wt"], c.h * c.w) == []
    hw = c.h * c.w
    start = rs.standard_normal((2, c.NV, hw, c.C)).astype(F32)
    tgt, dz = T(start, dev), T(c.d_zlat[0], dev)
    call("diner_train_bilinear_scatter", P_(dz), P_(d.taps), c.P, c.C, c.h, c.w, c.NV, 1, P_(tgt), ST(dev))
    got = tgt.cpu().numpy()
    assert ts.compare_bits("scene 0 of the target", got[0], start[0]) == []
    # += onto the starting value: one more term of that magnitude in the element's sum
    bound = r.lat_bound + (r.lat_terms[..., None] + 1) * ts.U32 * np.abs(start[1]) * (r.lat_terms[..., None] > 0)
    assert ts.compare_abs("scatter", got[1], start[1].astype(np.float64) + r.lat_ref, bound) == []
    untouched = np.broadcast_to(r.lat_terms[..., None] == 0, got[1].shape)
    assert ts.compare_bits("untouched texels", got[1][untouched], start[1][untouched]) == []
    err = np.abs(got[1] - start[1].astype(np.float64) - r.lat_ref)
    fig("scatter (error / bound)", r.cpu_rel["latent"] / r.bounds["wt"], float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)), 1.0)
    return tgt, got


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", GEN_CASES, ids=IDS(GEN_CASES))
def test_scatter_and_layout(case, mode, dev):
    d = on_device(case, dev)
    c = d.case
    tgt, got = run_scatter(d, mode, np.random.RandomState(5))
    N, hw = 2 * c.NV, c.h * c.w                                                        # N = SB NV = 6 images
    out = torch.full((N, c.C, hw), NAN, device=dev)
    call("diner_train_nhwc_to_nchw", P_(tgt), N, c.C, c.h, c.w, P_(out), ST(dev))
    assert ts.compare_bits("nchw", out.cpu().numpy(), ts.nhwc_to_nchw_ref(got, N, c.C, hw)) == []


@pytest.mark.parametrize("case", [ts.SCATTER_CONTENTION, ts.SCATTER_ONE], ids=IDS([ts.SCATTER_CONTENTION, ts.SCATTER_ONE]))
def test_scatter_contention_and_a_lone_point(case, dev):
    """thousands of rows onto the six texels of a 2 x 3 map (every atomic contended), and P = 1"""
    d = on_device(case, dev)
    for mode in (MODES[0], MODES[1], MODES[5]):
        run_scatter(d, mode, np.random.RandomState(6))


# ---- (c) point inputs, backward -----------------------------------------------------------------------------------------------------------
def starts(c, rs):
    return dict(image_shape=rs.standard_normal(2).astype(F32), depths=rs.standard_normal((c.SB, c.NV, c.H, c.W)).astype(F32))


def check_backward(c, r, got, start, sb, tag, with_far=True):
    """every output of one call against float64 autograd"""
    exp = dict(r.grads)
    if not with_far:
        exp["rays"] = exp["rays"].copy()
        exp["rays"][:, 7] = 0.0
    for k in ("rays", "focal", "c"):
        if got[k] is None:
            continue
        assert ts.compare_scaled(k, got[k][sb], exp[k], r.scales[k], r.rel[k]) == []
        fig(f"{tag}:{k}", r.cpu_rel[k], ts.scaled_error(got[k][sb], exp[k], r.scales[k]), float(np.max(r.rel[k])))
    if got["rays"] is not None:
        assert np.all(got["rays"][sb][:, 6] == 0) and ts.compare_bits("d_far", got["rays"][sb][:, 7], exp["rays"][:, 7]) == []
    if got["poses"] is not None:
        assert ts.compare_scaled("poses", got["poses"][sb][:, :3], exp["poses"][:, :3], r.scales["poses"][:, :3], r.rel["poses"]) == []
        assert np.all(got["poses"][sb][:, 3] == SENTINEL)                            # row 3: untouched
        fig(f"{tag}:poses", r.cpu_rel["poses"], ts.scaled_error(got["poses"][sb][:, :3], exp["poses"][:, :3], r.scales["poses"][:, :3]), r.rel["poses"])
    if got["image_shape"] is not None:
        s0 = start["image_shape"].astype(np.float64)
        scale = r.scales["image_shape"] + np.abs(s0)
        assert ts.compare_scaled("image_shape", got["image_shape"], s0 + exp["image_shape"], scale, r.rel["image_shape"] + ts.U32) == []
        fig(f"{tag}:image_shape", r.cpu_rel["image_shape"], ts.scaled_error(got["image_shape"], s0 + exp["image_shape"], scale), r.rel["image_shape"])
    if got["depths"] is not None:
        s0 = start["depths"][sb].astype(np.float64)
        rows = r.scales["depth_rows"]
        scale = r.scales["depths"] + np.abs(s0) * (rows > 0)
        assert ts.compare_scaled("depths", got["depths"][sb], s0 + exp["depths"], scale, r.rel["depths"] + ts.U32) == []
        assert ts.compare_bits("untouched depth texels", got["depths"][sb][rows == 0], start["depths"][sb][rows == 0]) == []
        fig(f"{tag}:depths", r.cpu_rel["depths"], ts.scaled_error(got["depths"][sb], s0 + exp["depths"], scale), float(np.max(r.rel["depths"])))
    for k in ts.LEAVES:                                                               # the other scenes' parts: as they were
        if got[k] is not None and k != "image_shape":
            for s in range(c.SB):
                if s != sb:
                    rest = got[k][s]
                    assert np.isnan(rest).all() or np.all(rest == SENTINEL) or k == "depths"


def backward_and_rerun(d, entry, mode, tag):
    c = d.case
    r = c.refs(mode)
    st = starts(c, np.random.RandomState(8))
    got = d.backward(entry, mode, start=st)
    check_backward(c, r, got, st, 0, tag)
    if mode[0] == "nearest":                                                          # no grid gradient: nothing reaches the intrinsics
        assert np.all(got["focal"][0] == 0) and np.all(got["c"][0] == 0) and ts.compare_bits("image_shape", got["image_shape"], st["image_shape"]) == []
    again = d.backward(entry, mode, start=st)                                         # the reductions run in a fixed order
    for k in ("rays", "poses", "focal", "c", "image_shape"):
        assert ts.compare_bits(k + " of a second run", again[k], got[k]) == []
    return got, st


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", TRAIN_STAGE_CASES + ts.BOUNDARY_CASES[1:], ids=IDS(TRAIN_STAGE_CASES + ts.BOUNDARY_CASES[1:]))
def test_point_inputs_backward(case, mode, dev):
    backward_and_rerun(on_device(case, dev), "std", mode, "bwd")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", GEN_FWD, ids=IDS(GEN_FWD))
def test_point_inputs_backward_gen(case, mode, dev):
    backward_and_rerun(on_device(case, dev), "gen", mode, "bwd_gen")


@pytest.mark.parametrize("case", ts.REDUCE_CASES, ids=IDS(ts.REDUCE_CASES))
def test_camera_reduction_sizes(case, dev):
    """P <= 256 (one partial per view), P = 5 * 256 + 7 (a ragged last chunk), P = 256 * 256 + 300 (the CAMG_BLOCKS cap: chunks larger
    than a block)"""
    assert case.P in (117, 5 * 256 + 7, 256 * 256 + 300)
    backward_and_rerun(on_device(case, dev), "gen", MODES[0], "bwd_reduce")


@pytest.mark.parametrize("entry, case", [("std", TRAIN_STAGE_CASES[6]), ("gen", GEN_CASES[0])], ids=["std", "gen"])
def test_backward_output_pointers_null_in_turn(entry, case, dev):
    d = on_device(case, dev)
    c, mode = d.case, MODES[0]
    r = c.refs(mode)
    st = starts(c, np.random.RandomState(9))
    full = d.backward(entry, mode, start=st)
    for k in ts.LEAVES:
        got = d.backward(entry, mode, omit=(k,), start=st)
        assert got[k] is None
        check_backward(c, r, got, st, 0, "bwd_null")
        for o in ("rays", "poses", "focal", "c", "image_shape"):
            if o != k:
                assert ts.compare_bits(f"{o} without {k}", got[o], full[o]) == []
    got = d.backward(entry, mode, with_far=False, start=st)                           # d_far NULL: column 7 is 0
    assert np.all(got["rays"][0][:, 7] == 0)
    check_backward(c, r, got, st, 0, "bwd_null", with_far=False)


def test_backward_of_scene_1(dev):
    d = on_device(ts.SB2_CASE, dev)
    c = d.case
    for entry in ("std", "gen"):
        st = starts(c, np.random.RandomState(10))
        got = d.backward(entry, MODES[0], sb=1, start=st)
        check_backward(c, c.refs(MODES[0], sb=1), got, st, 1, "bwd_sb1")
        assert ts.compare_bits("scene 0's depth gradients", got["depths"][0], st["depths"][0]) == []


# ---- (d) view mean and head ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NV", [1, 2, 3, 4])
@pytest.mark.parametrize("PC", [1, 255, 257, 65 * 512])
def test_view_mean(PC, NV, dev):
    rs = np.random.RandomState(PC + NV)
    x = (rs.standard_normal((NV, PC)) * np.exp(rs.uniform(-3, 3, (NV, PC)))).astype(F32)
    out, xd = torch.full((PC,), NAN, device=dev), T(x, dev)
    call("diner_train_view_mean", P_(xd), PC, NV, P_(out), 0, ST(dev))
    tol = (NV + 1) * ts.EPS32 * np.abs(x.astype(np.float64)).sum(0) / NV             # (NV + 1) ulp of sum |x| / NV
    assert ts.compare_abs("view mean", out.cpu().numpy(), ts.view_mean_ref(x, NV), tol) == []
    g = x[0]
    dx, gd = torch.full((NV, PC), NAN, device=dev), T(g, dev)
    call("diner_train_view_mean", P_(gd), PC, NV, P_(dx), 1, ST(dev))
    ref = ts.view_mean_ref(g, NV, backward=True)
    assert ts.compare_abs("view mean backward", dx.cpu().numpy(), ref, ts.EPS32 * np.abs(ref)) == []      # 1 ulp


@pytest.mark.parametrize("n4", [4, 1020, 4 * 257, 4 * 1000 + 4])
def test_head(n4, dev):
    rs = np.random.RandomState(n4)
    v = rs.uniform(-100, 100, n4).astype(F32)
    v[: n4 // 2] = rs.standard_normal(n4 // 2).astype(F32)
    sig = np.arange(3, n4, 4)
    v[sig[::5]], v[sig[1::5]], v[sig[2::5]], v[sig[3::7]] = 0.0, -0.0, F32(-1e-30), F32(1e-30)   # the gate's neighbourhood
    v[0:3] = [0.0, -0.0, 100.0]
    assert n4 % 256
    out, vd = torch.full((n4,), NAN, device=dev), T(v, dev)             # (every device tensor is held in a name while a kernel reads it)
    call("diner_train_head", P_(vd), None, None, n4, P_(out), 0, ST(dev))
    y = out.cpu().numpy()
    ref = ts.head_ref(v)
    with np.errstate(over="ignore"):
        cpu = np.abs(ts.head_ref(v, F32).astype(np.float64) - ref)
    colour = (np.arange(n4) & 3) < 3
    tol = ts.MARGIN * cpu[colour].max() + ts.EPS32 * np.abs(ref) + 2.0 ** -149
    assert ts.compare_abs("head", y[colour], ref[colour], tol[colour]) == []
    assert np.array_equal(y[~colour], np.maximum(v[~colour], 0))                      # the relu: exact
    fig("head", float(cpu[colour].max()), float(np.abs(y - ref)[colour].max()), float(tol[colour].max()))
    g = (rs.standard_normal(n4) + 2.5).astype(F32)
    d_out, gd = torch.full((n4,), NAN, device=dev), T(g, dev)
    call("diner_train_head", P_(vd), P_(out), P_(gd), n4, P_(d_out), 1, ST(dev))
    got = d_out.cpu().numpy()
    ref_b = ts.head_bwd_ref(v, y, g)                                                  # of the saved y
    assert ts.compare_bits("sigma gate", got[~colour], ref_b[~colour].astype(F32)) == []                    # 0 at out <= 0, g otherwise
    assert ((v[~colour] <= 0) & (got[~colour] != 0)).sum() == 0 and (v[~colour] <= 0).sum() >= 1
    # g y (1 - y): three float32 roundings
    assert ts.compare_abs("colour gradient", got[colour], ref_b[colour], 4 * ts.U32 * np.abs(ref_b[colour]) + 2.0 ** -149) == []


# ---- (e) reductions -------------------------------------------------------------------------------------------------------------------------
def amax_word(x, dev, n=None):
    word = torch.full((1,), -1, dtype=torch.int32, device=dev)
    xt = T(x, dev)
    call("diner_train_amax", P_(xt), x.size if n is None else n, P_(word), ST(dev))
    return word.cpu().numpy().view(np.uint32)[0]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 256 * 2048 + 6])
def test_amax(n, dev):
    rs = np.random.RandomState(n % 1000)
    base = rs.standard_normal(n).astype(F32)
    bits = lambda a: np.array([np.abs(a).max()], F32).view(np.uint32)[0]
    for where, val in ((n - 1, 77.0), (0, 78.0), (n - 1, -79.0), (n // 2, -80.0), (None, None)):      # tail, first element, negative, as is
        x = base.copy()
        if where is not None:
            x[where] = val
        assert amax_word(x, dev) == bits(x) == ts.amax_ref(x).view(np.uint32), (n, where)
    sub = np.zeros(n, F32)
    sub[n - 1] = F32(-1e-40)                                                           # a subnormal maximum, in the tail
    assert amax_word(sub, dev) == bits(sub) != 0
    assert amax_word(np.zeros(n, F32), dev) == 0                                       # all zero: word 0
    assert amax_word(np.full(max(n, 4), 5.0, F32), dev, n=0) == 0                      # empty


def colsum_bound(dY, db0):
    """relative to sum |terms| (+ |db0|): 4 x the worse of a sequential and a pairwise float32 CPU sum + M x 2^-24"""
    ref = ts.colsum_ref(dY, db0)
    scale = ts.colsum_ref(dY, None, absolute=True) + np.abs(db0)
    seq = dY.sum(0, dtype=F32).astype(np.float64) + db0                               # (numpy adds rows of a C-ordered matrix in sequence)
    pair = np.ascontiguousarray(dY.T).sum(1, dtype=F32).astype(np.float64) + db0
    cpu = max(ts.scaled_error(seq, ref, scale), ts.scaled_error(pair, ref, scale))
    return ref, scale, ts.MARGIN * cpu + (dY.shape[0] + 1) * ts.U32, cpu


def strided(dY, pad, dev):
    """dY as a view of a wider matrix: ld = N + pad; the columns beside it hold NaN"""
    M, N = dY.shape
    wide = torch.full((M, N + pad), NAN, device=dev)
    wide[:, :N] = T(dY, dev)
    return wide, wide[:, :N]


COLSUM_SHAPES = [(M, N) for N in (4, 56, 100, 512) for M in (1, 255, 4097)] + [(512 * 4096 + 9, 4)]


@pytest.mark.parametrize("M, N", COLSUM_SHAPES)
def test_colsum(M, N, dev):
    rs = np.random.RandomState(M % 1000 + N)
    for kind, pad in (("random", 0), ("integers", 8), ("random", 3)):
        # integers: small whole numbers, whose partial sums are exact in float32 in any order -- a lost row shows in the last bit
        dY = rs.standard_normal((M, N)).astype(F32) if kind == "random" else rs.randint(-4, 5, (M, N)).astype(F32)
        db0 = (rs.standard_normal(N) * (1 + 0.05 * np.abs(dY).sum(0))).astype(F32) if kind == "random" else rs.randint(-9, 10, N).astype(F32)
        keep, view = strided(dY, pad, dev)
        db = T(db0, dev)
        call("diner_train_colsum", P_(view), M, N, view.stride(0), P_(db), ST(dev))
        got = db.cpu().numpy()
        ref, scale, rel, cpu = colsum_bound(dY, db0.astype(np.float64))
        assert ts.compare_scaled("colsum", got, ref, scale, rel) == []
        if kind == "integers":
            assert ts.compare_bits("colsum of whole numbers", got, ref.astype(F32)) == []
        else:
            fig("colsum", cpu, ts.scaled_error(got, ref, scale), rel)


COLSUM_AMAX_SHAPES = [(M, N) for N in (4, 8, 64, 512, 1024) for M in (1, 3, 4097)] + [(2048 * 256 + 5, 4)]     # the last: past 2048 x lanes


@pytest.mark.parametrize("M, N", COLSUM_AMAX_SHAPES)
def test_colsum_amax(M, N, dev):
    rs = np.random.RandomState(M % 1000 + N)
    for kind, pad in (("random", 0), ("integers", 4)):
        dY = rs.standard_normal((M, N)).astype(F32) if kind == "random" else rs.randint(-4, 5, (M, N)).astype(F32)
        dY[M - 1, N - 1] = -90.0 if kind == "random" else -5.0                         # the maximum: negative, last row, last column
        db0 = (rs.standard_normal(N) * (1 + 0.05 * np.abs(dY).sum(0))).astype(F32) if kind == "random" else rs.randint(-9, 10, N).astype(F32)
        keep, view = strided(dY, pad, dev)
        ref, scale, rel, cpu = colsum_bound(dY, db0.astype(np.float64))
        want = np.array([np.abs(dY).max()], F32).view(np.uint32)[0]
        for with_db, with_amax in ((True, True), (True, False), (False, True)):
            db = T(db0, dev) if with_db else None
            word = torch.full((1,), -1, dtype=torch.int32, device=dev) if with_amax else None
            call("diner_train_colsum_amax", P_(view), M, N, view.stride(0), P_(db), P_(word), ST(dev))
            if with_db:
                assert ts.compare_scaled("colsum_amax", db.cpu().numpy(), ref, scale, rel) == []
                if kind == "integers":
                    assert ts.compare_bits("colsum_amax of whole numbers", db.cpu().numpy(), ref.astype(F32)) == []
                else:
                    fig("colsum_amax", cpu, ts.scaled_error(db.cpu().numpy(), ref, scale), rel)
            if with_amax:
                assert word.cpu().numpy().view(np.uint32)[0] == want
