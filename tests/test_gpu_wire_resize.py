"""GPU tests of the image resizes (diner_amd/csrc/image_resize.hip through diner_amd/wire.py and diner_amd/glue.py) against the
restatement tests/wire_resize_ref.py, which tests/test_wire_resize_host.py ties to PIL, to ATen and to the reference's own statements.

Bars.  The integer resampler: byte-equal to the restatement and to PIL's stored output.  Nearest planes and alphas: bit-equal.  The float
resamplers against the float64 restatement on the same decoded source (the kernel's root of gammaCorrect is the correctly rounded one, as
the restatement's: the one-ulp convention of tests/wire_images_ref.py concerns the reference's decoded source and is applied there, in the
host test): twice the larger of ATen-fp32's own distance to float64 on the case (the fixture) and (n_w + n_h + 6) 2^-24 max|value|
(wire_resize_ref.float_bar); the cases without a stored distance (rows longer than a staged chunk, the full-size image) take the second
term alone, the smaller bar.  Every float test also shows that the comparison rejects a wrong kernel: on a downscale the
``antialias=False`` result misses the bar by a factor of 100 or more.
Two runs give the same bits; outputs pre-filled with NaN are fully overwritten; the aligned 4-pixel loads and the 1-pixel loads agree bit
for bit; glue.encoder_input / glue.encode from bytes with a size equal the same from the resized floats; refusals come before any launch.
Reads tests/golden only."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import wire_images_ref as W
from tests import wire_resize_ref as R
from tests.test_wire_resize_host import FORMATS, fixture, pil_source, source

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def fmt_of(name, sym):
    from diner_amd import wire
    rule, bg, gamma = W.FORMATS[name]
    return wire.ImageFormat(rule, bg, gamma, sym)


def bits(t):
    return t.detach().cpu().numpy()


def _st(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check_float(got, want64, bar, what):
    got = bits(got)
    err = float(np.abs(got.astype(np.float64) - want64).max())
    print(f"{what}: max |error| {err:.3e}, bar {bar:.3e}")
    assert got.shape == want64.shape and got.dtype == np.float32 and err <= bar, (what, err, bar)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", ["odd", "up", "mf", "one"])
def test_decode_resized_against_float64(case, fmt, dev):
    from diner_amd import wire
    fx = fixture()
    full, size = R.SIZES[case]
    px, a, sym = source(case, fmt)
    f = fmt_of(fmt, sym)
    outs = {}
    for aa in (True, False):
        want, want_a = R.decode_resized(px, a, fmt, sym, size, aa)
        rgb, alpha = wire.decode_image_u8(px, a, f, device=dev, size=size, antialias=aa)
        again = wire.decode_image_u8(px, a, f, device=dev, size=size, antialias=aa)
        bar = R.float_bar(fx[f"{case}/{fmt}/aa{int(aa)}/aten_distance"], full, size, np.abs(want).max(), aa)
        check_float(rgb, want, bar, f"{case}/{fmt}/aa{int(aa)}")
        assert torch.equal(rgb, again[0])                                            # two runs: the same bits
        if want_a is None:
            assert alpha is None
        else:
            assert np.array_equal(bits(alpha), want_a) and np.array_equal(bits(alpha), fx[f"{case}/{fmt}/alpha"]) and torch.equal(alpha, again[1])
        outs[aa] = (rgb, want, bar)
    if case in ("odd", "mf"):           # a downscale: the other filter is a wrong kernel, and the comparison says so
        miss = float(np.abs(bits(outs[False][0]).astype(np.float64) - outs[True][1]).max())
        assert miss > 100 * outs[True][2], (miss, outs[True][2])


@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_is_the_unresized_decode(fmt, dev):
    from diner_amd import glue, wire
    px, a, sym = source("ident", fmt)
    f = fmt_of(fmt, sym)
    plain = wire.decode_image_u8(px, a, f, device=dev)
    same = wire.decode_image_u8(px, a, f, device=dev, size=R.SIZES["ident"][1])
    assert torch.equal(plain[0], same[0]) and (plain[1] is None) == (same[1] is None) and (plain[1] is None or torch.equal(plain[1], same[1]))
    assert W.compare(bits(same[0]), W.decode_image(px, a, *W.FORMATS[fmt], sym)[0]) == ""
    pxd = torch.from_numpy(px).to(dev)
    ad = None if a is None else torch.from_numpy(a).to(dev)
    assert torch.equal(glue.encoder_input(pxd, 4, 2, alpha=ad, image_format=f, size=(33, 64)), glue.encoder_input(pxd, 4, 2, alpha=ad, image_format=f))
    # the kernels themselves at the identity's tables copy the decode too (weights 1 and 0)
    L, lib = wire._lib.lib(), wire._lib
    N, H, Wd, Cc = px.shape
    (bx, wx, tx), (by, wy, ty) = wire.resize_table(Wd, Wd, "bilinear_aa", dev), wire.resize_table(H, H, "bilinear_aa", dev)
    tmp, rgb = torch.empty((N, 3, H, Wd), device=dev), torch.full((N, 3, H, Wd), float("nan"), device=dev)
    lib.check(L.diner_decode_image_u8_resized(pxd.data_ptr(), None if ad is None else ad.data_ptr(), N, H, Wd, Cc, lib.BG_RULES[f.bg_rule], f.bg,
                                              int(f.gamma), int(f.symmetric_range), H, Wd, bx.data_ptr(), wx.data_ptr(), tx, by.data_ptr(),
                                              wy.data_ptr(), ty, tmp.data_ptr(), rgb.data_ptr(), None, _st(dev)), "resized")
    assert torch.equal(rgb, plain[0])


@pytest.mark.parametrize("Wd", [2500, 2501])
def test_rows_longer_than_a_staged_chunk_and_two_column_tiles(Wd, dev):
    """2500 -> 300 columns: the first tile's 256 columns read more than 2048 source pixels (two chunks), the second tile starts inside the
    row; width 2500 takes the 4-pixel loads, 2501 the 1-pixel loads"""
    from diner_amd import wire
    rs = np.random.RandomState(Wd)
    px = rs.randint(0, 256, (2, 3, Wd, 3)).astype(np.uint8)
    a = np.array([0, 127, 128, 254, 255], np.uint8)[rs.randint(0, 5, (2, 3, Wd))]
    size = (2, 300)
    want, want_a = R.decode_resized(px, a, "multiface", True, size)
    rgb, alpha = wire.decode_image_u8(px, a, wire.MULTIFACE_RGB._replace(symmetric_range=True), device=dev, size=size)
    check_float(rgb, want, R.float_bar(0.0, (3, Wd), size, np.abs(want).max()), f"W={Wd}")
    assert np.array_equal(bits(alpha), want_a)
    plain = R.decode_resized(px, a, "multiface", True, size, False)[0]
    assert np.abs(plain - want).max() > 100 * R.float_bar(0.0, (3, Wd), size, 1.0)


def test_full_size_multiface_image(dev):
    """2048 x 1334 -> 256 x 160 (N = 1): more rows than a workgroup's, every column in one tile"""
    from diner_amd import wire
    rs = np.random.RandomState(5)
    H, Wd = 2048, 1334
    size = wire.multiface_size(H, Wd)
    assert size == (256, 160)
    px = rs.randint(0, 256, (1, H, Wd, 3)).astype(np.uint8)
    a = np.array([0, 254, 255, 255, 255], np.uint8)[rs.randint(0, 5, (1, H, Wd))]
    want, want_a = R.decode_resized(px, a, "multiface", False, size)
    pxd, ad = torch.from_numpy(px).to(dev), torch.from_numpy(a).to(dev)
    rgb, alpha = wire.decode_multiface_image(pxd, ad, device=dev, size=size)
    check_float(rgb, want, R.float_bar(0.0, (H, Wd), size, np.abs(want).max()), "2048x1334")
    assert np.array_equal(bits(alpha), want_a)
    again = wire.decode_multiface_image(pxd, ad, device=dev, size=size)
    assert torch.equal(rgb, again[0]) and torch.equal(alpha, again[1])


def test_both_load_paths_agree_and_every_element_is_written(dev):
    """33 x 64 from an aligned base: four pixels per load; the same bytes at an odd address: one pixel per load; NaN-filled outputs"""
    from diner_amd import _lib
    L = _lib.lib()
    from diner_amd import wire
    px4 = fixture()["ident/pixels"]
    N, H, Wd, _ = px4.shape
    h, w = 16, 20
    (bx, wx, tx), (by, wy, ty) = wire.resize_table(Wd, w, "bilinear_aa", dev), wire.resize_table(H, h, "bilinear_aa", dev)
    results = []
    for Cc, rule, gamma in ((4, 1, 0), (3, 2, 1)):
        px = np.ascontiguousarray(px4[..., :Cc])
        plane = np.ascontiguousarray(px4[..., 3]) if Cc == 3 else None
        for odd in (False, True):
            buf = torch.empty(px.size + 32, dtype=torch.uint8, device=dev)
            p = buf[16 + odd:16 + odd + px.size].view(px.shape)
            p.copy_(torch.from_numpy(px))
            assert p.data_ptr() % 16 == int(odd)
            pl = None
            if plane is not None:
                pl = torch.empty(plane.size + 32, dtype=torch.uint8, device=dev)[16 + odd:16 + odd + plane.size].view(plane.shape)
                pl.copy_(torch.from_numpy(plane))
            tmp = torch.full((N, 3, H, w), float("nan"), device=dev)
            rgb, a = torch.full((N, 3, h, w), float("nan"), device=dev), torch.full((N, 1, h, w), float("nan"), device=dev)
            _lib.check(L.diner_decode_image_u8_resized(p.data_ptr(), None if pl is None else pl.data_ptr(), N, H, Wd, Cc, rule, 1.0, gamma, 1, h, w,
                                                       bx.data_ptr(), wx.data_ptr(), tx, by.data_ptr(), wy.data_ptr(), ty, tmp.data_ptr(),
                                                       rgb.data_ptr(), a.data_ptr(), _st(dev)), "resized")
            assert not bool(torch.isnan(tmp).any()) and not bool(torch.isnan(rgb).any()) and not bool(torch.isnan(a).any())
            results.append((rgb, a))
        assert torch.equal(results[-1][0], results[-2][0]) and torch.equal(results[-1][1], results[-2][1])
    d16 = torch.from_numpy(fixture()["sample/depth"].view(np.int16)).to(dev)
    outs = [torch.full((d16.shape[0], 1, 9, 80), float("nan"), device=dev) for _ in range(3)]
    _lib.check(L.diner_decode_depth_u16_mf_nearest(d16.data_ptr(), None, d16.shape[0], d16.shape[1], d16.shape[2], 9, 80, 1e-4, 0.0, 0.0, 1e-3,
                                                   *[o.data_ptr() for o in outs], _st(dev)), "nearest")
    assert not any(bool(torch.isnan(o).any()) for o in outs)


@pytest.mark.parametrize("name", list(R.PIL_SIZES))
def test_resize_u8_equals_pil(name, dev):
    from diner_amd import wire
    full, size = R.PIL_SIZES[name]
    for C_ in (3, 1):
        src = pil_source(name, C_)
        got = wire.resize_u8(src, size, device=dev)
        assert got.dtype == torch.uint8 and np.array_equal(bits(got), fixture()[f"pil/{name}/c{C_}"])
        assert np.array_equal(bits(got), R.resize_pil_u8(src, size)) and torch.equal(got, wire.resize_u8(src, size, device=dev))
    flat = wire.resize_u8(src[0, ..., 0], size, device=dev)                         # [H, W]
    assert flat.shape == size and torch.equal(flat, got[0, ..., 0])
    assert torch.equal(wire.resize_u8(src, full, device=dev), torch.from_numpy(src).to(dev))      # no pass at all: a copy


def test_dtu_downsample(dev):
    """DTU's shape, 512 x 640 -> 256 x 320 (dtu.py:81-82 at downsample = .5), and an odd one, where int() truncates"""
    from diner_amd import wire
    rs = np.random.RandomState(9)
    px = rs.randint(0, 256, (512, 640, 3)).astype(np.uint8)
    px[100:200, 300:500] = 255
    px[300:310] = 0
    small = R.resize_pil_u8(px, (256, 320))
    got = wire.decode_dtu_rgb(px, symmetric_range=True, downsample=.5, device=dev)
    assert got.shape == (1, 3, 256, 320) and W.compare(bits(got), W.decode_image(small, None, "none", 1.0, False, True)[0]) == ""
    assert torch.equal(got, wire.decode_dtu_rgb(wire.resize_u8(px, (256, 320), device=dev), symmetric_range=True, device=dev))
    odd = fixture()["odd/pixels"][..., :3]
    got = wire.decode_dtu_rgb(odd, downsample=.5, device=dev)
    assert got.shape == (3, 3, 18, 26) and W.compare(bits(got), W.decode_image(fixture()["pil/odd/c3"], None, "none", 1.0, False, False)[0]) == ""
    assert torch.equal(wire.decode_dtu_rgb(odd, downsample=None, device=dev), wire.decode_dtu_rgb(odd, device=dev))


def test_multiface_sample(dev):
    """a sample as multiface.py:341-359 leave it: the images under the float bar, the rest bit-equal to the reference's outputs"""
    from diner_amd import wire
    fx = fixture()
    px = fx["sample/pixels"]
    H, Wd = px.shape[1:3]
    size = wire.multiface_size(H, Wd, int(fx["sample/downsample"]))
    assert size == tuple(fx["sample/size"])
    rgb8, a8 = np.ascontiguousarray(px[..., :3]), np.ascontiguousarray(px[..., 3])
    for aa in (True, False):
        key = f"sample/aa{int(aa)}"
        rgb, alpha = wire.decode_multiface_image(rgb8, a8, device=dev, size=size, antialias=aa)
        want = R.decode_resized(rgb8, a8, "multiface", False, size, aa)[0]
        check_float(rgb, want, R.float_bar(fx[f"{key}/aten_distance"], (H, Wd), size, np.abs(want).max(), aa), key)
        assert np.array_equal(bits(alpha), np.concatenate([fx[f"{key}/src_alphas"], fx[f"{key}/target_alpha"][None]]))
        d, s, m = wire.decode_multiface(fx["sample/depth"], fx["sample/conf"], size=size, device=dev, want_mask=True)
        assert np.array_equal(bits(d), fx[f"{key}/src_depths"]) and np.array_equal(bits(s), fx[f"{key}/src_depth_stds"])
        assert np.array_equal(bits(m), (fx[f"{key}/src_depths"] > 0).astype(np.float32))
        K = wire.scale_intrinsics(torch.from_numpy(fx["sample/intrinsics"]).to(dev), (H, Wd), size)
        assert np.array_equal(bits(K), np.concatenate([fx[f"{key}/src_intrinsics"], fx[f"{key}/target_intrinsics"][None]]))


@pytest.mark.parametrize("size", [(32, 32), (80, 100), (53, 20), (1, 1)])
def test_nearest_planes(size, dev):
    from diner_amd import wire
    fx = fixture()
    d16, c16 = fx["sample/depth"], fx["sample/conf"]
    for conf in (None, c16):
        want = [R.resize_nearest(x, size) for x in W.decode_multiface_depth(d16, conf)]
        got = wire.decode_multiface(d16, conf, size=size, device=dev, want_mask=True)
        assert all(g.shape == (d16.shape[0], 1) + size and np.array_equal(bits(g), w) for g, w in zip(got, want))
        assert (bits(got[1])[bits(got[0]) == 0] == 0).all()                            # the zero-depth rule, on the selected texel
        assert all(torch.equal(g, h) for g, h in zip(got, wire.decode_multiface(d16, conf, size=size, device=dev, want_mask=True)))
    same = wire.decode_multiface(d16, c16, size=d16.shape[1:], device=dev)
    assert all(torch.equal(g, h) for g, h in zip(same, wire.decode_multiface(d16, c16, device=dev)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_encoder_input_from_bytes_with_a_size(fmt, dev):
    from diner_amd import glue, wire
    px, a, sym = source("odd", fmt)
    f = fmt_of(fmt, sym)
    pxd = torch.from_numpy(px).to(dev)
    ad = None if a is None else torch.from_numpy(a).to(dev)
    for aa in (True, False):
        rgb = wire.decode_image_u8(pxd, ad, f, device=dev, size=(18, 26), antialias=aa)[0]
        for pad, pe in ((0, -1), (4, 2)):
            got = glue.encoder_input(pxd, pad, pe, alpha=ad, image_format=f, size=(18, 26), antialias=aa)
            assert got.shape == (3, 3 + (10 if pad else 0), 18 + 2 * pad, 26 + 2 * pad) and torch.equal(got, glue.encoder_input(rgb, pad, pe))


def test_encode_from_bytes_with_a_size(dev):
    from diner_amd import glue, wire
    from tests import test_gpu_encode as E
    s = E.scene(dev)
    g = torch.Generator().manual_seed(62)
    H, Wd = 2 * E.H + 3, 3 * E.W + 1
    px = torch.randint(0, 256, (E.SB, E.NV, H, Wd, 4), generator=g, dtype=torch.uint8).to(dev)
    fmt = wire.FACESCAPE_RGBA
    rgb = wire.decode_image_u8(px.flatten(0, 1), None, fmt, device=dev, size=(E.H, E.W))[0].reshape(E.SB, E.NV, 3, E.H, E.W)
    m = E.model(dev).eval()
    with torch.no_grad():
        glue.encode(m, rgb, *E.args(s)[1:])
        want = m.encoder.latent.clone()
        m.encoder.latent = None
        assert glue.encode(m, px, *E.args(s)[1:], image_format=fmt, image_size=(E.H, E.W)) is None
    assert glue.latent_is_packed(m.encoder.latent) and torch.equal(m.encoder.latent, want) and float(want.abs().max()) > 0
    assert m.image_shape.tolist() == [E.W, E.H] and m.encoder.normals.shape == (E.SB, E.NV, 3, E.H, E.W)


def test_refusals_come_before_any_launch(dev):
    from diner_amd import _lib, glue, wire
    L = _lib.lib()
    px = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=dev)
    d16 = torch.zeros((1, 8, 8), dtype=torch.int16, device=dev)
    out = torch.full((4096,), float("nan"), device=dev)             # large enough for every call below, should one launch
    out8 = torch.full((4096,), 171, dtype=torch.uint8, device=dev)
    (bx, wx, tx), (kb, kw, kt) = wire.resize_table(8, 4, "bilinear_aa", dev), wire.resize_table(8, 4, "bicubic_u8", dev)
    st, P, O, O8 = _st(dev), px.data_ptr(), out.data_ptr(), out8.data_ptr()
    B, Wt, KB, KW = bx.data_ptr(), wx.data_ptr(), kb.data_ptr(), kw.data_ptr()
    img = lambda **k: L.diner_decode_image_u8_resized(k.get("px", P), None, k.get("N", 1), 8, k.get("W", 8), k.get("C", 4), k.get("rule", 0), 1.0, 0, 0,
                                                      k.get("h", 4), 4, k.get("bx", B), Wt, k.get("tx", tx), B, k.get("wy", Wt), tx,
                                                      k.get("tmp", O), k.get("rgb", O), k.get("a_out"), st)
    u8 = lambda **k: L.diner_resize_u8(k.get("px", P), 1, 8, 8, k.get("C", 3), k.get("h", 4), k.get("w", 4), k.get("kb", KB), KW, k.get("kt", kt),
                                       KB, k.get("kw", KW), kt, k.get("tmp", O8), k.get("out", O8), st)
    mf = lambda **k: L.diner_decode_depth_u16_mf_nearest(k.get("d", d16.data_ptr()), None, k.get("N", 1), 8, 8, k.get("h", 4), k.get("w", 4), 1e-4,
                                                         0.0, 0.0, 1e-3, k.get("o", O), k.get("s", O), None, st)
    refused = [img(px=None), img(rgb=None), img(tmp=None), img(bx=None), img(wy=None), img(C=5), img(C=1), img(C=3, rule=2), img(rule=3),
               img(C=3, a_out=O), img(h=0), img(W=0), img(N=0), img(tx=0),
               u8(px=None), u8(out=None), u8(C=4), u8(C=2), u8(h=0), u8(w=-1), u8(kb=None), u8(kw=None), u8(kt=0), u8(tmp=None),
               mf(d=None), mf(o=None), mf(s=None), mf(h=0), mf(w=0), mf(N=0)]
    assert refused == [-1] * len(refused)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((out8 == 171).all())            # nothing was launched
    assert u8(h=8, tmp=None) == 0 and img(tmp=O + 4 * 2048) == 0                  # (one pass needs no tmp)
    torch.cuda.synchronize()
    assert not bool((out8[:96] == 171).all()) and bool((out8[96:] == 171).all())
    # the Python layer
    rgb3 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    for bad in (lambda: wire.resize_u8(px, (4, 4), device=dev),                                       # RGBA: PIL premultiplies
                lambda: wire.resize_u8(rgb3, (4, 4), resample="bilinear", device=dev),
                lambda: wire.resize_u8(rgb3, (0, 4), device=dev),
                lambda: wire.resize_u8(rgb3, 4, device=dev),
                lambda: wire.decode_image_u8(rgb3, device=dev, size=(4, -1)),
                lambda: wire.decode_image_u8(rgb3, fmt=wire.MULTIFACE_RGB, device=dev, size=(4, 4)),    # a rule without an alpha
                lambda: wire.decode_multiface(d16, size=(4, 4), stride=2, device=dev),
                lambda: wire.decode_multiface(d16, size=(4, 0), device=dev),
                lambda: glue.encoder_input(torch.zeros((1, 3, 8, 8), device=dev), 4, 2, size=(4, 4)),
                lambda: glue.encoder_input(rgb3, 4, 2, image_format=wire.DTU_RGB, size=(4,))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU only"):
        wire.resize_u8(np.zeros((8, 8, 3), np.uint8), (4, 4), device="cpu")
    from tests import test_gpu_encode as E
    s, m = E.scene(dev), E.model(dev).eval()
    with pytest.raises(ValueError):
        glue.encode(m, *E.args(s), image_size=(E.H, E.W))                           # float images take no size
    assert m.encoder.latent is None and m.poses is None
