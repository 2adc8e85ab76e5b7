"""GPU tests of the image wire format and Multiface's depth planes (diner_amd/csrc/image_wire.hip through diner_amd/wire.py and
diner_amd/glue.py): every case of tests/golden/wire_images.npz (outputs of the reference's own readers) through wire.*, bit-equal to the
restatement tests/wire_images_ref.py -- and hence to the reference under the bars of tests/test_wire_images_host.py: bit-equal, except
one ulp of gammaCorrect's root inside the fixture's mask.  The 4-pixel and the 1-pixel path agree bit for bit; every output element is
written; glue.encoder_input and glue.encode from bytes equal the same from the decoded floats; the refusals come before any launch.
Reads tests/golden only."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import wire_images_ref as R
from tests.test_wire_images_host import CASES, DEPTH_CASES, fixture, image_variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def fmt_of(kw):
    from diner_amd import wire
    return wire.ImageFormat(kw["bg_rule"], kw["bg"], kw["gamma"], kw["symmetric_range"])


def through_wire(key, kw, dev):
    """a fixture variant through the wrapper named after the reader it replaces"""
    from diner_amd import wire
    dataset, sym = key.split("/")[1], kw["symmetric_range"]
    if dataset == "facescape":
        return wire.decode_facescape_rgba(kw["pixels"], symmetric_range=sym, bg=kw["bg"], device=dev)
    if dataset == "dtu":
        return wire.decode_dtu_rgb(kw["pixels"], symmetric_range=sym, device=dev), None
    return wire.decode_multiface_image(kw["pixels"], kw["alpha"], symmetric_range=sym, device=dev)


def bits(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_fixture_case_through_wire(case, dev):
    fx = fixture()
    for key, kw, mkey in image_variants(case):
        rgb, a = through_wire(key, kw, dev)
        want_rgb, want_a = R.decode_image(**kw)
        assert R.compare(bits(rgb), want_rgb) == "", key                                            # the restatement: bit for bit
        assert R.compare(bits(rgb), fx[key + "/rgb"], None if mkey is None else fx[mkey]) == "", key   # the reference: its bars
        if key + "/alpha" in fx:
            assert R.compare(bits(a), want_a) == "" and R.compare(bits(a), fx[key + "/alpha"]) == "", key
        else:
            assert a is None


@pytest.mark.parametrize("case", list(DEPTH_CASES))
def test_multiface_depth(case, dev):
    from diner_amd import wire
    fx = fixture()
    conf = None if DEPTH_CASES[case] is None else fx[f"depth/{DEPTH_CASES[case]}"]
    d, s, m = wire.decode_multiface(fx["depth/depth"], conf, device=dev, want_mask=True)
    assert d.shape == s.shape == m.shape == (2, 1, 48, 48)
    assert R.compare(bits(d), fx[f"depth/{case}/depth"]) == "" and R.compare(bits(s), fx[f"depth/{case}/std"]) == ""
    assert np.array_equal(bits(m), (fx[f"depth/{case}/depth"] > 0).astype(np.float32))
    for stride in (2, 3):
        want = R.decode_multiface_depth(fx["depth/depth"], conf, stride=stride)
        got = wire.decode_multiface(fx["depth/depth"], conf, stride=stride, device=dev, want_mask=True)
        assert got[0].shape == (2, 1, 48 // stride, 48 // stride)
        assert all(R.compare(bits(g), w) == "" for g, w in zip(got, want)), stride
    if conf is None:
        s2 = wire.decode_multiface(fx["depth/depth"], None, 2.5e-3, device=dev)[1]
        assert R.compare(bits(s2), R.decode_multiface_depth(fx["depth/depth"], None, const_std=2.5e-3)[1]) == ""


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("dataset", ["facescape", "dtu", "multiface"])
def test_both_paths_agree(dataset, N, dev):
    """width 64: four pixels per thread; width 7, or the same bytes at an odd address: one pixel per thread"""
    from diner_amd import wire
    fx = fixture()
    rule, bg, gamma = R.FORMATS[dataset]
    fmt = wire.ImageFormat(rule, bg, gamma, True)
    for case, vec in (("rand33x64", True), ("rand5x7", False)):
        px = fx[f"{case}/pixels"][:N]
        a = np.ascontiguousarray(px[..., 3]) if dataset == "multiface" else None
        px = np.ascontiguousarray(px[..., :3]) if dataset != "facescape" else px
        want = R.decode_image(px, a, rule, bg, gamma, True)
        got = wire.decode_image_u8(px, a, fmt, device=dev)
        again = wire.decode_image_u8(px, a, fmt, device=dev)
        assert R.compare(bits(got[0]), want[0]) == "" and torch.equal(got[0], again[0])              # two runs: the same bits
        if want[1] is not None:
            assert R.compare(bits(got[1]), want[1]) == "" and torch.equal(got[1], again[1])
        if not vec:
            continue
        # the same bytes one byte into a larger allocation: no aligned load is possible
        buf = torch.empty(px.size + 1 + 15, dtype=torch.uint8, device=dev)
        odd = buf[1:1 + px.size].view(px.shape)
        odd.copy_(torch.from_numpy(px))
        assert odd.data_ptr() % 2 == 1 and torch.from_numpy(px).to(dev).data_ptr() % 16 == 0
        abuf = None
        if a is not None:
            abuf = torch.empty(a.size + 16, dtype=torch.uint8, device=dev)[1:1 + a.size].view(a.shape)
            abuf.copy_(torch.from_numpy(a))
        slow = wire.decode_image_u8(odd, abuf, fmt, device=dev)
        assert torch.equal(slow[0], got[0]) and (slow[1] is None or torch.equal(slow[1], got[1]))


def test_three_dimensional_input_and_want_alpha(dev):
    from diner_amd import wire
    px = fixture()["ramp/pixels"][0]
    rgb, a = wire.decode_image_u8(px, fmt=wire.FACESCAPE_RGBA, device=dev)
    assert rgb.shape == (1, 3, 16, 16) and a.shape == (1, 1, 16, 16)
    assert wire.decode_image_u8(px, fmt=wire.FACESCAPE_RGBA, want_alpha=False, device=dev)[1] is None
    assert wire.decode_image_u8(torch.from_numpy(px[..., :3].copy()), fmt=wire.DTU_RGB, device=dev)[1] is None
    assert wire.FACESCAPE_RGBA._replace(symmetric_range=True, bg=0.) == wire.ImageFormat("below_half", 0., False, True)
    assert wire.DTU_RGB.bg_rule == "none" and wire.MULTIFACE_RGB == wire.ImageFormat("below_one", 1.0, True, False)
    with pytest.raises(AttributeError):
        wire.DTU_RGB.gamma = True


def _st(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("case", ["rand33x64", "rand5x7", "one"])
def test_every_output_element_is_written(case, dev):
    from diner_amd import _lib
    fx = fixture()
    px = torch.from_numpy(fx[f"{case}/pixels"]).to(dev)
    N, H, W, _ = px.shape
    rgb = torch.full((N, 3, H, W), float("nan"), device=dev)
    a = torch.full((N, 1, H, W), float("nan"), device=dev)
    _lib.check(_lib.lib().diner_decode_image_u8(px.data_ptr(), None, N, H, W, 4, 1, 1.0, 0, 0, rgb.data_ptr(), a.data_ptr(), _st(dev)), "decode")
    assert not bool(torch.isnan(rgb).any()) and not bool(torch.isnan(a).any())
    # three channels with the alpha in a plane of its own (the gamma format), and the same source through the encoder's head
    px3, plane = px[..., :3].contiguous(), px[..., 3].contiguous()
    rgb.fill_(float("nan")), a.fill_(float("nan"))
    _lib.check(_lib.lib().diner_decode_image_u8(px3.data_ptr(), plane.data_ptr(), N, H, W, 3, 2, 1.0, 1, 1, rgb.data_ptr(), a.data_ptr(), _st(dev)),
               "decode")
    assert not bool(torch.isnan(rgb).any()) and not bool(torch.isnan(a).any())
    pad = 3
    xs, ys = torch.linspace(-1, 1, W + 2 * pad, device=dev), torch.linspace(-1, 1, H + 2 * pad, device=dev)
    for C_, src, pl, rule in ((3, px3, plane.data_ptr(), 2), (4, px, None, 1)):
        x = torch.full((N, 3 + 6, H + 2 * pad, W + 2 * pad), float("nan"), device=dev)
        _lib.check(_lib.lib().diner_encoder_input_u8(src.data_ptr(), pl, C_, rule, 1.0, int(C_ == 3), 0, N, H, W, pad, 1, xs.data_ptr(), ys.data_ptr(),
                                                     0.485, 0.456, 0.406, 0.229, 0.224, 0.225, x.data_ptr(), _st(dev)), "encoder_input_u8")
        assert not bool(torch.isnan(x).any()), C_
    conf = torch.from_numpy(fx["depth/conf"].view(np.int16)).to(dev)
    d16 = torch.from_numpy(fx["depth/depth"].view(np.int16)).to(dev)
    outs = [torch.full((2, 1, 24, 24), float("nan"), device=dev) for _ in range(3)]
    _lib.check(_lib.lib().diner_decode_depth_u16_mf(d16.data_ptr(), None, 2, 48, 48, 2, 1e-4, 0.0, 0.0, 1e-3, *[o.data_ptr() for o in outs],
                                                    _st(dev)), "decode_mf")
    assert not any(bool(torch.isnan(o).any()) for o in outs)
    for o in outs:
        o.fill_(float("nan"))
    _lib.check(_lib.lib().diner_decode_depth_u16_mf(d16.data_ptr(), conf.data_ptr(), 2, 48, 48, 2, 1e-4, -1.582e-2, 1.649e-2, 1e-3,
                                                    *[o.data_ptr() for o in outs], _st(dev)), "decode_mf")
    assert not any(bool(torch.isnan(o).any()) for o in outs)


@pytest.mark.parametrize("dataset", ["facescape", "dtu", "multiface"])
def test_encoder_input_from_bytes(dataset, dev):
    from diner_amd import glue, wire
    fx = fixture()
    rule, bg, gamma = R.FORMATS[dataset]
    for case in ("ramp_rev", "rand5x7"):                      # 16 x 16 (N = 1) and 5 x 7 (N = 3)
        px = fx[f"{case}/pixels"]
        a = torch.from_numpy(np.ascontiguousarray(px[..., 3])).to(dev) if dataset == "multiface" else None
        px = torch.from_numpy(np.ascontiguousarray(px[..., :3]) if dataset != "facescape" else px).to(dev)
        for sym in (False, True):
            fmt = wire.ImageFormat(rule, bg, gamma, sym)
            rgb = wire.decode_image_u8(px, a, fmt, device=dev)[0]
            for pad in (0, 4):
                for pe in (-1, 2):
                    want = glue.encoder_input(rgb, pad, pe)
                    got = glue.encoder_input(px, pad, pe, alpha=a, image_format=fmt)
                    assert got.shape == want.shape == (px.shape[0], 3 + (10 if pad and pe >= 0 else 0), px.shape[1] + 2 * pad, px.shape[2] + 2 * pad)
                    assert torch.equal(got, want), (case, sym, pad, pe)
    # leading dimensions [SB, NV, ...] and other constants
    px5 = px.reshape(1, 3, *px.shape[1:])
    a5 = None if a is None else a.reshape(1, 3, *a.shape[1:])
    got = glue.encoder_input(px5, 4, 2, [0.1, 0.2, 0.3], [0.5, 1.5, 2.0], alpha=a5, image_format=fmt)
    assert torch.equal(got, glue.encoder_input(rgb, 4, 2, [0.1, 0.2, 0.3], [0.5, 1.5, 2.0]))


def test_encode_from_bytes(dev):
    from diner_amd import glue, wire
    from tests import test_gpu_encode as E
    s = E.scene(dev)
    g = torch.Generator().manual_seed(61)
    px = torch.randint(0, 256, (E.SB, E.NV, E.H, E.W, 4), generator=g, dtype=torch.uint8).to(dev)
    fmt = wire.FACESCAPE_RGBA
    rgb = wire.decode_image_u8(px.flatten(0, 1), None, fmt, device=dev)[0].reshape(E.SB, E.NV, 3, E.H, E.W)
    m = E.model(dev).eval()
    with torch.no_grad():
        glue.encode(m, rgb, *E.args(s)[1:])
        want = m.encoder.latent.clone()
        m.encoder.latent = None
        assert glue.encode(m, px, *E.args(s)[1:], image_format=fmt) is None
    assert glue.latent_is_packed(m.encoder.latent) and torch.equal(m.encoder.latent, want) and float(want.abs().max()) > 0
    assert m.image_shape.tolist() == [E.W, E.H] and m.encoder.normals.shape == (E.SB, E.NV, 3, E.H, E.W)


def test_refusals_come_before_any_launch(dev):
    from diner_amd import _lib, glue, wire
    L = _lib.lib()
    px = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=dev)
    plane = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev)
    d16 = torch.zeros((1, 8, 8), dtype=torch.int16, device=dev)
    out = torch.full((1, 13, 16, 16), float("nan"), device=dev)     # large enough for every call below, should one launch
    st, P, O = _st(dev), px.data_ptr(), out.data_ptr()
    xs = torch.linspace(-1, 1, 16, device=dev)
    img = lambda **k: L.diner_decode_image_u8(k.get("px", P), k.get("alpha"), 1, 8, 8, k.get("C", 4), k.get("rule", 0), 1.0, 0, 0,
                                              k.get("rgb", O), k.get("a_out"), st)
    enc = lambda **k: L.diner_encoder_input_u8(k.get("px", P), k.get("alpha"), k.get("C", 4), k.get("rule", 0), 1.0, 0, 0, 1, 8, 8, 4, 2,
                                               xs.data_ptr(), xs.data_ptr(), 0.5, 0.5, 0.5, 0.2, 0.2, 0.2, k.get("out", O), st)
    mf = lambda **k: L.diner_decode_depth_u16_mf(k.get("d", d16.data_ptr()), None, 1, 8, 8, k.get("stride", 1), 1e-4, 0.0, 0.0, 1e-3,
                                                 k.get("o", O), k.get("s", O), None, st)
    refused = [img(px=None), img(rgb=None), img(C=5), img(C=2), img(C=3, rule=1), img(C=3, rule=2), img(rule=3), img(C=3, a_out=O),
               enc(px=None), enc(out=None), enc(C=5), enc(C=3, rule=1), enc(C=3, rule=2),
               mf(d=None), mf(o=None), mf(s=None), mf(stride=3), mf(stride=0)]
    assert refused == [-1] * len(refused)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                           # nothing was launched: every call above would have written into `out`
    assert img(C=3, rule=2, alpha=plane.data_ptr()) == 0          # (a plane is an alpha: accepted; it writes 3 x 64 floats)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.flatten()[192:]).all()) and not bool(torch.isnan(out.flatten()[:192]).any())
    # the Python layer raises the same refusals itself
    rgb3 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    for bad in (lambda: wire.decode_image_u8(rgb3, fmt=wire.FACESCAPE_RGBA, device=dev),
                lambda: wire.decode_image_u8(rgb3, fmt=wire.MULTIFACE_RGB, device=dev),
                lambda: wire.decode_image_u8(torch.zeros((1, 8, 8, 5), dtype=torch.uint8, device=dev), device=dev),
                lambda: wire.decode_image_u8(rgb3, fmt=wire.ImageFormat("below_two"), device=dev),
                lambda: wire.decode_image_u8(rgb3, plane[:, :4], wire.MULTIFACE_RGB, device=dev),
                lambda: wire.decode_multiface(d16, stride=3, device=dev),
                lambda: glue.encoder_input(rgb3, 4, 2),                                            # bytes without a format
                lambda: glue.encoder_input(rgb3, 4, 2, image_format=wire.FACESCAPE_RGBA),          # a rule without an alpha
                lambda: glue.encoder_input(torch.zeros((1, 3, 8, 8), device=dev), 4, 2, image_format=wire.DTU_RGB),
                lambda: glue.encoder_input(torch.zeros((1, 3, 8, 8), device=dev), 4, 2, alpha=plane)):
        with pytest.raises(ValueError):
            bad()
    # encode refuses a byte source before it touches the model
    from tests import test_gpu_encode as E
    s, m = E.scene(dev), E.model(dev).eval()
    px5 = torch.zeros((E.SB, E.NV, E.H, E.W, 3), dtype=torch.uint8, device=dev)
    for kw in (dict(), dict(image_format=wire.FACESCAPE_RGBA), dict(image_format="facescape")):
        with pytest.raises(ValueError):
            glue.encode(m, px5, *E.args(s)[1:], **kw)
    with pytest.raises(ValueError):
        glue.encode(m, *E.args(s), image_format=wire.DTU_RGB)
    enc = m.encoder
    assert enc.latent is None and m.poses is None and getattr(enc, "depths", None) is None and getattr(enc, "normals", None) is None
    with pytest.raises(AssertionError):
        wire.decode_image_u8(np.zeros((8, 8, 3), np.float32), device=dev)
    with pytest.raises(RuntimeError, match="GPU only"):
        wire.decode_image_u8(np.zeros((8, 8, 3), np.uint8), device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        wire.decode_multiface(np.zeros((1, 8, 8), np.uint16), device="cpu")
