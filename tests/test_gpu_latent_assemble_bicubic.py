"""GPU tests of the bicubic latent assembly (glue.assemble_latent_bicubic: diner_assemble_latent_bicubic / _backward), of the renderer and
the training path on its packed latent, and of glue.encode with upsample_interp="bicubic".  Cases, inputs, references and the two bounds
come from tests/latent_bicubic_ref.py, whose restatement tests/test_latent_assemble_bicubic_host.py proves against CPU torch.

Forward: against torch's own CPU fp32 F.interpolate(mode="bicubic", align_corners=True), per level and elementwise, within
C_F * 2^-23 * max|level|, C_F = 30 * 1.375^2 = 56.72 <= 64: 30 roundings on the way to one value (src and the longest coefficient per axis,
8 + 8; 4 products + 3 additions of the inner and of the outer sum, 7 + 7) times the absolute weight sum (sum |w| <= 1.375 per axis, at
t = 1/2) -- the derivation is written out next to C_F.  A same-size level is bit-identical to its input; the bilinear kernel's output on the
same inputs lies outside the bound.
Backward: against the float64 restatement with fp32-placed taps, Wy^T d Wx, per element |err| <= (n + C_B) * 2^-23 * A with
A = |Wy|^T |d_out| |Wx| in float64, n = the largest number of fine pixels with a non-zero weight on one coarse texel of the level (from the
restatement's matrices) and C_B = 16 = the roundings of one term's weight: the longest coefficient per axis (6 + 6), wy * wx, the product
with d_out, and one addition per axis where clamped taps coincide (written out next to C_B).  Two calls are bit-identical; a same-size
level's gradient is the transposed copy, bit-equal.
Adjoint identity <A x, g> = <x, A^T g> to 1e-5 relative on positive inputs.  Autograd function: a non-NHWC incoming gradient gives the NHWC
one's result; only the levels that need a gradient get one; dtypes come back; the no-grad call equals the autograd call bit for bit.
Renderer: forward() and render_image() on the packed latent equal those on latent.contiguous() bit for bit, on the pack's own pointer.
Training: one step through the packed route; every level's gradient equals assemble_latent_bicubic_backward(latent.grad) bit for bit (the
wiring, without comparing two forward passes across ReLU kinks: see _train_pyramid of tests/test_gpu_latent_assemble.py).
glue.encode with upsample_interp="bicubic": as tests/test_gpu_encode.py for the bilinear tail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import encoder_input_ref as ER
from tests import latent_bicubic_ref as R

pytestmark = pytest.mark.gpu

ULP = R.ULP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _nhwc(t5):
    """the same values with NHWC storage (logical shape unchanged)"""
    return t5.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_forward_against_torch_cpu(name, dev):
    from diner_amd import glue
    r = R.ref(name)
    assert R.C_F <= 64
    lv = [t.to(dev) for t in r.levels]
    lat = glue.assemble_latent_bicubic(lv, r.SB, r.NV)
    h, w = r.size
    assert lat.shape == (r.SB, r.NV, r.C, h, w) and lat.dtype == torch.float32 and not lat.requires_grad
    assert glue.latent_is_packed(lat) and lat.permute(0, 1, 3, 4, 2).is_contiguous()
    got = lat.cpu().reshape(r.SB * r.NV, r.C, h, w)
    bil = glue.assemble_latent(lv, r.SB, r.NV).cpu().reshape(r.SB * r.NV, r.C, h, w)
    off = 0
    for t, spec in zip(r.levels, r.specs):
        c, hl, wl = spec
        sl = slice(off, off + c)
        unit = ULP * float(t.abs().max())
        bound = R.C_F * unit
        err = float((got[:, sl] - r.out[:, sl]).abs().max())
        err_bil = float((bil[:, sl] - r.out[:, sl]).abs().max())
        print(f"{name} level {c}x{hl}x{wl}: max err {err / unit:.2f} units of 2^-23 max|level| (bound {R.C_F:.2f}); bilinear kernel {err_bil / unit:.3e}")
        if (hl, wl) == (h, w):
            assert torch.equal(got[:, sl], t), "a same-size level must come out bit-identical"
        assert err <= bound, (name, spec, err, bound)
        # the check rejects a wrong implementation: the bilinear kernel lies outside the bound wherever a level is resampled, has more
        # than one texel and an output pixel falls between texels (an output of 1 x 1 is the corner texel in both)
        if r.resampled(spec) and (h, w) != (1, 1):
            assert err_bil > bound, (name, spec, err_bil, bound)
        off += c


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_against_the_float64_restatement(name, dev):
    from diner_amd import glue
    r = R.ref(name)
    assert R.C_B <= 16
    h, w = r.size
    d5 = _nhwc(r.d_out.to(dev).reshape(r.SB, r.NV, r.C, h, w))
    shapes = [tuple(t.shape) for t in r.levels]
    got = glue.assemble_latent_bicubic_backward(d5, shapes)
    again = glue.assemble_latent_bicubic_backward(d5, shapes)
    off = 0
    for g, g2, ref, A, n, (c, hl, wl) in zip(got, again, r.grads, r.A, r.n, r.specs):
        assert g.shape == ref.shape and g.dtype == torch.float32
        assert torch.equal(g, g2), "two backward calls must be bit-identical"
        err = (g.cpu().double() - ref).abs()
        bound = (n + R.C_B) * ULP * A
        print(f"{name} level {c}x{hl}x{wl}: n = {n}, max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (name, c, hl, wl, float((err - bound).max()))
        if (hl, wl) == (h, w):     # a plain transposed copy
            assert torch.equal(g.cpu(), r.d_out[:, off:off + c])
        off += c


@pytest.mark.parametrize("name", ["ragged_five_levels", "downsample"])
def test_adjoint_identity(name, dev):
    from diner_amd import glue
    r = R.ref(name)
    gen = torch.Generator().manual_seed(5)
    x = [(torch.rand(t.shape, generator=gen) + 0.5).to(dev) for t in r.levels]       # positive: the dot products do not cancel
    g = _nhwc((torch.rand((r.SB, r.NV, r.C, *r.size), generator=gen) + 0.5).to(dev))
    Ax = glue.assemble_latent_bicubic(x, r.SB, r.NV)
    Atg = glue.assemble_latent_bicubic_backward(g, [tuple(t.shape) for t in x])
    lhs = float((Ax.double() * g.double()).sum())
    rhs = sum(float((a.double() * b.double()).sum()) for a, b in zip(x, Atg))
    print(f"{name}: <Ax, g> = {lhs:.10e}, <x, A^T g> = {rhs:.10e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs)


def test_autograd_function(dev):
    """a non-NHWC incoming gradient gives the NHWC one's result; only the levels that need a gradient get one; dtypes come back"""
    from diner_amd import glue
    r = R.ref("ragged_five_levels")
    lv = [t.to(dev).requires_grad_(i != 1) for i, t in enumerate(r.levels)]
    lv[2] = lv[2].detach().half().requires_grad_(True)
    lat = glue.assemble_latent_bicubic(lv, r.SB, r.NV)
    assert lat.requires_grad and glue.latent_is_packed(lat)
    need = [t for t in lv if t.requires_grad]
    d_nchw = r.d_out.to(dev).reshape(lat.shape)
    assert d_nchw.is_contiguous()
    a = torch.autograd.grad(lat, need, d_nchw, retain_graph=True)
    b = torch.autograd.grad(lat, need, _nhwc(d_nchw), retain_graph=True)
    for x, y, t in zip(a, b, need):
        assert torch.equal(x, y) and x.dtype == t.dtype and x.shape == t.shape
    assert a[1].dtype == torch.float16
    (lat * d_nchw).sum().backward()
    assert lv[1].grad is None and torch.equal(lv[0].grad, a[0])
    want = glue.assemble_latent_bicubic_backward(d_nchw, [tuple(t.shape) for t in lv])
    assert torch.equal(lv[3].grad, want[3]) and torch.equal(lv[2].grad, want[2].half())
    with torch.no_grad():
        assert torch.equal(glue.assemble_latent_bicubic(lv, r.SB, r.NV), lat)      # the no-grad call's values, bit for bit


# ---- renderer: the zero-copy branch ------------------------------------------------------------------------------------------------
PYRAMID = [(64, 1), (64, 2), (128, 4), (256, 8)]      # (channels, stride) of the ResNet levels: C = 512
K, NC, G = 16, 64, 5
RENDER_MODES = {
    # name: (precision, model arguments)
    "standard_f16x3": ("f16x3", {}),
    "d_hidden128_fp32": ("fp32", dict(d_hidden=128)),
}


def _pyramid(NV, h, w, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((NV, c, -(-h // s), -(-w // s)), generator=g).to(dev) for c, s in PYRAMID]


def _scene_model(NV, dev, model_kw, seed=0):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(32, 32, NV, seed=seed, feature_padding=4)
    dims = {k: v for k, v in model_kw.items() if k.startswith("d_")}
    w = synth.make_mlp_weights(seed + 1, bias_scale=0.1, **dims)
    return sc, model_from_scene(sc, w, device=dev, **model_kw)


@pytest.mark.parametrize("mode", sorted(RENDER_MODES))
def test_renderer_takes_the_packed_latent_as_it_is(mode, dev):
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    precision, model_kw = RENDER_MODES[mode]
    NV = 2
    sc, m = _scene_model(NV, dev, model_kw)
    h, w = sc.latent.shape[-2:]
    packed = glue.assemble_latent_bicubic(_pyramid(NV, h, w, dev, seed=3), 1, NV)
    assert packed.shape == sc.latent.shape and glue.latent_is_packed(packed)
    nchw = packed.contiguous()
    assert not glue.latent_is_packed(nchw) and torch.equal(nchw, packed)
    rays = torch.from_numpy(sc.target_rays()[:, ::3]).to(dev)
    noise = tuple(torch.from_numpy(n).to(dev)[None] for n in synth.make_noise(rays.shape[1], NC, G, K, seed=2))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E, Kt = t(sc.target_extrinsics)[None], t(sc.target_intrinsics)[None] * 0.5
    Kt[:, 2, 2] = 1.0
    outs = {}
    for route, lat in (("packed", packed), ("nchw", nchw)):
        m.encoder.latent = lat
        r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=sc.white_bkgd)
        r.precision = precision
        with torch.no_grad():
            o = r(m, rays, want_weights=True, noise=noise).fine
            r.seed, r._calls = 7, 0
            img, depth = r.render_image(m, E, Kt, 16, 16, sc.near, sc.far, return_depth=True)
        shared = r._latent_pack.data_ptr() == lat.data_ptr()
        assert shared == (route == "packed") and r.memory_report(m)["latent_zero_copy"] == shared
        assert r._latent_pack.shape == (1, NV, h, w, 512) and r._latent_pack.is_contiguous()
        outs[route] = (o.rgb, o.depth, o.weights, img, depth)
    for a, b in zip(outs["packed"], outs["nchw"]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert float(outs["packed"][0].std()) > 1e-3       # (a frame with content)


def test_training_step_through_the_packed_route(dev):
    """the wiring of one training step: the renderer's gradient arrives at the latent in its own (NHWC) strides and every level's gradient
    is the adjoint kernel's of exactly that, bit for bit"""
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    NV = 2
    sc, m = _scene_model(NV, dev, {}, seed=20)
    h, w = sc.latent.shape[-2:]
    rays = torch.from_numpy(sc.target_rays()[:, ::4]).to(dev)
    assert rays.shape[1] == 256
    noise = tuple(torch.from_numpy(n).to(dev)[None] for n in synth.make_noise(256, NC, G, K, seed=4))
    gen = torch.Generator().manual_seed(9)
    c_rgb, c_depth = torch.randn((1, 256, 3), generator=gen).to(dev), torch.randn((1, 256), generator=gen).to(dev)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    lv = [t.requires_grad_(True) for t in _pyramid(NV, h, w, dev, seed=6)]
    latent = glue.assemble_latent_bicubic(lv, 1, NV)
    latent.retain_grad()
    m.encoder.latent = latent
    assert glue.latent_is_packed(latent) and latent.requires_grad
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=sc.white_bkgd)
    r.precision = "fp32"
    out = r(m, rays, noise=noise).fine
    ((out.rgb * c_rgb).sum() + (out.depth * c_depth).sum()).backward()
    assert latent.grad is not None and latent.grad.shape == latent.shape
    want = glue.assemble_latent_bicubic_backward(latent.grad, [tuple(t.shape) for t in lv])
    for i, (t, g) in enumerate(zip(lv, want)):
        assert t.grad is not None and torch.equal(t.grad, g), i
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, i
    gm = m.mlp_fine.lin_in.weight.grad
    assert gm is not None and bool(torch.isfinite(gm).all()) and float(gm.abs().max()) > 0


# ---- glue.encode with upsample_interp="bicubic" ----------------------------------------------------------------------------------------
SB, NV_E, H, W, PAD = 1, 2, 24, 32, 8

_scene = {}


def scene(dev):
    """the inputs of encode (seeded, made once, left unchanged) and the synthetic scene they come from"""
    if not _scene:
        from synthetic import synth
        sc = synth.make_scene(H, W, NV_E, seed=30, feature_padding=PAD // 2, with_latent=False)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        g = torch.Generator().manual_seed(31)
        _scene.update(sc=sc, images=torch.rand((SB, NV_E, 3, H, W), generator=g).to(dev), depths=t(sc.depths), depths_std=t(sc.depths_std),
                      extrinsics=t(sc.poses), intrinsics=t(np.tile(synth.intrinsics(W, H), (SB, NV_E, 1, 1))))
    return _scene


def args(s):
    return s["images"], s["depths"], s["depths_std"], s["extrinsics"], s["intrinsics"]


def model(dev, **kw):
    from synthetic.encoder_stub import encoder_model
    return encoder_model(device=dev, seed=32, image_padding=PAD, upsample_interp="bicubic", **kw)


def levels_by_hand(enc, x):
    """the trunk of image_encoder.py:242-260 on conv1's input x"""
    t = enc.model
    x = t.relu(t.bn1(t.conv1(x)))
    lv = [x]
    if enc.num_layers > 1:
        if enc.use_first_pool:
            x = t.maxpool(x)
        x = t.layer1(x)
        lv.append(x)
    for i in (2, 3, 4):
        if enc.num_layers > i:
            x = getattr(t, f"layer{i}")(x)
            lv.append(x)
    return lv


@pytest.mark.parametrize("kw", [dict(), dict(num_layers=5)], ids=["default", "five_layers"])
def test_encode_wiring(kw, dev):
    from diner_amd import glue
    from synthetic.encoder_stub import CHANNELS
    s = scene(dev)
    m = model(dev, **kw).eval()
    enc = m.encoder
    assert enc.upsample_interp == "bicubic"
    with torch.no_grad():
        assert glue.encode(m, *args(s)) is None
        lv = levels_by_hand(enc, glue.encoder_input(s["images"], PAD, enc.padding_pe))
        want = glue.assemble_latent_bicubic(lv, SB, NV_E)
        other = glue.assemble_latent(lv, SB, NV_E)
    assert len(lv) == enc.num_layers and enc.latent.shape == (SB, NV_E, sum(CHANNELS[:enc.num_layers]), (H + 2 * PAD) // 2, (W + 2 * PAD) // 2)
    assert glue.latent_is_packed(enc.latent) and torch.equal(enc.latent, want)
    assert not torch.equal(enc.latent, other)          # (the bilinear tail gives another latent)
    assert torch.equal(enc.normals, glue.depth2normal(s["depths"].flatten(0, 1), s["intrinsics"].flatten(0, 1)).reshape(SB, NV_E, 3, H, W))
    assert enc.depths is s["depths"] and enc.depths_std is s["depths_std"] and enc.nviews == NV_E and enc.nobjects == SB
    assert m.poses is s["extrinsics"]
    assert torch.equal(m.c, s["intrinsics"][:, :, :2, -1]) and m.c.shape == (SB, NV_E, 2)
    assert torch.equal(m.focal, s["intrinsics"][:, :, torch.tensor([0, 1]), torch.tensor([0, 1])]) and m.focal.shape == (SB, NV_E, 2)
    assert m.image_shape.tolist() == [W, H] and m.image_shape.device == s["images"].device


def test_encode_against_the_references_arithmetic(dev):
    """as tests/test_gpu_encode.py::test_against_the_references_arithmetic with mode="bicubic": conv1's weights on the encoding's channels
    are scaled by 1e-4 so that the encoding's tolerance stays two orders below the forward bound through the trunk"""
    from diner_amd import glue
    s = scene(dev)
    m = model(dev).eval()
    enc = m.encoder
    with torch.no_grad():
        enc.model.conv1.weight[:, 3:] *= 1e-4
        glue.encode(m, *args(s))
        img = s["images"].cpu().flatten(0, 1)
        mean, std = torch.tensor(ER.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(ER.IMAGENET_STD).view(1, 3, 1, 1)
        x = F.pad((img - mean) / std, [PAD] * 4, mode="replicate")
        x = torch.cat((x, ER.encoder_input_ref(img, PAD, enc.padding_pe)[:, 3:]), dim=1)
        lv = [t.cpu() for t in levels_by_hand(enc, x.to(dev))]
        want = torch.cat([F.interpolate(t, size=lv[0].shape[-2:], mode="bicubic", align_corners=True) for t in lv], 1)
    got = enc.latent.cpu().flatten(0, 1)
    assert got.shape == want.shape
    off = 0
    for t in lv:
        c = t.shape[1]
        unit = ULP * float(t.abs().max())
        err = float((got[:, off:off + c] - want[:, off:off + c]).abs().max())
        print(f"level {tuple(t.shape)}: max |level| {float(t.abs().max()):.3f}, max err {err / unit:.2f} units (bound {R.C_F:.2f})")
        assert float(t.abs().max()) > 1e-3 and err <= R.C_F * unit
        off += c


def _rays(s, dev):
    return torch.from_numpy(s["sc"].target_rays()[:, ::3]).to(dev)


def test_encode_drop_in_render(dev):
    from diner_amd import NeRFRendererDGS, glue
    s = scene(dev)
    m = model(dev).eval()
    rays = _rays(s, dev)
    assert rays.shape == (1, 256, 8)
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=s["sc"].white_bkgd)
    r.precision = "fp32"
    with torch.no_grad():
        glue.encode(m, *args(s))
        out = r(m, rays, want_weights=True).fine
    lat = m.encoder.latent
    assert bool(torch.isfinite(out.rgb).all()) and bool(torch.isfinite(out.depth).all()) and out.rgb.shape == (1, 256, 3)
    assert float(out.rgb.std()) > 1e-3       # (a frame with content)
    assert r._latent_pack.data_ptr() == lat.data_ptr() and r.memory_report(m)["latent_zero_copy"]
    assert r._latent_pack.shape == (SB, NV_E, *lat.shape[-2:], lat.shape[2]) and r._latent_pack.is_contiguous()


def test_encode_drop_in_training_step(dev):
    from diner_amd import NeRFRendererDGS, glue
    s = scene(dev)
    m = model(dev).train()
    conv1 = m.encoder.model.conv1
    r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=s["sc"].white_bkgd, train_any_shape=True)
    r.precision = "fp32"
    glue.encode(m, *args(s))
    assert m.encoder.latent.requires_grad and glue.latent_is_packed(m.encoder.latent)
    out = r(m, _rays(s, dev)).fine
    g = torch.Generator().manual_seed(33)
    loss = (out.rgb * torch.randn((1, 256, 3), generator=g).to(dev)).sum() + (out.depth * torch.randn((1, 256), generator=g).to(dev)).sum()
    loss.backward()
    gw = conv1.weight.grad
    assert gw is not None and gw.shape == conv1.weight.shape and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    assert float(gw[:, 3:].abs().max()) > 0          # the encoding's channels feed conv1 too
