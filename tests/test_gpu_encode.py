"""GPU tests of glue.encode, the drop-in for PixelNeRF.encode (reference src/models/pixelnerf.py:35-53 with SpatialEncoder.forward,
src/models/image_encoder.py:206-272): head kernel -> the model's own trunk modules -> assemble_latent, plus depth2normal.  The trunk is
synthetic/encoder_stub.py's (plain torch.nn; torchvision is not needed).

Wiring: the latent is bit-equal to assemble_latent of the same modules applied by hand to glue.encoder_input, packed; the normals are
glue.depth2normal's; every attribute the reference's encode sets is set the same way.
Arithmetic: against a torch restatement of encode (normalise, F.pad(replicate), tests/encoder_input_ref.py's encoding, the trunk,
F.interpolate(align_corners=True) + cat on the CPU) with tests/test_gpu_latent_assemble.py's forward tolerance, 16 * 2^-23 * max|level| per
level; conv1's weights on the encoding's channels are scaled by 1e-4 so that tol_pe (1.3e-5 per input value, 882 taps of |w| ~ 4e-6:
below 5e-8 after conv1) stays two orders below that tolerance through the trunk.
Drop-in: NeRFRendererDGS.forward runs on the encoded model and takes the latent buffer as it is; under autograd a training step reaches
the trunk's conv1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import encoder_input_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SB, NV, H, W, PAD = 1, 2, 24, 32, 8
K, NC, G = 16, 64, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_scene = {}


def scene(dev):
    """the inputs of encode (seeded, made once, left unchanged) and the synthetic scene they come from"""
    if not _scene:
        from synthetic import synth
        sc = synth.make_scene(H, W, NV, seed=30, feature_padding=PAD // 2, with_latent=False)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        g = torch.Generator().manual_seed(31)
        _scene.update(sc=sc, images=torch.rand((SB, NV, 3, H, W), generator=g).to(dev), depths=t(sc.depths), depths_std=t(sc.depths_std),
                      extrinsics=t(sc.poses), intrinsics=t(np.tile(synth.intrinsics(W, H), (SB, NV, 1, 1))))
    return _scene


def args(s):
    return s["images"], s["depths"], s["depths_std"], s["extrinsics"], s["intrinsics"]


def model(dev, **kw):
    from synthetic.encoder_stub import encoder_model
    return encoder_model(device=dev, seed=32, image_padding=PAD, **kw)


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


@pytest.mark.parametrize("kw", [dict(), dict(use_first_pool=False), dict(num_layers=2), dict(num_layers=5), dict(padding_pe=-1)],
                         ids=["default", "no_first_pool", "two_layers", "five_layers", "no_pe"])
def test_wiring(kw, dev):
    from diner_amd import glue
    from synthetic.encoder_stub import CHANNELS
    s = scene(dev)
    m = model(dev, **kw).eval()
    enc = m.encoder
    with torch.no_grad():
        assert glue.encode(m, *args(s)) is None
        x = glue.encoder_input(s["images"], PAD, enc.padding_pe)
        lv = levels_by_hand(enc, x)
        want = glue.assemble_latent(lv, SB, NV)
    assert x.shape == (SB * NV, 3 if enc.padding_pe < 0 else 21, H + 2 * PAD, W + 2 * PAD)
    assert len(lv) == enc.num_layers and enc.latent.shape == (SB, NV, sum(CHANNELS[:enc.num_layers]), (H + 2 * PAD) // 2, (W + 2 * PAD) // 2)
    assert glue.latent_is_packed(enc.latent) and torch.equal(enc.latent, want)
    assert torch.equal(enc.normals, glue.depth2normal(s["depths"].flatten(0, 1), s["intrinsics"].flatten(0, 1)).reshape(SB, NV, 3, H, W))
    assert enc.depths is s["depths"] and enc.depths_std is s["depths_std"] and enc.nviews == NV and enc.nobjects == SB
    assert m.poses is s["extrinsics"]
    assert torch.equal(m.c, s["intrinsics"][:, :, :2, -1]) and m.c.shape == (SB, NV, 2)
    assert torch.equal(m.focal, s["intrinsics"][:, :, torch.tensor([0, 1]), torch.tensor([0, 1])]) and m.focal.shape == (SB, NV, 2)
    assert m.image_shape.tolist() == [W, H] and m.image_shape.device == s["images"].device
    # the values the synthetic scene was built with
    sc = s["sc"]
    assert np.array_equal(m.focal.cpu().numpy(), sc.focal) and np.array_equal(m.c.cpu().numpy(), sc.c)
    assert np.array_equal(m.image_shape.cpu().numpy(), sc.image_shape)


def test_normalize_constants_come_from_the_model(dev):
    from types import SimpleNamespace as NS

    from diner_amd import glue
    s = scene(dev)
    m = model(dev).eval()
    m.normalize_rgb = NS(mean=[0.1, 0.2, 0.3], std=[0.5, 1.5, 2.0])
    with torch.no_grad():
        glue.encode(m, *args(s))
        want = glue.assemble_latent(levels_by_hand(m.encoder, glue.encoder_input(s["images"], PAD, 4, [0.1, 0.2, 0.3], [0.5, 1.5, 2.0])), SB, NV)
    assert torch.equal(m.encoder.latent, want)


def test_against_the_references_arithmetic(dev):
    from diner_amd import glue
    s = scene(dev)
    m = model(dev).eval()
    enc = m.encoder
    with torch.no_grad():
        enc.model.conv1.weight[:, 3:] *= 1e-4
        glue.encode(m, *args(s))
        # the reference's sequence, restated: Normalize, ReplicationPad2d, the encoding, cat -- then the same trunk modules
        img = s["images"].cpu().flatten(0, 1)
        mean, std = torch.tensor(R.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(R.IMAGENET_STD).view(1, 3, 1, 1)
        x = F.pad((img - mean) / std, [PAD] * 4, mode="replicate")
        pe = R.encoder_input_ref(img, PAD, enc.padding_pe)[:, 3:]
        x = torch.cat((x, pe), dim=1)
        lv = [t.cpu() for t in levels_by_hand(enc, x.to(dev))]
        want = torch.cat([F.interpolate(t, size=lv[0].shape[-2:], mode="bilinear", align_corners=True) for t in lv], 1)
    got = enc.latent.cpu().flatten(0, 1)
    assert got.shape == want.shape
    off = 0
    for t in lv:
        c = t.shape[1]
        bound = 16 * ULP * float(t.abs().max())
        err = float((got[:, off:off + c] - want[:, off:off + c]).abs().max())
        print(f"level {tuple(t.shape)}: max |level| {float(t.abs().max()):.3f}, max err {err:.3e}, bound {bound:.3e}")
        assert float(t.abs().max()) > 1e-3 and err <= bound
        off += c


def _rays(s, dev):
    return torch.from_numpy(s["sc"].target_rays()[:, ::3]).to(dev)


def test_drop_in_render(dev):
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
    assert r._latent_pack.shape == (SB, NV, *lat.shape[-2:], lat.shape[2]) and r._latent_pack.is_contiguous()


def test_drop_in_training_step(dev):
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
    assert r.last_route == "train_gen"
    gw = conv1.weight.grad
    assert gw is not None and gw.shape == conv1.weight.shape and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    assert float(gw[:, 3:].abs().max()) > 0          # the encoding's channels feed conv1 too
    gm = m.mlp_fine.lin_in.weight.grad
    assert gm is not None and bool(torch.isfinite(gm).all()) and float(gm.abs().max()) > 0


def test_other_upsample_interp_raises_before_any_device_work(dev, monkeypatch):
    from diner_amd import glue
    s = scene(dev)
    m = model(dev, upsample_interp="nearest")

    def boom(*a, **k):
        raise AssertionError("device work before the mode check")

    for name in ("encoder_input", "depth2normal", "assemble_latent"):
        monkeypatch.setattr(glue, name, boom)
    with pytest.raises(NotImplementedError, match="'nearest'"):
        glue.encode(m, *args(s))
    assert m.encoder.latent is None and m.poses is None
