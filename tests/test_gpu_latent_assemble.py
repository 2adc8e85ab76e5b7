"""GPU tests of the latent assembly (glue.assemble_latent: diner_assemble_latent / _backward) and of the zero-copy branch it opens in the
renderer and the training path.  The oracle of the assembly is torch's own CPU F.interpolate(mode="bilinear", align_corners=True) + cat.

Forward: a level of the output's size is bit-identical to its input; every other element within 16 * 2^-23 * max|level| of torch CPU fp32
(the expression has at most 8 roundings, each at most one ulp of a magnitude <= max|level|; the factor 16 leaves a margin of two for FMA
contraction differences); the align_corners=False result on the same inputs lies outside that bound.
Backward: against float64 torch CPU autograd on the same d_out, per element |err| <= (n + 8) * 2^-23 * A, A = the float64 adjoint applied
to |d_out|, n = the largest number of fine pixels in one coarse texel's support for that level (the standard bound of an n-term sum in
any order); two calls bit-identical; <A x, g> = <x, A^T g> to 1e-5 relative; a non-NHWC incoming gradient gives the NHWC one's result.
Renderer: forward() and render_image() on the packed latent equal those on latent.contiguous() bit for bit, on the pack's own pointer.
Training: the gradients of the MLP parameters, the rays and every pyramid level through the packed route against the NCHW route (the
same pyramid through torch's interpolate + cat on the GPU), with tests/test_training.py's tolerances."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23

# name -> (SB, NV, [(C_l, h_l, w_l), ...]); the output takes the first level's size
CASES = {
    "ragged_five_levels": (2, 3, [(8, 11, 13), (8, 6, 7), (16, 3, 4), (24, 2, 2), (8, 1, 1)]),   # 143 pixels: ragged tiles; in = 1; C = 64
    "out_1x1": (1, 2, [(8, 1, 1), (8, 3, 3)]),                                                    # out = 1: scale 0
    "resnet": (1, 2, [(64, 20, 20), (64, 10, 10), (128, 5, 5), (256, 3, 3)]),
    "c1024": (1, 1, [(256, 6, 6), (256, 3, 3), (256, 2, 2), (128, 1, 1), (128, 4, 5)]),
    # levels larger than the output.  Kept small (src <= 8): the float64 oracle places its taps in double, ATen's fp32 kernel and ours in
    # fp32 -- up to an ulp of src in every weight, which the backward bound's derivation does not count and n = 1..4 terms do not hide
    "downsample": (1, 3, [(8, 5, 6), (16, 7, 9), (8, 5, 9)]),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _taps(n_in, n_out):
    """ATen's align_corners=True taps in fp32: i0, i1 per output index"""
    f = np.float32
    s = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    src = s * np.arange(n_out, dtype=f)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1)


def _support(n_in, n_out):
    """the largest number of fine indices whose i0 or i1 is one coarse index"""
    i0, i1 = _taps(n_in, n_out)
    return max(int(((i0 == k) | (i1 == k)).sum()) for k in range(n_in))


def _upcat(levels, size, align_corners=True):
    return torch.cat([F.interpolate(t, size=size, mode="bilinear", align_corners=align_corners) for t in levels], 1)


class Ref:
    """inputs and CPU references of one case, computed once and left unchanged"""

    def __init__(self, name):
        self.SB, self.NV, self.specs = CASES[name]
        N = self.SB * self.NV
        g = torch.Generator().manual_seed(sorted(CASES).index(name) + 11)
        self.levels = [torch.randn((N, c, h, w), generator=g) * (1.0 + i) for i, (c, h, w) in enumerate(self.specs)]
        self.size = self.specs[0][1:]
        self.C = sum(c for c, _, _ in self.specs)
        self.out = _upcat(self.levels, self.size)                                  # fp32 CPU oracle [N, C, h, w]
        self.out_false = _upcat(self.levels, self.size, align_corners=False)
        self.d_out = torch.randn((N, self.C, *self.size), generator=g)
        lv64 = [t.double().requires_grad_(True) for t in self.levels]
        self.grads = torch.autograd.grad(_upcat(lv64, self.size), lv64, self.d_out.double())
        self.A = torch.autograd.grad(_upcat(lv64, self.size), lv64, self.d_out.double().abs())
        self.n = [_support(h, self.size[0]) * _support(w, self.size[1]) for _, h, w in self.specs]


_refs = {}


def _ref(name):
    if name not in _refs:
        _refs[name] = Ref(name)
    return _refs[name]


def _nhwc(t5):
    """the same values with NHWC storage (logical shape unchanged)"""
    return t5.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_against_torch_cpu(name, dev):
    from diner_amd import glue
    r = _ref(name)
    lat = glue.assemble_latent([t.to(dev) for t in r.levels], r.SB, r.NV)
    h, w = r.size
    assert lat.shape == (r.SB, r.NV, r.C, h, w) and lat.dtype == torch.float32 and not lat.requires_grad
    assert glue.latent_is_packed(lat) and lat.permute(0, 1, 3, 4, 2).is_contiguous()
    assert not glue.latent_is_packed(lat.contiguous()) or r.size == (1, 1)     # (1 x 1: both layouts are the same bytes)
    got = lat.cpu().reshape(r.SB * r.NV, r.C, h, w)
    off, wrong = 0, 0
    for t, (c, hl, wl) in zip(r.levels, r.specs):
        sl = slice(off, off + c)
        bound = 16 * ULP * float(t.abs().max())
        err = float((got[:, sl] - r.out[:, sl]).abs().max())
        print(f"{name} level {c}x{hl}x{wl}: max err {err:.3e}, bound {bound:.3e}")
        if (hl, wl) == (h, w):
            assert torch.equal(got[:, sl], t), "a same-size level must come out bit-identical"
        assert err <= bound, (name, c, hl, wl, err, bound)
        wrong += int(((got[:, sl] - r.out_false[:, sl]).abs() > bound).sum())
        off += c
    # the check rejects a wrong implementation: align_corners=False lies outside the bound wherever a level is resampled
    if any((hl, wl) != (h, w) and hl * wl > 1 for _, hl, wl in r.specs):
        assert wrong > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_against_float64_autograd(name, dev):
    from diner_amd import glue
    r = _ref(name)
    h, w = r.size
    d5 = _nhwc(r.d_out.to(dev).reshape(r.SB, r.NV, r.C, h, w))
    shapes = [tuple(t.shape) for t in r.levels]
    got = glue.assemble_latent_backward(d5, shapes)
    again = glue.assemble_latent_backward(d5, shapes)
    off = 0
    for g, g2, ref, A, n, (c, hl, wl) in zip(got, again, r.grads, r.A, r.n, r.specs):
        assert g.shape == ref.shape and g.dtype == torch.float32
        assert torch.equal(g, g2), "two backward calls must be bit-identical"
        err = (g.cpu().double() - ref).abs()
        bound = (n + 8) * ULP * A
        print(f"{name} level {c}x{hl}x{wl}: n = {n}, max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (name, c, hl, wl, float((err - bound).max()))
        if (hl, wl) == (h, w):     # a plain transposed copy
            assert torch.equal(g.cpu(), r.d_out[:, off:off + c])
        off += c


@pytest.mark.parametrize("name", ["ragged_five_levels", "downsample"])
def test_adjoint_identity(name, dev):
    from diner_amd import glue
    r = _ref(name)
    gen = torch.Generator().manual_seed(5)
    x = [(torch.rand(t.shape, generator=gen) + 0.5).to(dev) for t in r.levels]       # positive: the dot products do not cancel
    g = _nhwc((torch.rand((r.SB, r.NV, r.C, *r.size), generator=gen) + 0.5).to(dev))
    Ax = glue.assemble_latent(x, r.SB, r.NV)
    Atg = glue.assemble_latent_backward(g, [tuple(t.shape) for t in x])
    lhs = float((Ax.double() * g.double()).sum())
    rhs = sum(float((a.double() * b.double()).sum()) for a, b in zip(x, Atg))
    print(f"{name}: <Ax, g> = {lhs:.10e}, <x, A^T g> = {rhs:.10e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs)


def test_autograd_function(dev):
    """a non-NHWC incoming gradient gives the NHWC one's result; only the levels that need a gradient get one; dtypes come back"""
    from diner_amd import glue
    r = _ref("ragged_five_levels")
    lv = [t.to(dev).requires_grad_(i != 1) for i, t in enumerate(r.levels)]
    lv[2] = lv[2].detach().half().requires_grad_(True)
    lat = glue.assemble_latent(lv, r.SB, r.NV)
    assert lat.requires_grad and glue.latent_is_packed(lat)
    need = [t for t in lv if t.requires_grad]
    d_nchw = r.d_out.to(dev).reshape(lat.shape)
    assert d_nchw.is_contiguous()
    a = torch.autograd.grad(lat, need, d_nchw, retain_graph=True)
    b = torch.autograd.grad(lat, need, _nhwc(d_nchw), retain_graph=True)
    for x, y, t in zip(a, b, need):
        assert torch.equal(x, y) and x.dtype == t.dtype and x.shape == t.shape
    (lat * d_nchw).sum().backward()
    assert lv[1].grad is None and torch.equal(lv[0].grad, a[0])
    ref0 = r.grads[0].float()
    assert float((lv[0].grad.cpu() - ref0).abs().max()) <= 16 * ULP * float(ref0.abs().max())
    with torch.no_grad():
        assert torch.equal(glue.assemble_latent(lv, r.SB, r.NV), lat)      # the no-grad call's values, bit for bit


# ---- renderer: the zero-copy branch ------------------------------------------------------------------------------------------------
PYRAMID = [(64, 1), (64, 2), (128, 4), (256, 8)]      # (channels, stride) of the ResNet levels: C = 512


def _pyramid(NV, h, w, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((NV, c, -(-h // s), -(-w // s)), generator=g).to(dev) for c, s in PYRAMID]


RENDER_MODES = {
    # name: (renderer switches, precision, model arguments)
    "standard_f16x3": ({}, "f16x3", {}),
    "standard_fp32": ({}, "fp32", {}),
    "d_hidden128_f16x3_any_shape": (dict(f16x3_any_shape=True), "f16x3", dict(d_hidden=128)),
    "zeros_padding_ix": ({}, "f16x3", dict(index_padding="zeros")),
    "bicubic_index": (dict(bicubic_index=True), "fp32", dict(index_interp="bicubic")),
}
K, NC, G = 16, 64, 5


def _scene_model(NV, dev, model_kw, seed=0):
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    sc = synth.make_scene(32, 32, NV, seed=seed, feature_padding=4)
    dims = {k: v for k, v in model_kw.items() if k.startswith("d_")}
    w = synth.make_mlp_weights(seed + 1, bias_scale=0.1, **dims)
    return sc, model_from_scene(sc, w, device=dev, **model_kw)


@pytest.mark.parametrize("NV", [2, 4])
@pytest.mark.parametrize("mode", sorted(RENDER_MODES))
def test_renderer_takes_the_packed_latent_as_it_is(mode, NV, dev):
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    switches, precision, model_kw = RENDER_MODES[mode]
    sc, m = _scene_model(NV, dev, model_kw)
    h, w = sc.latent.shape[-2:]
    packed = glue.assemble_latent(_pyramid(NV, h, w, dev, seed=3), 1, NV)
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
        r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=sc.white_bkgd, **switches)
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


# ---- training: packed route against the NCHW route ---------------------------------------------------------------------------------
TRAIN_MODES = {
    "standard_f16x3": ({}, "f16x3", {}),
    "standard_fp32": ({}, "fp32", {}),
    "d_hidden128_train_any_shape": (dict(train_any_shape=True), "fp32", dict(d_hidden=128)),
}


def _train_pyramid(NV, h, w, dev, seed):
    """A pyramid whose assembled latent has the same bits on both routes, so that the comparison sees the routes and not the ReLUs: a
    last-bit difference between torch's interpolate (contracted to FMAs on the GPU) and ours moves a few of the ~10^7 pre-activations of
    such a step across zero, and one flipped unit shifts single latent-gradient elements by 1e-3 of the largest (measured with a normal
    pyramid: 7.4e-4 on a scale of 0.18 in f16x3, 6e-5 .. 1e-4 of the scale in fp32 at d_hidden = 128 -- the forward's kinks, not the
    routes).  Level 0 has the output's size (a copy); the others are resampled along one axis only and hold signed powers of two, so every
    product of the interpolation is exact and its one sum rounds the same with and without contraction.  Their gradients still go through
    the resampling adjoint."""
    g = torch.Generator().manual_seed(seed)

    def pow2(shape):
        return (2.0 ** torch.randint(-1, 2, shape, generator=g).float()) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)

    return [torch.randn((NV, 64, h, w), generator=g).to(dev), pow2((NV, 64, h, w // 2)).to(dev), pow2((NV, 128, h // 4, w)).to(dev),
            pow2((NV, 256, 1, w // 8)).to(dev)]


@pytest.mark.parametrize("mode", sorted(TRAIN_MODES))
def test_training_gradients_through_the_packed_route(mode, dev):
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    switches, precision, model_kw = TRAIN_MODES[mode]
    NV = 2
    sc, m = _scene_model(NV, dev, model_kw, seed=20)
    h, w = sc.latent.shape[-2:]
    rays0 = torch.from_numpy(sc.target_rays()[:, ::4]).to(dev)
    assert rays0.shape[1] == 256
    noise = tuple(torch.from_numpy(n).to(dev)[None] for n in synth.make_noise(256, NC, G, K, seed=4))
    gen = torch.Generator().manual_seed(9)
    c_rgb, c_depth = torch.randn((1, 256, 3), generator=gen).to(dev), torch.randn((1, 256), generator=gen).to(dev)
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    res = {}
    for route in ("packed", "nchw"):
        lv = [t.requires_grad_(True) for t in _train_pyramid(NV, h, w, dev, seed=6)]
        rays = rays0.clone().requires_grad_(True)
        if route == "packed":
            m.encoder.latent = glue.assemble_latent(lv, 1, NV)
            assert glue.latent_is_packed(m.encoder.latent)
        else:
            m.encoder.latent = _upcat(lv, (h, w)).reshape(1, NV, 512, h, w)
            assert not glue.latent_is_packed(m.encoder.latent)
        r = NeRFRendererDGS(n_samples=K, n_depth_candidates=NC, n_gaussian=G, white_bkgd=sc.white_bkgd, **switches)
        r.precision = precision
        out = r(m, rays, noise=noise).fine
        loss = (out.rgb * c_rgb).sum() + (out.depth * c_depth).sum()
        params = list(m.mlp_fine.parameters())
        gs = torch.autograd.grad(loss, params + [rays] + lv)
        res[route] = dict(rgb=out.rgb.detach(), params=gs[:len(params)], rays=gs[len(params)], levels=gs[len(params) + 1:],
                          latent=m.encoder.latent.detach())
    a, b = res["packed"], res["nchw"]
    print(f"{mode}: latents of the two routes bit-identical: {torch.equal(a['latent'], b['latent'])}, "
          f"max |rgb difference| {float((a['rgb'] - b['rgb']).abs().max()):.3e}")
    assert float((a["rgb"] - b["rgb"]).abs().max()) <= 1e-4
    # tests/test_training.py's tolerances: the latent's gradient 2e-4 of its largest element (here: every level's and the rays');
    # a parameter's gradient 1e-4 of its norm on the norm, 2e-4 * 30 * norm / sqrt(size) per element
    for i, (x, y) in enumerate(zip(a["levels"] + (a["rays"],), b["levels"] + (b["rays"],))):
        scale = float(y.abs().max())
        err = float((x - y).abs().max())
        print(f"{mode} level/rays {i}: max err {err:.3e}, scale {scale:.3e}")
        assert scale > 0 and err <= 2e-4 * scale, (i, err, scale)
    for (name, _), x, y in zip(m.mlp_fine.named_parameters(), a["params"], b["params"]):
        norm = float(y.double().norm())
        assert norm > 0, name
        assert abs(float(x.double().norm()) - norm) <= 1e-4 * norm, name
        assert float((x - y).abs().max()) <= 2e-4 * norm / np.sqrt(y.numel()) * 30 + 1e-7, name
