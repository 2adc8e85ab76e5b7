"""GPU tests of the encoder's other latent lookup modes (SpatialEncoder index_interp nearest, index_padding zeros / reflection;
reference src/models/image_encoder.py:24-25,119-125) on every route:
(i) the ``index_*`` fixtures -- the unmodified reference built with each non-default mode (tools/gen_index_golden.py) -- within
    1e-4 abs on rgb, sigma and depth with the reference's samples injected: fp32, f16x3 with and without the lin_z maps (zeros
    padding: the ringed maps), the shape-general kernel for a non-standard model; nearest lookups compared on firm samples only;
(ii) training: gradients of both training fixtures in both precisions against the reference's autograd (tests/test_training.py's
    tolerances);
(iii) render_image equal to forward(gen_rays(...));
(iv) the default mode unchanged: the _ix entry points with bilinear / border bitwise equal to the old ones (goldens g0, g4)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"


def _render_names():
    from tools.gen_index_golden import CASES
    return sorted(CASES)


def _train_names():
    from tools.gen_index_golden import TRAIN_CASES
    return sorted(TRAIN_CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class IndexCase:
    def __init__(self, name, dev):
        from synthetic.model_stub import model_from_scene
        from tools.gen_index_golden import case_inputs, input_digests, mlp_dims
        self.name = name
        self.data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
        self.cfg = json.loads(str(self.data["config"]))
        self.scene, self.weights, self.rays, noise = case_inputs(self.cfg)
        assert json.loads(str(self.data["digests"])) == input_digests(self.scene, self.weights, self.rays, noise)
        self.dims = {k: v for k, v in mlp_dims(self.cfg).items() if k != "d_in"}
        self.standard = self.cfg["mlp"]["d_hidden"] == 512 and self.scene.C == 512
        self.model = self.make_model(self.cfg["interp"], self.cfg["padding"], dev)
        self.K = self.cfg["K"]
        self.firm = self.data["firm"]                                  # [NR, K]
        self.firm_rays = self.firm.all(-1)

    def make_model(self, interp, padding, dev):
        from synthetic.model_stub import model_from_scene
        return model_from_scene(self.scene, self.weights, device=dev, num_freqs=self.cfg["num_freqs"], index_interp=interp,
                                index_padding=padding, **self.dims)

    def renderer(self, precision="fp32", linz=True):
        from diner_amd import NeRFRendererDGS
        r = NeRFRendererDGS(n_samples=self.K, n_depth_candidates=self.cfg["NC"], n_gaussian=self.cfg["G"],
                            white_bkgd=self.scene.white_bkgd)
        r.precision = precision
        r.linz_maps = linz
        return r


_cases = {}


def _case(name, dev):
    if name not in _cases:
        _cases[name] = IndexCase(name, dev)
    return _cases[name]


def _assert_rgbsigma(got, ref, mask, what):
    got, ref = got[mask], ref[mask]
    err_rgb = np.abs(got[..., :3] - ref[..., :3]).max()
    s_ref = ref[..., 3]
    err_s = (np.abs(got[..., 3] - s_ref) / np.maximum(1.0, s_ref / 12.0)).max()   # the sigma bar of tests/test_gpu_parity.py
    assert err_rgb <= 1e-4 and err_s <= 1e-4, f"{what}: |rgb| {err_rgb:.2e}, |sigma| (relative to max(1, sigma/12)) {err_s:.2e}"


# (precision, lin_z maps) of a standard-shape case; a non-standard one runs fp32 on the shape-general kernel
_ROUTES = [("fp32", True), ("f16x3", True), ("f16x3", False)]


@pytest.mark.parametrize("route", _ROUTES, ids=["fp32", "f16x3-linz", "f16x3-nolinz"])
@pytest.mark.parametrize("name", _render_names())
def test_render_vs_reference(name, route, dev):
    c = _case(name, dev)
    precision, linz = route
    if not c.standard and route != ("fp32", True):
        pytest.skip("a non-standard model runs in fp32 on the shape-general kernel")
    r = c.renderer(precision, linz)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        pts = r.render_points(c.model, rays, z).cpu().numpy()[0]
        assert r.last_binding == "ctypes"
        assert r.last_route == ("points_mlp_gen" if not c.standard else "points_mlp_f16" if precision == "f16x3" else "points_mlp")
        if precision == "f16x3":
            assert (r._linz_pack is not None) == linz
            if linz and c.cfg["padding"] == "zeros":   # the ringed maps
                h, w = c.scene.latent.shape[-2:]
                assert tuple(r._linz_pack.shape[3:5]) == (h + 2, w + 2)
        out = r(c.model, rays, z_samples=z).fine
    _assert_rgbsigma(pts, c.data["rgbsigma"], c.firm, f"{name} {route} render_points")
    fr = c.firm_rays
    assert fr.mean() >= 0.9
    np.testing.assert_allclose(out.rgb.cpu().numpy()[0][fr], c.data["rgb"][fr], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.depth.cpu().numpy()[0][fr], c.data["depth"][fr], rtol=0, atol=1e-4)


@pytest.mark.parametrize("name", _render_names())
def test_the_mode_matters_and_linz_on_off_agree(name, dev):
    """the fixture is not what bilinear / border gives (the padding decides many lookups), and in f16x3 the lin_z maps on and off
    agree for the case's mode"""
    c = _case(name, dev)
    rays, z = T(c.rays, dev), T(c.data["z_fill"], dev)[None]
    with torch.no_grad():
        base = c.renderer().render_points(c.make_model("bilinear", "border", dev), rays, z).cpu().numpy()[0]
        assert np.abs(base - c.data["rgbsigma"]).max() > 1e-2
        if c.standard:
            on = c.renderer("f16x3", True).render_points(c.model, rays, z)
            off = c.renderer("f16x3", False).render_points(c.model, rays, z)
            assert float((on - off).abs().max()) <= 1e-4


def test_render_image_equals_forward(dev):
    """render_image (diner_render_image_ix) against gen_rays -> forward (diner_render_ix) with the same seed, bit for bit"""
    from diner_amd import glue
    for name, precision in (("index_zeros", "f16x3"), ("index_nearest_reflection", "fp32"), ("index_gen_zeros_h128", "fp32")):
        c = _case(name, dev)
        r = c.renderer(precision)
        sc = c.scene
        H, W = 20, 28
        E = torch.from_numpy(np.ascontiguousarray(sc.target_extrinsics, dtype=np.float32))[None].to(dev)
        Kt = torch.tensor([[[0.6 * W, 0, W / 2], [0, 0.6 * W, H / 2], [0, 0, 1]]], dtype=torch.float32, device=dev)
        near, far = float(sc.near), float(sc.far)
        r.seed, r._calls = 3, 0
        rgb, depth = r.render_image(c.model, E, Kt, H, W, near, far, return_depth=True)
        assert r.last_binding == "ctypes"
        rays = glue.gen_rays(E, Kt, W, H, torch.tensor([near], device=dev), torch.tensor([far], device=dev)).view(1, H * W, 8)
        r.seed, r._calls = 3, 0
        with torch.no_grad():
            ref = r(c.model, rays).fine
        assert r.last_binding == "ctypes"
        assert torch.equal(rgb, ref.rgb.view(1, H, W, 3).permute(0, 3, 1, 2)), name
        assert torch.equal(depth, ref.depth.view(1, H, W, 1).permute(0, 3, 1, 2)), name


# ---- training -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", _train_names())
def test_training_gradients_match_reference_autograd(name, precision, dev):
    from oracle.gen_golden import grad_probe_indices, train_cotangents
    c = _case(name, dev)
    gold = c.data
    m = c.model
    for p in m.mlp_fine.parameters():
        p.requires_grad_(True)
    m.encoder.latent = m.encoder.latent.clone().requires_grad_(True)
    r = c.renderer(precision)
    out = r(m, T(c.rays, dev), want_weights=True, z_samples=T(gold["z_fill"], dev))
    np.testing.assert_allclose(out.fine.rgb.detach().cpu().numpy(), gold["rgb"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.fine.depth.detach().cpu().numpy(), gold["depth"], rtol=0, atol=1e-4)
    c_rgb, c_depth = train_cotangents(c.rays.shape[1], c.cfg["cseed"])
    loss = (out.fine.rgb * T(c_rgb, dev)).sum() + (out.fine.depth * T(c_depth, dev)).sum()
    loss.backward()
    gl = m.encoder.latent.grad.cpu().numpy()
    ref = gold["latent_grad"]
    scale = np.abs(ref).max()
    assert np.abs(gl - ref).max() <= 2e-4 * scale, (np.abs(gl - ref).max(), scale)
    assert (ref != 0).mean() > 0.001
    for pname, p in m.mlp_fine.named_parameters():
        g = p.grad.cpu().numpy()
        norm = float(gold[f"g_norm/{pname}"])
        assert norm > 0, pname
        assert abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - norm) <= 1e-4 * norm, pname
        assert abs(g.astype(np.float64).sum() - float(gold[f"g_sum/{pname}"])) <= 2e-4 * norm * np.sqrt(g.size), pname
        idx = grad_probe_indices(g.shape)
        np.testing.assert_allclose(g.reshape(-1)[idx], gold[f"g_probe/{pname}"], rtol=0, atol=2e-4 * norm / np.sqrt(g.size) * 30 + 1e-7,
                                   err_msg=pname)
    # a fresh model: the gradients must not be cached state of this test
    _cases.pop(name, None)


# ---- the default mode is unchanged ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["g0_nv4_k16", "g4_nv4_k128_headline"])
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_ix_entry_points_with_the_default_mode_equal_the_old_ones(gname, precision, dev):
    from diner_amd import NeRFRendererDGS, _lib
    from diner_amd.renderer import _ptr, _stream
    from synthetic.model_stub import model_from_scene
    g = load_golden(gname)
    m = model_from_scene(g.scene, g.weights, device=dev)
    r = NeRFRendererDGS(n_samples=g.K, n_depth_candidates=g.NC, n_gaussian=g.G, white_bkgd=g.scene.white_bkgd)
    r.precision = precision
    L, prec, st = _lib.lib(), _lib.PRECISIONS[precision], _stream(dev)
    rays, z = T(g.rays, dev), T(g["z_fill"], dev)[None].contiguous()
    ix = _lib.DinerLatentIndex(0, 0)
    with torch.no_grad():
        packed = r._mlp(m)
        sc, _keep = r._scene(m, need_latent=True, packed_mlp=packed)
        SB, NR, K = z.shape
        n_scr = int(L.diner_render_points_scratch_floats(SB, sc.NV, prec))
        scr = torch.empty(max(n_scr, 1), dtype=torch.float32, device=dev)
        a, b = (torch.empty((SB, NR, K, 4), dtype=torch.float32, device=dev) for _ in range(2))
        assert L.diner_render_points(C.byref(sc), _ptr(packed), _ptr(rays), _ptr(z), NR, K, prec, _ptr(scr), _ptr(a), st) == 0
        assert L.diner_render_points_ix(C.byref(sc), C.byref(ix), _ptr(packed), _ptr(rays), _ptr(z), NR, K, prec, _ptr(scr), _ptr(b), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        # the whole path with the fixture's replayed noise
        cfg = r._cfg(g.K, g.NC, g.G)
        noise = [T(n, dev)[None].contiguous() for n in g.noise]
        ws = torch.empty(int(L.diner_render_workspace_floats(SB, NR, K, sc.NV, prec)), dtype=torch.float32, device=dev)
        outs = []
        for fn in ("diner_render", "diner_render_ix"):
            rgb = torch.empty((SB, NR, 3), dtype=torch.float32, device=dev)
            depth = torch.empty((SB, NR), dtype=torch.float32, device=dev)
            args = [C.byref(sc)] + ([C.byref(ix)] if fn.endswith("_ix") else []) + [
                _ptr(packed), _ptr(rays), NR, C.byref(cfg), int(bool(r.white_bkgd)), prec, *[_ptr(n) for n in noise], 1, _ptr(ws), _ptr(rgb),
                _ptr(depth), None, None, st]
            assert getattr(L, fn)(*args) == 0, fn
            torch.cuda.synchronize()
            outs.append((rgb, depth))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
