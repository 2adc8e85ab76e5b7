"""GPU tests of the frame output and the image scores (glue.torch_cmap, glue.depth_range, glue.frames_u8, glue.image_scores;
diner_amd/csrc/frame_out.hip) on every case of tests/golden/frame_out.npz, against the fixture's reference outputs and the numpy
restatement of tests/frame_out_ref.py (tests/test_frame_out_host.py proves on the CPU that it reproduces the fixture and that its
comparisons reject wrong forms).  They read only the fixture: no matplotlib, scipy or reference tree.

Bounds:
* torch_cmap: bit-equal to the UNMODIFIED reference's float64 outputs (the device's double subtract, divide and multiply are IEEE, so the
  index is numpy's); the range equals torch.amin / torch.amax exactly, NaN as np.min / np.max;
* frames_u8: bit-equal to the restatement and to the fixture's bytes, both rules, separate and stacked, on the 16-byte and on the 4-byte path;
* l1, l2: within 4 ulp (fp64) of the restatement (an exact integer, one conversion, one division); psnr: 1e-12 relative (a few fp64
  roundings and log10); ssim: n_windows * 2^-52 absolute (every window's |S| is at most 1 and is formed by the same fp64 operations as
  the restatement's: the a-priori bound of an fp64 sum taken in another order); the identical pair gives exactly 0, 0, inf, 1.0; two
  calls agree bit for bit.

Largest error / bound ratios measured on an MI355X over all cases: see DESIGN.md §7 "Frame output and scores"."""
import numpy as np
import pytest
import torch

from tests import frame_out_ref as R
from tests.test_frame_out_host import CMAP_CASES, SCORE_CASES, SCORES, fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table_arg(cfg, d, dev):
    """"viridis" (the shipped table) or the fixture's other table as a tensor"""
    return "viridis" if cfg["table"] == "table" else T(d[cfg["table"]], dev)


def misaligned(a, dev):
    """the same values in a contiguous view that starts one element into its buffer: 4-byte aligned only"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = T(a, dev).reshape(-1)
    v = buf[1:].view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("name", CMAP_CASES)
def test_torch_cmap_is_bit_equal_to_the_reference(name, dev):
    from diner_amd import glue
    index, d = fixture()
    cfg = index["cmap"][name]
    depth, want = d[f"cmap.{name}.depth"], d[f"cmap.{name}.out"]
    got = glue.torch_cmap(T(depth, dev), table_arg(cfg, d, dev), vmin=cfg["vmin"], vmax=cfg["vmax"])
    assert got.shape == want.shape and got.dtype == torch.float64 and got.device == dev
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    # the reference's other two input shapes: (1,H,W) and (H,W) of image 0 (the limits are per image: alone it has the same)
    for view in (depth[0], depth[0, 0]):
        g = glue.torch_cmap(T(view, dev), table_arg(cfg, d, dev), vmin=cfg["vmin"], vmax=cfg["vmax"])
        assert g.shape == want[0].shape and np.array_equal(g.cpu().numpy().view(np.uint64), want[0].view(np.uint64))
    # one element into the buffer (an odd pixel count or an unaligned output takes the 8-byte path anyway)
    again = glue.torch_cmap(misaligned(depth, dev), table_arg(cfg, d, dev), vmin=cfg["vmin"], vmax=cfg["vmax"])
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))


@pytest.mark.parametrize("name", CMAP_CASES)
def test_depth_range(name, dev):
    from diner_amd import glue
    _, d = fixture()
    depth = T(d[f"cmap.{name}.depth"], dev)
    for x in (depth, misaligned(d[f"cmap.{name}.depth"], dev)):
        got = glue.depth_range(x)
        assert got.shape == (depth.shape[0], 2) and got.dtype == torch.float64 and got.device == dev
        flat = x.reshape(x.shape[0], -1)
        want = torch.stack([torch.amin(flat, dim=1), torch.amax(flat, dim=1)], dim=1).double()
        assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))
        assert np.array_equal(got.cpu().numpy(), R.depth_range_ref(d[f"cmap.{name}.depth"]), equal_nan=True)
    if name == "nan_inf":
        assert bool(torch.isnan(got[0]).all()) and float(got[1, 1]) == float("inf") and bool(torch.isfinite(got[1, 0]))


def test_depth_range_over_many_blocks(dev):
    """more pixels than one block's share (4096) and than all 64 blocks' first pass, vector and scalar path; a NaN in the last block's share"""
    from diner_amd import glue
    g = torch.Generator(device=dev).manual_seed(5)
    for H, W in ((96, 128), (515, 1031)):
        x = torch.randn((2, 1, H, W), device=dev, generator=g)
        x[1, 0, H - 1, W - 2] = 1e9
        x[0, 0, 0, 0] = -1e9
        got = glue.depth_range(x)
        flat = x.reshape(2, -1)
        assert torch.equal(got, torch.stack([flat.amin(1), flat.amax(1)], 1).double())
        x[1, 0, H - 1, W - 1] = float("nan")
        got = glue.depth_range(x)
        assert bool(torch.isnan(got[1]).all()) and torch.equal(got[0], torch.stack([flat[0].amin(), flat[0].amax()]).double())


@pytest.mark.parametrize("rounding", R.ROUNDINGS)
@pytest.mark.parametrize("name", CMAP_CASES)
def test_frames_u8_is_bit_equal(name, rounding, dev):
    from diner_amd import glue
    index, d = fixture()
    cfg = index["frames"][name]
    rgb, depth = d[f"frames.{name}.rgb"], d[f"cmap.{name}.depth"]
    kw = dict(rounding=rounding, cmap=table_arg(cfg, d, dev), vmin=cfg["vmin"], vmax=cfg["vmax"])
    want_c, want_d = d[f"frames.{name}.rgb_u8.{rounding}"], d[f"frames.{name}.depth_u8.{rounding}"]
    ref_c, ref_d = R.frames_u8_ref(rgb, depth, rounding, table=d[cfg["table"]], vmin=cfg["vmin"], vmax=cfg["vmax"])
    assert np.array_equal(ref_c, want_c) and np.array_equal(ref_d, want_d)
    for c_in, d_in in ((T(rgb, dev), T(depth, dev)), (misaligned(rgb, dev), misaligned(depth, dev))):     # W % 4 == 0: 16-byte, then 4-byte
        c, dep = glue.frames_u8(c_in, d_in, **kw)
        assert c.dtype == dep.dtype == torch.uint8 and c.device == dev and c.shape == dep.shape == want_c.shape
        assert np.array_equal(c.cpu().numpy(), want_c) and np.array_equal(dep.cpu().numpy(), want_d)
        stacked = glue.frames_u8(c_in, d_in, stacked=True, **kw)
        assert stacked.shape == (cfg["N"], 2 * cfg["H"], cfg["W"], 3)
        assert np.array_equal(stacked.cpu().numpy(), np.concatenate([want_c, want_d], axis=1))
        only = glue.frames_u8(c_in, rounding=rounding)
        assert np.array_equal(only.cpu().numpy(), want_c)
    # any leading shape: [N,1,..] and a single frame [3,H,W]
    c, dep = glue.frames_u8(T(rgb, dev)[:, None], T(depth, dev)[:, None], **kw)
    assert c.shape == (cfg["N"], 1, cfg["H"], cfg["W"], 3) and np.array_equal(c.cpu().numpy()[:, 0], want_c)
    assert np.array_equal(dep.cpu().numpy()[:, 0], want_d)
    assert glue.frames_u8(T(rgb, dev)[0], rounding=rounding).shape == (cfg["H"], cfg["W"], 3)


@pytest.mark.parametrize("W", [24, 23])
@pytest.mark.parametrize("rounding", R.ROUNDINGS)
def test_byte_ramp_nan_and_saturation(rounding, W, dev):
    """k / 255, (k + 0.5) / 255 and their fp32 neighbours, the values outside [0, 1], NaN and the infinities, as a colour image of width 24
    (16-byte path) and 23 (4-byte path)"""
    from diner_amd import glue
    _, d = fixture()
    v, want = d["bytes.values"], d[f"bytes.u8.{rounding}"]
    H = -(-v.size // (3 * W))
    pad = 3 * H * W - v.size
    img = np.concatenate([v, np.full(pad, 0.25, np.float32)]).reshape(1, 3, H, W)
    got = glue.frames_u8(T(img, dev), rounding=rounding).cpu().numpy()
    assert np.array_equal(got, R.frames_u8_ref(img, rounding=rounding))
    flat = got[0].transpose(2, 0, 1).reshape(-1)[:v.size]
    assert np.array_equal(flat, want)
    assert (flat[np.isnan(v)] == 0).all() and (flat[v < 0] == 0).all() and (flat[v > 1.01] == 255).all()


def score_bounds(cfg):
    nwin = (cfg["H"] - 6) * (cfg["W"] - 6)
    return nwin * 2.0 ** -52


@pytest.mark.parametrize("name", SCORE_CASES)
def test_image_scores(name, dev):
    from diner_amd import glue
    index, d = fixture()
    cfg = index["scores"][name]
    pred, gt = d[f"scores.{name}.pred"], d[f"scores.{name}.gt"]
    got = glue.image_scores(T(pred, dev), T(gt, dev))
    again = glue.image_scores(T(pred, dev), T(gt, dev))
    want = R.image_scores_ref(pred, gt)
    assert sorted(got) == sorted(SCORES)
    for k in SCORES:
        assert got[k].shape == (cfg["N"],) and got[k].dtype == torch.float64 and got[k].device == dev
        assert torch.equal(got[k].view(torch.int64), again[k].view(torch.int64)), k             # two runs: bit-equal
    g = {k: got[k].cpu().numpy() for k in SCORES}
    for k in ("l1", "l2"):
        err, bound = np.abs(g[k] - want[k]), 4.0 * np.spacing(np.abs(want[k]))
        print(f"{name}: {k}: worst err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (k, err, bound)
    finite = np.isfinite(want["psnr"])
    assert np.array_equal(g["psnr"][~finite], want["psnr"][~finite])                              # +inf where the fixture says so
    assert np.array_equal(np.isinf(d[f"scores.{name}.psnr_exact"]), ~finite)
    err, bound = np.abs(g["psnr"][finite] - want["psnr"][finite]), 1e-12 * np.abs(want["psnr"][finite])
    if finite.any():
        print(f"{name}: psnr: worst err {float(err.max()):.3e}, bound {float(bound.min()):.3e}")
    assert (err <= bound).all(), (err, bound)
    err, bound = np.abs(g["ssim"] - want["ssim"]), score_bounds(cfg)
    print(f"{name}: ssim: worst err / bound {float(err.max() / bound):.3f} (bound {bound:.3e})")
    assert (err <= bound).all(), (err, bound)
    if name == "identical_20x24":
        assert (g["l1"][0], g["l2"][0], g["psnr"][0], g["ssim"][0]) == (0.0, 0.0, np.inf, 1.0)
    # a leading shape of its own, and one image of the batch alone: the same numbers
    one = glue.image_scores(T(pred, dev)[0], T(gt, dev)[0])
    for k in SCORES:
        assert one[k].shape == (1,) and torch.equal(one[k].view(torch.int64), got[k][:1].view(torch.int64)), k


def test_image_scores_refusals_come_before_any_launch(dev):
    from diner_amd import glue
    for shape in ((1, 6, 20, 3), (1, 20, 6, 3)):
        z = torch.zeros(shape, dtype=torch.uint8, device=dev)
        with pytest.raises(ValueError, match="7 x 7"):
            glue.image_scores(z, z)
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError, match="frames_u8"):
        glue.image_scores(u8.float(), u8)
    with pytest.raises(ValueError, match="shapes differ"):
        glue.image_scores(u8, u8[:, :, :7])
    with pytest.raises(ValueError):
        glue.frames_u8(torch.zeros((1, 3, 4, 4), device=dev), stacked=True)
    with pytest.raises(ValueError):
        glue.frames_u8(torch.zeros((1, 3, 4, 4), device=dev), torch.zeros((1, 1, 4, 5), device=dev))
    torch.cuda.synchronize()                                     # nothing was launched that could have failed


def test_render_to_scores_end_to_end(dev):
    """render_image(..., return_depth=True) -> frames_u8 -> image_scores against a perturbed copy: finite, and equal to the restatement
    applied to the same device outputs"""
    from diner_amd import NeRFRendererDGS, glue
    from synthetic import synth
    from synthetic.model_stub import model_from_scene
    H, W = 24, 32
    sc = synth.make_scene(H, W, 3, seed=5, feature_padding=4)
    m = model_from_scene(sc, synth.make_mlp_weights(6, bias_scale=0.1), device=dev)
    r = NeRFRendererDGS(n_samples=16, n_depth_candidates=128, n_gaussian=5, white_bkgd=sc.white_bkgd)
    with torch.no_grad():
        rgb, depth = r.render_image(m, T(sc.target_extrinsics, dev)[None], T(sc.target_intrinsics, dev)[None], H, W, sc.near, sc.far,
                                    return_depth=True)
        assert rgb.shape == (1, 3, H, W) and depth.shape == (1, 1, H, W)
        g = torch.Generator(device=dev).manual_seed(9)
        gt = (rgb + 0.05 * torch.randn(rgb.shape, device=dev, generator=g)).clamp(0, 1)
        _, table = glue._cmap_table("viridis")
        for rounding in R.ROUNDINGS:
            pred_u8, depth_u8 = glue.frames_u8(rgb, depth, rounding=rounding)
            gt_u8 = glue.frames_u8(gt, rounding=rounding)
            want_c, want_d = R.frames_u8_ref(rgb.cpu().numpy(), depth.cpu().numpy(), rounding, table=table.numpy())
            assert np.array_equal(pred_u8.cpu().numpy(), want_c) and np.array_equal(depth_u8.cpu().numpy(), want_d)
            stacked = glue.frames_u8(rgb, depth, rounding=rounding, stacked=True)
            assert torch.equal(stacked, torch.cat((pred_u8, depth_u8), dim=-3))
            assert np.array_equal(glue.torch_cmap(depth).cpu().numpy(), R.torch_cmap_ref(depth.cpu().numpy(), table.numpy()))
            got = glue.image_scores(pred_u8, gt_u8)
            want = R.image_scores_ref(pred_u8.cpu().numpy(), gt_u8.cpu().numpy())
            for k in SCORES:
                v = got[k].cpu().numpy()
                assert np.isfinite(v).all(), k
            assert (np.abs(got["l1"].cpu().numpy() - want["l1"]) <= 4.0 * np.spacing(want["l1"])).all()
            assert (np.abs(got["l2"].cpu().numpy() - want["l2"]) <= 4.0 * np.spacing(want["l2"])).all()
            assert (np.abs(got["psnr"].cpu().numpy() - want["psnr"]) <= 1e-12 * np.abs(want["psnr"])).all()
            assert (np.abs(got["ssim"].cpu().numpy() - want["ssim"]) <= score_bounds(dict(H=H, W=W))).all()
            assert 0.0 < float(got["ssim"][0]) < 1.0 and float(got["l1"][0]) > 0.0
