"""Host tests of the image resizes' restatement (tests/wire_resize_ref.py) against the library calls the kernels replace, as stored in
tests/golden/wire_resize.npz by tools/gen_wire_resize_golden.py: PIL's ``Image.resize`` (byte for byte), ATen's nearest indices (every
destination index of the listed size pairs), ATen's ``F.interpolate`` in float64 (1e-12), and Multiface's sample as the reference's own
statements resize it (src/data/multiface.py:341-359) -- the float images under the bar of wire_resize_ref.float_bar on the reference's
decoded images (tests/wire_images_ref.py's one-ulp convention of gammaCorrect's root, through the stored mask), alphas, depths, stds,
sizes and intrinsics bit for bit.  The tables the library tabulates on the host (``diner_resize_table``, no GPU) are held against the
restatement's as well.  Reads tests/golden only."""
import numpy as np
import pytest

from tests import wire_images_ref as W
from tests import wire_resize_ref as R
from tests.conftest import GOLDEN_DIR

FLOAT_CASES = tuple(R.SIZES)
FORMATS = tuple(W.FORMATS)

_fx = {}


def fixture():
    if not _fx:
        _fx.update(np.load(GOLDEN_DIR / "wire_resize.npz", allow_pickle=False))
    return _fx


def source(case, fmt):
    """(pixels, alpha, symmetric_range) of a float case in a format: what the fixture's generator decoded"""
    px = fixture()[f"{case}/pixels"]
    if fmt == "facescape":
        return px, None, False
    return np.ascontiguousarray(px[..., :3]), (np.ascontiguousarray(px[..., 3]) if fmt == "multiface" else None), fmt == "multiface"


def pil_source(name, C_):
    src = fixture()["thirds/pixels" if name == "thirds" else ("up/pixels" if name == "up" else "odd/pixels")]
    return np.ascontiguousarray(src[..., :C_])


def test_fixture_holds_the_cases():
    fx = fixture()
    for case, (full, size) in R.SIZES.items():
        px = fx[f"{case}/pixels"]
        assert px.shape[1:] == full + (4,) and px.dtype == np.uint8 and px.shape[0] == (1 if case == "mf" else 3)
        for a in (127, 128, 254, 255):
            assert (px[..., 3] == a).any() or case == "one", (case, a)
        assert (px[..., :3] == 0).any() and (px[..., :3] == 255).any()
        for fmt in FORMATS:
            for aa in (0, 1):
                assert fx[f"{case}/{fmt}/aa{aa}/aten_distance"] < 3e-5
    assert R.SIZES["mf"][0][1] / R.SIZES["mf"][1][1] == 8.35 and all(n in (17, 18) for n in R.longest_windows(*R.SIZES["mf"]))
    assert fx["mf/multiface/aa1/f64"].shape == (1, 3, 32, 20) and fx["odd/multiface/aa0/f32"].dtype == np.float32
    assert tuple(fx["sample/size"]) == (32, 32) and fx["sample/pixels"].shape[1:3] != (32, 32)


@pytest.mark.parametrize("name", list(R.PIL_SIZES))
def test_fixed_point_bicubic_equals_pil(name):
    full, size = R.PIL_SIZES[name]
    for C_ in (3, 1):
        want = fixture()[f"pil/{name}/c{C_}"]
        got = R.resize_pil_u8(pil_source(name, C_), size)
        assert got.shape == want.shape and np.array_equal(got, want), (name, C_, int((got != want).sum()))


def test_fixed_point_weights_stay_in_a_32_bit_accumulator():
    for n_in, n_out in ((640, 320), (53, 26), (40, 60), (48, 17), (1600, 800), (7, 1)):
        k = R.pil_table(n_in, n_out)[2]
        assert np.abs(k).sum(1).max() < 1.3 * (1 << R.PRECISION_BITS) and 255 * np.abs(k).sum(1).max() + (1 << 21) < 2 ** 31


@pytest.mark.parametrize("pair", R.NEAREST_PAIRS)
def test_nearest_equals_aten_indices(pair):
    want = fixture()[f"nearest/{pair[0]}_{pair[1]}"]
    assert want.shape == (pair[1],) and np.array_equal(R.nearest_index(*pair), want)


@pytest.mark.parametrize("case", FLOAT_CASES)
def test_float_resamplers_equal_aten_float64(case):
    fx = fixture()
    full, size = R.SIZES[case]
    seen = 0
    for fmt in FORMATS:
        px, a, sym = source(case, fmt)
        for aa in (True, False):
            key = f"{case}/{fmt}/aa{int(aa)}/f64"
            if key not in fx:
                continue
            got = R.decode_resized(px, a, fmt, sym, size, aa)[0][:fx[key].shape[0]]
            err = np.abs(got - fx[key]).max()
            print(key, err)
            assert got.shape == fx[key].shape and err <= 1e-12, key
            assert np.abs(fx[key] - fx[key[:-3] + "f32"]).max() <= fx[f"{case}/{fmt}/aa{int(aa)}/aten_distance"]
            seen += 1
        if a is not None or fmt == "facescape":
            got_a = R.decode_resized(px, a, fmt, sym, size)[1]
            assert np.array_equal(got_a, fx[f"{case}/{fmt}/alpha"]), (case, fmt)
    assert seen or case == "ident"


def test_the_two_bilinear_filters_differ_on_a_downscale_by_far_more_than_the_bar():
    """what the GPU tests rest on when they show that the comparison rejects a wrong kernel"""
    fx = fixture()
    for case in ("odd", "mf"):
        full, size = R.SIZES[case]
        px, a, sym = source(case, "multiface")
        aa, plain = (R.decode_resized(px, a, "multiface", sym, size, k)[0] for k in (True, False))
        bar = R.float_bar(fx[f"{case}/multiface/aa1/aten_distance"], full, size, np.abs(aa).max())
        assert np.abs(aa - plain).max() > 100 * bar and bar < 2e-5, (case, bar)


def reference_decoded(px, mask):
    """the images as the reference's readers decode them: the restatement with the root one ulp lower inside the mask (the convention of
    tests/wire_images_ref.py), white where alpha < 1"""
    v = np.ascontiguousarray(px[..., :3].transpose(0, 3, 1, 2)).astype(W.F) / W.F(255)
    root = np.sqrt(W.gamma_pre_root(v))
    rgb = W.gamma_post_root(np.where(mask, np.nextafter(root, W.F(0)), root))
    hole = (px[..., 3].astype(W.F) / W.F(255) < 1)[:, None]
    return np.where(np.broadcast_to(hole, rgb.shape), W.F(1), rgb).astype(W.F)


@pytest.mark.parametrize("aa", [True, False])
def test_multiface_sample_equals_the_reference_statements(aa):
    fx = fixture()
    px, mask = fx["sample/pixels"], fx["sample/sqrt_mask"]
    assert mask.mean() <= 0.02
    H, Wd = px.shape[1:3]
    size = R.multiface_size(H, Wd, int(fx["sample/downsample"]))
    assert size == tuple(fx["sample/size"])
    key = f"sample/aa{int(aa)}"
    got = R.resize_float(reference_decoded(px, mask), size, aa)
    want = np.concatenate([fx[f"{key}/src_rgbs"], fx[f"{key}/target_rgb"][None]])
    bar = R.float_bar(fx[f"{key}/aten_distance"], (H, Wd), size, np.abs(want).max(), aa)
    err = np.abs(got - want).max()
    print(key, err, bar)
    assert want.shape == got.shape and err <= bar < 5e-6
    # without the mask's convention the decoded source itself is one ulp of the root off inside the mask, and nowhere else
    plain = W.decode_image(px[..., :3], px[..., 3], "below_one", 1.0, True, False)[0]
    assert W.compare(plain, reference_decoded(px, mask), mask) == ""
    # alphas, depths and stds: the nearest texels, bit for bit
    a = (px[..., 3].astype(W.F) / W.F(255))[:, None]
    want_a = np.concatenate([fx[f"{key}/src_alphas"], fx[f"{key}/target_alpha"][None]])
    assert np.array_equal(R.resize_nearest(a, size), want_a)
    d, s, _ = W.decode_multiface_depth(fx["sample/depth"], fx["sample/conf"])
    assert np.array_equal(R.resize_nearest(d, size), fx[f"{key}/src_depths"]) and np.array_equal(R.resize_nearest(s, size), fx[f"{key}/src_depth_stds"])
    assert ((fx[f"{key}/src_depth_stds"] == 0) >= (fx[f"{key}/src_depths"] == 0)).all() and (fx[f"{key}/src_depths"] == 0).any()
    K = fx["sample/intrinsics"]
    want_K = np.concatenate([fx[f"{key}/src_intrinsics"], fx[f"{key}/target_intrinsics"][None]])
    assert np.array_equal(R.scale_intrinsics(K, (H, Wd), size), want_K) and np.array_equal(want_K[:, 2], K[:, 2])


def test_multiface_size_and_scale_intrinsics_of_the_package():
    import torch

    from diner_amd import wire
    fx = fixture()
    H, Wd = fx["sample/pixels"].shape[1:3]
    assert wire.multiface_size(H, Wd, int(fx["sample/downsample"])) == tuple(fx["sample/size"])
    assert wire.multiface_size(2048, 1334) == (256, 160) and wire.multiface_size(2048, 1334, 1) == (2048, 1312)
    K = torch.from_numpy(fx["sample/intrinsics"])
    got = wire.scale_intrinsics(K, (H, Wd), (32, 32))
    want = np.concatenate([fx["sample/aa1/src_intrinsics"], fx["sample/aa1/target_intrinsics"][None]])
    assert np.array_equal(got.numpy(), want) and np.array_equal(K.numpy(), fx["sample/intrinsics"])      # a new tensor


@pytest.mark.parametrize("mode", ["bilinear_aa", "bilinear", "bicubic_u8"])
def test_library_tables_equal_the_restatement(mode):
    """diner_resize_table (host, double): the same windows; fixed-point weights equal, fp32 weights the rounded float64 ones"""
    from diner_amd import _lib
    L = _lib.lib()
    table = dict(bilinear_aa=R.aa_table, bilinear=R.bilinear_table, bicubic_u8=R.pil_table)[mode]
    for n_in, n_out in ((53, 26), (40, 60), (167, 20), (267, 32), (7, 1), (64, 64), (1334, 160), (17, 53)):
        xmin, n, w = table(n_in, n_out)
        taps = L.diner_resize_taps(n_in, n_out, _lib.RESIZE_MODES[mode])
        assert taps == n.max()
        bounds = np.full((n_out, 2), -7, np.int32)
        weights = np.full((n_out, taps + 1), -7, np.int32 if mode == "bicubic_u8" else np.float32)
        assert L.diner_resize_table(n_in, n_out, _lib.RESIZE_MODES[mode], taps + 1, bounds.ctypes.data, weights.ctypes.data) == 0
        assert np.array_equal(bounds[:, 0], xmin) and np.array_equal(bounds[:, 1], n) and (weights[:, -1] == 0).all()
        if mode == "bicubic_u8":
            assert np.array_equal(weights[:, :taps], w)
        else:
            assert np.array_equal(weights[:, :taps], w.astype(np.float32))
    assert L.diner_resize_taps(0, 4, 1) == -1 and L.diner_resize_taps(4, 0, 1) == -1 and L.diner_resize_taps(4, 4, 0) == -1
    assert L.diner_resize_table(4, 2, 1, 1, bounds.ctypes.data, weights.ctypes.data) == -1      # taps below the longest window
    assert L.diner_resize_table(4, 2, 1, 4, None, weights.ctypes.data) == -1
