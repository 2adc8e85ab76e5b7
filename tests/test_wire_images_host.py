"""Host tests of the image wire format's restatement (tests/wire_images_ref.py) against the outputs of the reference's own readers
(tests/golden/wire_images.npz, written by tools/gen_wire_images_golden.py): read_rgba, read_rgb, read_img / read_alpha with gammaCorrect
and the white fill, Multiface's read_depth and std.

Bars: every non-gamma output and Multiface's depth and std bit-equal; the gamma outputs bit-equal outside the stored mask of entries
where the generating torch build's ``x ** 0.5`` is not the correctly rounded root, within one ulp of the root (2^-23) inside it, and the
mask at most 2 % of a case.  The same comparison must reject the wrong implementations of wire_images_ref.WRONG_IMAGE / WRONG_DEPTH on the
fixture's inputs.  One of them needs a word: `a <= 0.5` is the same function of an alpha byte as `a < 0.5` (no byte / 255 equals 0.5,
test_le_and_lt_coincide_at_one_half_on_bytes), so nothing can reject it at that threshold; "alpha_le" (<= at whichever threshold the rule
has) is rejected through the threshold 1, and the threshold 0.5 is pinned by its two one-byte neighbours."""
import numpy as np
import pytest

from tests import wire_images_ref as R
from tests.conftest import GOLDEN_DIR

CASES = ("ramp", "ramp_rev", "rand5x7", "rand33x64", "one")
DEPTH_CASES = {"const": None, "conf": "conf", "conf_high": "conf_high"}

_fx = {}


def fixture():
    if not _fx:
        _fx.update(np.load(GOLDEN_DIR / "wire_images.npz", allow_pickle=False))
    return _fx


def image_variants(case):
    """every (key, decode arguments, mask key) the fixture holds for a case: key + '/rgb' (and '/alpha') are the reference's outputs"""
    fx = fixture()
    px = fx[f"{case}/pixels"]
    for sym in (False, True):
        for bg in (1.0, 0.0):
            yield f"{case}/facescape/sym{int(sym)}/bg{int(bg)}", dict(pixels=px, alpha=None, bg_rule="below_half", bg=bg, gamma=False,
                                                                      symmetric_range=sym), None
        yield f"{case}/dtu/sym{int(sym)}", dict(pixels=px[..., :3], alpha=None, bg_rule="none", bg=1.0, gamma=False, symmetric_range=sym), None
        yield f"{case}/multiface/sym{int(sym)}", dict(pixels=px[..., :3], alpha=px[..., 3], bg_rule="below_one", bg=1.0, gamma=True,
                                                      symmetric_range=sym), f"{case}/multiface/sqrt_mask"


def image_failures(wrong=None):
    fx, out = fixture(), []
    for case in CASES:
        for key, kw, mkey in image_variants(case):
            rgb, a = R.decode_image(**kw, wrong=wrong)
            why = R.compare(rgb, fx[key + "/rgb"], None if mkey is None else fx[mkey])
            if not why and key + "/alpha" in fx:
                why = R.compare(a, fx[key + "/alpha"])
            if why:
                out.append(f"{key}: {why}")
    return out


def depth_failures(wrong=None):
    fx, out = fixture(), []
    for case, conf in DEPTH_CASES.items():
        d, s, _ = R.decode_multiface_depth(fx["depth/depth"], None if conf is None else fx[f"depth/{conf}"], wrong=wrong)
        for name, got in (("depth", d), ("std", s)):
            why = R.compare(got, fx[f"depth/{case}/{name}"])
            if why:
                out.append(f"depth/{case}/{name}: {why}")
    return out


def test_fixture_holds_the_cases():
    fx = fixture()
    i = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert fx["ramp/pixels"].shape == (1, 16, 16, 4) and all(np.array_equal(fx["ramp/pixels"][0, ..., c], i) for c in range(4))
    assert np.array_equal(fx["ramp_rev/pixels"][0, ..., :3], fx["ramp/pixels"][0, ..., :3]) and np.array_equal(fx["ramp_rev/pixels"][0, ..., 3], 255 - i)
    assert fx["rand5x7/pixels"].shape == (3, 5, 7, 4) and fx["rand33x64/pixels"].shape == (3, 33, 64, 4) and fx["one/pixels"].shape == (1, 1, 1, 4)
    for a in (127, 128, 254, 255):      # both sides of the two thresholds, in the random stacks too
        assert (fx["rand33x64/pixels"][..., 3] == a).any() and (fx["ramp/pixels"][..., 3] == a).any()
    d = fx["depth/depth"]
    assert d.shape == (2, 48, 48) and d.dtype == np.uint16 and 0.35 < (d == 0).mean() < 0.45
    assert ((fx["depth/conf_high/std"] == 0) & (fx["depth/conf_high/depth"] != 0)).mean() > 0.2      # the clip acts
    assert ((fx["depth/conf/std"] == 0) == (fx["depth/conf/depth"] == 0)).all()                       # and does not, there
    assert (fx["depth/const/std"][fx["depth/const/depth"] != 0] == np.float32(1e-3)).all()
    assert len([k for k in fx if k.endswith("/rgb")]) == len(CASES) * 8


def test_root_masks_are_small_and_not_empty():
    fx = fixture()
    masks = {c: fx[f"{c}/multiface/sqrt_mask"] for c in CASES}
    for c, m in masks.items():
        assert m.dtype == bool and m.shape == (fx[f"{c}/pixels"].shape[0], 3) + fx[f"{c}/pixels"].shape[1:3] and m.mean() <= 0.02, c
    print({c: f"{m.mean():.2%}" for c, m in masks.items()})
    # the ramp holds every (byte, channel) input once: the generating build's root was off for 7 of the 768 (4 red, 0 green, 3 blue)
    assert masks["ramp"].sum(axis=(0, 2, 3)).tolist() == [4, 0, 3]


def test_restatement_reproduces_the_readers_images():
    assert image_failures() == []


def test_restatement_reproduces_multiface_depth_and_std():
    assert depth_failures() == []


def test_the_gamma_outputs_differ_from_the_reference_only_by_the_root():
    """inside the mask the reference's value is the one a root one ulp lower gives, so the bar of one ulp is the tightest that holds"""
    fx = fixture()
    px, mask = fx["ramp/pixels"], fx["ramp/multiface/sqrt_mask"]
    v = np.ascontiguousarray(px[..., :3].transpose(0, 3, 1, 2)).astype(R.F) / R.F(255)
    root = np.sqrt(R.gamma_pre_root(v))
    lower = np.where(mask, np.nextafter(root, R.F(0)), root)
    want = np.where(np.broadcast_to((px[..., 3].astype(R.F) / R.F(255) < 1)[:, None], root.shape), R.F(1), R.gamma_post_root(lower))
    assert R.compare(want.astype(R.F), fx["ramp/multiface/sym0/rgb"]) == ""


@pytest.mark.parametrize("wrong", R.WRONG_IMAGE)
def test_comparison_rejects_a_wrong_image_decode(wrong):
    bad = image_failures(wrong)
    print(f"{wrong}: rejected on {len(bad)} outputs, e.g. {bad[:1]}")
    assert bad


@pytest.mark.parametrize("wrong", R.WRONG_DEPTH)
def test_comparison_rejects_a_wrong_depth_decode(wrong):
    bad = depth_failures(wrong)
    print(f"{wrong}: rejected on {len(bad)} outputs, e.g. {bad[:1]}")
    assert bad


def test_le_and_lt_coincide_at_one_half_on_bytes():
    a = np.arange(256).astype(R.F) / R.F(255)
    assert np.array_equal(a <= R.F(0.5), a < R.F(0.5)) and a[127] < 0.5 < a[128]
    assert not np.array_equal(a <= R.F(1), a < R.F(1))
    bad = image_failures("alpha_le")
    assert bad and all("/multiface/" in b for b in bad)          # told apart at the threshold 1 only


def test_division_and_reciprocal_differ_for_126_bytes():
    b = np.arange(256).astype(R.F)
    assert int((b / R.F(255) != b * (R.F(1) / R.F(255))).sum()) == 126
