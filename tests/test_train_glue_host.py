"""A training step's ray selection and photometric losses (diner_gen_rays_at / _backward, diner_photo_loss / _backward; glue.gen_rays_at,
glue.photo_loss, glue.calc_losses) as far as it goes without a GPU: the float64 restatement of tests/train_glue_ref.py reproduces every
case of tests/golden/train_glue.npz (written by tools/gen_golden_train_glue.py from the unmodified reference) -- the recorded float64
evaluation to 1e-12 relative, the reference's fp32 results within the deviation the fixture records for them, gt_colors bit for bit -- and
the same comparisons reject four deliberately wrong forms; every non-degenerate pooled difference of the fixture is at least 1e-4; the new
entry points are declared, exported and bound with the header's argument counts; bad arguments raise before any launch."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import train_glue_ref as R

ROOT = Path(__file__).resolve().parents[1]
REL = 1e-12
NEW_SYMBOLS = ("diner_gen_rays_at", "diner_gen_rays_at_backward_workspace_floats", "diner_gen_rays_at_backward",
               "diner_photo_loss_workspace_floats", "diner_photo_loss", "diner_photo_loss_backward")
_fixture = {}


def fixture():
    """{case name: (cfg, {field: array})} of tests/golden/train_glue.npz, read once"""
    if not _fixture:
        d = dict(np.load(ROOT / "tests" / "golden" / "train_glue.npz", allow_pickle=False))
        for name, cfg in json.loads(str(d["index"])).items():
            _fixture[name] = (cfg, {k.split(".", 1)[1]: v for k, v in d.items() if k.startswith(name + ".")})
    return _fixture


CASES = ("patch_s8_n3", "patch_s10_n2", "patch_s12_n2", "patch_s64_n3", "patch_s12_n2_equal_cell", "random_b1", "random_b130", "random_b128")


def _off(got, want64, want32, dev, what):
    """None, or why ``got`` (float64) is not the recorded evaluation: 1e-12 relative to the tensor's largest entry against the float64
    record, and the reference's fp32 record within its own recorded deviation of ``got``"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    if got.shape != want64.shape:
        return f"{what}: shape {got.shape} != {want64.shape}"
    scale = float(np.abs(want64).max()) if want64.size else 0.0
    err = float(np.abs(got - want64).max()) if want64.size else 0.0
    if not err <= REL * scale:
        return f"{what}: off the float64 record by {err:.3e} (scale {scale:.3e})"
    err32 = float(np.abs(np.asarray(want32, dtype=np.float64) - got).max()) if want64.size else 0.0
    if not err32 <= float(dev) + REL * scale:
        return f"{what}: the fp32 record is {err32:.3e} away, its recorded deviation is {float(dev):.3e}"
    return None


def camera_mismatch(name, variant=None):
    cfg, d = fixture()[name]
    grads = R.gen_rays_at_grads_ref(d["E"], d["K"], cfg["W"], cfg["H"], d["zn"], d["zf"], d["idx"], d["d_rays"], variant=variant)
    for k, g in zip(("dE", "dK", "dn", "df"), grads):
        why = _off(g.numpy(), d[k + "64"], d[k + "32"], d["dev_" + k], k)
        if why:
            return why
    return None


def loss_mismatch(name, variant=None):
    cfg, d = fixture()[name]
    patch = cfg.get("s")
    mse, ab, gt = R.photo_loss_ref(d["pred"], d["target"], d["idx"], patch, cfg.get("n", 3), variant=variant)
    if gt.dtype != torch.float32 or not np.array_equal(gt.numpy(), d["gt"]):
        return "gt_colors is not bit-equal"
    for k, v in (("mse", mse), ("ab", ab)):
        why = _off(v.numpy(), d[k + "64"], d[k + "32"], d["dev_" + k], k)
        if why:
            return why
    return None


def dpred_mismatch(name, variant=None):
    cfg, d = fixture()[name]
    got, mse_term, ab_term = R.photo_loss_dpred_ref(d["pred"], d["gt"], cfg.get("s"), cfg.get("n", 3), float(d["g"][0]), float(d["g"][1]),
                                                    variant=variant)
    assert torch.equal(got, mse_term + ab_term)
    return _off(got.numpy(), d["d_pred64"], d["d_pred32"], d["dev_d_pred"], "d_pred")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    cfg, d = fixture()[name]
    assert d["idx"].dtype == np.int64 and d["idx"].shape == (cfg["SB"], cfg["B"])
    assert camera_mismatch(name) is None
    assert loss_mismatch(name) is None
    assert dpred_mismatch(name) is None
    if "s" not in cfg:
        assert float(d["ab64"]) == 0.0 and float(d["ab32"]) == 0.0


def test_fixture_covers_the_stated_cases():
    fx = fixture()
    assert set(fx) == set(CASES)
    assert {(c["H"], c["W"]) for c, _ in fx.values()} == {(24, 40), (64, 64)} and {c["SB"] for c, _ in fx.values()} == {1, 2}
    assert {(c["s"], c["n"]) for c, _ in fx.values() if "s" in c} == {(8, 3), (10, 2), (12, 2), (64, 3)}
    assert {c["B"] for c, _ in fx.values() if "s" not in c} == {1, 130, 128}
    for name in ("random_b130", "random_b128"):
        cfg, d = fx[name]
        for row in d["idx"]:
            assert 0 in row and cfg["H"] * cfg["W"] - 1 in row and len(set(row.tolist())) < len(row)     # both ends, duplicates


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("patch")])
def test_no_pooled_difference_is_near_a_sign_flip(name):
    """every pooled difference is at least 1e-4 in magnitude, except the deliberate exact zeros of the equal cell"""
    cfg, d = fixture()[name]
    diff = R.pooled_diff_ref(torch.from_numpy(d["pred"]).double(), torch.from_numpy(d["gt"]).double(), cfg["s"], cfg["n"])
    zero = diff == 0
    if cfg.get("equal"):
        assert bool(zero[0, :, 1, 0].all()) and int(zero.sum()) == 3
        diff32 = R.pooled_diff_ref(torch.from_numpy(d["pred"]), torch.from_numpy(d["gt"]), cfg["s"], cfg["n"], )
        assert bool((diff32[0, :, 1, 0] == 0).all())               # separately pooled in the same order: exact in any precision
    else:
        assert not bool(zero.any())
    assert float(diff[~zero].abs().min()) >= float(fixture()[name][1]["min_abs_pooled_diff"]) * (1 - 1e-9) >= 1e-4 * (1 - 1e-9)


@pytest.mark.parametrize("variant, compare, name", [
    ("swap_xy", camera_mismatch, "random_b130"),
    ("swap_xy", camera_mismatch, "patch_s10_n2"),
    ("swap_xy", loss_mismatch, "random_b130"),
    ("ceil_pool", loss_mismatch, "patch_s10_n2"),
    ("ceil_pool", dpred_mismatch, "patch_s10_n2"),
    ("diff_pool_tiny_sign", dpred_mismatch, "patch_s12_n2_equal_cell"),
    ("mean_div_channels", loss_mismatch, "random_b1"),
    ("mean_div_channels", dpred_mismatch, "patch_s64_n3"),
])
def test_the_comparison_rejects_a_wrong_restatement(variant, compare, name):
    assert variant in R.VARIANTS
    assert compare(name) is None
    why = compare(name, variant)
    print(variant, name, "->", why)
    assert why is not None


def test_tiny_sign_variant_changes_the_equal_cell_only_in_the_gradient():
    """pooling the difference leaves the losses where they were (that wrong form shows in d_pred of the equal cell alone)"""
    assert loss_mismatch("patch_s12_n2_equal_cell", "diff_pool_tiny_sign") is None
    cfg, d = fixture()["patch_s12_n2_equal_cell"]
    s, p = cfg["s"], 2 ** cfg["n"]
    _, _, ab_term = R.photo_loss_dpred_ref(d["pred"], d["gt"], s, cfg["n"], 1.0, 1.0)
    ab = ab_term.view(cfg["SB"], s, s, 3)
    assert bool((ab[0, p:2 * p, :p] == 0).all()) and bool((ab[0, :p, :p] != 0).all())


def test_closed_form_d_pred_equals_float64_autograd():
    cfg, d = fixture()["patch_s10_n2"]
    pred = torch.from_numpy(d["pred"]).double().requires_grad_(True)
    mse, ab, _ = R.photo_loss_ref(pred, d["target"], d["idx"], cfg["s"], cfg["n"])
    want, = torch.autograd.grad(0.7 * mse + 1.3 * ab, pred)
    got, _, ab_term = R.photo_loss_dpred_ref(d["pred"], d["gt"], cfg["s"], cfg["n"], 0.7, 1.3)
    assert float((got - want).abs().max()) <= 1e-15
    img = ab_term.view(cfg["SB"], cfg["s"], cfg["s"], 3)
    assert bool((img[:, 8:] == 0).all()) and bool((img[:, :, 8:] == 0).all())       # the dropped remainder: no antibias gradient


def _params(decl):
    return [p for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",") if p.strip()]


def test_symbols_are_declared_exported_and_bound_with_the_headers_argument_counts():
    from diner_amd import _lib
    header = (ROOT / "include" / "diner_hip.h").read_text()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        m = re.search(rf"^int(64_t)? {name}\([^;]*\);", header, re.M)
        assert m, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        res, args = _lib.SYMBOLS[name]
        assert len(args) == len(_params(m.group(0))), name
    for cite in ("diner.py:224-227", "diner.py:265", "src/losses/antibiasloss.py"):
        assert cite in header, cite
    assert "train_glue.hip" in (ROOT / "diner_amd" / "csrc" / "Makefile").read_text()
    assert lib.diner_version() == _lib.ABI_VERSION == 3      # additions only


PTR = 4096    # a non-NULL dummy device pointer: never dereferenced, every call below is refused before a launch


@pytest.mark.parametrize("kw, code, word", [
    (dict(B=63, patch=8), -1, "patch * patch"),
    (dict(B=64, patch=8, pool=3), -1, "power of two"),
    (dict(B=16, patch=4, pool=8), -1, "smaller"),
    (dict(B=64 * 64, patch=64, pool=64), -3, "pool=64"),
    (dict(B=0), -1, "no rays"),
    (dict(H=0), -1, "bad size"),
    (dict(pred=None), -1, "NULL"),
    (dict(B=64, patch=8, pool=8, sign=None), -1, "NULL"),
])
def test_photo_loss_bad_arguments_return_their_code_before_any_launch(kw, code, word):
    from diner_amd import _lib
    lib = _lib.lib()
    a = dict(pred=PTR, target=PTR, idx=PTR, SB=1, B=16, H=8, W=8, patch=0, pool=1, sign=PTR)
    a.update(kw)
    rc = lib.diner_photo_loss(a["pred"], a["target"], a["idx"], 1, a["SB"], a["B"], a["H"], a["W"], a["patch"], a["pool"], PTR, PTR, a["sign"],
                              PTR, None)
    msg = lib.diner_last_error().decode()
    assert rc == code and word in msg and msg.startswith("photo_loss"), (rc, msg)


def test_gen_rays_at_bad_arguments_return_their_code_before_any_launch():
    from diner_amd import _lib
    lib = _lib.lib()
    for kw, code in ((dict(W=0), -1), (dict(B=-1), -1), (dict(E=None), -1), (dict(SB=70000), -3)):
        a = dict(E=PTR, SB=1, B=4, H=8, W=8)
        a.update(kw)
        rc = lib.diner_gen_rays_at(a["E"], PTR, PTR, PTR, PTR, 1, a["SB"], a["B"], a["H"], a["W"], PTR, None)
        assert rc == code and lib.diner_last_error().decode().startswith("gen_rays_at:"), (kw, rc)
        rc = lib.diner_gen_rays_at_backward(a["E"], PTR, PTR, PTR, 1, a["SB"], a["B"], a["H"], a["W"], PTR, PTR, PTR, PTR, PTR, None)
        assert rc == code and lib.diner_last_error().decode().startswith("gen_rays_at_backward:"), (kw, rc)
    assert lib.diner_gen_rays_at_backward_workspace_floats(2, 4096) == 2 * 16 * 18 * 2      # a function of SB and B only
    assert lib.diner_gen_rays_at_backward_workspace_floats(1, 10 ** 6) == 64 * 18 * 2
    assert lib.diner_gen_rays_at_backward_workspace_floats(-1, 4) == -1
    assert lib.diner_photo_loss_workspace_floats(4, 4096, 64, 8) == 4 * 8 * 4 and lib.diner_photo_loss_workspace_floats(1, 15, 4, 2) == -1


def test_python_side_refuses_before_the_device():
    from diner_amd import glue
    E, K = torch.eye(4).expand(2, 4, 4), torch.eye(3).expand(2, 3, 3)
    H, W = 6, 9
    ok = torch.tensor([[0, 5], [H * W - 1, 7]])
    for bad in (-1, H * W):
        idx = ok.clone()
        idx[1, 1] = bad
        with pytest.raises(IndexError, match=r"outside \[0, H\*W = 54\)"):
            glue.gen_rays_at(E, K, W, H, 0.5, 2.5, idx, check_indices=True)
        with pytest.raises(IndexError):
            glue.gen_rays_at(E, K, W, H, 0.5, 2.5, idx.int(), check_indices=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.gen_rays_at(E, K, W, H, 0.5, 2.5, ok, check_indices=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.gen_rays_at(E, K, W, H, 0.5, 2.5, ok)
    with pytest.raises(ValueError, match="int64 or int32"):
        glue.gen_rays_at(E, K, W, H, 0.5, 2.5, ok.float())
    pred, target, idx = torch.zeros(2, 16, 3), torch.zeros(2, 3, H, W), torch.zeros(2, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="smaller than the 8 x 8 pooling cell"):
        glue.photo_loss(pred, target, idx, patch=4, antibias_downsampling=3)
    with pytest.raises(ValueError, match="patch \\* patch"):
        glue.photo_loss(pred, target, idx, patch=5, antibias_downsampling=1)
    with pytest.raises(ValueError, match=r"\[SB, B, 3\]"):
        glue.photo_loss(pred[..., :2], target, idx)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.photo_loss(pred, target, idx, patch=4, antibias_downsampling=2)
    with pytest.raises(RuntimeError, match="GPU only"):
        glue.photo_loss(pred, target, idx)
    with pytest.raises(ValueError, match="need the patch side"):
        glue.calc_losses(None, None, dict(target_rgb=target), 0.5, 2.5, idx, w_antibias=0.1)
    with pytest.raises(ValueError, match="needs vggloss"):
        glue.calc_losses(None, None, dict(target_rgb=target), 0.5, 2.5, idx, patch=4, w_vgg=0.1)
