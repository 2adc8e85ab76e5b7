"""The NOVEL point model under autograd, restated in torch (tests/novel_point_ref.py's building blocks), and the comparison of a set of
gradients with a ``tests/golden/novel_train_*.npz`` fixture (tools/gen_novel_train_golden.py: the unmodified reference's autograd).

``novel_train_forward``  novel_point_ref.novel_point_forward with the tensors that train taken as given (no cast that would cut the graph);
                         ``variant`` names a deliberately wrong form (the host tests prove the fixtures reject them).
``TrainableNovelModel``  the stand-in model of the GPU tests under autograd (the PyTorch route of a training step).
``reference_grads``      rgb-sigma and the gradients of ``(rgbsigma * cotangent).sum()`` by torch's autograd, in float64 or float32.
``check_fixture``        the bars of the GPU tests, in one place: the forward at tests/test_gpu_novel_point.py's (rgb 1e-4, sigma 1e-4
                         relative), parameter and latent gradients at tests/test_gpu_train_shapes.py's (``_check_params`` and its latent
                         checks), gen_latent's whole gradient at 2e-4 max|ref| + 1e-6 where the fixture stores it whole.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from tests import novel_point_ref as R
from tools.gen_novel_train_golden import CASES, case_inputs, cotangent, gen_grad_stored_whole, input_digests, latent_probe_indices

GOLDEN = Path(__file__).resolve().parent / "golden"
# the gen_latent gradient taken from view 0 only (the sum over the views left out) | the general lookup's feature_padding scaled by the
# encoder map's size instead of the general map's own
WRONG_VARIANTS = ("gen_grad_one_view", "gen_padding_of_encoder_map")

_loaded = {}


def load(name):
    """(inputs rebuilt from CASES' seeds and digest-checked, the fixture as a dict): built once, never changed"""
    if name not in _loaded:
        data = dict(np.load(GOLDEN / f"{name}.npz", allow_pickle=False))
        cfg = json.loads(str(data["config"]))
        assert cfg == json.loads(json.dumps(CASES[name])), name
        inp = case_inputs(cfg)
        assert json.loads(str(data["digests"])) == input_digests(inp), name
        _loaded[name] = (inp, data)
    return _loaded[name]


def novel_train_forward(xyz, gen_xyz, viewdirs, *, latent, gen_latent, weights, inp, variant=None):
    """-> rgb-sigma [SB,P,4] in the dtype of ``xyz``; ``latent`` [SB,NV,C,h,w], ``gen_latent`` [C,hg,wg] and ``weights`` (the fusion MLP's
    state dict) are used as they are (leaves of the caller's graph), every other tensor comes from ``inp`` (case_inputs)"""
    assert variant is None or variant in WRONG_VARIANTS
    cfg, d = inp["cfg"], inp["dims"]
    dt = xyz.dtype
    t = lambda a: torch.as_tensor(a).to(dtype=dt, device=xyz.device)
    poses, focal, c, image_shape, depths = [t(inp[k]) for k in ("poses", "focal", "c", "image_shape", "depths")]
    gen_poses, gen_focal, gen_c, gen_image_shape = [t(inp[k]) for k in ("gen_poses", "gen_focal", "gen_c", "gen_image_shape")]
    fp, interp, padding = cfg["scene"]["feature_padding"], cfg["index_interp"], cfg["index_padding"]
    n_blocks, combine_layer, beta, num_freqs = d["n_blocks"], d["combine_layer"], d["beta"], cfg["num_freqs"]
    SB, P, _ = xyz.shape
    NV = poses.shape[1]
    cam, uv = R._project(xyz, poses, focal, c, image_shape)
    _, gen_uv = R._project(t(gen_xyz), gen_poses.expand(-1, NV, -1, -1), gen_focal.expand(-1, NV, -1), gen_c.expand(-1, NV, -1), gen_image_shape)
    dirs = torch.matmul(poses[:, :, :3, :3], t(viewdirs).unsqueeze(1).expand(-1, NV, -1, -1).transpose(-1, -2)).transpose(-1, -2)
    x_in = torch.cat((R._posenc(cam, num_freqs, 6.28), dirs), dim=-1)
    z = None
    if min(combine_layer, n_blocks) > 0:
        z = R._lookup(latent.flatten(0, 1), uv.flatten(0, 1), fp, interp, padding).view(SB, NV, P, -1)
        guv = gen_uv.flatten(0, 1)
        if variant == "gen_padding_of_encoder_map":
            own = torch.tensor([gen_latent.shape[-1], gen_latent.shape[-2]], dtype=dt)
            enc = torch.tensor([latent.shape[-1], latent.shape[-2]], dtype=dt)
            guv = guv * ((enc - fp * 2) / enc) / ((own - fp * 2) / own)           # _lookup then applies the general map's own scale
        g = R._lookup(gen_latent.repeat(SB * NV, 1, 1, 1), guv, fp, interp, padding).view(SB, NV, P, -1)
        if variant == "gen_grad_one_view":
            g = torch.cat((g[:, :1], g[:, 1:].detach()), dim=1)
        z = g + z                                                                                         # novel_pixelnerf.py:196
    ref_depth = F.grid_sample(depths.flatten(0, 1), uv.flatten(0, 1).unsqueeze(2), align_corners=False, mode="nearest",
                              padding_mode="border")[:, 0, :, 0].view(SB, NV, P)
    delta = ref_depth - cam[..., -1]
    x = torch.cat((x_in, R._posenc(delta.unsqueeze(-1), num_freqs, 6.28)), dim=-1)
    act = (lambda v: F.softplus(v, beta=beta)) if beta > 0 else torch.relu
    lin = lambda name, v: F.linear(v, weights[name + ".weight"], weights[name + ".bias"])
    x = lin("lin_in", x)
    for b in range(n_blocks):
        if b == combine_layer:
            x = x.mean(dim=1)
        if b < combine_layer:
            x = x + lin(f"lin_z.{b}", z)
        net = lin(f"blocks.{b}.fc_0", act(x))
        x = x + lin(f"blocks.{b}.fc_1", act(net))
    out = lin("lin_out", act(x)).reshape(SB, P, 4)
    return torch.cat((torch.sigmoid(out[..., :3]), torch.relu(out[..., 3:4])), dim=-1)


class TrainableNovelModel(R.NovelPointModel):
    """novel_point_ref.NovelPointModel whose call keeps the graph to the fusion MLP's parameters as well (that one hands the MLP's
    ``state_dict()``, detached, to the restatement): what the PyTorch route of a training step evaluates.  ``case_inputs``: the case's
    inputs (cameras, maps, configuration), set by the caller."""

    def forward(self, xyz, gen_xyz, viewdirs=None):
        self.calls += 1
        return novel_train_forward(xyz.float(), gen_xyz, viewdirs, latent=self.encoder.latent, gen_latent=self.gen_latent,
                                   weights=dict(self.mlp_fine.named_parameters()), inp=self.case_inputs)


def reference_grads(inp, dtype=torch.float64, variant=None):
    """-> dict(rgbsigma, params {name: grad}, latent, gen): numpy arrays, by torch's autograd on the CPU in ``dtype``"""
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)
    w = {k: leaf(v) for k, v in inp["weights"].items()}
    latent, gen_latent = leaf(inp["latent"]), leaf(inp["gen_latent"])
    out = novel_train_forward(torch.from_numpy(inp["xyz_in"]).to(dtype), inp["xyz_gen"], inp["viewdirs"], latent=latent,
                              gen_latent=gen_latent, weights=w, inp=inp, variant=variant)
    (out * torch.from_numpy(cotangent(inp["cfg"])).to(dtype)).sum().backward()
    g = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
    return dict(rgbsigma=out.detach().numpy(), params={k: g(v) for k, v in w.items()}, latent=g(latent), gen=g(gen_latent))


def as_fixture(grads, cfg):
    """a ``reference_grads``-style dict in the record format of a fixture (what tools/gen_novel_train_golden.py stores), so that
    ``check_fixture`` can hold one evaluation to another at the same bars"""
    from oracle.gen_golden import grad_probe_indices
    from tools.gen_novel_train_golden import latent_record
    data = dict(rgbsigma=np.asarray(grads["rgbsigma"], np.float32)) if "rgbsigma" in grads else {}
    for pname, g in grads["params"].items():
        g = np.asarray(g)
        data[f"g_sum/{pname}"] = np.float64(g.astype(np.float64).sum())
        data[f"g_norm/{pname}"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        data[f"g_probe/{pname}"] = g.reshape(-1)[grad_probe_indices(g.shape)]
    data.update(latent_record("latent", np.asarray(grads["latent"])))
    data.update(latent_record("gen", np.asarray(grads["gen"])))
    if gen_grad_stored_whole(cfg):
        data["gen_grad"] = np.asarray(grads["gen"], np.float32)
    return data


def check_fixture(got, data, cfg, label="", forward=True):
    """``got``: reference_grads' dict (of any source) against the fixture ``data``; prints every figure next to its bound before asserting.
    ``forward`` False: the gradients only (the caller holds its own outputs to its own bar)"""
    from oracle.gen_golden import grad_probe_indices
    fails = []

    def hold(what, err, bound):
        print(f"{label} {what}: {err:.3e} (bound {bound:.3e})")
        if not err <= bound:
            fails.append((what, err, bound))

    if forward:
        e_rgb, e_sigma = R.rgbsigma_errors(got["rgbsigma"], data["rgbsigma"])
        hold("rgb", e_rgb, 1e-4)
        hold("sigma (relative to max(1, sigma/12))", e_sigma, 1e-4)
    for pname, g in got["params"].items():                         # tests/test_gpu_train_shapes.py::_check_params
        g = np.asarray(g)
        norm = float(data[f"g_norm/{pname}"])
        hold(f"{pname} norm", abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - norm), 1e-4 * norm)
        hold(f"{pname} sum", abs(g.astype(np.float64).sum() - float(data[f"g_sum/{pname}"])), 2e-4 * norm * np.sqrt(g.size))
        idx = grad_probe_indices(g.shape)
        hold(f"{pname} probes", float(np.abs(g.reshape(-1)[idx] - data[f"g_probe/{pname}"]).max()), 2e-4 * norm / np.sqrt(g.size) * 30 + 1e-7)
    for key in ("latent", "gen"):                                  # its latent checks
        g = np.asarray(got[key])
        lmax, lnorm = float(data[f"{key}_grad_max"]), float(data[f"{key}_grad_norm"])
        hold(f"{key} grad norm", abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - lnorm), 1e-4 * lnorm + 1e-6)
        hold(f"{key} grad max", abs(float(np.abs(g).max()) - lmax), 2e-4 * lmax + 1e-6)
        hold(f"{key} grad probes", float(np.abs(g.reshape(-1)[latent_probe_indices(g.shape)] - data[f"{key}_grad_probe"]).max()),
             2e-4 * lmax + 1e-6)
        if min(cfg["mlp"].get("combine_layer", 1000), cfg["mlp"]["n_blocks"]) == 0:
            hold(f"{key} grad nonzeros", float(np.count_nonzero(g)), 0.0)
    assert gen_grad_stored_whole(cfg) == ("gen_grad" in data)
    if "gen_grad" in data:
        ref = data["gen_grad"]
        hold("gen grad, whole map", float(np.abs(np.asarray(got["gen"]) - ref).max()), 2e-4 * float(np.abs(ref).max()) + 1e-6)
    assert not fails, fails
