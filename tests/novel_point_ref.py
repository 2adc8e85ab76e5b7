"""A torch restatement of the fork's NOVEL point model (reference src/models/novel/novel_pixelnerf.py:143-242 with
src/models/resnetfc.py:129-159, src/models/positional_encoding.py:33-53 and src/models/image_encoder.py:97-151), written from its
description: PixelNeRF evaluated at GIVEN points, with a learned latent, looked up at one general camera per scene, added to the
encoder's latent in every view before the fusion MLP.  It takes tensors, not the reference's classes, and computes in the dtype of
``xyz`` (float32 or float64; every other tensor is cast to it, so the float64 form is the same function of the same float32 data).

``novel_point_forward``  the restatement; ``variant`` names a deliberately wrong form (the host tests prove the fixtures reject them).
``NovelPointModel``      the stand-in model of the GPU tests and the bench, where the reference does not exist: synthetic.model_stub's
                         attribute surface + the ``gen_*`` state, callable like the reference (``model(xyz, gen_xyz, viewdirs=...)``).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from synthetic.model_stub import PixelNeRFState

WRONG_VARIANTS = ("no_gen", "swapped", "gen_once")   # gen lookup dropped | xyz_gen and xyz_in swapped | gen latent added in view 0 only


def _project(p, poses, focal, c, image_shape):
    """world points [SB,P,3], cameras [SB,NV,..] -> camera points [SB,NV,P,3], uv [SB,NV,P,2] (novel_pixelnerf.py:159-161, :177-180)"""
    NV = poses.shape[1]
    p = p.unsqueeze(1).expand(-1, NV, -1, -1)
    cam = torch.matmul(poses[:, :, :3, :3], p.transpose(-2, -1)).transpose(-2, -1) + poses[:, :, :3, -1].unsqueeze(-2)
    uv = cam[..., :2] / cam[..., 2:]
    uv = uv * focal.unsqueeze(-2)
    uv = uv + c.unsqueeze(-2)
    uv = uv / image_shape * 2 - 1
    return cam, uv


def _lookup(maps, uv, feature_padding, interp, padding):
    """maps [N,C,h,w], uv [N,P,2] -> [N,P,C]: SpatialEncoder.index (image_encoder.py:97-127) / PixelNeRF.index (:108-141)"""
    size = torch.tensor([maps.shape[-1], maps.shape[-2]], dtype=uv.dtype, device=uv.device)
    uv = uv * ((size - feature_padding * 2) / size).view(1, 1, 2)
    s = F.grid_sample(maps, uv.unsqueeze(2), align_corners=False, mode=interp, padding_mode=padding)
    return s[:, :, :, 0].transpose(-1, -2)


def _posenc(x, num_freqs, freq_factor):
    """positional_encoding.py:33-53 with include_input; the frequencies are the reference's float32 values"""
    freqs = (np.float32(freq_factor) * np.float32(2.0) ** np.arange(num_freqs, dtype=np.float32)).astype(np.float32)
    fr = torch.as_tensor(np.repeat(freqs, 2), dtype=x.dtype, device=x.device).view(1, -1, 1)
    ph = torch.zeros(2 * num_freqs, dtype=torch.float32)
    ph[1::2] = math.pi * 0.5
    ph = ph.to(dtype=x.dtype, device=x.device).view(1, -1, 1)
    flat = x.reshape(-1, x.shape[-1])
    e = torch.sin(torch.addcmul(ph, flat.unsqueeze(1).repeat(1, 2 * num_freqs, 1), fr)).view(flat.shape[0], -1)
    return torch.cat((flat, e), dim=-1).reshape(*x.shape[:-1], -1)


def novel_point_forward(xyz, gen_xyz, viewdirs, *, poses, focal, c, image_shape, depths, latent, gen_latent, gen_poses, gen_focal, gen_c,
                        gen_image_shape, weights, n_blocks, combine_layer, beta=0.0, num_freqs=6, freq_factor=6.28, feature_padding=0.0,
                        index_interp="bilinear", index_padding="border", variant=None):
    """-> rgb-sigma [SB,P,4].  poses [SB,NV,4,4], focal / c [SB,NV,2], image_shape [2] (W,H), depths [SB,NV,1,H,W], latent
    [SB,NV,C,h,w]; gen_latent [C,hg,wg], gen_poses [SB,1,4,4], gen_focal / gen_c [SB,1,2], gen_image_shape [2]; ``weights``: the
    fusion MLP's state dict (name -> tensor)."""
    assert variant is None or variant in WRONG_VARIANTS
    dt, dev = xyz.dtype, xyz.device
    t = lambda a: torch.as_tensor(a).to(dtype=dt, device=dev)
    poses, focal, c, image_shape, depths, latent = [t(a) for a in (poses, focal, c, image_shape, depths, latent)]
    gen_latent, gen_poses, gen_focal, gen_c, gen_image_shape = [t(a) for a in (gen_latent, gen_poses, gen_focal, gen_c, gen_image_shape)]
    w = {k: t(v) for k, v in weights.items()}
    gen_xyz, viewdirs = t(gen_xyz), t(viewdirs)
    if variant == "swapped":
        xyz, gen_xyz = gen_xyz, xyz
    SB, P, _ = xyz.shape
    NV = poses.shape[1]
    cam, uv = _project(xyz, poses, focal, c, image_shape)
    _, gen_uv = _project(gen_xyz, gen_poses.expand(-1, NV, -1, -1), gen_focal.expand(-1, NV, -1), gen_c.expand(-1, NV, -1), gen_image_shape)
    dirs = torch.matmul(poses[:, :, :3, :3], viewdirs.unsqueeze(1).expand(-1, NV, -1, -1).transpose(-1, -2)).transpose(-1, -2)
    x_in = torch.cat((_posenc(cam, num_freqs, freq_factor), dirs), dim=-1)
    nlz = min(combine_layer, n_blocks)
    z = None
    if nlz > 0:
        z = _lookup(latent.flatten(0, 1), uv.flatten(0, 1), feature_padding, index_interp, index_padding).view(SB, NV, P, -1)
        if variant != "no_gen":
            g = _lookup(gen_latent.repeat(SB * NV, 1, 1, 1), gen_uv.flatten(0, 1), feature_padding, index_interp, index_padding)
            g = g.view(SB, NV, P, -1)
            if variant == "gen_once":
                g = torch.cat((g[:, :1], torch.zeros_like(g[:, 1:])), dim=1)
            z = g + z                                                                                     # :196
    ref_depth = F.grid_sample(depths.flatten(0, 1), uv.flatten(0, 1).unsqueeze(2), align_corners=False, mode="nearest",
                              padding_mode="border")[:, 0, :, 0].view(SB, NV, P)
    delta = ref_depth - cam[..., -1]                                                                      # :199-200
    x = torch.cat((x_in, _posenc(delta.unsqueeze(-1), num_freqs, freq_factor)), dim=-1)                   # :225 (after the latent)
    act = (lambda v: F.softplus(v, beta=beta)) if beta > 0 else torch.relu
    lin = lambda name, v: F.linear(v, w[name + ".weight"], w[name + ".bias"])
    x = lin("lin_in", x)                                                                                  # resnetfc.py:143
    for b in range(n_blocks):
        if b == combine_layer:
            x = x.mean(dim=1)                                                                             # :148-151
        if b < combine_layer:
            x = x + lin(f"lin_z.{b}", z)                                                                  # :153-155
        net = lin(f"blocks.{b}.fc_0", act(x))                                                             # :62-69
        x = x + lin(f"blocks.{b}.fc_1", act(net))
    out = lin("lin_out", act(x)).reshape(SB, P, 4)                                                        # :158, novel_pixelnerf.py:234
    return torch.cat((torch.sigmoid(out[..., :3]), torch.relu(out[..., 3:4])), dim=-1)


class NovelPointModel(PixelNeRFState):
    """synthetic.model_stub's state + the NOVEL model's ``gen_latent`` parameter and ``gen_*`` camera buffers; calling it evaluates
    ``novel_point_forward`` in float32 on the tensors' device, like the reference's ``forward(xyz, gen_xyz, viewdirs)``."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.gen_latent = torch.nn.Parameter(torch.zeros(1, 1, 1), requires_grad=False)
        self.gen_poses = self.gen_focal = self.gen_c = self.gen_image_shape = None
        self.calls = 0

    def forward(self, xyz, gen_xyz, viewdirs=None):
        self.calls += 1
        e, m = self.encoder, self.mlp_fine
        beta = float(getattr(m.activation, "beta", 0.0)) if isinstance(m.activation, torch.nn.Softplus) else 0.0
        return novel_point_forward(
            xyz.float(), gen_xyz, viewdirs, poses=self.poses, focal=self.focal, c=self.c, image_shape=self.image_shape, depths=e.depths,
            latent=e.latent, gen_latent=self.gen_latent, gen_poses=self.gen_poses, gen_focal=self.gen_focal, gen_c=self.gen_c,
            gen_image_shape=self.gen_image_shape, weights=dict(m.state_dict()), n_blocks=m.n_blocks, combine_layer=m.combine_layer,
            beta=beta, num_freqs=self.poscode.num_freqs, freq_factor=float(self.poscode.freqs[0]), feature_padding=e.feature_padding,
            index_interp=e.index_interp, index_padding=e.index_padding)


def model_from_inputs(inp, device="cuda") -> NovelPointModel:
    """the stand-in of one case of tools/gen_novel_point_golden.py (``case_inputs``)"""
    cfg = inp["cfg"]
    d = inp["dims"]
    m = NovelPointModel(feature_padding=cfg["scene"]["feature_padding"], num_freqs=cfg["num_freqs"],
                        **{k: d[k] for k in ("d_latent", "d_hidden", "n_blocks", "combine_layer", "beta")})
    m.mlp_fine.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp["weights"].items()}, strict=True)
    m.gen_latent = torch.nn.Parameter(torch.from_numpy(inp["gen_latent"]), requires_grad=False)
    m = m.to(device)
    for p in m.parameters():
        p.requires_grad_(False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    for k in ("poses", "focal", "c", "image_shape", "gen_poses", "gen_focal", "gen_c", "gen_image_shape"):
        setattr(m, k, t(inp[k]))
    e = m.encoder
    e.depths, e.depths_std, e.normals, e.latent = t(inp["depths"]), t(inp["depths_std"]), t(inp["normals"]), t(inp["latent"])
    e.nviews, e.nobjects = inp["poses"].shape[1], inp["poses"].shape[0]
    e.index_interp, e.index_padding = cfg["index_interp"], cfg["index_padding"]
    return m.eval()


def rgbsigma_errors(got, ref):
    """(max |rgb| error, max sigma error relative to max(1, sigma / 12)): the bars of tests/test_gpu_mlp_shapes*.py, both 1e-4"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    s = ref[..., 3]
    return float(np.abs(got[..., :3] - ref[..., :3]).max()), float((np.abs(got[..., 3] - s) / np.maximum(1.0, s / 12.0)).max())
