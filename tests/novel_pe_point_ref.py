"""A torch restatement of the fork's NOVEL_PE point model (reference src/models/novel_pe/pe_novel_pixelnerf.py:200-292 with
src/models/resnetfc.py:129-159, src/models/positional_encoding.py:33-53 and src/models/image_encoder.py:97-151), written from its
description: the NOVEL model of tests/novel_point_ref.py with a third point set projected by one target camera per scene, two
3-channel pos-encoding lookups (per view at the encoder lookup's uv; once per point at the target uv), a linear deformation layer on
cat(latent, src_pe, tgt_pe) whose output is added to the general latent's lookup, and the six pe values behind the latent in the
fusion MLP's input.  It takes tensors, not the reference's classes, and computes in the dtype of ``xyz`` (float32 or float64).

``novel_pe_point_forward``  the restatement; ``variant`` names a deliberately wrong form (the host tests prove the fixtures reject
                            them); ``hoisted`` evaluates the deformation layer the way the kernels do: its latent part applied to
                            the latent's texels (a map), looked up, then the head b_d + W6 . pe6 added.
``NovelPePointModel``       the stand-in model of the GPU tests and the bench, where the reference does not exist, callable like the
                            reference (``model(xyz, gen_xyz, tgt_xyz, viewdirs=...)``).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from synthetic.model_stub import PixelNeRFState
from tests.novel_point_ref import _lookup, _posenc, _project, rgbsigma_errors  # noqa: F401  (rgbsigma_errors: the tests' bars)

# the deformation layer dropped | the target lookup at xyz_in | src_pe and tgt_pe swapped | the pe columns dropped from the MLP's input
# | the target pe taken per view through the source cameras
WRONG_VARIANTS = ("no_deform", "tgt_at_in", "pe_swapped", "pe_dropped", "tgt_per_view")


def novel_pe_point_forward(xyz, gen_xyz, tgt_xyz, viewdirs, *, poses, focal, c, image_shape, depths, latent, pos_encodings, gen_latent,
                           gen_poses, gen_focal, gen_c, gen_image_shape, tgt_pos_encoding, tgt_poses, tgt_focal, tgt_c, tgt_image_shape,
                           deform_w, deform_b, weights, n_blocks, combine_layer, beta=0.0, num_freqs=6, freq_factor=6.28,
                           feature_padding=0.0, index_interp="bilinear", index_padding="border", variant=None, hoisted=False):
    """-> rgb-sigma [SB,P,4].  The NOVEL arguments of novel_point_forward (latent [SB,NV,C,h,w]) + pos_encodings [SB,NV,3,hp,wp],
    tgt_pos_encoding [SB,1,3,ht,wt], tgt_poses [SB,1,4,4], tgt_focal / tgt_c [SB,1,2], tgt_image_shape [2] (W,H), deform_w
    [C,C+6], deform_b [C]; ``weights``: the fusion MLP's state dict with lin_z of C + 6 columns."""
    assert variant is None or variant in WRONG_VARIANTS
    dt, dev = xyz.dtype, xyz.device
    t = lambda a: torch.as_tensor(a).to(dtype=dt, device=dev)
    poses, focal, c, image_shape, depths, latent, pos_encodings = [t(a) for a in (poses, focal, c, image_shape, depths, latent, pos_encodings)]
    gen_latent, gen_poses, gen_focal, gen_c, gen_image_shape = [t(a) for a in (gen_latent, gen_poses, gen_focal, gen_c, gen_image_shape)]
    tgt_pos_encoding, tgt_poses, tgt_focal, tgt_c, tgt_image_shape = [t(a) for a in (tgt_pos_encoding, tgt_poses, tgt_focal, tgt_c, tgt_image_shape)]
    deform_w, deform_b = t(deform_w), t(deform_b)
    w = {k: t(v) for k, v in weights.items()}
    gen_xyz, tgt_xyz, viewdirs = t(gen_xyz), t(tgt_xyz), t(viewdirs)
    if variant == "tgt_at_in":
        tgt_xyz = xyz
    SB, P, _ = xyz.shape
    NV = poses.shape[1]
    Cc = deform_w.shape[0]
    look = lambda maps, uv: _lookup(maps, uv.flatten(0, 1), feature_padding, index_interp, index_padding).view(SB, NV, P, -1)
    per_view = lambda a: a.expand(-1, NV, *a.shape[2:])
    cam, uv = _project(xyz, poses, focal, c, image_shape)                                                  # :216-218, :238-241
    _, gen_uv = _project(gen_xyz, per_view(gen_poses), per_view(gen_focal), per_view(gen_c), gen_image_shape)
    if variant == "tgt_per_view":
        _, tgt_uv = _project(tgt_xyz, poses, focal, c, image_shape)
    else:
        _, tgt_uv = _project(tgt_xyz, per_view(tgt_poses), per_view(tgt_focal), per_view(tgt_c), tgt_image_shape)   # :224-226, :248-251
    dirs = torch.matmul(poses[:, :, :3, :3], viewdirs.unsqueeze(1).expand(-1, NV, -1, -1).transpose(-1, -2)).transpose(-1, -2)
    x_in = torch.cat((_posenc(cam, num_freqs, freq_factor), dirs), dim=-1)
    nlz = min(combine_layer, n_blocks)
    z = None
    if nlz > 0:
        src_pe = look(pos_encodings.flatten(0, 1), uv)                                                    # :134-165, :260
        tgt_pe = look(tgt_pos_encoding.reshape(SB, 1, *tgt_pos_encoding.shape[-3:]).repeat(1, NV, 1, 1, 1).flatten(0, 1), tgt_uv)   # :262
        if variant == "pe_swapped":
            src_pe, tgt_pe = tgt_pe, src_pe
        g = look(gen_latent.repeat(SB * NV, 1, 1, 1), gen_uv)                                             # :256
        if variant == "no_deform":
            cond = look(latent.flatten(0, 1), uv)
        elif hoisted:
            dmap = torch.einsum("oc,nchw->nohw", deform_w[:, :Cc], latent.flatten(0, 1))                  # W_d[:, :C] on every texel
            cond = look(dmap, uv) + (F.linear(src_pe, deform_w[:, Cc:Cc + 3]) + F.linear(tgt_pe, deform_w[:, Cc + 3:Cc + 6]) + deform_b)
        else:
            cond = F.linear(torch.cat((look(latent.flatten(0, 1), uv), src_pe, tgt_pe), dim=-1), deform_w, deform_b)   # :265-266
        final = g + cond                                                                                  # :268
        if variant == "pe_dropped":
            src_pe, tgt_pe = torch.zeros_like(src_pe), torch.zeros_like(tgt_pe)
        z = torch.cat((final, src_pe, tgt_pe), dim=-1)                                                    # :275
    ref_depth = F.grid_sample(depths.flatten(0, 1), uv.flatten(0, 1).unsqueeze(2), align_corners=False, mode="nearest",
                              padding_mode="border")[:, 0, :, 0].view(SB, NV, P)
    delta = ref_depth - cam[..., -1]                                                                      # :271-272
    x = torch.cat((x_in, _posenc(delta.unsqueeze(-1), num_freqs, freq_factor)), dim=-1)                   # :275 (after the latent and the pe)
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
    out = lin("lin_out", act(x)).reshape(SB, P, 4)                                                        # :158, pe_novel_pixelnerf.py:284
    return torch.cat((torch.sigmoid(out[..., :3]), torch.relu(out[..., 3:4])), dim=-1)


class NovelPePointModel(PixelNeRFState):
    """synthetic.model_stub's state with a fusion MLP of d_latent = C + 6, + the NOVEL_PE model's ``gen_latent`` parameter,
    ``deformation_layer``, ``gen_*`` / ``tgt_*`` buffers and ``pos_encodings``; calling it evaluates ``novel_pe_point_forward`` in float32
    on the tensors' device, like the reference's ``forward(xyz, gen_xyz, tgt_xyz, viewdirs)``."""

    def __init__(self, C, **kw):
        super().__init__(d_latent=C + 6, **kw)
        self.encoder.latent_size = C
        self.deformation_layer = torch.nn.Linear(C + 6, C)
        self.gen_latent = torch.nn.Parameter(torch.zeros(1, 1, 1), requires_grad=False)
        self.gen_poses = self.gen_focal = self.gen_c = self.gen_image_shape = None
        self.tgt_poses = self.tgt_focal = self.tgt_c = self.tgt_image_shape = self.tgt_pos_encoding = self.pos_encodings = None
        self.calls = 0

    def forward(self, xyz, gen_xyz, tgt_xyz, viewdirs=None):
        self.calls += 1
        e, m = self.encoder, self.mlp_fine
        beta = float(getattr(m.activation, "beta", 0.0)) if isinstance(m.activation, torch.nn.Softplus) else 0.0
        return novel_pe_point_forward(
            xyz.float(), gen_xyz, tgt_xyz, viewdirs, poses=self.poses, focal=self.focal, c=self.c, image_shape=self.image_shape,
            depths=e.depths, latent=e.latent, pos_encodings=self.pos_encodings, gen_latent=self.gen_latent, gen_poses=self.gen_poses,
            gen_focal=self.gen_focal, gen_c=self.gen_c, gen_image_shape=self.gen_image_shape, tgt_pos_encoding=self.tgt_pos_encoding,
            tgt_poses=self.tgt_poses, tgt_focal=self.tgt_focal, tgt_c=self.tgt_c, tgt_image_shape=self.tgt_image_shape,
            deform_w=self.deformation_layer.weight, deform_b=self.deformation_layer.bias, weights=dict(m.state_dict()),
            n_blocks=m.n_blocks, combine_layer=m.combine_layer, beta=beta, num_freqs=self.poscode.num_freqs,
            freq_factor=float(self.poscode.freqs[0]), feature_padding=e.feature_padding, index_interp=e.index_interp,
            index_padding=e.index_padding)


CAMERA_KEYS = ("poses", "focal", "c", "image_shape", "gen_poses", "gen_focal", "gen_c", "gen_image_shape", "tgt_poses", "tgt_focal", "tgt_c",
               "tgt_image_shape", "pos_encodings", "tgt_pos_encoding")


def model_from_inputs(inp, device="cuda") -> NovelPePointModel:
    """the stand-in of one case of tools/gen_novel_pe_point_golden.py (``case_inputs``)"""
    cfg = inp["cfg"]
    d = inp["dims"]
    m = NovelPePointModel(cfg["scene"]["C"], feature_padding=cfg["scene"]["feature_padding"], num_freqs=cfg["num_freqs"],
                          **{k: d[k] for k in ("d_hidden", "n_blocks", "combine_layer", "beta")})
    m.mlp_fine.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp["weights"].items()}, strict=True)
    m.deformation_layer.load_state_dict({"weight": torch.from_numpy(inp["deform_w"]), "bias": torch.from_numpy(inp["deform_b"])}, strict=True)
    m.gen_latent = torch.nn.Parameter(torch.from_numpy(inp["gen_latent"]), requires_grad=False)
    m = m.to(device)
    for p in m.parameters():
        p.requires_grad_(False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    for k in CAMERA_KEYS:
        setattr(m, k, t(inp[k]))
    e = m.encoder
    e.depths, e.depths_std, e.normals, e.latent = t(inp["depths"]), t(inp["depths_std"]), t(inp["normals"]), t(inp["latent"])
    e.nviews, e.nobjects = inp["poses"].shape[1], inp["poses"].shape[0]
    e.index_interp, e.index_padding = cfg["index_interp"], cfg["index_padding"]
    return m.eval()
