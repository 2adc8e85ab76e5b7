"""The renderer of the fork's NOVEL / NOVEL_PE configurations (reference ``src/models/novel/nerf_novel_renderer.py`` and
``src/models/novel_pe/pe_nerf_novel_renderer.py``) on the device: ``renderer.module: diner_amd.novel.NeRFRendererDGS``.

Every candidate and every sample is moved by the offset of its nearest mesh vertex before a source view or the model sees it:

* ``sample_depthguided``  -- three launches: ``diner_sample_coarse`` (the stratified depths), ``diner_deform_ray_points`` (the points
  of those depths, deformed by ``tgt_in_offsets``) and ``diner_sample_depthguided_points`` (csrc/sampler_points.hip: the depth-guided
  sampler on given candidate points).  One seed per call: the noise is the stream contract of ``diner_sample_depthguided``.
* ``fill_up_uniform_samples`` -- inherited.
* ``composite``           -- ``glue.deform_ray_points`` with both offset sets from one search, the model on the deformed points in
  the reference's chunks, then ``diner_composite`` under autograd (``diner_composite_backward``): gradient to the model's
  rgb-sigma, hence to its parameters, and to nothing else.
* ``forward``             -- the reference's three stages and its output object.

The point model is any callable ``model(in_deformed, gen_deformed[, points], viewdirs=dirs) -> [SB,B',4]`` with ``poses``, ``focal``,
``c``, ``image_shape`` and an ``encoder`` holding ``depths``, ``depths_std``, ``normals``; it runs on PyTorch unless the renderer was
constructed with ``hip_point_model=True`` and the model is the NOVEL ``PixelNeRF`` (reference src/models/novel/novel_pixelnerf.py):

* ``render_points_novel`` -- that model on the shape-general point/MLP kernels' "novel" form (csrc/points_mlp_gen_nv.hip,
  points_mlp_gen_f16_nv.hip through ``diner_render_points_novel``): given points, per-point viewdirs, and the model's learned
  ``gen_latent`` looked up at the general camera and added to the encoder's latent.  Inference: grad mode off, or no parameter of
  the model requiring grad.
* ``_train_points_novel`` -- with ``train_hip_point_model=True`` as well, the same model under autograd (an MLP parameter,
  ``encoder.latent`` or ``gen_latent`` requires grad): ``diner_amd/training_novel.py`` on the shape-general training path --
  ``diner_train_point_inputs_novel`` and ``diner_train_novel_gen_scatter`` (csrc/train_novel.hip) around the layer schedule of
  ``diner_amd/training_gen.py``, in exact fp32 or (``precision == "f16x3"`` with ``train_f16x3_any_shape``) in f16x3: gradients to the
  MLP's parameters, ``encoder.latent`` and ``gen_latent``; ``last_route`` "novel_train_gen" / "novel_train_gen_f16".  Without that
  switch training stays on PyTorch (``last_route == "torch"``).
* ``render_points_novel_pe`` -- with ``pass_points``, the NOVEL_PE ``PixelNeRF`` (reference src/models/novel_pe/pe_novel_pixelnerf.py)
  on the "novel_pe" form (csrc/points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip through ``diner_render_points_novel_pe``): a
  third point set for the target camera, two 3-channel pos-encoding lookups, and the deformation layer applied to the latent's
  texels once per encode (csrc/novel_pe_map.hip).  Inference only: NOVEL_PE trains on PyTorch.
"""
from __future__ import annotations

import ctypes as C
import warnings
from types import SimpleNamespace

import torch
from torch.autograd.function import once_differentiable

from . import _lib, deform
from ._lib import check
from .renderer import NeRFRendererDGS as _Renderer
from .renderer import RenderOutput, _f32c, _ptr, _Sources, _stream


class _MapsModel:
    """what ``_scene(model, need_latent=False)`` reads, of a model that need not be a ``PixelNeRF``: the cameras and the encoder's
    depth / std / normal maps; the fields of the latent lookup and the positional code, which no sampler reads, take defaults"""

    def __init__(self, model):
        enc = model.encoder
        self.poses, self.focal, self.c, self.image_shape = model.poses, model.focal, model.c, model.image_shape
        self.encoder = SimpleNamespace(depths=enc.depths, depths_std=enc.depths_std, normals=enc.normals,
                                       feature_padding=float(getattr(enc, "feature_padding", 0.0)))
        self.poscode = SimpleNamespace(num_freqs=0, freqs=[1.0])


class _PaddedMlp:
    """the NOVEL_PE model's fusion MLP as the point kernels see it: d_latent = C + 6 padded to C + 8, ``lin_z`` the padded copies of
    ``NeRFRendererDGS._pe_mlp_pack`` (None where only the shape is read); every other attribute is the MLP's own"""

    def __init__(self, mlp, lin_z):
        self._mlp, self.lin_z, self.d_latent = mlp, lin_z, int(mlp.d_latent) + 2

    def __getattr__(self, k):
        return getattr(self._mlp, k)


class _CompositeFn(torch.autograd.Function):
    """rgbsigma [SB,B,K,4] -> (weights, rgb, depth) by ``diner_composite``; backward by ``diner_composite_backward`` (gradient to
    rgbsigma only: rays and depths are data here)"""

    @staticmethod
    def forward(ctx, rgbsigma, rays, z, white, status):
        c = _f32c(rgbsigma)
        SB, NR, K = z.shape
        dev = rays.device
        weights = torch.empty((SB, NR, K), dtype=torch.float32, device=dev)
        rgb = torch.empty((SB, NR, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((SB, NR), dtype=torch.float32, device=dev)
        check(_lib.lib().diner_composite(_ptr(rays), _ptr(z), _ptr(c), SB * NR, K, int(white), _ptr(rgb), _ptr(depth), _ptr(weights),
                                         _ptr(status), _stream(dev)), "diner_composite")
        ctx.save_for_backward(rgbsigma, rays, z)   # (the inputs themselves; rays and z arrive fp32 and contiguous from composite)
        ctx.set_materialize_grads(False)       # an output the loss does not read hands backward None, diner_composite_backward's NULL
        ctx.white, ctx.dtype = int(white), rgbsigma.dtype
        return weights, rgb, depth

    @staticmethod
    @once_differentiable                       # the hand-written backward has no graph of its own: a double backward raises
    def backward(ctx, d_weights, d_rgb, d_depth):
        rgbsigma, rays, z = ctx.saved_tensors
        c = _f32c(rgbsigma)
        SB, NR, K = z.shape
        dev = rays.device
        g = torch.zeros((SB, NR, 3), dtype=torch.float32, device=dev) if d_rgb is None else _f32c(d_rgb)
        gd = None if d_depth is None else _f32c(d_depth)
        gw = None if d_weights is None else _f32c(d_weights)
        out = torch.empty((SB, NR, K, 4), dtype=torch.float32, device=dev)
        check(_lib.lib().diner_composite_backward(_ptr(rays), _ptr(z), _ptr(c), _ptr(g), _ptr(gd), _ptr(gw), SB * NR, K, ctx.white,
                                                  _ptr(out), _stream(dev)), "diner_composite_backward")
        return out.to(ctx.dtype), None, None, None, None


class NeRFRendererDGS(_Renderer):
    """The NOVEL renderer (reference nerf_novel_renderer.py:13-38): the constructor of the reference, and ``pass_points``: True for
    NOVEL_PE, whose model takes the undeformed points as a third argument (pe_nerf_novel_renderer.py)."""

    def __init__(self, n_samples=40, n_depth_candidates=1000, n_gaussian=15, eval_batch_size=100000, white_bkgd=True, pass_points=False,
                 hip_point_model=False, f16x3_any_shape=False, train_hip_point_model=False, train_f16x3_any_shape=False):
        super().__init__(n_samples=n_samples, n_depth_candidates=n_depth_candidates, n_gaussian=n_gaussian,
                         eval_batch_size=eval_batch_size, white_bkgd=white_bkgd, f16x3_any_shape=f16x3_any_shape,
                         train_f16x3_any_shape=train_f16x3_any_shape)
        self.pass_points = bool(pass_points)
        # composite() evaluates the NOVEL PixelNeRF with one render_points_novel call for all B K points instead of the chunked
        # PyTorch calls, when gradients are off (or no parameter of the model requires grad), the model is recognisably that one (its
        # gen_latent and gen_* buffers, a fusion MLP _validate accepts, no deformation_layer), pass_points is False and the encoder's
        # lookup is a 4-tap mode.  Anything else -- training (without train_hip_point_model, below), a bicubic encoder, another
        # callable -- goes the PyTorch way, as with the switch off.  last_route: "novel_points_gen" / "novel_points_gen_f16" (precision == "f16x3" with f16x3_any_shape,
        # as on the plain renderer) or "torch".  Opt-in; a plain attribute, so that a config can set it (renderer.kwargs.hip_point_model).
        self.hip_point_model = bool(hip_point_model)
        # Training of that model on the HIP path: with hip_point_model AND train_hip_point_model, grad mode on, and an MLP parameter,
        # encoder.latent or gen_latent requiring grad, composite() evaluates the NOVEL PixelNeRF by diner_amd/training_novel.py
        # (csrc/train_novel.hip + the shape-general training GEMMs; any shape of the envelope, the standard one included) instead of
        # the chunked PyTorch model: gradients to those three, last_route "novel_train_gen", or "novel_train_gen_f16" when precision ==
        # "f16x3" and train_f16x3_any_shape is set (the plain renderer's switch: the GEMMs in f16x3).  Off: such a call stays on
        # PyTorch, as before.  NOVEL_PE (pass_points) and a bicubic encoder always do.  Opt-in; plain attributes, so that a config can
        # set them (renderer.kwargs.train_hip_point_model, renderer.kwargs.train_f16x3_any_shape).
        self.train_hip_point_model = bool(train_hip_point_model)
        self._gen_latent_key = self._gen_latent_pack = None      # the model's gen_latent, NHWC
        self._gen_cam_key = self._gen_cam_pack = None            # its general cameras, fp32 and contiguous
        # With pass_points the same switch serves the NOVEL_PE PixelNeRF (a deformation_layer Linear(C + 6 -> C), the gen_* and tgt_*
        # state, pos_encodings; a fusion MLP inside the envelope once its d_latent C + 6 is padded to C + 8) through
        # render_points_novel_pe: last_route "novel_pe_points_gen" / "novel_pe_points_gen_f16".  Its packs, each under a _Sources key:
        self._pe_linz_key = self._pe_linz_pad = None             # lin_z[b].weight padded with two zero columns
        self._pe_map_key = self._pe_map_pack = None              # the deformation map W_d[:, :C] . latent (encoder.latent, deformation_layer.weight)
        self._pe_head_key = self._pe_head_pack = None            # the [C][8] head table (deformation_layer.weight, .bias)
        self._pe_pos_key = self._pe_pos_pack = None              # pos_encodings and tgt_pos_encoding, NHWC with 4 channels
        self._pe_cam_key = self._pe_cam_pack = None              # the target cameras

    def deform_points(self, points, target_vertices, offsets):
        """reference :40-50"""
        return deform.deform_points(points, target_vertices, offsets)

    @torch.no_grad()
    def sample_depthguided(self, rays, model, n_samples, n_candidates, target_vertices, tgt_in_offsets, depth_diff_max=0.05,
                           n_gaussian=None, *, noise=None, return_internals=False):
        """Depth-guided short-list + gaussian samples of the DEFORMED candidates (reference :79-167): returns z [SB,NR,n_samples]
        before fill-up (0 = empty slot).  ``noise=(u_coarse, n_gauss, u_fill)``: dense tensors (any of them None) replacing the
        Philox streams 0 / 1 / 2 of the call's one seed.  ``return_internals``: also a dict with ``z_cand`` [SB,NR,NC], ``xyz_cand``
        [SB,NR,NC,3], ``likelihood`` [SB,NR,NC], ``z_dg`` (the return value), ``z`` (filled and sorted) and ``seed``."""
        G = self.n_gaussian if n_gaussian is None else n_gaussian
        out = self._sample_deformed(rays, model, int(n_samples), int(n_candidates), G, target_vertices, tgt_in_offsets, depth_diff_max,
                                    noise, want_lik=return_internals)
        return (out["z_dg"], out) if return_internals else out["z_dg"]

    def _sample_deformed(self, rays, model, K, NC, G, target_vertices, tgt_in_offsets, depth_diff_max, noise, want_lik):
        r = self._check_rays(rays)
        SB, NR, _ = r.shape
        dev = r.device
        sc, _keep = self._scene(_MapsModel(model), need_latent=False)
        assert SB == sc.SB
        cfg = self._cfg(K, NC, G, depth_diff_max)
        u_c = n_g = u_f = None
        if noise is not None:
            u_c, n_g, u_f = [None if t is None else _f32c(t).to(dev) for t in noise]
            if u_c is not None: assert u_c.numel() == SB * NR * NC
            if n_g is not None: assert n_g.numel() == SB * NR * G
            if u_f is not None: assert u_f.numel() == SB * NR * K
        L, st, seed = _lib.lib(), _stream(dev), self._next_seed()
        z_cand = torch.empty((SB, NR, NC), dtype=torch.float32, device=dev)
        # (the global ray index sb * NR + ray is the Philox ray counter of both launches)
        check(L.diner_sample_coarse(_ptr(r), SB * NR, NC, _ptr(u_c), seed, _ptr(z_cand), st), "diner_sample_coarse")
        xyz = deform.deform_ray_points(r, z_cand, target_vertices, tgt_in_offsets, method="auto")      # [SB, NR*NC, 3]
        z = torch.empty((SB, NR, K), dtype=torch.float32, device=dev)
        z_dg = torch.empty_like(z)
        lik = torch.empty((SB, NR, NC), dtype=torch.float32, device=dev) if want_lik else None
        check(L.diner_sample_depthguided_points(C.byref(sc), _ptr(r), _ptr(z_cand), _ptr(xyz), NR, C.byref(cfg), _ptr(n_g), _ptr(u_f),
                                                seed, _ptr(z), _ptr(z_dg), _ptr(lik), st), "diner_sample_depthguided_points")
        return dict(z_cand=z_cand, xyz_cand=xyz.view(SB, NR, NC, 3), likelihood=lik, z_dg=z_dg, z=z, seed=seed)

    @staticmethod
    def _no_data_grad(**tensors):
        """rays, depths, vertices and offsets are data here: one that requires grad is refused, never silently left without a gradient"""
        if not torch.is_grad_enabled():
            return
        for name, t in tensors.items():
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise NotImplementedError(f"diner_amd.novel.NeRFRendererDGS: {name} requires grad, but the NOVEL compositing carries "
                                          "gradient to the model's rgb-sigma only (vertices and offsets are data, as in the reference); "
                                          "the training path with ray and camera gradients is diner_amd.NeRFRendererDGS.forward "
                                          "(diner_amd/training.py), which serves the plain renderer")

    # ------------------------------------------------------------------------------------------------------------------------------
    # the NOVEL point model on the HIP kernels
    # ------------------------------------------------------------------------------------------------------------------------------
    _GEN_STATE = ("gen_latent", "gen_poses", "gen_focal", "gen_c", "gen_image_shape")

    def _novel_gen(self, model, dev):
        """``model``'s general latent and cameras as a DinerNovelGen (+ the tensors it points into).  gen_latent [C,h,w] is packed to
        NHWC by diner_pack_latent (N = 1) and cached under a _Sources key like the encoder's latent: an optimizer step re-packs it."""
        gl = model.gen_latent
        if gl.dim() != 3:
            raise ValueError(f"gen_latent must be [C, h, w], not {tuple(gl.shape)}")
        if self._gen_latent_key is None or not self._gen_latent_key.valid_for([gl]):
            src = _f32c(gl).to(dev)
            Cc, h, w = src.shape
            pack = torch.empty((h, w, Cc), dtype=torch.float32, device=dev)
            check(_lib.lib().diner_pack_latent(_ptr(src), 1, Cc, h, w, _ptr(pack), _stream(dev)), "diner_pack_latent")
            torch.cuda.current_stream(dev).synchronize()     # `src` may be a temporary
            self._gen_latent_pack, self._gen_latent_key = pack, _Sources([gl])
        cams = [model.gen_poses, model.gen_focal, model.gen_c, model.gen_image_shape]
        if self._gen_cam_key is None or not self._gen_cam_key.valid_for(cams):
            poses = _f32c(model.gen_poses).to(dev)
            poses = poses.reshape(-1, *poses.shape[-2:])                       # [SB,1,4,4] (encode_gen) or [SB,4,4]; 3 x 4 accepted
            if poses.shape[-2:] != (4, 4):
                full = torch.zeros((poses.shape[0], 4, 4), dtype=torch.float32, device=dev)
                full[:, :3, :] = poses[:, :3, :]
                full[:, 3, 3] = 1
                poses = full
            ishape = [float(v) for v in model.gen_image_shape.detach().float().cpu()]   # (W, H), novel_pixelnerf.py:80-81
            self._gen_cam_pack = (poses.contiguous(), _f32c(model.gen_focal).to(dev).reshape(-1, 2).contiguous(),
                                  _f32c(model.gen_c).to(dev).reshape(-1, 2).contiguous(), ishape)
            self._gen_cam_key = _Sources(cams)
        pack, (poses, focal, c, ishape) = self._gen_latent_pack, self._gen_cam_pack
        g = _lib.DinerNovelGen()
        g.latent, (g.h, g.w, g.C) = pack.data_ptr(), pack.shape
        g.poses, g.focal, g.c = poses.data_ptr(), focal.data_ptr(), c.data_ptr()
        g.image_w, g.image_h = ishape
        return g, (pack, poses, focal, c)

    def memory_report(self, model=None, rays_per_call=None, n_views=None):
        """the plain renderer's report + ``cached["gen_latent_nhwc"]``: the packed copy of the NOVEL model's general latent, and of the
        NOVEL_PE route ``cached["novel_pe_map"]`` (the deformation map: the latent's byte size) and ``cached["novel_pe_pos_encodings"]``
        (both packed pos-encoding maps); 0 until that route has run"""
        rep = super().memory_report(model, rays_per_call=rays_per_call, n_views=n_views)
        nb = lambda t: 0 if t is None else t.numel() * t.element_size()
        rep["cached"]["gen_latent_nhwc"] = nb(self._gen_latent_pack)
        rep["cached"]["novel_pe_map"] = nb(self._pe_map_pack)
        rep["cached"]["novel_pe_pos_encodings"] = sum(nb(t) for t in (self._pe_pos_pack or ()))
        rep["cached"]["total"] = sum(v for k, v in rep["cached"].items() if k != "total")
        return rep

    @torch.no_grad()
    def render_points_novel(self, model, in_points, gen_points, viewdirs):
        """rgb-sigma of the NOVEL PixelNeRF (reference novel_pixelnerf.py:143-242) at given points, in one kernel launch:
        ``in_points`` / ``gen_points`` / ``viewdirs`` [SB,P,3] -> [SB,P,4].  Any fusion MLP of the shape-general envelope, the standard
        one included; every 4-tap lookup mode of the encoder, applied to both latents.  Exact fp32, or f16x3 under ``precision ==
        "f16x3"`` with ``f16x3_any_shape``.  Raises ``NotImplementedError`` for what this form does not serve (a bicubic encoder)."""
        missing = [k for k in self._GEN_STATE if getattr(model, k, None) is None]
        if missing:
            raise TypeError(f"render_points_novel: the model has no {', '.join(missing)} (not the NOVEL PixelNeRF, or encode_gen() was not called)")
        if getattr(model.encoder, "index_interp", "bilinear") == "bicubic":
            raise NotImplementedError("render_points_novel: index_interp='bicubic' is not served by the novel point kernels "
                                      "(bilinear or nearest, any padding); composite() evaluates such a model with PyTorch")
        shape = self._validate(model)
        xi, xg, vd = _f32c(in_points), _f32c(gen_points), _f32c(viewdirs)
        if not xi.is_cuda:
            raise RuntimeError("diner_amd.novel.NeRFRendererDGS runs on the GPU only (points are on %s)" % xi.device)
        assert xi.dim() == 3 and xi.shape[-1] == 3 and xg.shape == xi.shape and vd.shape == xi.shape
        SB, P, _ = xi.shape
        dev = xi.device
        f16 = self.precision == "f16x3" and bool(self.f16x3_any_shape)
        if f16:
            self.effective_precision = "f16x3"
        else:
            if self.precision != "fp32" and not self._warned_precision:
                warnings.warn(f"diner_amd.novel.NeRFRendererDGS: precision={self.precision!r} reaches the NOVEL point model only with "
                              "f16x3_any_shape set; it runs in exact fp32 (renderer.effective_precision)", stacklevel=3)
                self._warned_precision = True
            self.effective_precision = "fp32"
        packed, _gshape = self._gen_packs(model, shape, f16)
        sc, _keep = self._scene(model, need_latent=True)
        assert SB == sc.SB                                                      # novel_pixelnerf.py:156
        g, _gkeep = self._novel_gen(model, dev)
        ix = self._latent_index(model)
        cs = shape.c_struct()
        out = torch.empty((SB, P, 4), dtype=torch.float32, device=dev)
        check(_lib.lib().diner_render_points_novel(C.byref(sc), C.byref(ix) if ix is not None else None, C.byref(g), C.byref(cs), _ptr(packed),
                                                   _ptr(xi), _ptr(xg), _ptr(vd), P, _lib.PRECISIONS["f16x3" if f16 else "fp32"], _ptr(out),
                                                   _stream(dev)), "diner_render_points_novel")
        self.last_route, self.last_binding = ("novel_points_gen_f16" if f16 else "novel_points_gen"), "ctypes"
        return out

    # ------------------------------------------------------------------------------------------------------------------------------
    # the NOVEL_PE point model on the HIP kernels
    # ------------------------------------------------------------------------------------------------------------------------------
    _PE_STATE = _GEN_STATE + ("deformation_layer", "pos_encodings", "tgt_pos_encoding", "tgt_poses", "tgt_focal", "tgt_c", "tgt_image_shape")

    def _validate_pe(self, model):
        """the shape of the NOVEL_PE model's fusion MLP as the kernels see it: d_latent = C + 6 padded to C + 8, which must lie in the
        shape-general envelope (``_validate`` keeps refusing C + 6 for every other route)"""
        dl = getattr(model, "deformation_layer", None)
        Cc = int(getattr(dl, "out_features", -1))
        if dl is None or int(dl.in_features) != Cc + 6 or int(model.mlp_fine.d_latent) != Cc + 6:
            raise NotImplementedError("not the NOVEL_PE PixelNeRF: deformation_layer must be Linear(C + 6 -> C) and the fusion MLP's "
                                      "d_latent C + 6 (pe_novel_pixelnerf.py:21-28)")
        if Cc < 8 or Cc % 8:
            raise NotImplementedError(f"encoder latent_size C={Cc} unsupported by the NOVEL_PE point kernels (a multiple of 8 in [8, 1016])")
        shim = SimpleNamespace(encoder=model.encoder, mlp_fine=_PaddedMlp(model.mlp_fine, None), poscode=model.poscode,
                               depthcode=model.depthcode)
        return self._validate(shim)

    def _pe_mlp_pack(self, model, shape, f16):
        """the packed image of the fusion MLP with every lin_z[b].weight [d_hidden, C + 6] padded with two zero columns: on copies, cached
        under the weights they were made from; the packer's own cache then sees stable tensors"""
        mlp = model.mlp_fine
        nlz = min(shape.combine_layer, shape.n_blocks)
        src = [mlp.lin_z[b].weight for b in range(nlz)]
        if self._pe_linz_key is None or not self._pe_linz_key.valid_for(src):
            pads = [torch.nn.functional.pad(_f32c(w.detach()), (0, 2)).contiguous() for w in src]
            self._pe_linz_pad = [SimpleNamespace(weight=p, bias=mlp.lin_z[b].bias) for b, p in enumerate(pads)]
            self._pe_linz_key = _Sources(src)
        shim = SimpleNamespace(mlp_fine=_PaddedMlp(mlp, self._pe_linz_pad))
        return self._mlp_shape_general(shim, shape, f16)

    @staticmethod
    def _cams(poses, focal, c, image_shape, dev):
        """one camera per scene, [SB,1,..] (encode_gen / encode_tgt) or [SB,..]; 3 x 4 poses accepted -> fp32, contiguous, (W, H)"""
        poses = _f32c(poses).to(dev)
        poses = poses.reshape(-1, *poses.shape[-2:])
        if poses.shape[-2:] != (4, 4):
            full = torch.zeros((poses.shape[0], 4, 4), dtype=torch.float32, device=dev)
            full[:, :3, :] = poses[:, :3, :]
            full[:, 3, 3] = 1
            poses = full
        ishape = [float(v) for v in image_shape.detach().float().cpu()]
        return poses.contiguous(), _f32c(focal).to(dev).reshape(-1, 2).contiguous(), _f32c(c).to(dev).reshape(-1, 2).contiguous(), ishape

    def _novel_pe(self, model, sc, latent, dev, need_maps):
        """``model``'s deformation map, head table, pos-encoding maps and target cameras as a DinerNovelPe (+ the tensors it points into),
        each cached under the tensors it was made from: an in-place update of one rebuilds its pack.  ``latent``: the NHWC pack ``sc``
        points to.  ``need_maps`` False (combine_layer 0): nothing but the cameras is read or built."""
        L, st = _lib.lib(), _stream(dev)
        dl, enc = model.deformation_layer, model.encoder
        pe = _lib.DinerNovelPe()
        keep = []
        if need_maps:
            Cc = int(dl.out_features)
            msrc = [enc.latent, dl.weight]
            if self._pe_map_key is None or not self._pe_map_key.valid_for(msrc):
                wl = _f32c(dl.weight.detach()[:, :Cc]).to(dev).contiguous()
                n = int(L.diner_novel_pe_map_floats(C.byref(sc)))
                if n < 0:
                    check(n, "diner_novel_pe_map_floats")
                assert n == latent.numel()
                dmap = torch.empty(tuple(latent.shape), dtype=torch.float32, device=dev)
                check(L.diner_pack_novel_pe_map(C.byref(sc), _ptr(wl), _ptr(dmap), st), "diner_pack_novel_pe_map")
                torch.cuda.current_stream(dev).synchronize()     # `wl` is a temporary
                self._pe_map_pack, self._pe_map_key = dmap, _Sources(msrc)
            hsrc = [dl.weight, dl.bias]
            if self._pe_head_key is None or not self._pe_head_key.valid_for(hsrc):
                w, b = _f32c(dl.weight.detach()).to(dev), _f32c(dl.bias.detach()).to(dev)
                self._pe_head_pack = torch.cat((w[:, Cc:Cc + 6], b[:, None], torch.zeros_like(b[:, None])), dim=1).contiguous()
                self._pe_head_key = _Sources(hsrc)
            psrc = [model.pos_encodings, model.tgt_pos_encoding]
            if self._pe_pos_key is None or not self._pe_pos_key.valid_for(psrc):
                s = _f32c(model.pos_encodings).to(dev)                          # [SB,NV,3,H,W]
                t = _f32c(model.tgt_pos_encoding).to(dev)                       # [SB,1,3,H,W] (encode_tgt) or [SB,3,H,W]
                t = t.reshape(-1, *t.shape[-3:])
                if s.dim() != 5 or s.shape[2] != 3 or t.shape[1] != 3:
                    raise ValueError(f"pos_encodings must be [SB,NV,3,H,W] and tgt_pos_encoding [SB,(1,)3,H,W], not {tuple(s.shape)} / {tuple(t.shape)}")
                nhwc4 = lambda m: torch.nn.functional.pad(m.movedim(-3, -1), (0, 1)).contiguous()   # a zero 4th channel: 16-byte texels
                self._pe_pos_pack, self._pe_pos_key = (nhwc4(s), nhwc4(t)), _Sources(psrc)
            spe, tpe = self._pe_pos_pack
            assert spe.shape[:2] == (sc.SB, sc.NV) and tpe.shape[0] == sc.SB
            pe.map, pe.head, pe.src_pe, pe.tgt_pe = (t.data_ptr() for t in (self._pe_map_pack, self._pe_head_pack, spe, tpe))
            (pe.src_h, pe.src_w), (pe.tgt_h, pe.tgt_w) = spe.shape[2:4], tpe.shape[1:3]
            keep += [self._pe_map_pack, self._pe_head_pack, spe, tpe]
        else:
            pe.src_h = pe.src_w = pe.tgt_h = pe.tgt_w = 1
        cams = [model.tgt_poses, model.tgt_focal, model.tgt_c, model.tgt_image_shape]
        if self._pe_cam_key is None or not self._pe_cam_key.valid_for(cams):
            self._pe_cam_pack, self._pe_cam_key = self._cams(*cams, dev), _Sources(cams)
        poses, focal, c, ishape = self._pe_cam_pack
        pe.poses, pe.focal, pe.c = poses.data_ptr(), focal.data_ptr(), c.data_ptr()
        pe.image_w, pe.image_h = ishape
        return pe, keep + [poses, focal, c]

    @torch.no_grad()
    def render_points_novel_pe(self, model, in_points, gen_points, tgt_points, viewdirs):
        """rgb-sigma of the NOVEL_PE PixelNeRF (reference pe_novel_pixelnerf.py:200-292) at given points, in one kernel launch:
        ``in_points`` / ``gen_points`` / ``tgt_points`` / ``viewdirs`` [SB,P,3] -> [SB,P,4].  The deformation layer's latent part is
        applied to the encoder's latent once per encode (the deformation map, cached like the latent's pack).  Any fusion MLP whose
        d_latent = C + 6, padded to C + 8, lies in the shape-general envelope (C <= 1016); every 4-tap lookup mode, applied to all
        four lookups.  Exact fp32, or f16x3 under ``precision == "f16x3"`` with ``f16x3_any_shape``.  Raises ``NotImplementedError``
        for what this form does not serve (a bicubic encoder, C = 1024)."""
        missing = [k for k in self._PE_STATE if getattr(model, k, None) is None]
        if missing:
            raise TypeError(f"render_points_novel_pe: the model has no {', '.join(missing)} (not the NOVEL_PE PixelNeRF, or encode() / "
                            "encode_gen() / encode_tgt() was not called)")
        if getattr(model.encoder, "index_interp", "bilinear") == "bicubic":
            raise NotImplementedError("render_points_novel_pe: index_interp='bicubic' is not served by the novel_pe point kernels "
                                      "(bilinear or nearest, any padding); composite() evaluates such a model with PyTorch")
        shape = self._validate_pe(model)
        xi, xg, xt, vd = _f32c(in_points), _f32c(gen_points), _f32c(tgt_points), _f32c(viewdirs)
        if not xi.is_cuda:
            raise RuntimeError("diner_amd.novel.NeRFRendererDGS runs on the GPU only (points are on %s)" % xi.device)
        assert xi.dim() == 3 and xi.shape[-1] == 3 and xg.shape == xi.shape and xt.shape == xi.shape and vd.shape == xi.shape
        SB, P, _ = xi.shape
        dev = xi.device
        f16 = self.precision == "f16x3" and bool(self.f16x3_any_shape)
        if f16:
            self.effective_precision = "f16x3"
        else:
            if self.precision != "fp32" and not self._warned_precision:
                warnings.warn(f"diner_amd.novel.NeRFRendererDGS: precision={self.precision!r} reaches the NOVEL_PE point model only with "
                              "f16x3_any_shape set; it runs in exact fp32 (renderer.effective_precision)", stacklevel=3)
                self._warned_precision = True
            self.effective_precision = "fp32"
        packed = self._pe_mlp_pack(model, shape, f16)
        sc, keep = self._scene(model, need_latent=True)
        assert SB == sc.SB                                                      # pe_novel_pixelnerf.py:213
        if sc.C != shape.d_latent - 8:
            raise ValueError(f"encoder latent has {sc.C} channels, deformation_layer.out_features is {shape.d_latent - 8}")
        g, _gkeep = self._novel_gen(model, dev)
        pe, _pkeep = self._novel_pe(model, sc, keep[4], dev, need_maps=min(shape.combine_layer, shape.n_blocks) > 0)
        ix = self._latent_index(model)
        cs = shape.c_struct()
        out = torch.empty((SB, P, 4), dtype=torch.float32, device=dev)
        check(_lib.lib().diner_render_points_novel_pe(C.byref(sc), C.byref(ix) if ix is not None else None, C.byref(g), C.byref(pe),
                                                      C.byref(cs), _ptr(packed), _ptr(xi), _ptr(xg), _ptr(xt), _ptr(vd), P,
                                                      _lib.PRECISIONS["f16x3" if f16 else "fp32"], _ptr(out), _stream(dev)),
              "diner_render_points_novel_pe")
        self.last_route, self.last_binding = ("novel_pe_points_gen_f16" if f16 else "novel_pe_points_gen"), "ctypes"
        return out

    def _hip_pe_model_ok(self, model) -> bool:
        """composite() may hand ``model`` to render_points_novel_pe: see ``hip_point_model`` in the constructor"""
        if not self.hip_point_model or not self.pass_points:
            return False
        if any(getattr(model, k, None) is None for k in self._PE_STATE + ("mlp_fine", "poscode", "depthcode", "encoder")):
            return False
        dl, enc = model.deformation_layer, model.encoder
        if not hasattr(dl, "in_features") or int(dl.in_features) != int(dl.out_features) + 6 or getattr(dl, "bias", None) is None:
            return False
        if getattr(enc, "latent", None) is None or getattr(enc, "index_interp", "bilinear") == "bicubic":
            return False
        if torch.is_grad_enabled():
            params = list(model.parameters()) if isinstance(model, torch.nn.Module) else \
                list(model.mlp_fine.parameters()) + list(dl.parameters())
            if any(p.requires_grad for p in params + [model.gen_latent, enc.latent]):
                return False
        try:
            self._validate_pe(model)
        except (NotImplementedError, AttributeError):
            return False
        return True

    def _novel_model_ok(self, model) -> bool:
        """``model`` is recognisably the NOVEL PixelNeRF with a fusion MLP and a lookup the novel kernels serve (everything
        ``hip_point_model`` asks for but the gradient state)"""
        if not self.hip_point_model or self.pass_points:
            return False
        if any(getattr(model, k, None) is None for k in self._GEN_STATE + ("mlp_fine", "poscode", "depthcode", "encoder")):
            return False
        if getattr(model, "deformation_layer", None) is not None:              # NOVEL_PE
            return False
        enc = model.encoder
        if getattr(enc, "latent", None) is None or getattr(enc, "index_interp", "bilinear") == "bicubic":
            return False
        try:
            self._validate(model)
        except (NotImplementedError, AttributeError):
            return False
        return True

    @staticmethod
    def _any_requires_grad(model) -> bool:
        if not torch.is_grad_enabled():
            return False
        params = list(model.parameters()) if isinstance(model, torch.nn.Module) else list(model.mlp_fine.parameters())
        return any(p.requires_grad for p in params + [model.gen_latent, model.encoder.latent])

    def _hip_point_model_ok(self, model) -> bool:
        """composite() may hand ``model`` to render_points_novel: see ``hip_point_model`` in the constructor"""
        return self._novel_model_ok(model) and not self._any_requires_grad(model)

    def _hip_point_model_trains(self, model) -> bool:
        """composite() may hand ``model`` to training_novel.render_points_with_grad: see ``train_hip_point_model`` in the constructor"""
        if not self.train_hip_point_model or not torch.is_grad_enabled() or not self._novel_model_ok(model):
            return False
        from .training_gen import mlp_params
        return any(p.requires_grad for p in mlp_params(model.mlp_fine) + [model.encoder.latent, model.gen_latent])

    def _train_points_novel(self, model, in_points, gen_points, viewdirs):
        """rgb-sigma [SB,P,4] of the NOVEL PixelNeRF under autograd (diner_amd/training_novel.py)"""
        from . import training_novel
        shape = self._validate(model)
        f16 = self.precision == "f16x3" and bool(self.train_f16x3_any_shape)
        if f16:
            self.effective_precision = "f16x3"
        else:
            if self.precision != "fp32" and not self._warned_precision:
                warnings.warn(f"diner_amd.novel.NeRFRendererDGS: precision={self.precision!r} reaches the NOVEL point model's training "
                              "path only with train_f16x3_any_shape set; it runs in exact fp32 (renderer.effective_precision)", stacklevel=4)
                self._warned_precision = True
            self.effective_precision = "fp32"
        out = training_novel.render_points_with_grad(self, model, in_points, gen_points, viewdirs, shape, f16=f16)
        self.last_route, self.last_binding = ("novel_train_gen_f16" if f16 else "novel_train_gen"), "ctypes"
        return out

    def composite(self, model, rays, z_samp, target_vertices, tgt_in_offsets, tgt_gen_offsets, *, _sync=False):
        """Alpha compositing of the model's rgb-sigma on the deformed sample points (reference :394-477) -> (weights, rgb, depth).
        Differentiable to what the model's output depends on (its parameters); rays, depths, vertices or offsets that require grad raise."""
        self._no_data_grad(rays=rays, z_samp=z_samp, target_vertices=target_vertices, tgt_in_offsets=tgt_in_offsets,
                           tgt_gen_offsets=tgt_gen_offsets)
        r = self._check_rays(rays)
        z = _f32c(z_samp.detach())
        SB, B, K = z.shape
        with torch.no_grad():
            sets = deform.deform_ray_points(r, z, target_vertices, tgt_in_offsets, tgt_gen_offsets, return_points=self.pass_points)
            dirs = r[..., None, 3:6].expand(-1, -1, K, -1).reshape(SB, B * K, 3)       # :413, :432
        if self._hip_point_model_ok(model):
            out = self.render_points_novel(model, sets[0], sets[1], dirs).reshape(SB, B, K, 4)
        elif self._hip_point_model_trains(model):
            out = self._train_points_novel(model, sets[0], sets[1], dirs).reshape(SB, B, K, 4)
        elif self._hip_pe_model_ok(model):
            out = self.render_points_novel_pe(model, sets[0], sets[1], sets[2], dirs).reshape(SB, B, K, 4)
        else:
            chunk = (int(self.eval_batch_size) - 1) // SB + 1                           # :433
            split = [torch.split(t, chunk, dim=1) for t in sets]
            vals = [model(*pts, viewdirs=d) for *pts, d in zip(*split, torch.split(dirs, chunk, dim=1))]   # :440-444
            out = torch.cat(vals, dim=1).reshape(SB, B, K, -1)                          # :450-451
            self.last_route = "torch"
        dev = r.device
        self._poll_status()
        weights, rgb, depth = _CompositeFn.apply(out, r, z, bool(self.white_bkgd), self._status_word(dev))
        self._after_launch(dev, sync=_sync)
        return weights, rgb, depth

    def forward(self, model, rays, target_vertices, tgt_in_offsets, tgt_gen_offsets, want_weights=False, *, noise=None):
        """Reference :511-540: sample_depthguided -> fill_up_uniform_samples -> composite; ``out.fine.rgb`` [SB,B,3],
        ``out.fine.depth`` [SB,B], ``out.fine.weights`` [SB,B,K] iff ``want_weights``.  (The sampler kernel fills and sorts in the
        same launch, under the call's seed: that result is what the compositing gets.)"""
        assert len(rays.shape) == 3
        self._no_data_grad(rays=rays, target_vertices=target_vertices, tgt_in_offsets=tgt_in_offsets, tgt_gen_offsets=tgt_gen_offsets)
        with torch.no_grad():
            internals = self._sample_deformed(rays, model, int(self.n_samples), int(self.n_depth_candidates), self.n_gaussian,
                                              target_vertices, tgt_in_offsets, 0.05, noise, want_lik=False)
        big = want_weights or rays.shape[0] * rays.shape[1] > int(self.finite_sync_rays)
        weights, rgb, depth = self.composite(model, rays, internals["z"], target_vertices, tgt_in_offsets, tgt_gen_offsets, _sync=big)
        return RenderOutput(fine=self._format_outputs(weights, rgb, depth, want_weights=want_weights))

    render_rays = forward
