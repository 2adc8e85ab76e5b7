"""HIP versions of the two per-image producers next to the render path,
with the reference's own function signatures so they can replace them in place:

* :func:`gen_rays`      -- reference ``src/util/cam_geometry.py:36-79`` (differentiable in the cameras, near and far, like the
  reference's plain-torch version: the backward is ``diner_gen_rays_backward``)
* :func:`depth2normal`  -- reference ``src/util/depth2normal.py:7-87``

and the tail of the encoder: :func:`assemble_latent` -- reference ``src/models/image_encoder.py:262-272`` (the feature levels upsampled to
the first one's size and concatenated), written once in the NHWC layout the render and training kernels read
(:func:`assemble_latent_bicubic` for ``upsample_interp="bicubic"``);
its head: :func:`encoder_input` -- reference ``src/models/pixelnerf.py:44`` + ``src/models/image_encoder.py:222-232`` (conv1's input: the
images normalised and replicate-padded, plus the positional encoding of the padding);
and both around the model's own CNN trunk: :func:`encode`, with ``PixelNeRF.encode``'s signature (reference
``src/models/pixelnerf.py:35-53`` + ``SpatialEncoder.forward``, ``src/models/image_encoder.py:206-272``);
and a training step around the renderer: :func:`gen_rays_at` (gen_rays at the selected pixels only), :func:`photo_loss` (ground-truth
gather, MSE and antibias loss) and :func:`calc_losses`, which assembles ``DINER.calc_losses`` (reference ``src/models/diner.py:217-290``);
and the way from a rendered frame to its files and scores: :func:`torch_cmap` (reference ``src/util/torch_helpers.py:43-76``),
:func:`frames_u8` (the quantisation of ``save_image`` and ``save_torch_video``, ``src/models/diner.py:129-133, :209-214``) and
:func:`image_scores` (l1, l2, psnr, ssim of ``evaluate_folder``, ``src/evaluation/eval_suite.py:63-68``);
and rendering inside a scene bounding box: :func:`ray_box` (``FacescapeDataSet.get_near_far`` + ``get_mask_at_box``,
``src/data/facescape.py:128-185``, on the project's rays), :func:`box_rays` (the hit pixels' rays, compacted) and :func:`frame_from_hits`;
and the deformation of the fork's NOVEL renderers (``src/models/novel/nerf_novel_renderer.py:40-50``): :func:`nearest_vertex`,
:func:`deform_points` and :func:`deform_ray_points`, which live in :mod:`diner_amd.deform`.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check


def _f(t):
    return t.detach().to(torch.float32).contiguous()


def _st(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _per_camera(v, B, dev):
    """z_near / z_far as B contiguous fp32 values: a tensor of B elements, or one value (a scalar, a 1-element tensor) for all"""
    t = _f(torch.as_tensor(v, device=dev)).reshape(-1)
    if t.numel() == 1 and B != 1:
        t = t.expand(B).contiguous()
    if t.numel() != B:
        raise ValueError(f"gen_rays: z_near / z_far must hold 1 or B={B} values, not {t.numel()}")
    return t


def _gen_rays(e, k, zn, zf, W, H):
    B = e.shape[0]
    out = torch.empty((B, int(H), int(W), 8), dtype=torch.float32, device=e.device)
    check(_lib.lib().diner_gen_rays(e.data_ptr(), k.data_ptr(), zn.data_ptr(), zf.data_ptr(), B, int(H), int(W),
                                    out.data_ptr(), _st(e.device)), "diner_gen_rays")
    return out


def gen_rays_backward(e, k, d_rays, H, W):
    """Backward of :func:`gen_rays` on fp32 contiguous cameras e [B,4,4], k [B,3,3] and d_rays [B,H*W,8] (or [B,H,W,8]):
    -> d_extrinsics [B,4,4], d_intrinsics [B,3,3], d_near [B], d_far [B] in fp32 (diner_gen_rays_backward: fixed-order sums,
    bitwise reproducible)."""
    B, dev = e.shape[0], e.device
    g = _f(d_rays)
    assert g.numel() == B * int(H) * int(W) * 8, "gen_rays_backward: d_rays must be [B, H, W, 8]"
    L = _lib.lib()
    n = int(L.diner_gen_rays_backward_workspace_floats(B, int(H), int(W)))
    if n < 0:
        raise ValueError(f"gen_rays_backward: bad sizes B={B}, H={H}, W={W}")
    ws = torch.empty(max(n, 2), dtype=torch.float32, device=dev)
    d_e = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    d_k = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    d_n = torch.empty(B, dtype=torch.float32, device=dev)
    d_f = torch.empty(B, dtype=torch.float32, device=dev)
    check(L.diner_gen_rays_backward(e.data_ptr(), k.data_ptr(), g.data_ptr(), B, int(H), int(W), d_e.data_ptr(), d_k.data_ptr(),
                                    d_n.data_ptr(), d_f.data_ptr(), ws.data_ptr(), _st(dev)), "diner_gen_rays_backward")
    return d_e, d_k, d_n, d_f


def _like(g, t):
    """a gradient computed for B per-camera values, in the shape / dtype / device of the input ``t`` it belongs to"""
    if not isinstance(t, torch.Tensor):
        return None
    if t.numel() == 1 and g.numel() != 1:
        g = g.sum()
    return g.reshape(t.shape).to(dtype=t.dtype, device=t.device)


class _GenRaysFn(torch.autograd.Function):
    """gen_rays with a backward: forward = diner_gen_rays (the no-grad call's values, bit for bit), backward = diner_gen_rays_backward"""

    @staticmethod
    def forward(ctx, extrinsics, intrinsics, z_near, z_far, W, H):
        e, k = _f(extrinsics), _f(intrinsics)
        B = e.shape[0]
        out = _gen_rays(e, k, _per_camera(z_near, B, e.device), _per_camera(z_far, B, e.device), W, H)
        ctx.save_for_backward(extrinsics, intrinsics)    # (version-checked by autograd: an in-place edit before backward raises)
        ctx.e, ctx.k, ctx.HW = e, k, (int(H), int(W))
        ctx.zs = (z_near, z_far)
        return out

    @staticmethod
    def backward(ctx, d_rays):
        extrinsics, intrinsics = ctx.saved_tensors
        H, W = ctx.HW
        d_e, d_k, d_n, d_f = gen_rays_backward(ctx.e, ctx.k, d_rays, H, W)
        z_near, z_far = ctx.zs
        return (_like(d_e, extrinsics) if ctx.needs_input_grad[0] else None,
                _like(d_k, intrinsics) if ctx.needs_input_grad[1] else None,
                _like(d_n, z_near) if ctx.needs_input_grad[2] else None,
                _like(d_f, z_far) if ctx.needs_input_grad[3] else None, None, None)


def gen_rays(extrinsics, intrinsics, W, H, z_near, z_far):
    """extrinsics [B,4,4], intrinsics [B,3,3], z_near/z_far [B] (or one value for all) -> rays [B,H,W,8]
    (origin, unit direction, near, far; pixel centres, OpenCV convention).  Differentiable with respect to every tensor input, as the
    reference's gen_rays is: the gradient reaches extrinsics rows 0..2, the intrinsics entries fx, fy, cx, cy (the others get exactly 0),
    near and far; the forward values are those of the no-grad call, bit for bit."""
    if not extrinsics.is_cuda:
        raise RuntimeError("diner_amd.glue.gen_rays runs on the GPU only")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                       for t in (extrinsics, intrinsics, z_near, z_far)):
        return _GenRaysFn.apply(extrinsics, intrinsics, z_near, z_far, W, H)
    with torch.no_grad():
        e, k = _f(extrinsics), _f(intrinsics)
        B = e.shape[0]
        return _gen_rays(e, k, _per_camera(z_near, B, e.device), _per_camera(z_far, B, e.device), W, H)


@torch.no_grad()
def depth2normal(dmap, K):
    """dmap [N,1,H,W], K [N,3,3] -> normals [N,3,H,W]."""
    d, k = _f(dmap), _f(K)
    if not d.is_cuda:
        raise RuntimeError("diner_amd.glue.depth2normal runs on the GPU only")
    N, _, H, W = d.shape
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=d.device)
    check(_lib.lib().diner_depth2normal(d.data_ptr(), k.data_ptr(), N, H, W, out.data_ptr(), _st(d.device)),
          "diner_depth2normal")
    return out


@torch.no_grad()
def pack_maps_from_depth(depths, depths_std, intrinsics):
    """depth2normal fused into the renderer's map packing: depths, depths_std [SB,NV,1,H,W], intrinsics
    [SB,NV,3,3] -> packed maps [SB,NV,H,W,8] (nx ny nz depth | sigma 0 0 0), the layout ``DinerScene.maps`` takes."""
    d, s, k = _f(depths), _f(depths_std), _f(intrinsics)
    SB, NV, _, H, W = d.shape
    out = torch.empty((SB, NV, H, W, 8), dtype=torch.float32, device=d.device)
    check(_lib.lib().diner_pack_maps_from_depth(d.data_ptr(), s.data_ptr(), k.data_ptr(), SB * NV, H, W, out.data_ptr(),
                                                _st(d.device)), "diner_pack_maps_from_depth")
    return out


def _levels_struct(ts):
    lv = _lib.DinerLatentLevels()
    for i, t in enumerate(ts):
        lv.level[i].data, lv.level[i].C, lv.level[i].h, lv.level[i].w = t.data_ptr(), t.shape[1], t.shape[2], t.shape[3]
    return lv


def _assemble_check(levels, SB, NV, who):
    levels = list(levels)
    if not 1 <= len(levels) <= _lib.LATENT_MAX_LEVELS:
        raise ValueError(f"{who}: {len(levels)} levels, expected 1..{_lib.LATENT_MAX_LEVELS}")
    N = int(SB) * int(NV)
    for t in levels:
        if not t.is_cuda:
            raise RuntimeError(f"diner_amd.glue.{who} runs on the GPU only")
        if t.dim() != 4 or t.shape[0] != N:
            raise ValueError(f"{who}: a level must be [SB*NV = {N}, C_l, h_l, w_l], not {tuple(t.shape)}")
    return levels


def _assemble(lv, SB, NV, fn="diner_assemble_latent"):
    """fp32 contiguous levels [SB*NV, C_l, h_l, w_l] -> the NHWC buffer [SB, NV, h, w, C]"""
    h, w = lv[0].shape[2:]
    out = torch.empty((SB, NV, h, w, sum(t.shape[1] for t in lv)), dtype=torch.float32, device=lv[0].device)
    check(getattr(_lib.lib(), fn)(C.byref(_levels_struct(lv)), len(lv), SB * NV, h, w, out.data_ptr(), _st(out.device)), fn)
    return out


def _assemble_backward(d_latent, level_shapes, fn):
    SB, NV, _, h, w = d_latent.shape
    g = d_latent.detach().permute(0, 1, 3, 4, 2)
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.to(torch.float32).contiguous()
    grads = [torch.empty(tuple(s), dtype=torch.float32, device=g.device) for s in level_shapes]
    check(getattr(_lib.lib(), fn)(g.data_ptr(), len(grads), SB * NV, h, w, C.byref(_levels_struct(grads)), _st(g.device)), fn)
    return grads


def assemble_latent_backward(d_latent, level_shapes):
    """Adjoint of :func:`assemble_latent`: d_latent of logical shape [SB, NV, C, h, w] (made NHWC-strided fp32 once if it is not) ->
    the levels' gradients [SB*NV, C_l, h_l, w_l] in fp32 (``diner_assemble_latent_backward``: gather form, bitwise reproducible)."""
    return _assemble_backward(d_latent, level_shapes, "diner_assemble_latent_backward")


def assemble_latent_bicubic_backward(d_latent, level_shapes):
    """Adjoint of :func:`assemble_latent_bicubic`, with :func:`assemble_latent_backward`'s contract
    (``diner_assemble_latent_bicubic_backward``: gather form, bitwise reproducible)."""
    return _assemble_backward(d_latent, level_shapes, "diner_assemble_latent_bicubic_backward")


class _AssembleLatentFn(torch.autograd.Function):
    """assemble_latent with a backward: forward = diner_assemble_latent (the no-grad call's values), backward = its adjoint kernel"""

    @staticmethod
    def forward(ctx, SB, NV, *levels):
        lv = [_f(t) for t in levels]
        ctx.shapes, ctx.dtypes = [tuple(t.shape) for t in lv], [t.dtype for t in levels]
        return _assemble(lv, SB, NV).permute(0, 1, 4, 2, 3)

    @staticmethod
    def backward(ctx, d_latent):
        grads = assemble_latent_backward(d_latent, ctx.shapes)
        return (None, None, *[g.to(dt) if need else None for g, dt, need in zip(grads, ctx.dtypes, ctx.needs_input_grad[2:])])


def assemble_latent(levels, SB, NV, mode="bilinear"):
    """The tail of ``SpatialEncoder.forward`` (reference src/models/image_encoder.py:262-272) in one kernel: ``levels`` = the feature
    pyramid, a list of 1..5 tensors [SB*NV, C_l, h_l, w_l]; every level is upsampled to ``levels[0]``'s (h, w) like
    ``F.interpolate(mode="bilinear", align_corners=True)`` and the results are concatenated along the channels.
    Returns the latent in its logical shape [SB, NV, C, h, w] with NHWC storage: ``buf.permute(0, 1, 4, 2, 3)`` of a contiguous
    [SB, NV, h, w, C] buffer, the layout the render and training kernels read -- :func:`latent_is_packed` is true for it and the renderer
    then takes the buffer as it is (no copy, no re-pack).  ``.shape``, ``grid_sample`` and indexing see an ordinary tensor.
    Differentiable with respect to every level (``diner_assemble_latent_backward``, deterministic)."""
    if mode == "bicubic":
        raise NotImplementedError("assemble_latent: upsample mode 'bicubic' is not implemented by this function (it is bilinear, "
                                  "align_corners=True): call assemble_latent_bicubic")
    if mode != "bilinear":   # (the reference's nearest branch is unreachable: it compares with "nearest ", image_encoder.py:262)
        raise NotImplementedError(f"assemble_latent: upsample mode {mode!r} is not implemented (the encoder's tail is bilinear, "
                                  "align_corners=True)")
    levels = _assemble_check(levels, SB, NV, "assemble_latent")
    SB, NV = int(SB), int(NV)
    if torch.is_grad_enabled() and any(t.requires_grad for t in levels):
        return _AssembleLatentFn.apply(SB, NV, *levels)
    with torch.no_grad():
        return _assemble([_f(t) for t in levels], SB, NV).permute(0, 1, 4, 2, 3)


class _AssembleLatentBicubicFn(torch.autograd.Function):
    """assemble_latent_bicubic with a backward: forward = diner_assemble_latent_bicubic (the no-grad call's values), backward = its
    adjoint kernel"""

    @staticmethod
    def forward(ctx, SB, NV, *levels):
        lv = [_f(t) for t in levels]
        ctx.shapes, ctx.dtypes = [tuple(t.shape) for t in lv], [t.dtype for t in levels]
        return _assemble(lv, SB, NV, "diner_assemble_latent_bicubic").permute(0, 1, 4, 2, 3)

    @staticmethod
    def backward(ctx, d_latent):
        grads = assemble_latent_bicubic_backward(d_latent, ctx.shapes)
        return (None, None, *[g.to(dt) if need else None for g, dt, need in zip(grads, ctx.dtypes, ctx.needs_input_grad[2:])])


def assemble_latent_bicubic(levels, SB, NV):
    """:func:`assemble_latent` for ``SpatialEncoder(upsample_interp="bicubic")``: every level is upsampled to ``levels[0]``'s (h, w) like
    ``F.interpolate(mode="bicubic", align_corners=True)`` (ATen's upsample_bicubic2d: 16 taps, A = -0.75, clamped at the borders) and the
    results are concatenated along the channels.  The same contract: the logical shape [SB, NV, C, h, w] over a contiguous
    [SB, NV, h, w, C] buffer (:func:`latent_is_packed` is true for it), a level of the output's size bit-identical, differentiable with
    respect to every level (``diner_assemble_latent_bicubic_backward``, deterministic)."""
    levels = _assemble_check(levels, SB, NV, "assemble_latent_bicubic")
    SB, NV = int(SB), int(NV)
    if torch.is_grad_enabled() and any(t.requires_grad for t in levels):
        return _AssembleLatentBicubicFn.apply(SB, NV, *levels)
    with torch.no_grad():
        return _assemble([_f(t) for t in levels], SB, NV, "diner_assemble_latent_bicubic").permute(0, 1, 4, 2, 3)


def nhwc_strided(t) -> bool:
    """a 5-d fp32 tensor of logical shape [SB, NV, C, h, w] whose storage is a contiguous [SB, NV, h, w, C] buffer"""
    return isinstance(t, torch.Tensor) and t.dim() == 5 and t.dtype == torch.float32 and t.permute(0, 1, 3, 4, 2).is_contiguous()


def latent_is_packed(t) -> bool:
    """True when ``t`` [SB, NV, C, h, w] already has the layout the kernels read (what :func:`assemble_latent` returns):
    ``t.permute(0, 1, 3, 4, 2)`` is a contiguous fp32 CUDA tensor."""
    return nhwc_strided(t) and t.is_cuda


# ---- the head of the encoder: conv1's input -----------------------------------------------------------------------------------------
IMAGENET_MEAN = (0.485, 0.456, 0.406)    # PixelNeRF.normalize_rgb (reference src/models/pixelnerf.py:32-33)
IMAGENET_STD = (0.229, 0.224, 0.225)

_pixel_coords = {}    # (Hp, Wp, device) -> (xs [Wp], ys [Hp]): they depend on nothing but the sizes
_PIXEL_COORDS_MAX = 8  # sizes kept (oldest dropped first): a training run has one or two, and an entry is two short vectors


def _coords(Hp, Wp, dev):
    """The pixel coordinates of a padded size, made once.  They are written on the stream that is current at the first call and read by
    launches on whatever stream is current later; torch's caching allocator does not reuse their memory while the cache holds them, and
    the first launch that reads them is queued on their own stream, behind the fill: a later launch on another stream is ordered after it
    only if the caller has ordered its streams, as for any tensor shared between streams."""
    key = (Hp, Wp, str(dev))
    if key not in _pixel_coords:
        while len(_pixel_coords) >= _PIXEL_COORDS_MAX:
            _pixel_coords.pop(next(iter(_pixel_coords)))
        with torch.no_grad():
            _pixel_coords[key] = (torch.linspace(-1, 1, Wp, device=dev), torch.linspace(-1, 1, Hp, device=dev))   # image_encoder.py:228-229
    return _pixel_coords[key]


def _three(v, what):
    v = [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]
    if len(v) != 3:
        raise ValueError(f"encoder_input: {what} must hold 3 values, not {len(v)}")
    return v


def _pe_channels(pad, F):
    return 2 * (1 + 2 * F) if F >= 0 and pad > 0 else 0


def _encoder_input(x, pad, F, mean, std):
    """fp32 contiguous x [N,3,H,W] -> [N, 3 + Cpe, H + 2 pad, W + 2 pad]"""
    N, _, H, W = x.shape
    Cpe = _pe_channels(pad, F)
    Hp, Wp = H + 2 * pad, W + 2 * pad
    if pad < 0 or Hp < 2 or Wp < 2 or N < 1:
        raise ValueError(f"encoder_input: bad sizes N={N}, H={H}, W={W}, image_padding={pad}")
    xs, ys = _coords(Hp, Wp, x.device) if Cpe else (None, None)
    out = torch.empty((N, 3 + Cpe, Hp, Wp), dtype=torch.float32, device=x.device)
    check(_lib.lib().diner_encoder_input(x.data_ptr(), N, H, W, pad, F, xs.data_ptr() if Cpe else None, ys.data_ptr() if Cpe else None,
                                         *mean, *std, out.data_ptr(), _st(x.device)), "diner_encoder_input")
    return out


def encoder_input_backward(d_out, image_padding, padding_pe, std=IMAGENET_STD):
    """Adjoint of :func:`encoder_input` to the images: d_out [N, 3 + Cpe, Hp, Wp] -> d_images [N,3,H,W] in fp32: every image pixel sums
    the gradient of the padded pixels copied from it, divided by std (``diner_encoder_input_backward``: gather form, bitwise
    reproducible); the encoding's channels carry no gradient."""
    pad, F = int(image_padding), max(int(padding_pe), -1)
    g = _f(d_out)
    if not g.is_cuda:
        raise RuntimeError("diner_amd.glue.encoder_input_backward runs on the GPU only")
    N, Ct, Hp, Wp = g.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    if Ct != 3 + _pe_channels(pad, F) or H < 1 or W < 1:
        raise ValueError(f"encoder_input_backward: d_out {tuple(g.shape)} does not belong to image_padding={pad}, padding_pe={F}")
    d_img = torch.empty((N, 3, H, W), dtype=torch.float32, device=g.device)
    check(_lib.lib().diner_encoder_input_backward(g.data_ptr(), N, H, W, pad, F, *_three(std, "std"), d_img.data_ptr(), _st(g.device)),
          "diner_encoder_input_backward")
    return d_img


class _EncoderInputFn(torch.autograd.Function):
    """encoder_input with a backward: forward = diner_encoder_input (the no-grad call's values, bit for bit), backward = its adjoint"""

    @staticmethod
    def forward(ctx, images, pad, F, mean, std):
        ctx.pad, ctx.F, ctx.std, ctx.shape, ctx.dtype = pad, F, std, images.shape, images.dtype
        return _encoder_input(_f(images).reshape(-1, *images.shape[-3:]), pad, F, mean, std)

    @staticmethod
    def backward(ctx, d_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return encoder_input_backward(d_out, ctx.pad, ctx.F, ctx.std).reshape(ctx.shape).to(ctx.dtype), None, None, None, None


def _encoder_input_u8(images, alpha, fmt, pad, F, mean, std):
    """uint8 images [..., H, W, C] (, alpha [..., H, W]) -> [N, 3 + Cpe, H + 2 pad, W + 2 pad]: diner_encoder_input_u8"""
    from . import wire
    px, a, N, H, W, Cc, rule = wire.image_source(images, alpha, fmt, images.device, "encoder_input")
    Cpe = _pe_channels(pad, F)
    Hp, Wp = H + 2 * pad, W + 2 * pad
    if pad < 0 or Hp < 2 or Wp < 2:
        raise ValueError(f"encoder_input: bad sizes N={N}, H={H}, W={W}, image_padding={pad}")
    xs, ys = _coords(Hp, Wp, px.device) if Cpe else (None, None)
    out = torch.empty((N, 3 + Cpe, Hp, Wp), dtype=torch.float32, device=px.device)
    check(_lib.lib().diner_encoder_input_u8(px.data_ptr(), None if a is None else a.data_ptr(), Cc, rule, float(fmt.bg), int(bool(fmt.gamma)),
                                            int(bool(fmt.symmetric_range)), N, H, W, pad, F, xs.data_ptr() if Cpe else None,
                                            ys.data_ptr() if Cpe else None, *mean, *std, out.data_ptr(), _st(px.device)),
          "diner_encoder_input_u8")
    return out


def encoder_input(images, image_padding, padding_pe, mean=IMAGENET_MEAN, std=IMAGENET_STD, *, alpha=None, image_format=None, size=None,
                  antialias=True):
    """conv1's input in one kernel (reference src/models/pixelnerf.py:44 + src/models/image_encoder.py:222-232): ``images``
    [..., 3, H, W] -> [N, 3 + Cpe, H + 2 image_padding, W + 2 image_padding] in fp32, N = the product of the leading dimensions.
    Channels 0..2: ``(images - mean) / std`` replicate-padded by ``image_padding``, bit-equal to ``Normalize`` + ``ReplicationPad2d``;
    with ``padding_pe >= 0`` and ``image_padding > 0`` the Cpe = 2 (1 + 2 padding_pe) channels of ``PositionalEncoding(padding_pe,
    freq_factor=pi, d_in=2)`` of the pixel coordinates follow, zero over the image's own pixels.
    Differentiable with respect to the images (``diner_encoder_input_backward``, deterministic).
    ``images`` of dtype uint8 are the datasets' bytes [..., H, W, C] (``alpha``: an optional uint8 plane [..., H, W]), read by the
    arithmetic of ``image_format`` (a ``wire.ImageFormat``, required): the result is that of ``wire.decode_image_u8``'s rgb put through
    this function, bit for bit, in one launch and without the fp32 images (``diner_encoder_input_u8``; bytes carry no gradient).
    With ``size`` = (h, w) other than (H, W) the bytes are decoded and resized first (``wire.decode_image_u8(.., size=, antialias=)``,
    the resize kernels) and the floats take the route above: the same bits as calling the two in turn."""
    if isinstance(images, torch.Tensor) and images.dtype == torch.uint8:
        if image_format is None:
            raise ValueError("encoder_input: uint8 images need image_format (a wire.ImageFormat)")
        if not images.is_cuda:
            raise RuntimeError("diner_amd.glue.encoder_input runs on the GPU only")
        pad, F = int(image_padding), max(int(padding_pe), -1)
        with torch.no_grad():
            if size is not None:
                from . import wire
                if wire._hw(size, "encoder_input") != tuple(images.shape[-3:-1]):
                    rgb = wire.decode_image_u8(images, alpha, image_format, want_alpha=False, device=images.device, size=size,
                                               antialias=antialias)[0]
                    return _encoder_input(rgb, pad, F, _three(mean, "mean"), _three(std, "std"))
            return _encoder_input_u8(images, alpha, image_format, pad, F, _three(mean, "mean"), _three(std, "std"))
    if image_format is not None or alpha is not None or size is not None:
        raise ValueError("encoder_input: image_format, alpha and size go with uint8 images only")
    if not isinstance(images, torch.Tensor) or images.dim() < 3 or images.shape[-3] != 3:
        raise ValueError("encoder_input: images must be [..., 3, H, W]")
    if not images.is_cuda:
        raise RuntimeError("diner_amd.glue.encoder_input runs on the GPU only")
    pad, F = int(image_padding), max(int(padding_pe), -1)
    mean, std = _three(mean, "mean"), _three(std, "std")
    if torch.is_grad_enabled() and images.requires_grad:
        return _EncoderInputFn.apply(images, pad, F, mean, std)
    with torch.no_grad():
        return _encoder_input(_f(images).reshape(-1, *images.shape[-3:]), pad, F, mean, std)


def encode(model, images, depths, depths_std, extrinsics, intrinsics, image_format=None, alpha=None, image_size=None, antialias=True):
    """Drop-in for ``PixelNeRF.encode`` (reference src/models/pixelnerf.py:35-53) with ``SpatialEncoder.forward``
    (src/models/image_encoder.py:206-272) inside: images [SB,NV,3,H,W], depths, depths_std [SB,NV,1,H,W], extrinsics [SB,NV,4,4],
    intrinsics [SB,NV,3,3].  Or from the source views' bytes: images uint8 [SB,NV,H,W,C] with ``image_format`` (a ``wire.ImageFormat``)
    and optionally ``alpha`` uint8 [SB,NV,H,W], as :func:`encoder_input` takes them; ``image_size`` = (h, w): the bytes are resized to the
    size of the depths and intrinsics first (:func:`encoder_input`'s ``size`` and ``antialias``).
    The head (:func:`encoder_input`), the normals (:func:`depth2normal`) and the tail (:func:`assemble_latent`,
    or :func:`assemble_latent_bicubic` for ``upsample_interp="bicubic"``) run on the HIP kernels; the model's own trunk modules
    (``model.encoder.model``: conv1, bn1, relu, maxpool, layer1..) run unchanged on PyTorch in between.  Leaves the model in the state the
    reference's encode leaves it in, with ``encoder.latent`` in the layout the render and training kernels read
    (:func:`latent_is_packed`).  ``model.encode = functools.partial(glue.encode, model)``."""
    enc = model.encoder
    if enc.upsample_interp not in ("bilinear", "bicubic"):   # before any device work; there is no eager fallback
        raise NotImplementedError(f"encode: upsample_interp {enc.upsample_interp!r} is not implemented (the two modes torch accepts with "
                                  "align_corners=True, 'bilinear' and 'bicubic', are)")
    if images.dtype == torch.uint8:   # the refusals of a byte source come before the model is touched
        from . import wire
        if image_format is None:
            raise ValueError("encode: uint8 images need image_format (a wire.ImageFormat)")
        if images.dim() != 5:
            raise ValueError(f"encode: uint8 images must be [SB, NV, H, W, C], not {tuple(images.shape)}")
        wire.image_source(images, alpha, image_format, images.device, "encode")
        SB, NV, H, W, _ = images.shape
        if image_size is not None:
            H, W = wire._hw(image_size, "encode")
    else:
        if image_format is not None or alpha is not None or image_size is not None:
            raise ValueError("encode: image_format, alpha and image_size go with uint8 images only")
        SB, NV, _, H, W = images.shape
    norm = getattr(model, "normalize_rgb", None)
    mean, std = getattr(norm, "mean", None), getattr(norm, "std", None)
    enc.depths, enc.depths_std = depths, depths_std
    enc.normals = depth2normal(depths.flatten(0, 1), intrinsics.flatten(0, 1)).reshape(SB, NV, 3, H, W)
    enc.nviews, enc.nobjects = NV, SB
    x = encoder_input(images, enc.image_padding, enc.padding_pe, IMAGENET_MEAN if mean is None else mean,
                      IMAGENET_STD if std is None else std, alpha=alpha, image_format=image_format, size=image_size,
                      antialias=antialias)
    trunk = enc.model
    x = trunk.relu(trunk.bn1(trunk.conv1(x)))
    levels = [x]
    if enc.num_layers > 1:
        if enc.use_first_pool:
            x = trunk.maxpool(x)
        x = trunk.layer1(x)
        levels.append(x)
    for i in (2, 3, 4):
        if enc.num_layers > i:
            x = getattr(trunk, f"layer{i}")(x)
            levels.append(x)
    if enc.upsample_interp == "bicubic":
        enc.latent = assemble_latent_bicubic(levels, SB, NV)
    else:
        enc.latent = assemble_latent(levels, SB, NV, mode=enc.upsample_interp)
    model.poses = extrinsics
    model.c = intrinsics[:, :, :2, -1]
    model.focal = torch.stack((intrinsics[:, :, 0, 0], intrinsics[:, :, 1, 1]), dim=-1)
    shape = getattr(model, "image_shape", None)
    if not (isinstance(shape, torch.Tensor) and shape.numel() >= 2 and shape.device == images.device):
        model.image_shape = shape = torch.empty(2, dtype=torch.float32, device=images.device)
    with torch.no_grad():
        shape[0] = W
        shape[1] = H
    return None


# ---- a training step around renderer.forward: ray selection and the photometric losses --------------------------------------------------
def _indices(pix_idcs, SB, who):
    """pix_idcs as the kernels read it: [SB, B], int64 or int32, contiguous -> (tensor, is_int64)"""
    if not isinstance(pix_idcs, torch.Tensor) or pix_idcs.dim() != 2 or pix_idcs.shape[0] != SB:
        raise ValueError(f"{who}: pix_idcs must be a tensor [SB = {SB}, B]")
    if pix_idcs.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: pix_idcs must be int64 or int32, not {pix_idcs.dtype}")
    return pix_idcs.contiguous(), int(pix_idcs.dtype == torch.int64)


def _check_indices(pix_idcs, npix, who):
    if pix_idcs.numel():
        lo, hi = (int(v) for v in torch.aminmax(pix_idcs))
        if lo < 0 or hi >= npix:
            raise IndexError(f"{who}: pix_idcs spans [{lo}, {hi}], outside [0, H*W = {npix})")


def _gen_rays_at(e, k, zn, zf, idx, is64, W, H):
    SB, B = idx.shape
    out = torch.empty((SB, B, 8), dtype=torch.float32, device=e.device)
    check(_lib.lib().diner_gen_rays_at(e.data_ptr(), k.data_ptr(), zn.data_ptr(), zf.data_ptr(), idx.data_ptr(), is64, SB, B, int(H), int(W),
                                       out.data_ptr(), _st(e.device)), "diner_gen_rays_at")
    return out


def gen_rays_at_backward(e, k, d_rays, pix_idcs, H, W):
    """Backward of :func:`gen_rays_at` on fp32 contiguous cameras e [SB,4,4], k [SB,3,3], d_rays [SB,B,8] and pix_idcs [SB,B]:
    -> d_extrinsics [SB,4,4], d_intrinsics [SB,3,3], d_near [SB], d_far [SB] in fp32 (diner_gen_rays_at_backward: it reads d_rays and the
    indices only; fixed-order fp64 sums, bitwise reproducible)."""
    SB, dev = e.shape[0], e.device
    idx, is64 = _indices(pix_idcs, SB, "gen_rays_at_backward")
    B = idx.shape[1]
    g = _f(d_rays)
    assert g.numel() == SB * B * 8, "gen_rays_at_backward: d_rays must be [SB, B, 8]"
    L = _lib.lib()
    n = int(L.diner_gen_rays_at_backward_workspace_floats(SB, B))
    if n < 0:
        raise ValueError(f"gen_rays_at_backward: bad sizes SB={SB}, B={B}")
    ws = torch.empty(max(n, 2), dtype=torch.float32, device=dev)
    d_e = torch.empty((SB, 4, 4), dtype=torch.float32, device=dev)
    d_k = torch.empty((SB, 3, 3), dtype=torch.float32, device=dev)
    d_n = torch.empty(SB, dtype=torch.float32, device=dev)
    d_f = torch.empty(SB, dtype=torch.float32, device=dev)
    check(L.diner_gen_rays_at_backward(e.data_ptr(), k.data_ptr(), g.data_ptr(), idx.data_ptr(), is64, SB, B, int(H), int(W), d_e.data_ptr(),
                                       d_k.data_ptr(), d_n.data_ptr(), d_f.data_ptr(), ws.data_ptr(), _st(dev)), "diner_gen_rays_at_backward")
    return d_e, d_k, d_n, d_f


class _GenRaysAtFn(torch.autograd.Function):
    """gen_rays_at with a backward: forward = diner_gen_rays_at (the no-grad call's values, bit for bit), backward = diner_gen_rays_at_backward"""

    @staticmethod
    def forward(ctx, extrinsics, intrinsics, z_near, z_far, W, H, idx, is64):
        e, k = _f(extrinsics), _f(intrinsics)
        SB = e.shape[0]
        out = _gen_rays_at(e, k, _per_camera(z_near, SB, e.device), _per_camera(z_far, SB, e.device), idx, is64, W, H)
        ctx.save_for_backward(extrinsics, intrinsics, idx)    # (version-checked by autograd: an in-place edit before backward raises)
        ctx.e, ctx.k, ctx.HW = e, k, (int(H), int(W))
        ctx.zs = (z_near, z_far)
        return out

    @staticmethod
    def backward(ctx, d_rays):
        extrinsics, intrinsics, idx = ctx.saved_tensors
        H, W = ctx.HW
        d_e, d_k, d_n, d_f = gen_rays_at_backward(ctx.e, ctx.k, d_rays, idx, H, W)
        z_near, z_far = ctx.zs
        return (_like(d_e, extrinsics) if ctx.needs_input_grad[0] else None,
                _like(d_k, intrinsics) if ctx.needs_input_grad[1] else None,
                _like(d_n, z_near) if ctx.needs_input_grad[2] else None,
                _like(d_f, z_far) if ctx.needs_input_grad[3] else None, None, None, None, None)


def gen_rays_at(extrinsics, intrinsics, W, H, z_near, z_far, pix_idcs, check_indices=False):
    """:func:`gen_rays` at selected pixels only, in one kernel (reference src/models/diner.py:224-227 + :257-258): extrinsics [SB,4,4],
    intrinsics [SB,3,3], z_near / z_far [SB] (or one value for all), pix_idcs [SB,B] (int64 or int32, on the device, ``idx = x + y * W`` as in
    diner.py:246) -> rays [SB,B,8], bit-equal to ``gen_rays(...).view(SB, H*W, 8)[b, pix_idcs[b]]``.  Differentiable with respect to the same
    inputs as gen_rays (``diner_gen_rays_at_backward``: it reads d_rays [SB,B,8] and the indices, not a full-image gradient; deterministic;
    duplicate indices are separate terms).
    ``check_indices=True``: one host-side ``aminmax`` (a device synchronisation) raises ``IndexError`` for an index outside [0, H*W) before
    anything is launched.  With ``False`` the kernel clamps an index into [0, H*W): it never reads or writes out of bounds, and the result for
    such an index is unspecified."""
    SB = extrinsics.shape[0]
    idx, is64 = _indices(pix_idcs, SB, "gen_rays_at")
    if check_indices:
        _check_indices(idx, int(H) * int(W), "gen_rays_at")
    if not extrinsics.is_cuda or not idx.is_cuda:
        raise RuntimeError("diner_amd.glue.gen_rays_at runs on the GPU only")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                       for t in (extrinsics, intrinsics, z_near, z_far)):
        return _GenRaysAtFn.apply(extrinsics, intrinsics, z_near, z_far, W, H, idx, is64)
    with torch.no_grad():
        e, k = _f(extrinsics), _f(intrinsics)
        return _gen_rays_at(e, k, _per_camera(z_near, SB, e.device), _per_camera(z_far, SB, e.device), idx, is64, W, H)


def _photo_loss(p, t, idx, is64, patch, pool):
    """fp32 contiguous pred [SB,B,3], target [SB,3,H,W] -> (losses [2], gt_colors [SB,B,3], cell_sign [SB,3,nc,nc] or None)"""
    SB, B, _ = p.shape
    H, W = t.shape[2:]
    L = _lib.lib()
    n = int(L.diner_photo_loss_workspace_floats(SB, B, patch, pool))
    if n < 0:
        raise ValueError(f"photo_loss: bad sizes SB={SB}, B={B}, patch={patch}, pool={pool}")
    ws = torch.empty(max(n, 2), dtype=torch.float32, device=p.device)
    gt = torch.empty((SB, B, 3), dtype=torch.float32, device=p.device)
    losses = torch.empty(2, dtype=torch.float32, device=p.device)
    nc = patch // pool if patch else 0
    sign = torch.empty((SB, 3, nc, nc), dtype=torch.float32, device=p.device) if patch else None
    check(L.diner_photo_loss(p.data_ptr(), t.data_ptr(), idx.data_ptr(), is64, SB, B, H, W, patch, pool, gt.data_ptr(), losses.data_ptr(),
                             sign.data_ptr() if patch else None, ws.data_ptr(), _st(p.device)), "diner_photo_loss")
    return losses, gt, sign


def photo_loss_backward(pred, gt_colors, cell_sign, g_mse, g_ab, patch, pool):
    """d_pred [SB,B,3] in fp32 from fp32 contiguous pred, gt_colors and the cell signs :func:`photo_loss` kept; g_mse / g_ab: the two losses'
    gradients as fp32 device scalars, or None for 0 (``diner_photo_loss_backward``: one elementwise kernel)."""
    SB, B, _ = pred.shape
    d = torch.empty((SB, B, 3), dtype=torch.float32, device=pred.device)
    check(_lib.lib().diner_photo_loss_backward(pred.data_ptr(), gt_colors.data_ptr(), cell_sign.data_ptr() if patch else None,
                                               None if g_mse is None else g_mse.data_ptr(), None if g_ab is None else g_ab.data_ptr(),
                                               SB, B, patch, pool, d.data_ptr(), _st(pred.device)), "diner_photo_loss_backward")
    return d


class _PhotoLossFn(torch.autograd.Function):
    """photo_loss with a backward to pred: forward = diner_photo_loss (the no-grad call's values), backward = diner_photo_loss_backward"""

    @staticmethod
    def forward(ctx, pred, t, idx, is64, patch, pool):
        p = _f(pred)
        losses, gt, sign = _photo_loss(p, t, idx, is64, patch, pool)
        ctx.save_for_backward(pred)      # (version-checked by autograd: an in-place edit before backward raises)
        ctx.p, ctx.gt, ctx.sign, ctx.patch, ctx.pool = p, gt, sign, patch, pool
        ctx.mark_non_differentiable(gt)
        ctx.set_materialize_grads(False)
        return losses[0], losses[1], gt

    @staticmethod
    def backward(ctx, g_mse, g_ab, _g_gt):
        pred, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        g_mse, g_ab = (None if g is None else _f(g) for g in (g_mse, g_ab))
        d = photo_loss_backward(ctx.p, ctx.gt, ctx.sign, g_mse, g_ab, ctx.patch, ctx.pool)
        return d.reshape(pred.shape).to(pred.dtype), None, None, None, None, None


def photo_loss(pred, target_rgb, pix_idcs, patch=None, antibias_downsampling=3):
    """The photometric losses of ``DINER.calc_losses`` after the renderer (reference src/models/diner.py:265-267, :280-282 and
    src/losses/antibiasloss.py) in one kernel and a one-block sum: pred [SB,B,3] (the renderer's ``fine.rgb``), target_rgb [SB,3,H,W],
    pix_idcs [SB,B] (as for :func:`gen_rays_at`; an index outside [0, H*W) is clamped, the result is then unspecified)
    -> ``(mse, antibias, gt_colors)``:

    * ``gt_colors`` [SB,B,3] = ``target_rgb.view(SB, 3, -1).permute(0, 2, 1)[b, pix_idcs[b]]`` (what the caller's VGG loss needs too);
    * ``mse`` = ``MSELoss(reduction="mean")(pred, gt_colors)``;
    * ``antibias`` = ``AntibiasLoss(antibias_downsampling)`` on the two patches ``x.view(SB, s, s, 3).permute(0, 3, 1, 2)`` with
      ``patch = s`` (``B == s * s``, rays row-major): ``AvgPool2d(p)``, ``p = 2 ** antibias_downsampling``, of both (floor semantics:
      ``s // p`` cells per side, trailing rows and columns that fill no cell are ignored), then the L1 mean over the
      ``SB * 3 * (s // p) ** 2`` cells.  With ``patch=None`` it is a zero scalar and no pooling runs.  ``s < p`` raises ``ValueError``
      (the reference's pool fails there).

    Sums are fp64 per workgroup, added in block order (no atomics: two runs agree bit for bit).  Differentiable with respect to ``pred``
    (``diner_photo_loss_backward``); ``target_rgb`` and ``pix_idcs`` get no gradient."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or pred.shape[-1] != 3:
        raise ValueError("photo_loss: pred must be [SB, B, 3]")
    SB, B, _ = pred.shape
    if not isinstance(target_rgb, torch.Tensor) or target_rgb.dim() != 4 or target_rgb.shape[:2] != (SB, 3):
        raise ValueError(f"photo_loss: target_rgb must be [SB = {SB}, 3, H, W]")
    idx, is64 = _indices(pix_idcs, SB, "photo_loss")
    if idx.shape[1] != B or SB < 1 or B < 1:
        raise ValueError(f"photo_loss: pix_idcs {tuple(idx.shape)} does not belong to pred {tuple(pred.shape)} (at least one ray)")
    pool = 1
    if patch is not None:
        patch, n = int(patch), int(antibias_downsampling)
        if n < 0 or patch < 1 or patch * patch != B:
            raise ValueError(f"photo_loss: patch={patch} needs B == patch * patch (B = {B}) and antibias_downsampling >= 0")
        pool = 2 ** n
        if patch < pool:
            raise ValueError(f"photo_loss: a {patch} x {patch} patch is smaller than the {pool} x {pool} pooling cell "
                             f"(antibias_downsampling={n})")
    patch = patch or 0
    if not (pred.is_cuda and target_rgb.is_cuda and idx.is_cuda):
        raise RuntimeError("diner_amd.glue.photo_loss runs on the GPU only")
    t = _f(target_rgb)
    if torch.is_grad_enabled() and pred.requires_grad:
        return _PhotoLossFn.apply(pred, t, idx, is64, patch, pool)
    with torch.no_grad():
        losses, gt, _ = _photo_loss(_f(pred), t, idx, is64, patch, pool)
        return losses[0], losses[1], gt


def calc_losses(nerf, renderer, batch, znear, zfar, pix_idcs, patch=None, w_vgg=0., vggloss=None, w_antibias=0., antibias_downsampling=3):
    """``DINER.calc_losses`` (reference src/models/diner.py:217-290) assembled from the HIP pieces: ``nerf.encode`` (whatever the model has
    bound, e.g. ``functools.partial(glue.encode, nerf)``) on the batch's source views, :func:`gen_rays_at` for the selected target pixels,
    ``renderer.forward(model=nerf, rays=rays)``, :func:`photo_loss`, and -- with ``w_vgg > 0`` -- the caller's ``vggloss`` on the NCHW
    patches.  ``batch``: the reference's keys (``src_rgbs, src_depths, src_depth_stds, src_extrinsics, src_intrinsics, target_rgb,
    target_extrinsics, target_intrinsics``); ``znear`` / ``zfar``: one value or [SB].  Returns the reference's dict ``rgb_fine, vgg_fine,
    antibias, total`` with ``total = rgb_fine + w_vgg * vgg_fine + w_antibias * antibias`` (terms with a zero weight are the float 0. and
    are left out).  ``total`` is a new tensor: the reference adds in place into ``rgb_fine``, which therefore aliases its ``total``.

    ``pix_idcs`` [SB,B] is an argument, the random draw stays the caller's.  The reference's two draws (diner.py:229-247), on the device:

        pix_idcs = torch.randint(0, H * W, (SB, ray_batch_size), device=dev)                       # w_vgg == 0

        s, pad = vgg_spatch, (vgg_spatch + 1) // 2                                                   # w_vgg > 0: an s x s patch
        fg = batch["target_alpha"][:, 0].clone()
        fg[..., :pad] = 0; fg[..., :pad, :] = 0; fg[..., -pad:] = 0; fg[..., -pad:, :] = 0
        centre = torch.multinomial(fg.view(SB, H * W), 1)                                            # [SB,1]
        ys, xs = torch.meshgrid(torch.arange(s, device=dev), torch.arange(s, device=dev), indexing="ij")
        pix_idcs = ((centre % W).view(SB, 1, 1) + xs - pad + ((centre // W).view(SB, 1, 1) + ys - pad) * W).flatten(1)   # patch=s

    ``patch`` is required when ``w_vgg > 0`` or ``w_antibias > 0``."""
    SB, _, H, W = batch["target_rgb"].shape
    if (w_vgg > 0 or w_antibias > 0) and patch is None:
        raise ValueError("calc_losses: w_vgg > 0 and w_antibias > 0 need the patch side (patch=s, B == s * s)")
    if w_vgg > 0 and vggloss is None:
        raise ValueError("calc_losses: w_vgg > 0 needs vggloss")
    nerf.encode(images=batch["src_rgbs"], depths=batch["src_depths"], depths_std=batch["src_depth_stds"],
                extrinsics=batch["src_extrinsics"], intrinsics=batch["src_intrinsics"])
    rays = gen_rays_at(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, pix_idcs)
    pred = renderer.forward(model=nerf, rays=rays).fine.rgb
    loss_fine, loss_antibias, gt_colors = photo_loss(pred, batch["target_rgb"], pix_idcs, patch=patch if w_antibias > 0 else None,
                                                     antibias_downsampling=antibias_downsampling)
    total = loss_fine
    loss_vgg = 0.
    if w_vgg > 0:
        s = int(patch)
        loss_vgg = vggloss(pred.view(SB, s, s, 3).permute(0, 3, 1, 2), gt_colors.view(SB, s, s, 3).permute(0, 3, 1, 2))
        total = total + w_vgg * loss_vgg
    if w_antibias > 0:
        total = total + w_antibias * loss_antibias
    else:
        loss_antibias = 0.
    return dict(rgb_fine=loss_fine, vgg_fine=loss_vgg, antibias=loss_antibias, total=total)


# ---- frame output and image scores (csrc/frame_out.hip) --------------------------------------------------------------------------------
_tables = {}       # (key, device, kind) -> the float64 / quantised uint8 table on the device; "viridis" -> the shipped table on the host


def _cmap_table(cmap):
    """(cache key or None, float64 CPU tensor [nc + 3, 3]) of a colour map: the shipped viridis, a [nc + 3, 3] tensor, or any other
    name through matplotlib"""
    if isinstance(cmap, torch.Tensor):
        if cmap.dim() != 2 or cmap.shape[1] != 3 or cmap.shape[0] < 4 or cmap.dtype != torch.float64:
            raise ValueError("a colour table must be a float64 tensor [N + 3, 3] (N colours, then under, over, bad)")
        return None, cmap.detach()
    if cmap == "viridis":
        if "viridis" not in _tables:
            from .viridis_lut import VIRIDIS_LUT   # matplotlib's 259-row table (256 colours, under, over, bad) as a literal
            _tables["viridis"] = torch.tensor(VIRIDIS_LUT, dtype=torch.float64)
        return "viridis", _tables["viridis"]
    try:
        import matplotlib
    except ImportError as e:
        raise ImportError(f"the colour map {cmap!r} is looked up through matplotlib, which is not importable here (only 'viridis' ships "
                          "with diner_amd); pass the [N + 3, 3] float64 table instead") from e
    import numpy as np
    cm = matplotlib.colormaps[cmap]
    cm._init()                                          # fills _lut [N + 3, 4]: the colours, under, over, bad
    return str(cmap), torch.from_numpy(np.ascontiguousarray(cm._lut[:, :3], dtype=np.float64))


def _quantise_table(table, rounding):
    """the float64 table as bytes by diner_frames_u8's rule for ``rounding``, in double (what the reference does to the float64 colours)"""
    if rounding == "save_image":
        v = table * 255.0 + 0.5
    else:
        v = table * 255.0
    return torch.nan_to_num(v, nan=0.0).clamp(0.0, 255.0).to(torch.uint8)       # the cast truncates


def _device_table(cmap, dev, rounding=None):
    key, table = _cmap_table(cmap)
    slot = (key, dev, rounding)
    if key is not None and slot in _tables:
        return _tables[slot]
    t = (table if rounding is None else _quantise_table(table, rounding)).to(dev).contiguous()
    if key is not None:
        _tables[slot] = t
    return t


def _depth32(x, who):
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"{who}: a float32 (or half / bfloat16) tensor is needed: the kernels read fp32, and a float64 input would be rounded")
    if not x.is_cuda:
        raise RuntimeError(f"diner_amd.glue.{who} runs on the GPU only")
    return _f(x)


def depth_range(depth):
    """depth [N,1,H,W] (or [N,H,W]) -> float64 [N,2] on the device: each image's (min, max), exact; a NaN anywhere in an image makes both
    NaN, as ``np.min`` / ``np.max`` do (reference src/util/torch_helpers.py:64-65).  No host synchronisation."""
    d = _depth32(depth, "depth_range")
    if d.dim() == 4 and d.shape[1] == 1:
        d = d[:, 0]
    if d.dim() != 3 or d.numel() == 0:
        raise ValueError("depth_range: depth must be [N, 1, H, W] or [N, H, W] with at least one pixel")
    N, H, W = d.shape
    L = _lib.lib()
    n = int(L.diner_depth_range_workspace_floats(N, H, W))
    if n < 0:
        raise ValueError(f"depth_range: bad sizes N={N}, H={H}, W={W}")
    ws = torch.empty(n, dtype=torch.float32, device=d.device)
    out = torch.empty((N, 2), dtype=torch.float64, device=d.device)
    check(L.diner_depth_range(d.data_ptr(), N, H, W, out.data_ptr(), ws.data_ptr(), _st(d.device)), "diner_depth_range")
    return out


def _limits(d, vmin, vmax):
    """(range pointer or None, vmin, vmax, has_vmin, has_vmax, keep-alive): a limit of None or 0 is taken per image from the data -- the
    reference's ``vmin if vmin else np.min(...)`` (src/util/torch_helpers.py:64-65), which treats a given 0 as absent"""
    has_lo, has_hi = bool(vmin), bool(vmax)
    rng = None if has_lo and has_hi else depth_range(d)
    return (None if rng is None else rng.data_ptr(), float(vmin) if has_lo else 0.0, float(vmax) if has_hi else 0.0, int(has_lo), int(has_hi),
            rng)


def torch_cmap(x, cmap="viridis", vmin=None, vmax=None):
    """Drop-in for the reference's ``torch_cmap`` (src/util/torch_helpers.py:43-76) that stays on the device: x (B,1,H,W), (1,H,W) or (H,W)
    -> the same shape with 3 channels, float64, on ``x``'s device, bit-equal to the reference (numpy in float64 and matplotlib 3.10's
    ``Colormap._get_rgba_and_mask``; csrc/frame_out.hip states the index rule).  An image whose range is flat is black (0 / 0 selects the
    "bad" colour), as in the reference.

    ``cmap``: "viridis" (the table ships with the package), any other matplotlib name (looked up lazily; ``ImportError`` without
    matplotlib), or a float64 tensor [N + 3, 3].  ``vmin`` / ``vmax``: one scalar each, or None for the image's own minimum / maximum
    (computed on the device, no host synchronisation).  A ``vmin`` or ``vmax`` of 0 counts as absent: that is the reference's
    ``vmin if vmin else ...``.  Per-image arrays of limits are not supported."""
    d = _depth32(x, "torch_cmap")
    shape = x.shape
    if d.dim() < 2 or d.dim() > 4:
        raise ValueError("torch_cmap: x must be (B,1,H,W), (1,H,W) or (H,W)")
    d = d.reshape((1,) * (4 - d.dim()) + tuple(shape))
    if d.shape[1] != 1 or d.numel() == 0:
        raise ValueError("torch_cmap: x must have one channel and at least one pixel")
    N, _, H, W = d.shape
    table = _device_table(cmap, d.device)
    rng, lo, hi, has_lo, has_hi, _keep = _limits(d, vmin, vmax)
    out = torch.empty((N, 3, H, W), dtype=torch.float64, device=d.device)
    check(_lib.lib().diner_depth_cmap(d.data_ptr(), N, H, W, rng, lo, hi, has_lo, has_hi, table.data_ptr(), table.shape[0] - 3,
                                      out.data_ptr(), _st(d.device)), "diner_depth_cmap")
    return out.reshape(list(shape[:-3]) + [3] + list(shape[-2:]))


def frames_u8(rgb, depth=None, *, rounding="save_image", stacked=False, cmap="viridis", vmin=None, vmax=None):
    """Frames as the image / video writers take them, in one kernel: rgb [..,3,H,W] (and depth [..,1,H,W], coloured as :func:`torch_cmap`
    does) -> uint8 HWC on the device.  Returns ``rgb_u8`` [..,H,W,3]; with a depth ``(rgb_u8, depth_u8)``, or, with ``stacked=True``, one
    tensor [..,2H,W,3] with the colour above the depth -- ``cat((rgbs, depths), dim=-2)`` of ``create_cam_sweep`` (reference
    src/models/diner.py:209).  ``rounding``:

    * ``"save_image"``: ``(uint8) clamp(x * 255 + 0.5, 0, 255)``, torchvision's ``save_image`` (diner.py:129-133);
    * ``"video"``: ``(uint8) (double(x) * 255)``, ``save_torch_video`` (src/util/torch_helpers.py:91).

    A value outside the byte range saturates and NaN gives 0 (numpy's cast is undefined there).  The depth's colours are quantised from
    the float64 table by the same rule, so they equal the reference's bytes for its float64 colour map.  Ground-truth and source images
    go through the same function; quantising ``gt`` here gives the bytes the reference scores after its PNG round trip (PNG is lossless)."""
    if rounding not in _lib.ROUNDINGS:
        raise ValueError(f"frames_u8: rounding must be one of {sorted(_lib.ROUNDINGS)}")
    c = _depth32(rgb, "frames_u8")
    if c.dim() < 3 or c.shape[-3] != 3 or c.numel() == 0:
        raise ValueError("frames_u8: rgb must be [.., 3, H, W] with at least one pixel")
    lead, (H, W) = tuple(c.shape[:-3]), c.shape[-2:]
    c = c.reshape(-1, 3, H, W)
    N, dev = c.shape[0], c.device
    L = _lib.lib()
    if depth is None:
        if stacked:
            raise ValueError("frames_u8: stacked=True needs a depth")
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        check(L.diner_frames_u8(c.data_ptr(), None, N, H, W, _lib.ROUNDINGS[rounding], 0, None, 0.0, 0.0, 0, 0, None, 0, out.data_ptr(), None,
                                _st(dev)), "diner_frames_u8")
        return out.reshape(lead + (H, W, 3))
    d = _depth32(depth, "frames_u8")
    if d.dim() < 3 or tuple(d.shape[-3:]) != (1, H, W) or d.numel() != N * H * W:
        raise ValueError(f"frames_u8: depth must be [.., 1, {H}, {W}] for the same {N} frames")
    d = d.reshape(N, 1, H, W)
    table = _device_table(cmap, dev, rounding)
    rng, lo, hi, has_lo, has_hi, _keep = _limits(d, vmin, vmax)
    out = torch.empty((N, 2 * H if stacked else H, W, 3), dtype=torch.uint8, device=dev)
    out_d = None if stacked else torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    check(L.diner_frames_u8(c.data_ptr(), d.data_ptr(), N, H, W, _lib.ROUNDINGS[rounding], int(stacked), rng, lo, hi, has_lo, has_hi,
                            table.data_ptr(), table.shape[0] - 3, out.data_ptr(), None if stacked else out_d.data_ptr(), _st(dev)),
          "diner_frames_u8")
    if stacked:
        return out.reshape(lead + (2 * H, W, 3))
    return out.reshape(lead + (H, W, 3)), out_d.reshape(lead + (H, W, 3))


def image_scores(pred_u8, gt_u8):
    """The scores ``evaluate_folder`` takes from a PNG pair (reference src/evaluation/eval_suite.py:63-68), for uint8 HWC images
    [..,H,W,3] on the device (what :func:`frames_u8` returns): a dict ``ssim, psnr, l2, l1`` of float64 tensors [N] (N = the leading
    dimensions flattened) on the device, without a host synchronisation.  ``ssim`` is skimage's ``structural_similarity(pred, gt,
    channel_axis=-1, data_range=1)`` with its defaults (uniform 7 x 7 window, sample covariance), ``psnr`` its
    ``peak_signal_noise_ratio`` (+inf for equal images), ``l2`` / ``l1`` the mean squared / absolute difference of ``uint8 / 255``.
    The sums are exact integers and each window's value is formed in float64, so the results differ from the reference's float32
    evaluation by that evaluation's own rounding.  Two calls agree bit for bit.  LPIPS stays on PyTorch."""
    for t in (pred_u8, gt_u8):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError("image_scores takes uint8 HWC images: quantise float frames with glue.frames_u8 first")
    if pred_u8.shape != gt_u8.shape:
        raise ValueError(f"image_scores: the shapes differ: {tuple(pred_u8.shape)} and {tuple(gt_u8.shape)}")
    if pred_u8.dim() < 3 or pred_u8.shape[-1] != 3:
        raise ValueError("image_scores: images must be [.., H, W, 3]")
    H, W = pred_u8.shape[-3:-1]
    if H < 7 or W < 7:
        raise ValueError(f"image_scores: a {H} x {W} image is smaller than the 7 x 7 window")
    if not (pred_u8.is_cuda and gt_u8.is_cuda):
        raise RuntimeError("diner_amd.glue.image_scores runs on the GPU only")
    p, g = pred_u8.detach().reshape(-1, H, W, 3).contiguous(), gt_u8.detach().reshape(-1, H, W, 3).contiguous()
    N, dev = p.shape[0], p.device
    if N == 0:
        raise ValueError("image_scores: no images")
    L = _lib.lib()
    n = int(L.diner_image_scores_workspace_floats(N, H, W))
    if n < 0:
        raise ValueError(f"image_scores: bad sizes N={N}, H={H}, W={W}")
    ws = torch.empty(n // 2, dtype=torch.float64, device=dev)
    out = torch.empty((4, N), dtype=torch.float64, device=dev)
    check(L.diner_image_scores(p.data_ptr(), g.data_ptr(), N, H, W, out.data_ptr(), ws.data_ptr(), _st(dev)), "diner_image_scores")
    return dict(ssim=out[0], psnr=out[1], l2=out[2], l1=out[3])


# ---- rendering inside a scene bounding box (csrc/ray_box.hip) ----------------------------------------------------------------------------
BOX_OFFSET = (-0.01, 0.01)    # get_near_far's boffset (reference src/data/facescape.py:153)


def _box_args(extrinsics, intrinsics, W, H, z_near, z_far, bounds, box_offset, who):
    """the cameras as a DinerTargetCam, the bounds as fp32 [SB,2,3] on the cameras' device, the two offsets; + what keeps them alive"""
    if not isinstance(extrinsics, torch.Tensor) or not extrinsics.is_cuda:
        raise RuntimeError(f"diner_amd.glue.{who} runs on the GPU only")
    if extrinsics.dim() != 3 or tuple(extrinsics.shape[1:]) != (4, 4) or tuple(intrinsics.shape) != (extrinsics.shape[0], 3, 3):
        raise ValueError(f"{who}: extrinsics must be [SB,4,4] and intrinsics [SB,3,3]")
    H, W = int(H), int(W)
    if H < 0 or W < 0:
        raise ValueError(f"{who}: negative image size H={H}, W={W}")
    dev, SB = extrinsics.device, extrinsics.shape[0]
    e, k = _f(extrinsics), _f(intrinsics).to(dev)
    zn, zf = _per_camera(z_near, SB, dev), _per_camera(z_far, SB, dev)
    if not isinstance(bounds, torch.Tensor):
        import numpy as np
        bounds = torch.from_numpy(np.array(bounds, dtype=np.float32))       # (a copy: the array may be read-only)
    b = bounds.detach().to(device=dev, dtype=torch.float32)
    if tuple(b.shape) == (2, 3):
        b = b.expand(SB, 2, 3)
    if tuple(b.shape) != (SB, 2, 3):
        raise ValueError(f"{who}: bounds must be [SB = {SB}, 2, 3] or [2, 3] (min corner, max corner), not {tuple(b.shape)}")
    b = b.contiguous()
    lo, hi = (float(v) for v in box_offset)
    cam = _lib.DinerTargetCam()
    cam.extrinsics, cam.intrinsics, cam.z_near, cam.z_far, cam.H, cam.W = e.data_ptr(), k.data_ptr(), zn.data_ptr(), zf.data_ptr(), H, W
    return cam, b, lo, hi, (e, k, zn, zf)


def _ray_box_select(cam, SB, b, lo, hi, dev, want_near_far):
    """-> near_far [SB,H W,2] or None, idx [SB,H W], slot [SB,H W], count [SB] (int32, on the device)"""
    L = _lib.lib()
    npix = cam.H * cam.W
    n = int(L.diner_ray_box_select_workspace_floats(SB, cam.H, cam.W))
    if n < 0:
        raise ValueError(f"ray_box: bad sizes SB={SB}, H={cam.H}, W={cam.W}")
    ws = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    near_far = torch.empty((SB, npix, 2), dtype=torch.float32, device=dev) if want_near_far else None
    idx = torch.empty((SB, npix), dtype=torch.int32, device=dev)
    slot = torch.empty((SB, npix), dtype=torch.int32, device=dev)
    count = torch.zeros(SB, dtype=torch.int32, device=dev)
    check(L.diner_ray_box_select(C.byref(cam), SB, b.data_ptr(), lo, hi, None if near_far is None else near_far.data_ptr(), idx.data_ptr(),
                                 slot.data_ptr(), count.data_ptr(), ws.data_ptr(), _st(dev)), "diner_ray_box_select")
    return near_far, idx, slot, count


@torch.no_grad()
def ray_box(extrinsics, intrinsics, W, H, z_near, z_far, bounds, box_offset=BOX_OFFSET):
    """The device form of ``FacescapeDataSet.get_near_far`` + ``get_mask_at_box`` (reference src/data/facescape.py:128-185) on the project's
    rays (:func:`gen_rays`: pixel centres, unit directions): extrinsics [SB,4,4], intrinsics [SB,3,3], z_near / z_far [SB] (or one value),
    ``bounds`` [SB,2,3] or [2,3] (min corner, max corner; a tensor on any device or an array, e.g. ``load_face_bounds``' result)
    -> ``near`` [SB,H,W], ``far`` [SB,H,W] (fp32), ``mask`` [SB,H,W] (bool).  The box is ``bounds[0] + box_offset[0]`` ..
    ``bounds[1] + box_offset[1]``; near / far are the ray's signed entry / exit parameters clamped to [z_near, z_far]; a pixel whose ray
    misses the box holds z_near, z_far.  Two deliberate differences from ``get_near_far``: a box behind the camera is a miss (the
    reference's unsigned distances mirror it to the front), and a camera inside the box gets ``near = z_near`` (the reference takes the
    nearer face, which may be the one behind the camera).  Carries no gradient: near and far are constants of any later backward."""
    cam, b, lo, hi, _keep = _box_args(extrinsics, intrinsics, W, H, z_near, z_far, bounds, box_offset, "ray_box")
    SB, dev = b.shape[0], b.device
    near_far, _, slot, _ = _ray_box_select(cam, SB, b, lo, hi, dev, True)
    near_far = near_far.view(SB, cam.H, cam.W, 2)
    return near_far[..., 0], near_far[..., 1], (slot >= 0).view(SB, cam.H, cam.W)


@torch.no_grad()
def box_rays(extrinsics, intrinsics, W, H, z_near, z_far, bounds, box_offset=BOX_OFFSET):
    """The rays of :func:`ray_box`'s hit pixels only, compacted in pixel order (the arguments are :func:`ray_box`'s)
    -> ``(rays [SB,B,8], idx [SB,B], slot [SB,H*W], counts [SB])`` with ``B = counts.max()``:

    * ``rays[sb, j]`` for ``j < counts[sb]``: :func:`gen_rays`' ray at pixel ``idx[sb, j]`` (origin and direction bit for bit) with
      components 6, 7 = the box's near, far of that ray; from ``counts[sb]`` on: padding that repeats the scene's last hit (a scene
      without hits repeats pixel 0 with z_near, z_far) -- render it, never read its results;
    * ``idx`` (int32): the hit pixels ``x + y * W`` ascending, -1 in the padding; ``slot`` (int32): the rank of each pixel among its
      scene's hits or -1, what :func:`frame_from_hits` gathers through; ``counts`` (int32, on the device).

    Reads the counts on the host: one synchronisation of SB ints.  ``B = 0`` gives empty tensors and no second launch.  ``rays`` can be
    fed to ``renderer.forward`` like any other rays, under autograd too (near is a constant there, far enters through the last
    sample's interval only)."""
    cam, b, lo, hi, _keep = _box_args(extrinsics, intrinsics, W, H, z_near, z_far, bounds, box_offset, "box_rays")
    SB, dev = b.shape[0], b.device
    _, idx, slot, count = _ray_box_select(cam, SB, b, lo, hi, dev, False)
    host = count.cpu()                                       # the one synchronisation
    B = int(host.max()) if SB else 0
    rays = torch.empty((SB, B, 8), dtype=torch.float32, device=dev)
    if B > 0:
        host_c = (C.c_int32 * SB)(*host.tolist())
        check(_lib.lib().diner_gen_rays_box(C.byref(cam), SB, b.data_ptr(), lo, hi, idx.data_ptr(), count.data_ptr(), host_c, B,
                                            rays.data_ptr(), _st(dev)), "diner_gen_rays_box")
    return rays, idx[:, :B], slot, count


@torch.no_grad()
def frame_from_hits(rgb_c, depth_c, slot, H, W, white_bkgd, return_mask=False):
    """The frame of a boxed render from its compact results: rgb_c [SB,B,3], depth_c [SB,B] (what ``renderer.forward`` returned for
    :func:`box_rays`' rays), ``slot`` [SB,H*W] (:func:`box_rays`) -> ``rgb`` [SB,3,H,W], ``depth`` [SB,1,H,W] in the reference's image
    layout (views of pixel-major buffers, as ``render_image`` returns them).  A missed pixel is the background: 1 with ``white_bkgd``
    else 0, depth 0.  One thread per pixel gathers: every output element is written.  ``return_mask=True`` adds ``mask`` [SB,1,H,W]
    (bool)."""
    if not isinstance(slot, torch.Tensor) or not slot.is_cuda:
        raise RuntimeError("diner_amd.glue.frame_from_hits runs on the GPU only")
    H, W = int(H), int(W)
    if slot.dim() != 2 or slot.dtype != torch.int32 or slot.shape[1] != H * W:
        raise ValueError(f"frame_from_hits: slot must be int32 [SB, H*W = {H * W}]")
    SB, dev = slot.shape[0], slot.device
    c, d = _f(rgb_c), _f(depth_c)
    if c.dim() != 3 or c.shape[0] != SB or c.shape[2] != 3 or tuple(d.shape) != tuple(c.shape[:2]):
        raise ValueError(f"frame_from_hits: rgb_c must be [SB = {SB}, B, 3] and depth_c [SB, B]")
    B = c.shape[1]
    s = slot.contiguous()
    rgb = torch.empty((SB, H * W, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((SB, H * W), dtype=torch.float32, device=dev)
    mask = torch.empty((SB, H * W), dtype=torch.uint8, device=dev) if return_mask else None
    check(_lib.lib().diner_frame_from_hits(c.data_ptr() if B else None, d.data_ptr() if B else None, s.data_ptr(), SB, B, H, W,
                                           int(bool(white_bkgd)), rgb.data_ptr(), depth.data_ptr(),
                                           None if mask is None else mask.data_ptr(), _st(dev)), "diner_frame_from_hits")
    out = rgb.view(SB, H, W, 3).permute(0, 3, 1, 2), depth.view(SB, H, W, 1).permute(0, 3, 1, 2)
    if return_mask:
        return out + (mask.view(SB, 1, H, W).bool(),)
    return out


# ---- nearest mesh vertex and the NOVEL renderers' deformation (csrc/nearest_vertex.hip) -------------------------------------------------
from .deform import deform_points, deform_ray_points, nearest_vertex  # noqa: E402,F401
