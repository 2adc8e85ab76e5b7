"""HIP versions of the two per-image producers next to the render path,
with the reference's own function signatures so they can replace them in place:

* :func:`gen_rays`      -- reference ``src/util/cam_geometry.py:36-79`` (differentiable in the cameras, near and far, like the
  reference's plain-torch version: the backward is ``diner_gen_rays_backward``)
* :func:`depth2normal`  -- reference ``src/util/depth2normal.py:7-87``

and the tail of the encoder: :func:`assemble_latent` -- reference ``src/models/image_encoder.py:262-272`` (the feature levels upsampled to
the first one's size and concatenated), written once in the NHWC layout the render and training kernels read;
its head: :func:`encoder_input` -- reference ``src/models/pixelnerf.py:44`` + ``src/models/image_encoder.py:222-232`` (conv1's input: the
images normalised and replicate-padded, plus the positional encoding of the padding);
and both around the model's own CNN trunk: :func:`encode`, with ``PixelNeRF.encode``'s signature (reference
``src/models/pixelnerf.py:35-53`` + ``SpatialEncoder.forward``, ``src/models/image_encoder.py:206-272``).
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


def _assemble_check(levels, SB, NV, mode):
    if mode != "bilinear":   # (the reference's nearest branch is unreachable: it compares with "nearest ", image_encoder.py:262)
        raise NotImplementedError(f"assemble_latent: upsample mode {mode!r} is not implemented (the encoder's tail is bilinear, "
                                  "align_corners=True)")
    levels = list(levels)
    if not 1 <= len(levels) <= _lib.LATENT_MAX_LEVELS:
        raise ValueError(f"assemble_latent: {len(levels)} levels, expected 1..{_lib.LATENT_MAX_LEVELS}")
    N = int(SB) * int(NV)
    for t in levels:
        if not t.is_cuda:
            raise RuntimeError("diner_amd.glue.assemble_latent runs on the GPU only")
        if t.dim() != 4 or t.shape[0] != N:
            raise ValueError(f"assemble_latent: a level must be [SB*NV = {N}, C_l, h_l, w_l], not {tuple(t.shape)}")
    return levels


def _assemble(lv, SB, NV):
    """fp32 contiguous levels [SB*NV, C_l, h_l, w_l] -> the NHWC buffer [SB, NV, h, w, C]"""
    h, w = lv[0].shape[2:]
    out = torch.empty((SB, NV, h, w, sum(t.shape[1] for t in lv)), dtype=torch.float32, device=lv[0].device)
    check(_lib.lib().diner_assemble_latent(C.byref(_levels_struct(lv)), len(lv), SB * NV, h, w, out.data_ptr(), _st(out.device)),
          "diner_assemble_latent")
    return out


def assemble_latent_backward(d_latent, level_shapes):
    """Adjoint of :func:`assemble_latent`: d_latent of logical shape [SB, NV, C, h, w] (made NHWC-strided fp32 once if it is not) ->
    the levels' gradients [SB*NV, C_l, h_l, w_l] in fp32 (``diner_assemble_latent_backward``: gather form, bitwise reproducible)."""
    SB, NV, _, h, w = d_latent.shape
    g = d_latent.detach().permute(0, 1, 3, 4, 2)
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.to(torch.float32).contiguous()
    grads = [torch.empty(tuple(s), dtype=torch.float32, device=g.device) for s in level_shapes]
    check(_lib.lib().diner_assemble_latent_backward(g.data_ptr(), len(grads), SB * NV, h, w, C.byref(_levels_struct(grads)), _st(g.device)),
          "diner_assemble_latent_backward")
    return grads


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
    levels = _assemble_check(levels, SB, NV, mode)
    SB, NV = int(SB), int(NV)
    if torch.is_grad_enabled() and any(t.requires_grad for t in levels):
        return _AssembleLatentFn.apply(SB, NV, *levels)
    with torch.no_grad():
        return _assemble([_f(t) for t in levels], SB, NV).permute(0, 1, 4, 2, 3)


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


def encoder_input(images, image_padding, padding_pe, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """conv1's input in one kernel (reference src/models/pixelnerf.py:44 + src/models/image_encoder.py:222-232): ``images``
    [..., 3, H, W] -> [N, 3 + Cpe, H + 2 image_padding, W + 2 image_padding] in fp32, N = the product of the leading dimensions.
    Channels 0..2: ``(images - mean) / std`` replicate-padded by ``image_padding``, bit-equal to ``Normalize`` + ``ReplicationPad2d``;
    with ``padding_pe >= 0`` and ``image_padding > 0`` the Cpe = 2 (1 + 2 padding_pe) channels of ``PositionalEncoding(padding_pe,
    freq_factor=pi, d_in=2)`` of the pixel coordinates follow, zero over the image's own pixels.
    Differentiable with respect to the images (``diner_encoder_input_backward``, deterministic)."""
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


def encode(model, images, depths, depths_std, extrinsics, intrinsics):
    """Drop-in for ``PixelNeRF.encode`` (reference src/models/pixelnerf.py:35-53) with ``SpatialEncoder.forward``
    (src/models/image_encoder.py:206-272) inside: images [SB,NV,3,H,W], depths, depths_std [SB,NV,1,H,W], extrinsics [SB,NV,4,4],
    intrinsics [SB,NV,3,3].  The head (:func:`encoder_input`), the normals (:func:`depth2normal`) and the tail (:func:`assemble_latent`)
    run on the HIP kernels; the model's own trunk modules (``model.encoder.model``: conv1, bn1, relu, maxpool, layer1..) run unchanged on
    PyTorch in between.  Leaves the model in the state the reference's encode leaves it in, with ``encoder.latent`` in the layout the
    render and training kernels read (:func:`latent_is_packed`).  ``model.encode = functools.partial(glue.encode, model)``."""
    enc = model.encoder
    if enc.upsample_interp != "bilinear":   # before any device work; there is no eager fallback
        raise NotImplementedError(f"encode: upsample_interp {enc.upsample_interp!r} is not implemented (assemble_latent is bilinear, "
                                  "align_corners=True)")
    SB, NV, _, H, W = images.shape
    norm = getattr(model, "normalize_rgb", None)
    mean, std = getattr(norm, "mean", None), getattr(norm, "std", None)
    enc.depths, enc.depths_std = depths, depths_std
    enc.normals = depth2normal(depths.flatten(0, 1), intrinsics.flatten(0, 1)).reshape(SB, NV, 3, H, W)
    enc.nviews, enc.nobjects = NV, SB
    x = encoder_input(images, enc.image_padding, enc.padding_pe, IMAGENET_MEAN if mean is None else mean,
                      IMAGENET_STD if std is None else std)
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
