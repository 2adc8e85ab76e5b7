"""``NeRFRendererDGS`` -- the MI355X-native drop-in for the reference renderer plug-in.

Mirrors ``src/models/nerf_renderer.py:12-430`` of tancredeguillou/diner: same constructor
kwargs, same mutable attributes (``n_samples``/``n_gaussian`` are re-assigned after loading a
checkpoint, ``python_scripts/create_prediction_folder.py:49-52``), same
``forward(model, rays, want_weights)`` contract and the same stage methods.  Selecting it is a
one-line YAML change (``renderer.module: diner_amd.NeRFRendererDGS``, resolved by
``src/util/import_helper.py:16-24`` at ``src/models/diner.py:48``).

All arithmetic runs in the hand-written HIP kernels of ``libdiner_hip.so`` through the C ABI in
``include/diner_hip.h``; PyTorch only owns device memory and the stream.  There is no CPU or
eager fallback: without the library the import of this module's dependencies fails.

The module holds no parameters or buffers (reference checkpoints load with ``strict=True``); it
keeps an identity-keyed cache of re-packed copies of the model's maps and MLP weights: an entry is
valid only while the very tensor OBJECTS it was packed from are alive (weak references, compared with
``is``) and their ``_version`` counters are unchanged -- a fresh tensor that the caching allocator
happens to place at a freed tensor's address is a different object and invalidates the entry, as does
every ``encode()`` of the reference, which re-binds ``encoder.latent/depths/...`` to new tensors
(src/models/image_encoder.py:214-218,271-272).  No strong reference to the sources is kept.
"""
from __future__ import annotations

import ctypes as C
import warnings
import weakref
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import DinerMlpRaw, DinerSamplerCfg, DinerScene, check
from .glue import latent_is_packed


class MlpShape(NamedTuple):
    """The fusion-MLP / positional-encoding shape of a PixelNeRF (reference src/models/pixelnerf.py:14-24,
    src/models/resnetfc.py:72-127): what ``NeRFRendererDGS._validate_model`` returns."""
    d_in: int
    d_latent: int
    d_hidden: int
    n_blocks: int
    combine_layer: int
    num_freqs: int
    beta: float = 0.0          # Softplus beta; 0 = ReLU

    @property
    def standard(self) -> bool:
        """the one model the 512-wide kernels are built for (include/diner_hip.h DINER_D_*)"""
        return self == STANDARD_SHAPE

    def c_struct(self) -> _lib.DinerMlpShape:
        return _lib.DinerMlpShape(self.d_in, self.d_latent, self.d_hidden, self.n_blocks, self.combine_layer, self.num_freqs,
                                  float(self.beta), 4, 0)


STANDARD_SHAPE = MlpShape(55, 512, 512, 5, 3, 6, 0.0)


class _Route(NamedTuple):
    """What one inference call runs, settled once per call from (model, f16_ok) by ``NeRFRendererDGS._resolve``."""
    shape: MlpShape
    gen: bool                      # a shape-general kernel (the *_gen entry points), else the 512-wide ones
    f16: bool                      # ... its split-fp16 form
    lookup: object                 # the latent lookup: None (bilinear / border), a DinerLatentIndex, or the int padding of a bicubic one
    effective_precision: str
    stem: str                      # last_route, short of the "_lz" of a call that read lin_z maps

    @property
    def op_ok(self) -> bool:
        """the torch_ops binding serves this route (the standard model with the default lookup)"""
        return not self.gen and self.lookup is None


class _Keep(NamedTuple):
    """The tensors a ``DinerScene`` points into (``NeRFRendererDGS._scene``); unused ones are None."""
    maps: torch.Tensor
    poses: torch.Tensor
    focal: torch.Tensor
    c: torch.Tensor
    latent: Optional[torch.Tensor]
    linz: Optional[torch.Tensor]
    linz_gen: Optional[torch.Tensor] = None    # the lin_z maps of a shape-general route


class RenderOutput(dict):
    """Attribute dict standing in for ``dotmap.DotMap`` (reference nerf_renderer.py:421-430)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


class _Sources:
    """Identity + version of the tensors a packed copy was made from (SURVEY.md §8(b) ownership row): weak
    references only, so the cache neither extends a source's lifetime nor can be fooled by address reuse."""

    __slots__ = ("refs", "versions", "shapes")

    def __init__(self, tensors):
        self.refs = [weakref.ref(t) for t in tensors]
        self.versions = [t._version for t in tensors]
        self.shapes = [(tuple(t.shape), t.dtype, t.device) for t in tensors]

    def valid_for(self, tensors) -> bool:
        return len(tensors) == len(self.refs) and all(
            r() is t and v == t._version and sh == (tuple(t.shape), t.dtype, t.device)
            for r, v, sh, t in zip(self.refs, self.versions, self.shapes, tensors))


class _FiniteGuard:
    """The non-finite status of the frames a renderer has issued (its own object so that a ``weakref.finalize`` of the renderer can
    run the last check without keeping the renderer alive).  The compositing kernel ORs DINER_STATUS_NONFINITE into the device word;
    a copy to pinned host memory + an event follow every call; ``poll`` examines the copies that have completed (all, if ``wait``)."""

    unreported = []          # messages of non-finite frames found where nothing could be raised (a finalizer): raised by the next call

    def __init__(self):
        self.status = None   # device int32 word
        self.pending = []    # [(event, pinned host word)] oldest first
        self.free = []       # examined (event, word) pairs, reused by after_launch
        self.precision = "f16x3"

    def word(self, dev):
        if self.status is None or self.status.device != dev:
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self.pending = []
        return self.status

    def message(self):
        return ("diner_amd.NeRFRendererDGS: a rendered rgb-sigma sample was inf/NaN" +
                (" -- in precision='f16x3' an MLP activation left the fp16 range (|x| >= ~1e6, see DESIGN.md); set "
                 "renderer.precision = 'fp32' (exact fp32 MFMA) for this model" if self.precision == "f16x3" else
                 " -- the model itself produces non-finite values for these inputs"))

    def poll(self, wait=False, keep=0):
        """examine the completed copies; with ``wait`` block for all but the ``keep`` youngest; raise if a frame went non-finite"""
        if _FiniteGuard.unreported:
            msg, _FiniteGuard.unreported[:] = _FiniteGuard.unreported[0], []
            raise RuntimeError(msg + " (found when an earlier renderer was collected: its last frames had not been examined)")
        bad = False
        while self.pending and ((wait and len(self.pending) > keep) or self.pending[0][0].query()):
            ev, host = self.pending.pop(0)
            ev.synchronize()
            bad |= bool(int(host[0]) & 1)
            if len(self.free) < 8:
                self.free.append((ev, host))
        if bad:
            self.pending = []
            self.status.zero_()
            raise RuntimeError(self.message())

    def after_launch(self, dev):
        # pinned host words and events are recycled (a pinned allocation per call costs tens of microseconds of host time:
        # 64 calls per 512 x 512 image in the reference's 4096-ray chunks)
        ev, host = self.free.pop() if self.free else (torch.cuda.Event(), torch.empty(1, dtype=torch.int32, pin_memory=True))
        host.copy_(self.status, non_blocking=True)
        ev.record(torch.cuda.current_stream(dev))
        self.pending.append((ev, host))

    def finalize(self):
        """weakref.finalize of the renderer (garbage collection, or interpreter exit): the frames nobody examined.  An exception
        cannot leave a finalizer, so: at interpreter exit the process ends with a non-zero status and the message on stderr; earlier,
        the message is parked and raised by the next call of any renderer."""
        import sys
        if not self.pending:
            return
        try:
            bad = False
            for ev, host in self.pending:
                ev.synchronize()
                bad |= bool(int(host[0]) & 1)
            self.pending = []
        except Exception:      # the HIP runtime is already gone: nothing left to examine with
            return
        if bad:
            if _EXITING[0]:
                sys.stderr.write("RuntimeError: " + self.message() + " (found at interpreter exit: the last frames were never examined; "
                                 "call renderer.check_finite() after the last forward())\n")
                sys.stderr.flush()
                import os
                os._exit(70)
            _FiniteGuard.unreported.append(self.message())


_EXITING = [False]


def _mark_exit():
    _EXITING[0] = True


import atexit  # noqa: E402
# weakref.finalize callbacks run from an atexit hook registered when the FIRST finalize object is created; atexit runs hooks
# last-in-first-out, so this one (registered at import, i.e. before any renderer exists ... but possibly after another module's
# finalize) is re-registered by every renderer constructor to be sure it runs before them
atexit.register(_mark_exit)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class NeRFRendererDGS(torch.nn.Module):
    """NeRF renderer with depth-guided sampling (reference nerf_renderer.py:12-37).

    :param n_samples: samples per ray
    :param n_depth_candidates: stratified candidates that are short-listed by surface likelihood
    :param n_gaussian: samples drawn from the gaussian fitted to the occlusion-aware likelihoods
    :param eval_batch_size: kept for signature compatibility (the fused kernel needs no chunking)
    :param white_bkgd: white instead of black background
    """

    def __init__(self, n_samples=40, n_depth_candidates=1000, n_gaussian=15, eval_batch_size=100000,
                 white_bkgd=True, train_any_shape=False, f16x3_any_shape=False, train_f16x3_any_shape=False, bicubic_index=False,
                 linz_maps_any_shape=False):
        super().__init__()
        self.n_samples = n_samples
        self.n_depth_candidates = n_depth_candidates
        self.n_gaussian = n_gaussian
        self.eval_batch_size = eval_batch_size
        self.white_bkgd = white_bkgd
        self.seed = 0            # base seed of the in-kernel Philox generator (perf mode)
        # arithmetic of the fusion-MLP GEMMs (build-only extra): "f16x3" = fp32 operands split into fp16
        # hi+lo, 3 fp16 MFMAs per product, fp32 accumulate (fp32-grade, ~3x faster); "fp32" = fp32 MFMA
        self.precision = "f16x3"
        # profiling hook (bench.py): when a list, forward() launches the three stage kernels through
        # their own C-ABI entry points (exactly what diner_render does internally) and appends
        # (ev0, ev1, ev2, ev3) torch.cuda.Events bracketing sampler | points+MLP | compositing
        self.stage_events = None
        self._calls = 0
        self._maps_key = self._maps_pack = None      # packed depth/sigma/normal maps + cameras
        self._latent_key = self._latent_pack = None  # packed NHWC latent
        self._latent_shared = False                  # the pack IS encoder.latent's storage (glue.assemble_latent's layout)
        self._linz_key = self._linz_pack = None      # lin_z[b](latent) feature maps (f16x3 mode)
        # f16x3 mode: hoist lin_z from per point to per latent texel (linear map and bilinear interpolation
        # commute; diner_pack_linz_maps).  Costs 3x the latent's memory per encode(); set False to keep
        # lin_z as per-point GEMMs.
        # Binding of the two whole-path entry points: "torch_ops" = torch.ops.diner.render / render_image (diner_amd/ops.py, the
        # torch C++ extension north_star names), "ctypes" = the C ABI directly.  Same C functions either way; the build-only
        # arguments (replayed noise, stage events) always take the ctypes route.  Default: the ops when the extension is built.
        from . import ops as _ops
        self.binding = "torch_ops" if _ops.available() else "ctypes"
        self.linz_maps = True
        # Memory budget of that hoist: the lin_z maps are 3x the latent (2.5 GB at the headline config, 16 GB for a 1024^2 x 8-view
        # encode).  Above this many bytes the maps are NOT built and lin_z stays a per-point gather + GEMM (the kernel's LINZ = false
        # instantiation: same results, ~1.3x the frame time); None = no limit.  See memory_report().
        self.linz_maps_max_bytes = 64 << 30
        # informational (bench.py's executed-FLOP count): the f16x3 kernel applies block 2's fc_1 once to the mean over views
        self.fc1_on_mean = True
        self._mlp_key = None
        self._mlp_pack = None
        # Models of any other shape (MlpShape) run on the shape-general fp32 kernel (points_mlp_gen.hip) through the *_gen entry
        # points, always through ctypes.  After every inference call: `last_route` = the point kernel that ran ("points_mlp_f16",
        # "points_mlp", "points_mlp_gen" or "points_mlp_gen_f16", with "_lz" appended when linz_maps_any_shape's maps were read), `last_binding` = "torch_ops" or "ctypes", `effective_precision` = the arithmetic that ran.
        self._mlp_gen_key = self._mlp_gen_pack = None
        self.last_route = self.last_binding = self.effective_precision = None
        self.last_box_hits = None     # after render_image(bounds=...): the number of rays rendered per scene (a list of ints)
        self._warned_precision = False
        self._force_gen = False      # test-only: run the standard shape on the shape-general kernel as well
        # Training (autograd through forward() / composite()) of a model of any shape of the shape-general envelope: the exact fp32
        # path of diner_amd/training_gen.py (last_route "train_gen").  Opt-in: when False a non-standard model under autograd raises,
        # as before.  A plain attribute, so that a config can set it (renderer.kwargs.train_any_shape).
        self.train_any_shape = bool(train_any_shape)
        self._force_gen_train = False   # test-only: train the standard shape on that path as well
        # Inference of a non-standard model in f16x3: with precision == "f16x3" such a model takes the shape-general split-fp16 kernel
        # (points_mlp_gen_f16.hip, last_route "points_mlp_gen_f16", effective_precision "f16x3", no warning) instead of the exact fp32
        # one.  Opt-in: when False the model runs in fp32 behind the precision warning, as before.  The standard model keeps its own
        # kernels and training stays exact fp32 either way.  A plain attribute, so that a config can set it
        # (renderer.kwargs.f16x3_any_shape).
        self.f16x3_any_shape = bool(f16x3_any_shape)
        self._mlp_gen_f16_key = self._mlp_gen_f16_pack = None
        # Training of a non-standard model in f16x3: together with train_any_shape and precision == "f16x3" the shape-general training
        # path runs its GEMMs in the split-fp16 arithmetic of the standard path (csrc/train_gen_f16.hip, last_route "train_gen_f16",
        # effective_precision "f16x3", no warning) instead of exact fp32.  Opt-in: when False that path trains in fp32 behind the
        # precision warning, as before.  A plain attribute, so that a config can set it (renderer.kwargs.train_f16x3_any_shape).
        self.train_f16x3_any_shape = bool(train_f16x3_any_shape)
        # An encoder with index_interp="bicubic" (grid_sample's 16-tap lookup, any index_padding): such a model of ANY shape, the standard
        # one included, is routed like a non-standard shape -- inference on the shape-general kernels' bicubic compilations
        # (points_mlp_gen_bc.hip / points_mlp_gen_f16_bc.hip: last_route "points_mlp_gen" / "points_mlp_gen_f16" under f16x3_any_shape),
        # training on diner_amd/training_gen.py (needs train_any_shape; train_f16x3_any_shape for f16x3).  The 512-wide kernels and the
        # lin_z maps do not serve bicubic.  Opt-in: when False a bicubic model raises, as before (the static _validate_model always
        # does).  A plain attribute, so that a config can set it (renderer.kwargs.bicubic_index).
        self.bicubic_index = bool(bicubic_index)
        # lin_z hoisted into per-texel maps for the models of the shape-general inference routes (any shape, any lookup mode, bicubic
        # included; both precisions): outside autograd such a model's maps M_b = lin_z[b].weight . latent (no bias; csrc/linz_maps_gen.hip)
        # are built once per encode() and weight version, and the point kernels' lin_z-map forms (last_route "points_mlp_gen_lz" /
        # "points_mlp_gen_f16_lz") gather d_hidden channels of them instead of gathering d_latent channels and multiplying per point,
        # view and block.  Costs min(combine_layer, n_blocks) * d_hidden / d_latent times the latent's memory, within
        # linz_maps_max_bytes (above it: no maps, the route without them, silently); see memory_report().  Opt-in: when False nothing
        # changes.  The standard model keeps its own kernels and maps; training builds none.  A plain attribute, so that a config can
        # set it (renderer.kwargs.linz_maps_any_shape).
        self.linz_maps_any_shape = bool(linz_maps_any_shape)
        self._linz_gen_key = self._linz_gen_pack = None
        from .training_gen import WeightSplitCache
        self._weight_split_cache = WeightSplitCache()   # that path's pre-split weights, per parameter version
        # render_image under autograd: rays per chunk of its backward, which re-runs the training path chunk by chunk (peak memory = one
        # chunk's training footprint + the frame's saved rays, samples and outputs).  A plain attribute, so that a config can set it.
        self.grad_chunk_rays = 4096
        self._latent_gen = self._mlp_gen = 0         # bumped by every re-pack; the lin_z maps depend on both
        # Non-finite guard.  The compositing kernel ORs DINER_STATUS_NONFINITE into a device word when an rgb-sigma
        # sample is inf/NaN (in f16x3 mode: an MLP activation beyond the fp16 range, |x| >= ~1e6).  The word is copied
        # to pinned host memory behind every call.  No frame can leave a program unexamined:
        #   * a call that carries more than `finite_sync_rays` rays (anything larger than the reference's 4096-ray chunk:
        #     a whole image / a large batch) or asks for the weights is examined before forward() returns (the wait is
        #     microseconds against >= 30 ms of rendering); render_image always is;
        #   * smaller chunks ("deferred"): forward() examines every copy that has completed and blocks only for frames
        #     older than the two youngest -- the host never stalls the GPU, and at most two chunks are unexamined at any time;
        #   * those last chunks are examined by check_finite(), by the next call of any renderer, and by a weakref.finalize of
        #     this module: at garbage collection the finding is raised by the next call, at interpreter exit the process ends
        #     with status 70 and the message on stderr (tests/test_gpu_edge.py).
        # "sync" waits at the end of every call; "off" never looks.
        self.finite_check = "deferred"
        self.finite_sync_rays = 4096
        self._guard = _FiniteGuard()
        atexit.unregister(_mark_exit)
        self._finalizer = weakref.finalize(self, self._guard.finalize)   # (registers weakref's own atexit hook the first time)
        atexit.register(_mark_exit)                  # ... and this one after it: atexit is LIFO, so the flag is set before the finalizers run

    # ------------------------------------------------------------------------------------------
    # model -> packed device state (cached)
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _validate_model(model) -> MlpShape:
        """The shape of ``model``'s fusion MLP and encodings; raises ``NotImplementedError`` naming what lies outside what the kernels
        serve: the standard shape (the 512-wide kernels) and the envelope of the shape-general kernel (include/diner_hip.h)."""
        NeRFRendererDGS._latent_index(model)
        return NeRFRendererDGS._validate_shape(model)

    @staticmethod
    def _validate_shape(model) -> MlpShape:
        """_validate_model without the latent lookup's check"""
        mlp = model.mlp_fine
        if getattr(mlp, "combine_type", "average") != "average":
            raise NotImplementedError(f"only combine_type='average' (resnetfc.py:9-14), not {mlp.combine_type!r}")
        act = getattr(mlp, "activation", torch.nn.ReLU())
        if isinstance(act, torch.nn.ReLU):
            beta = 0.0
        elif isinstance(act, torch.nn.Softplus) and act.beta > 0 and act.threshold == 20:
            beta = float(act.beta)
        else:
            raise NotImplementedError(f"activation {act!r} unsupported: ReLU or Softplus(beta > 0, threshold=20) (resnetfc.py:124-127)")
        for blk in getattr(mlp, "blocks", []):
            ba = getattr(blk, "activation", None)
            if ba is not None and (type(ba) is not type(act) or getattr(ba, "beta", None) != getattr(act, "beta", None)):
                raise NotImplementedError("every ResnetBlockFC must use the ResnetFC's activation (resnetfc.py:49-52, 117-119)")
        if mlp.d_out != 4:
            raise NotImplementedError(f"fusion MLP d_out={mlp.d_out} unsupported (PixelNeRF's head is rgb + sigma: 4)")
        poscode, depthcode = model.poscode, model.depthcode
        for pe in (poscode, depthcode):
            if not pe.include_input:
                raise NotImplementedError("positional encoding must have include_input=True")
        F = int(poscode.num_freqs)
        if int(depthcode.num_freqs) != F or float(depthcode.freqs[0]) != float(poscode.freqs[0]):
            raise NotImplementedError("poscode and depthcode must share num_freqs and freq_factor (pixelnerf.py:14-15)")
        shape = MlpShape(int(mlp.d_in), int(mlp.d_latent), int(mlp.d_hidden), int(mlp.n_blocks), int(mlp.combine_layer), F, beta)
        if shape.standard:
            return shape
        why = []
        if not (32 <= shape.d_hidden <= 512 and shape.d_hidden % 32 == 0):
            why.append(f"d_hidden={shape.d_hidden} (a multiple of 32 in [32, 512])")
        if not (8 <= shape.d_latent <= 1024 and shape.d_latent % 8 == 0):
            why.append(f"d_latent={shape.d_latent} (a multiple of 8 in [8, 1024])")
        if not 1 <= shape.n_blocks <= 64:
            why.append(f"n_blocks={shape.n_blocks} (1..64)")
        if shape.combine_layer < 0:
            why.append(f"combine_layer={shape.combine_layer} (>= 0)")
        if not (F >= 1 and 7 + 8 * F <= 512):
            why.append(f"num_freqs={F} (1..63)")
        elif shape.d_in != 7 + 8 * F:
            why.append(f"d_in={shape.d_in} (PixelNeRF: 7 + 8 * num_freqs = {7 + 8 * F})")
        if why:
            raise NotImplementedError("fusion MLP shape outside what the kernels serve: " + "; ".join(why) +
                                      f" (standard shape {tuple(STANDARD_SHAPE)[:6]} or the shape-general envelope, include/diner_hip.h)")
        return shape

    @staticmethod
    def _latent_index(model) -> Optional[_lib.DinerLatentIndex]:
        """The encoder's latent lookup (SpatialEncoder index_interp / index_padding, image_encoder.py:24-25,119-125): None for the
        default bilinear / border (the entry points and torch ops without _ix), else the DinerLatentIndex of the _ix entry points.
        Raises ``NotImplementedError`` for a mode these entry points do not serve; bicubic is one: it has entry points of its own,
        behind the renderer's ``bicubic_index`` switch (``_validate``)."""
        enc = model.encoder              # (one attribute lookup on the module: this runs several times per call)
        interp = getattr(enc, "index_interp", "bilinear")
        padding = getattr(enc, "index_padding", "border")
        if interp not in _lib.INDEX_INTERP or padding not in _lib.INDEX_PADDING:
            raise NotImplementedError(f"latent lookup index_interp={interp!r}, index_padding={padding!r} unsupported: index_interp in "
                                      f"{sorted(_lib.INDEX_INTERP)}, index_padding in {sorted(_lib.INDEX_PADDING)} (image_encoder.py:24-25); "
                                      "index_interp='bicubic' is served by a renderer constructed with bicubic_index=True "
                                      "(renderer.kwargs.bicubic_index: the shape-general kernels' 16-tap lookup)")
        if interp == "bilinear" and padding == "border":
            return None
        return _lib.DinerLatentIndex(_lib.INDEX_INTERP[interp], _lib.INDEX_PADDING[padding])

    def _bicubic_pad(self, model) -> Optional[int]:
        """the DINER_INDEX_PAD_* of ``model``'s lookup when it is bicubic and this renderer serves it (``bicubic_index``), else None.
        Read from the model wherever the routing needs it: no call depends on which model another call saw."""
        if model is None or not self.bicubic_index or getattr(model.encoder, "index_interp", "bilinear") != "bicubic":
            return None
        return _lib.INDEX_PADDING.get(getattr(model.encoder, "index_padding", "border"))

    def _validate(self, model) -> MlpShape:
        """_validate_model for this renderer's routing: with ``bicubic_index`` an encoder with index_interp="bicubic" and any of the
        three paddings is accepted and takes the shape-general routes"""
        if self._bicubic_pad(model) is not None:
            return self._validate_shape(model)
        return self._validate_model(model)

    def _index(self, model) -> Optional[_lib.DinerLatentIndex]:
        """_latent_index of ``model``; None for a bicubic one this renderer serves (``_bicubic_pad`` has its padding)"""
        return None if self._bicubic_pad(model) is not None else self._latent_index(model)

    def _needs_gen(self, shape: MlpShape, model=None) -> bool:
        """``model`` has no 512-wide kernel: another shape than the standard one, or the bicubic lookup"""
        return not shape.standard or self._bicubic_pad(model) is not None

    def _resolve(self, model, f16_ok=True, stacklevel=4) -> _Route:
        """validate ``model`` and settle what an inference call on it runs (``_Route``): the kernel family, the precision (a shape-general
        route is exact fp32, said once, unless f16x3_any_shape sends this call -- ``f16_ok`` -- to the split-fp16 kernel) and the latent
        lookup.  Every predicate is asked through ``self``, once.  ``stacklevel``: the precision warning's, as ``_settle_fp32`` takes it
        (4: the line that called this method's caller, i.e. the user's line behind a public door)"""
        shape = self._validate(model)
        pad = self._bicubic_pad(model)
        lookup = int(pad) if pad is not None else self._latent_index(model)
        gen = self._use_gen(shape, model)
        f16 = bool(gen and f16_ok and self._use_gen_f16(shape, model))
        if gen and not f16:
            self._settle_fp32(shape, stacklevel=stacklevel)
        prec = "f16x3" if f16 else "fp32" if gen else self.precision
        stem = self._gen_route(f16, None) if gen else "points_mlp_f16" if prec == "f16x3" else "points_mlp"
        return _Route(shape, gen, f16, lookup, prec, stem)

    def _route(self, model, f16_ok=True) -> MlpShape:
        """``_resolve`` for the callers that want the shape alone: ``effective_precision`` is set, the shape returned"""
        route = self._resolve(model, f16_ok, stacklevel=5)
        self.effective_precision = route.effective_precision
        return route.shape

    def _settle_fp32(self, shape: MlpShape, stacklevel=3):
        """the shape-general paths run in exact fp32: say so once when another precision was asked for"""
        if self.precision != "fp32" and not self._warned_precision:
            warnings.warn(f"diner_amd.NeRFRendererDGS: precision={self.precision!r} is available for the standard model only; "
                          f"the fusion MLP {tuple(shape)} runs in exact fp32 (renderer.effective_precision)", stacklevel=stacklevel)
            self._warned_precision = True
        self.effective_precision = "fp32"

    def _use_gen(self, shape: MlpShape, model=None) -> bool:
        return self._force_gen or self._needs_gen(shape, model)

    def _use_gen_f16(self, shape: MlpShape, model=None) -> bool:
        """inference of a non-standard model on the shape-general f16x3 kernel (f16x3_any_shape) instead of the fp32 one"""
        return bool(self.f16x3_any_shape) and self.precision == "f16x3" and self._needs_gen(shape, model) and not self._force_gen

    def _gen_entry(self, name: str, f16: bool):
        """the C entry point ``diner_<name>`` of the shape-general path, its _f16 form for the split-fp16 kernel: -> (function, its name)"""
        full = "diner_" + (name.replace("_gen", "_gen_f16") if f16 else name)
        return getattr(_lib.lib(), full), full

    def _entry(self, route: _Route, stem: str, lz, sc: DinerScene, packed, a: tuple, b: tuple, scratch=None):
        """The C entry point of ``stem`` ("render_points", "render" or "render_image") on ``route`` -> (function, its name for check(),
        its argument list).  ``a`` and ``b`` are the stem's own arguments; what depends on the route goes around them:

            standard                  diner_<stem>[_ix]                 (sc, [&index,] packed, *a, precision, [scratch,] *b)
            shape-general             diner_<stem>_gen[_f16][_ix|_bc]   (sc, [&index | padding,] &shape, packed, *a, *b)
            ... with lin_z maps lz    diner_<stem>_gen_lz               (sc, &index | NULL, &shape, packed, *a, *b, precision, padding | -1, lz)

        (``scratch`` is the point stage's, of the standard kernels only.)"""
        look = route.lookup
        bicubic = isinstance(look, int)
        prec = _lib.PRECISIONS[route.effective_precision]
        if not route.gen:
            full = "diner_" + stem + ("_ix" if look is not None else "")
            head = () if look is None else (C.byref(look),)
            mid, tail = ((prec, _ptr(scratch)) if stem == "render_points" else (prec,)), ()
        else:
            if lz is not None:    # one entry point for both precisions and every lookup
                full = "diner_" + stem + "_gen_lz"
                head = (None if bicubic or look is None else C.byref(look),)
                tail = (prec, look if bicubic else -1, _ptr(lz))
            else:
                full = "diner_" + stem + ("_gen_f16" if route.f16 else "_gen") + ("" if look is None else "_bc" if bicubic else "_ix")
                head = () if look is None else (look if bicubic else C.byref(look),)
                tail = ()
            head, mid = (*head, C.byref(route.shape.c_struct())), ()
        return getattr(_lib.lib(), full), full, (C.byref(sc), *head, _ptr(packed), *a, *mid, *b, *tail)

    def _gen_lookup(self, name: str, f16: bool, model):
        """a view of ``_entry`` kept for the host tests that predate it: the shape-general entry point ``diner_<name>`` (``name`` ends
        in "_gen") for ``model``'s lookup -> (function, its name, the arguments between the scene and the shape)"""
        pad = self._bicubic_pad(model)
        route = _Route(STANDARD_SHAPE, True, f16, int(pad) if pad is not None else self._latent_index(model), "fp32", "")
        fn, full, args = self._entry(route, name[:-len("_gen")], None, DinerScene(), None, (), ())
        return fn, full, args[1:-2]

    @staticmethod
    def _gen_route(f16: bool, lz) -> str:
        return ("points_mlp_gen_f16" if f16 else "points_mlp_gen") + ("_lz" if lz is not None else "")

    def _linz_gen_wanted(self, shape: MlpShape) -> bool:
        """this call reads lin_z maps of a shape-general route, if they fit: the switch is on, grad mode is off (even when nothing
        requires grad) and the shape has a lin_z layer"""
        return bool(self.linz_maps_any_shape) and not torch.is_grad_enabled() and min(shape.combine_layer, shape.n_blocks) > 0

    def _linz_maps_gen(self, shape: MlpShape, sc: DinerScene, latent: torch.Tensor) -> Optional[torch.Tensor]:
        """the lin_z maps of a shape-general inference route (``linz_maps_any_shape``): a single cached entry, rebuilt when the latent
        pack or an MLP pack was rebuilt; None (the route without maps) when the switch is off, grad mode is involved, the shape has no
        lin_z layer or the maps exceed ``linz_maps_max_bytes``"""
        if not self._linz_gen_wanted(shape):
            return None
        cs = shape.c_struct()
        n = int(_lib.lib().diner_linz_maps_gen_floats(C.byref(sc), C.byref(cs)))
        if n < 0:
            check(n, "diner_linz_maps_gen_floats")
        if n == 0 or (self.linz_maps_max_bytes is not None and 4 * n > self.linz_maps_max_bytes):
            return None
        packed = self._mlp_gen_pack       # the fp32 image: one exact fp32 builder serves both precisions
        key = (self._latent_gen, self._mlp_gen, shape)
        if key != self._linz_gen_key:
            dev = latent.device
            self._linz_gen_pack = self._linz_gen_key = None    # (never both generations at once)
            out = torch.empty(n, dtype=torch.float32, device=dev)
            check(_lib.lib().diner_pack_linz_maps_gen(C.byref(sc), C.byref(cs), _ptr(packed), _ptr(out), _stream(dev)), "diner_pack_linz_maps_gen")
            self._linz_gen_pack, self._linz_gen_key = out, key
        return self._linz_gen_pack

    def _use_gen_train(self, shape: MlpShape, model=None) -> bool:
        return self._force_gen_train or (self.train_any_shape and self._needs_gen(shape, model))

    def _use_gen_train_f16(self, shape: MlpShape, model=None) -> bool:
        """the shape-general training path in f16x3 (train_f16x3_any_shape) instead of exact fp32"""
        return self._use_gen_train(shape, model) and bool(self.train_f16x3_any_shape) and self.precision == "f16x3"

    def _gen_training_unsupported(self, shape: MlpShape, model=None):
        what = f"the shape {tuple(shape)}" + (" with index_interp='bicubic'" if self._bicubic_pad(model) is not None else "")
        raise NotImplementedError(f"training (autograd through the renderer) supports the standard fusion MLP {tuple(STANDARD_SHAPE)[:6]} "
                                  f"with a bilinear / nearest lookup only unless train_any_shape is set; {what} is supported for inference: call it under "
                                  "torch.no_grad() or with parameters that do not require grad, or construct the renderer with "
                                  "train_any_shape=True (renderer.train_any_shape: the shape-general fp32 training path)")

    def _scene(self, model, need_latent=True, packed_mlp=None, gen_shape: Optional[MlpShape] = None) -> Tuple[DinerScene, _Keep]:
        """``gen_shape``: the call is a shape-general inference route's (its fp32 MLP image is packed): ``linz_gen`` of the tensors
        returned is then that route's lin_z maps, or None (``_linz_maps_gen``)"""
        enc = model.encoder
        dev = enc.depths.device
        msrc = [model.poses, model.focal, model.c, model.image_shape, enc.depths, enc.depths_std, enc.normals]
        if self._maps_key is None or not self._maps_key.valid_for(msrc):
            SB, NV, _, H, W = enc.depths.shape
            maps = torch.empty((SB, NV, H, W, 8), dtype=torch.float32, device=dev)
            d, s, n = _f32c(enc.depths), _f32c(enc.depths_std), _f32c(enc.normals)
            check(_lib.lib().diner_pack_maps(_ptr(d), _ptr(s), _ptr(n), SB * NV, H, W, _ptr(maps), _stream(dev)),
                  "diner_pack_maps")
            poses = _f32c(model.poses)
            if poses.shape[-2:] != (4, 4):  # accept [.., 3, 4] poses
                full = torch.zeros((*poses.shape[:-2], 4, 4), dtype=torch.float32, device=dev)
                full[..., :3, :] = poses[..., :3, :]
                full[..., 3, 3] = 1
                poses = full.contiguous()
            torch.cuda.current_stream(dev).synchronize()  # d/s/n may be temporaries
            ishape = [float(v) for v in model.image_shape.detach().float().cpu()]  # (W, H), pixelnerf.py:50-51
            self._maps_pack, self._maps_key = (maps, poses, _f32c(model.focal), _f32c(model.c), ishape), _Sources(msrc)
        if need_latent:
            if self._latent_key is None or not self._latent_key.valid_for([enc.latent]):
                if latent_is_packed(enc.latent):   # glue.assemble_latent's layout: the latent's own buffer is the pack (no copy)
                    latent = enc.latent.detach().permute(0, 1, 3, 4, 2)
                else:
                    lat = _f32c(enc.latent)
                    SB, NV, Cc, h, w = lat.shape
                    latent = torch.empty((SB, NV, h, w, Cc), dtype=torch.float32, device=dev)
                    check(_lib.lib().diner_pack_latent(_ptr(lat), SB * NV, Cc, h, w, _ptr(latent), _stream(dev)),
                          "diner_pack_latent")
                    torch.cuda.current_stream(dev).synchronize()
                self._latent_pack, self._latent_key = latent, _Sources([enc.latent])
                self._latent_shared = latent.data_ptr() == enc.latent.data_ptr()   # (memory_report: one buffer, not two)
                self._latent_gen += 1
        maps, poses, focal, c, ishape = self._maps_pack
        latent = self._latent_pack if need_latent else None
        linz = None
        ix = self._index(model)      # (a bicubic model never comes with packed_mlp: no lin_z maps are built for it)
        ring = 2 if ix is not None and ix.padding == _lib.INDEX_PADDING["zeros"] else 0   # zeros padding: the ringed maps
        linz_bytes = 3 * latent.numel() // (latent.shape[2] * latent.shape[3]) * (latent.shape[2] + ring) * (latent.shape[3] + ring) * 4 \
            if latent is not None else 0
        if (need_latent and packed_mlp is not None and self.linz_maps and self.precision == "f16x3"
                and (self.linz_maps_max_bytes is None or linz_bytes <= self.linz_maps_max_bytes)):
            # generations of the two packs the maps were computed from, and the lookup mode (zeros padding: other maps)
            zkey = (self._latent_gen, self._mlp_gen, None if ix is None else (ix.interp, ix.padding))
            if zkey != self._linz_key:
                SB, NV, h, w, Cc = latent.shape
                if ix is None:
                    out = torch.empty((3, SB, NV, h, w, Cc), dtype=torch.float32, device=dev)
                    check(_lib.lib().diner_pack_linz_maps(_ptr(latent), SB * NV, h, w, _ptr(packed_mlp), _ptr(out), _stream(dev)),
                          "diner_pack_linz_maps")
                else:
                    out = torch.empty((3, SB, NV, h + ring, w + ring, Cc), dtype=torch.float32, device=dev)
                    assert out.numel() == int(_lib.lib().diner_linz_maps_floats(SB * NV, h, w, C.byref(ix)))
                    check(_lib.lib().diner_pack_linz_maps_ix(_ptr(latent), SB * NV, h, w, _ptr(packed_mlp), C.byref(ix), _ptr(out),
                                                             _stream(dev)), "diner_pack_linz_maps_ix")
                self._linz_pack, self._linz_key = out, zkey
            linz = self._linz_pack
        SB, NV, H, W, _ = maps.shape
        sc = DinerScene()
        sc.SB, sc.NV, sc.H, sc.W = SB, NV, H, W
        if latent is not None:
            assert latent.shape[:2] == (SB, NV)  # image_encoder.py:105
            sc.h, sc.w, sc.C = latent.shape[2], latent.shape[3], latent.shape[4]
        sc.image_w, sc.image_h = ishape
        sc.feature_padding = float(model.encoder.feature_padding)
        sc.num_freqs = int(model.poscode.num_freqs)
        sc.freq_factor = float(model.poscode.freqs[0])
        sc.poses, sc.focal, sc.c = poses.data_ptr(), focal.data_ptr(), c.data_ptr()
        sc.maps = maps.data_ptr()
        sc.latent = latent.data_ptr() if latent is not None else None
        sc.linz_maps = linz.data_ptr() if linz is not None else None
        return sc, _Keep(maps, poses, focal, c, latent, linz, None if gen_shape is None else self._linz_maps_gen(gen_shape, sc, latent))

    def memory_report(self, model=None, rays_per_call=None, n_views=None):
        """Bytes of device memory this renderer holds / will take, so that the appetite is a number and not a surprise:
        ``cached`` = what the pack caches hold right now (packed maps, NHWC latent, lin_z maps, packed MLP; ``latent_zero_copy``: the NHWC
        latent is the model's own buffer, glue.assemble_latent's, and no second copy exists); with ``rays_per_call``
        (and ``n_views``, default: the cached scene's) also ``per_call`` = workspace + outputs of one inference ``forward`` and
        ``training_step`` = the activations the differentiable path keeps alive between forward and backward
        (diner_amd/training.py: every layer's input in fp32, 24 GB for 4096 rays x 40 samples x 4 views)."""
        nb = lambda t: 0 if t is None else t.numel() * t.element_size()
        maps = self._maps_pack[0] if self._maps_pack is not None else None
        rep = {"cached": {"maps": nb(maps), "latent_nhwc": nb(self._latent_pack), "linz_maps": nb(self._linz_pack), "mlp_packed": nb(self._mlp_pack),
                         "mlp_gen_packed": nb(self._mlp_gen_pack), "mlp_gen_f16_packed": nb(self._mlp_gen_f16_pack),
                         # the lin_z maps of a shape-general route (linz_maps_any_shape): nlz * d_hidden / d_latent times the latent
                         "linz_maps_gen": nb(self._linz_gen_pack)}}
        rep["cached"]["total"] = sum(rep["cached"].values())
        # a latent in glue.assemble_latent's layout is counted once: "latent_nhwc" is then encoder.latent's own storage, not a second copy
        rep["latent_zero_copy"] = bool(self._latent_shared and self._latent_pack is not None)
        rep["linz_maps_max_bytes"] = self.linz_maps_max_bytes
        bicubic = self._bicubic_pad(model) is not None
        rep["bicubic_index"] = bicubic       # such a model builds no lin_z maps and keeps 16-float tap records per (view, point) row
        if rays_per_call is not None:
            NV = n_views if n_views is not None else (maps.shape[1] if maps is not None else 1)
            K, P = int(self.n_samples), int(rays_per_call) * int(self.n_samples)
            ws = int(_lib.lib().diner_render_workspace_floats(1, int(rays_per_call), K, NV, _lib.PRECISIONS[self.precision])) * 4
            rep["per_call"] = {"workspace": ws, "outputs": int(rays_per_call) * (4 + K) * 4}
            rows = NV * P
            # forward keeps: in56 + zlat + taps per (view, point); x, net of the 3 per-view blocks; the post-mean tensors per point
            rep["training_step"] = {"per_view_rows": rows,
                                    "saved_activations": rows * 4 * (56 + 512 + (16 if bicubic else 8) + 2 * 3 * 512) + P * 4 * (2 * 2 * 512 + 512 + 4),
                                    "note": "peak = saved activations + ~8 row-matrices [rows,512] fp32 of forward/backward temporaries "
                                            "(measured: 24.5 GB at 4096 rays x 40 samples x 4 views, tools/bench_train.py)"}
        return rep

    def _mlp(self, model) -> torch.Tensor:
        mlp = model.mlp_fine
        params = [mlp.lin_in.weight, mlp.lin_in.bias, mlp.lin_out.weight, mlp.lin_out.bias]
        for b in range(3):
            params += [mlp.lin_z[b].weight, mlp.lin_z[b].bias]
        for b in range(5):
            params += [mlp.blocks[b].fc_0.weight, mlp.blocks[b].fc_0.bias, mlp.blocks[b].fc_1.weight, mlp.blocks[b].fc_1.bias]
        if self._mlp_key is None or not self._mlp_key.valid_for(params):
            keep = [_f32c(p) for p in params]
            raw = DinerMlpRaw()
            raw.lin_in_w, raw.lin_in_b, raw.lin_out_w, raw.lin_out_b = [t.data_ptr() for t in keep[:4]]
            for b in range(3):
                raw.lin_z_w[b], raw.lin_z_b[b] = keep[4 + 2 * b].data_ptr(), keep[5 + 2 * b].data_ptr()
            for b in range(5):
                o = 10 + 4 * b
                raw.fc0_w[b], raw.fc0_b[b] = keep[o].data_ptr(), keep[o + 1].data_ptr()
                raw.fc1_w[b], raw.fc1_b[b] = keep[o + 2].data_ptr(), keep[o + 3].data_ptr()
            dev = keep[0].device
            packed = torch.empty(int(_lib.lib().diner_mlp_packed_floats()), dtype=torch.float32, device=dev)
            check(_lib.lib().diner_pack_mlp(C.byref(raw), _ptr(packed), _stream(dev)), "diner_pack_mlp")
            torch.cuda.current_stream(dev).synchronize()  # `keep` may be temporaries: finish before they die
            self._mlp_pack, self._mlp_key = packed, _Sources(params)
            self._mlp_gen += 1
        return self._mlp_pack

    def _gen_packs(self, model, shape: MlpShape, f16: bool) -> Tuple[torch.Tensor, Optional[MlpShape]]:
        """the packed MLP image of a shape-general inference call and the ``gen_shape`` argument of its ``_scene``: with
        ``linz_maps_any_shape`` (outside grad mode, a shape with lin_z layers) the fp32 image is packed as well, for the map builder"""
        lz = self._linz_gen_wanted(shape)
        if lz and f16:
            self._mlp_shape_general(model, shape, False)
        return self._mlp_shape_general(model, shape, f16), (shape if lz else None)

    def _mlp_shape_general(self, model, shape: MlpShape, f16=False) -> torch.Tensor:
        """the packed image of diner_pack_mlp_gen (``f16``: of diner_pack_mlp_gen_f16, in a cache of its own), cached like _mlp() (and
        on the shape)"""
        mlp = model.mlp_fine
        nlz = min(shape.combine_layer, shape.n_blocks)
        params = [mlp.lin_in.weight, mlp.lin_in.bias, mlp.lin_out.weight, mlp.lin_out.bias]
        for b in range(nlz):
            params += [mlp.lin_z[b].weight, mlp.lin_z[b].bias]
        for b in range(shape.n_blocks):
            params += [mlp.blocks[b].fc_0.weight, mlp.blocks[b].fc_0.bias, mlp.blocks[b].fc_1.weight, mlp.blocks[b].fc_1.bias]
        key = self._mlp_gen_f16_key if f16 else self._mlp_gen_key
        if key is None or key[0] != shape or not key[1].valid_for(params):
            keep = [_f32c(p) for p in params]
            ptrs = [t.data_ptr() for t in keep]
            arr = lambda xs: (C.c_void_p * max(1, len(xs)))(*xs)
            lz, blk = ptrs[4:4 + 2 * nlz], ptrs[4 + 2 * nlz:]
            arrays = [arr(lz[0::2]), arr(lz[1::2]), arr(blk[0::4]), arr(blk[1::4]), arr(blk[2::4]), arr(blk[3::4])]
            pp = lambda a: C.cast(a, C.POINTER(C.c_void_p))
            raw = _lib.DinerMlpGenRaw(ptrs[0], ptrs[1], *[pp(a) for a in arrays], ptrs[2], ptrs[3])
            cs = shape.c_struct()
            size_fn, size_name = self._gen_entry("mlp_gen_packed_floats", f16)
            pack_fn, pack_name = self._gen_entry("pack_mlp_gen", f16)
            n = int(size_fn(C.byref(cs)))
            if n < 0:
                check(n, size_name)
            dev = keep[0].device
            packed = torch.empty(n, dtype=torch.float32, device=dev)
            check(pack_fn(C.byref(cs), C.byref(raw), _ptr(packed), _stream(dev)), pack_name)
            torch.cuda.current_stream(dev).synchronize()  # `keep` may be temporaries: finish before they die
            if f16:
                self._mlp_gen_f16_pack, self._mlp_gen_f16_key = packed, (shape, _Sources(params))
            else:
                self._mlp_gen_pack, self._mlp_gen_key = packed, (shape, _Sources(params))
            self._mlp_gen += 1
        return self._mlp_gen_f16_pack if f16 else self._mlp_gen_pack

    # ------------------------------------------------------------------------------------------
    # non-finite guard
    # ------------------------------------------------------------------------------------------
    def _status_word(self, dev) -> Optional[torch.Tensor]:
        if self.finite_check == "off":
            return None
        return self._guard.word(dev)

    def _poll_status(self, wait=False, keep=0):
        """Examine the completed status copies (all but the ``keep`` youngest if ``wait``); raise if a frame went non-finite."""
        self._guard.precision = self.precision
        self._guard.poll(wait=wait, keep=keep)

    def _after_launch(self, dev, sync=False):
        if self._guard.status is None or self.finite_check == "off":
            return
        self._guard.after_launch(dev)
        if sync or self.finite_check == "sync":
            self._poll_status(wait=True)
        else:
            self._poll_status(wait=True, keep=2)     # never more than two small chunks unexamined; no stall: the GPU is two calls ahead

    def check_finite(self):
        """Wait for every render issued so far and raise ``RuntimeError`` if one produced inf/NaN samples."""
        self._poll_status(wait=True)

    @staticmethod
    def _check_rays(rays):
        assert len(rays.shape) == 3 and rays.shape[-1] == 8  # nerf_renderer.py:412
        if not rays.is_cuda:
            raise RuntimeError("diner_amd.NeRFRendererDGS runs on the GPU only (rays are on %s)" % rays.device)
        return _f32c(rays)

    def _next_seed(self) -> int:
        self._calls += 1
        return (int(self.seed) * 0x9E3779B97F4A7C15 + self._calls) & 0xFFFFFFFFFFFFFFFF

    def _cfg(self, n_samples, n_candidates, n_gaussian, depth_diff_max=0.05) -> DinerSamplerCfg:
        assert n_samples >= n_gaussian  # nerf_renderer.py:89
        cfg = DinerSamplerCfg()
        cfg.n_candidates, cfg.n_samples, cfg.n_gaussian = int(n_candidates), int(n_samples), int(n_gaussian)
        cfg.depth_diff_max = float(depth_diff_max)
        return cfg

    # ------------------------------------------------------------------------------------------
    # stages (reference signatures; keyword-only extras are build-only)
    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_coarse(self, rays, n_coarse=None, *, u_coarse=None):
        """Stratified candidates (reference nerf_renderer.py:39-63): rays [SB,B,8] -> [SB,B,Kc]."""
        n_coarse = n_coarse if n_coarse else self.n_coarse
        r = self._check_rays(rays.reshape(1, -1, 8))
        N = r.shape[1]
        z = torch.empty((N, n_coarse), dtype=torch.float32, device=r.device)
        u = None if u_coarse is None else _f32c(u_coarse).reshape(N, n_coarse)
        check(_lib.lib().diner_sample_coarse(_ptr(r), N, n_coarse, _ptr(u), self._next_seed(), _ptr(z), _stream(r.device)),
              "diner_sample_coarse")
        return z.view(*rays.shape[:-1], n_coarse)

    @torch.no_grad()
    def sample_depthguided(self, rays, model, n_samples, n_candidates, depth_diff_max=0.05, n_gaussian=None, *,
                           noise: Optional[Sequence[Optional[torch.Tensor]]] = None, z_cand=None,
                           return_internals=False):
        """Depth-guided short-list + gaussian samples (reference nerf_renderer.py:65-284).
        Returns z [SB,NR,n_samples] *before* fill-up (0 = empty slot), like the reference.
        ``noise=(u_coarse, n_gauss, u_fill)`` dense tensors for parity runs."""
        n_gaussian = n_gaussian if n_gaussian is not None else self.n_gaussian
        out = self._sample(rays, model, n_samples, n_candidates, n_gaussian, depth_diff_max, noise, z_cand,
                           want_dg=True, want_lik=return_internals)
        return (out["z_dg"], out) if return_internals else out["z_dg"]

    def _sample(self, rays, model, K, NC, G, depth_diff_max, noise, z_cand, want_dg=False, want_lik=False):
        r = self._check_rays(rays)
        SB, NR, _ = r.shape
        sc, _keep = self._scene(model, need_latent=False)
        assert SB == sc.SB
        cfg = self._cfg(K, NC, G, depth_diff_max)
        dev = r.device
        u_c, n_g, u_f = self._noise(noise, dev)
        if u_c is not None: assert u_c.numel() == SB * NR * NC
        if n_g is not None: assert n_g.numel() == SB * NR * G
        if u_f is not None: assert u_f.numel() == SB * NR * K
        zc = None if z_cand is None else _f32c(z_cand).to(dev)
        z = torch.empty((SB, NR, K), dtype=torch.float32, device=dev)
        z_dg = torch.empty_like(z) if want_dg else None
        lik = torch.empty((SB, NR, NC), dtype=torch.float32, device=dev) if want_lik else None
        check(_lib.lib().diner_sample_depthguided(C.byref(sc), _ptr(r), NR, C.byref(cfg), _ptr(u_c), _ptr(n_g), _ptr(u_f),
                                                  _ptr(zc), self._next_seed(), _ptr(z), _ptr(z_dg), _ptr(lik),
                                                  _stream(dev)), "diner_sample_depthguided")
        return dict(z=z, z_dg=z_dg, likelihood=lik)

    @torch.no_grad()
    def fill_up_uniform_samples(self, z_samples, rays, *, u_fill=None):
        """Uniform fill-up of the empty slots + sort (reference nerf_renderer.py:367-397)."""
        r = self._check_rays(rays)
        z = _f32c(z_samples)
        K = z.shape[-1]
        N = r.shape[0] * r.shape[1]
        out = torch.empty_like(z)
        u = None if u_fill is None else _f32c(u_fill).to(r.device)
        check(_lib.lib().diner_fill_up_uniform_samples(_ptr(r), _ptr(z), N, K, _ptr(u), self._next_seed(), _ptr(out),
                                                       _stream(r.device)), "diner_fill_up_uniform_samples")
        return out

    def render_points(self, model, rays, z_samp):
        """rgb-sigma of the sample points (the ``model(points, viewdirs)`` calls of composite(),
        reference nerf_renderer.py:304-339 + pixelnerf.py:55-145): -> [SB,B,K,4]."""
        self._require_no_grad(model)
        r = self._check_rays(rays)
        z = _f32c(z_samp)
        SB, NR, K = z.shape
        route = self._resolve(model)
        packed, sc, _keep, lz = self._prepare(model, route)
        assert SB == sc.SB  # pixelnerf.py:68
        out = torch.empty((SB, NR, K, 4), dtype=torch.float32, device=r.device)
        # (the standard kernels' scratch; a shape-general one takes none)
        n_scr = 0 if route.gen else int(_lib.lib().diner_render_points_scratch_floats(SB, sc.NV, _lib.PRECISIONS[route.effective_precision]))
        scr = torch.empty(n_scr, dtype=torch.float32, device=r.device) if n_scr else None
        self._points(route, lz, sc, packed, r, z, NR, K, scr, out, _stream(r.device))
        self._ran(route, lz, "ctypes")
        return out

    def _prepare(self, model, route: _Route, saved=False):
        """The device state of a call on ``route`` -> (packed MLP image, DinerScene, the tensors it points into, the route's lin_z maps
        or None).  ``saved``: the forward of an autograd frame (render_image), which is the training path's: no maps."""
        if not route.gen:
            packed = self._mlp(model)
            sc, keep = self._scene(model, need_latent=True, packed_mlp=packed)
        elif saved:
            packed = self._mlp_shape_general(model, route.shape, route.f16)
            sc, keep = self._scene(model, need_latent=True)
        else:
            packed, gshape = self._gen_packs(model, route.shape, route.f16)
            sc, keep = self._scene(model, need_latent=True, gen_shape=gshape)
        return packed, sc, keep, keep.linz_gen

    def _points(self, route: _Route, lz, sc, packed, r, z, NR, K, scratch, out, st):
        """the point stage: rgb-sigma ``out`` [SB*NR*K*4] of the samples ``z`` (render_points(), and the staged form of _launch)"""
        fn, name, args = self._entry(route, "render_points", lz, sc, packed, (_ptr(r), _ptr(z), NR, K), (_ptr(out), st), scratch)
        check(fn(*args), name)

    def _ran(self, route: _Route, lz, binding: str):
        """what an inference call leaves behind for its caller to read"""
        self.last_route, self.last_binding = route.stem + ("_lz" if lz is not None else ""), binding
        self.effective_precision = route.effective_precision

    @staticmethod
    def _noise(noise, dev):
        """(u_coarse, n_gauss, u_fill) of a replayed-noise argument, each fp32 on ``dev`` or None"""
        if noise is None:
            return None, None, None
        return [None if t is None else _f32c(t).to(dev) for t in noise]

    def composite(self, model, rays, z_samp, *, rgbsigma=None, _sync=False):
        """Alpha compositing (reference nerf_renderer.py:286-365) -> (weights, rgb, depth)."""
        r = self._check_rays(rays)
        z = _f32c(z_samp)
        SB, NR, K = z.shape
        if rgbsigma is None and self._wants_grad(model, rays):
            shape = self._validate(model)
            if self._use_gen_train(shape, model):
                out = self._forward_train_gen(model, rays, True, shape, z_samples=z).fine
                return out.weights, out.rgb, out.depth
            if self._needs_gen(shape, model):
                self._gen_training_unsupported(shape, model)
            out = self._forward_train(model, rays, True, z_samples=z).fine   # differentiable like the reference's composite
            return out.weights, out.rgb, out.depth
        if rgbsigma is None:
            rgbsigma = self.render_points(model, rays, z)
        c = _f32c(rgbsigma)
        dev = r.device
        weights = torch.empty((SB, NR, K), dtype=torch.float32, device=dev)
        rgb = torch.empty((SB, NR, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((SB, NR), dtype=torch.float32, device=dev)
        self._poll_status()
        check(_lib.lib().diner_composite(_ptr(r), _ptr(z), _ptr(c), SB * NR, K, int(bool(self.white_bkgd)), _ptr(rgb),
                                         _ptr(depth), _ptr(weights), _ptr(self._status_word(dev)), _stream(dev)), "diner_composite")
        self._after_launch(dev, sync=_sync)
        return weights, rgb, depth

    @staticmethod
    def _wants_grad(model, rays) -> bool:
        """True when autograd needs the training path: an MLP parameter, ``encoder.latent``, the rays, a camera tensor
        (poses, focal, c, image_shape) or ``encoder.depths`` requires grad."""
        if not torch.is_grad_enabled():
            return False
        if any(p.requires_grad for p in model.mlp_fine.parameters()) or model.encoder.latent.requires_grad:
            return True
        from .training import camera_leaves
        return any(t is not None and t.requires_grad for t in camera_leaves(model, rays))

    @staticmethod
    def _require_no_grad(model):
        if torch.is_grad_enabled() and any(p.requires_grad for p in model.mlp_fine.parameters()):
            raise RuntimeError(
                "render_points() is the fused inference kernel and carries no autograd graph: call forward()/composite() "
                "(they switch to the differentiable training path of diner_amd/training.py) or wrap it in torch.no_grad().")

    # ------------------------------------------------------------------------------------------
    def forward(self, model, rays, want_weights=False, *, noise=None, z_samples=None):
        """Reference nerf_renderer.py:399-424.
        :param model: ``PixelNeRF`` (encode() already called)
        :param rays: [SB,B,8] = origin, direction, near, far
        :param want_weights: also return the compositing weights [SB,B,K]
        :param noise: (build-only) dense ``(u_coarse, n_gauss, u_fill)`` replacing the in-kernel RNG
        :param z_samples: (build-only) inject sorted samples [SB,B,K] and skip the sampler
        :return: ``out.fine.rgb`` [SB,B,3], ``out.fine.depth`` [SB,B], ``out.fine.weights`` iff requested
        """
        assert len(rays.shape) == 3
        if self._wants_grad(model, rays):
            shape = self._validate(model)
            if self._use_gen_train(shape, model):
                return self._forward_train_gen(model, rays, want_weights, shape, noise=noise, z_samples=z_samples)
            if self._needs_gen(shape, model):
                self._gen_training_unsupported(shape, model)
            return self._forward_train(model, rays, want_weights, noise=noise, z_samples=z_samples)
        route = self._resolve(model) if z_samples is None else None     # (injected samples: composite() -> render_points() resolves)
        with torch.no_grad():
            r = self._check_rays(rays)
            big = want_weights or r.shape[0] * r.shape[1] > int(self.finite_sync_rays)   # examined before this call returns (see __init__)
            if z_samples is not None:
                weights, rgb, depth = self.composite(model, r, z_samples, _sync=big)
            else:
                rgb, depth, weights = self._launch(model, route, rays=r, want_weights=want_weights, noise=noise, sync=big)
        return RenderOutput(fine=self._format_outputs(weights, rgb, depth, want_weights=want_weights))

    def _launch(self, model, route: _Route, *, rays=None, cam=None, want_weights=False, noise=None, saved=None, sync=False):
        """The whole path -- sampler, point stage, compositing -- of one inference call on ``route``, under no_grad: of ``rays`` [SB,NR,8]
        (forward()), or of the target cameras ``cam`` = (extrinsics, intrinsics, z_near, z_far, H, W), whose rays the sampler generates
        (render_image: NR = H * W) -> (rgb [SB,NR,3], depth [SB,NR], weights [SB,NR,K] or None).
        The torch_ops binding takes the call where it serves it: ``route.op_ok``, ``binding``, and none of the build-only extras
        (replayed ``noise``, ``saved``, forward()'s ``stage_events``).  Else ctypes: the route's entry point, or under ``stage_events``
        the three stage entry points that it runs internally, bracketed by four events.
        ``saved`` (a dict; render_image under autograd) receives the generated rays, the samples the compositing used (workspace
        layout rays | z | ..., here z only: the rays go to their own tensor) and the flat rgb / depth.
        ``sync``: examine the frame before returning (``_after_launch``)."""
        image = rays is None
        if image:
            E, Ki, zn, zf, H, W = cam
            dev, SB, NR = E.device, E.shape[0], H * W
        else:
            dev, (SB, NR, _) = rays.device, rays.shape
        packed, sc, keep, lz = self._prepare(model, route, saved is not None)
        assert SB == sc.SB
        K = int(self.n_samples)
        cfg = self._cfg(K, self.n_depth_candidates, self.n_gaussian)
        white = int(bool(self.white_bkgd))
        staged = not image and self.stage_events is not None
        use_ops = route.op_ok and self.binding == "torch_ops" and noise is None and saved is None and not staged
        seed = self._next_seed()
        self._poll_status()
        status = self._status_word(dev)
        if use_ops:    # (the op allocates its own workspace and outputs: never both sets at once)
            from . import ops as _ops
            out = getattr(_ops.load(), "render_image" if image else "render")(
                *keep[:6], packed, *((E, Ki, zn, zf, H, W) if image else (rays,)), sc.image_w, sc.image_h, sc.feature_padding, sc.num_freqs,
                sc.freq_factor, cfg.n_candidates, cfg.n_samples, cfg.n_gaussian, cfg.depth_diff_max, bool(self.white_bkgd),
                _lib.PRECISIONS[route.effective_precision], seed - (1 << 64) if seed >= (1 << 63) else seed,
                *(() if image else (bool(want_weights),)), status)
            rgb, depth, weights = out[0], out[1], (out[2] if want_weights else None)
        else:
            L, st = _lib.lib(), _stream(dev)
            # workspace: by precision for the standard kernels (the point stage's scratch); a shape-general route takes the fp32 size
            wprec = _lib.PRECISIONS["fp32" if route.gen else route.effective_precision]
            n_ws = (L.diner_render_image_workspace_floats(SB, H, W, K, sc.NV, wprec) if image else
                    L.diner_render_workspace_floats(SB, NR, K, sc.NV, wprec))
            ws = torch.empty(int(n_ws), dtype=torch.float32, device=dev)
            rgb = torch.empty((SB, NR, 3), dtype=torch.float32, device=dev)
            depth = torch.empty((SB, NR), dtype=torch.float32, device=dev)
            weights = torch.empty((SB, NR, K), dtype=torch.float32, device=dev) if want_weights else None
            outs = (_ptr(rgb), _ptr(depth), _ptr(weights), _ptr(status), st)
            if image:
                tc = _lib.DinerTargetCam()
                tc.extrinsics, tc.intrinsics, tc.z_near, tc.z_far = E.data_ptr(), Ki.data_ptr(), zn.data_ptr(), zf.data_ptr()
                tc.H, tc.W = H, W
                rays_out = None if saved is None else torch.empty((SB, NR, 8), dtype=torch.float32, device=dev)
                stem, a, b = "render_image", (C.byref(tc), C.byref(cfg), white), (seed, _ptr(ws), _ptr(rays_out), *outs)
            else:
                u_c, n_g, u_f = self._noise(noise, dev)
                stem, a, b = "render", (_ptr(rays), NR, C.byref(cfg), white), (_ptr(u_c), _ptr(n_g), _ptr(u_f), seed, _ptr(ws), *outs)
            if not staged:
                fn, name, args = self._entry(route, stem, lz, sc, packed, a, b)
                check(fn(*args), name)
            else:
                n = SB * NR * K
                z, c, scr = ws[:n], ws[n:5 * n], ws[5 * n:]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                check(L.diner_sample_depthguided(C.byref(sc), _ptr(rays), NR, C.byref(cfg), _ptr(u_c), _ptr(n_g), _ptr(u_f),
                                                 None, seed, _ptr(z), None, None, st), "diner_sample_depthguided")
                ev[1].record()
                self._points(route, lz, sc, packed, rays, z, NR, K, scr if scr.numel() else None, c, st)
                ev[2].record()
                check(L.diner_composite(_ptr(rays), _ptr(z), _ptr(c), SB * NR, K, white, *outs), "diner_composite")
                ev[3].record()
                self.stage_events.append(ev)
            if saved is not None:
                n = SB * NR
                saved.update(rays=rays_out, z=ws[n * 8:n * (8 + K)].view(SB, NR, K).clone(), rgb=rgb, depth=depth)
        self._ran(route, lz, "torch_ops" if use_ops else "ctypes")
        self._after_launch(dev, sync=sync)
        return rgb, depth, weights

    def render_image(self, model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth=False, bounds=None,
                     box_offset=(-0.01, 0.01), return_mask=False):
        """The render half of ``DINER.predict_imgs_from_batch`` (reference src/models/diner.py:75-97) without the
        ray-batch loop and without a rays tensor round trip: ``gen_rays`` (src/util/cam_geometry.py:36-79) is evaluated
        inside the sampler kernel (``diner_render_image``), the whole target image is ONE launch per stage (no 4096-ray
        chunks, no ``torch.cat``), output in the reference's image layout.  Bit-identical to ``forward(gen_rays(...))``.
        Under autograd -- grad mode on and ``forward()``'s predicate (an MLP parameter, ``encoder.latent``, a source camera or
        ``encoder.depths`` requiring grad) or one of the four target-camera arguments requiring grad -- the same frame, bit for bit,
        gets a ``grad_fn``: its backward re-runs the training path (``forward()``'s arithmetic under autograd) on the saved rays and
        samples in chunks of ``grad_chunk_rays`` rays and takes the rays' gradient on to the target cameras (``_RenderImageFn``).
        With ``bounds`` ([SB,2,3] or [2,3]: the subject's axis-aligned box, e.g. ``load_face_bounds``' result) only the rays that meet
        the box ``bounds + box_offset`` are rendered, their samples spread over the box's own depth interval instead of
        [z_near, z_far]: ``glue.box_rays`` -> ``forward()``'s inference routing on the compact rays (any route, with its non-finite
        check, ``last_route`` and ``last_binding``) -> ``glue.frame_from_hits``; a missed pixel is the background colour with depth 0.
        ``last_box_hits`` then holds each scene's number of rendered rays; a box no ray meets returns the background without a render
        launch.  Inference only: under autograd it raises ``NotImplementedError`` (train inside a box with ``glue.box_rays`` +
        ``forward()``).  Without ``bounds`` nothing changes.
        :param target_extrinsics: [SB,4,4] world->cam;  target_intrinsics: [SB,3,3];  z_near, z_far: [SB] or scalars
        :param return_mask: (with ``bounds``) also return the hit mask [SB,1,H,W] (bool)
        :return: rgb [SB,3,H,W] (, depth [SB,1,H,W]) (, mask [SB,1,H,W])"""
        grad = torch.is_grad_enabled() and (self._wants_grad(model, None) or any(
            isinstance(t, torch.Tensor) and t.requires_grad for t in (target_extrinsics, target_intrinsics, z_near, z_far)))
        if bounds is not None:
            if grad:
                raise NotImplementedError(
                    "render_image(bounds=...) is inference only: the chunked backward of a boxed frame is not implemented.  To train "
                    "inside a box, take the hit rays from glue.box_rays and call forward() on them; or wrap the call in torch.no_grad().")
            return self._render_image_box(model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth, bounds, box_offset,
                                          return_mask)
        if return_mask:
            raise ValueError("render_image: return_mask needs bounds (without a box every pixel is rendered)")
        if grad:
            return self._render_image_grad(model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth)
        return self._render_image(model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth)

    @torch.no_grad()
    def _render_image_box(self, model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth, bounds, box_offset,
                          return_mask):
        """render_image inside a box: the hit rays (one host synchronisation of SB counts), forward()'s inference routing on them, the
        gather back to the frame"""
        from . import glue
        H, W = int(H), int(W)
        rays, _idx, slot, counts = glue.box_rays(target_extrinsics, target_intrinsics, W, H, z_near, z_far, bounds, box_offset)
        self.last_box_hits = [int(c) for c in counts.tolist()]
        SB, B, dev = rays.shape[0], rays.shape[1], rays.device
        if B > 0:
            fine = self.forward(model, rays).fine
            rgb_c, depth_c = fine.rgb, fine.depth
            if self.finite_check != "off":
                self.check_finite()                                   # once per frame: a NaN image never leaves this function
        else:
            rgb_c = torch.empty((SB, 0, 3), dtype=torch.float32, device=dev)
            depth_c = torch.empty((SB, 0), dtype=torch.float32, device=dev)
        rgb, depth, *mask = glue.frame_from_hits(rgb_c, depth_c, slot, H, W, self.white_bkgd, return_mask=return_mask)
        out = (rgb, *((depth,) if return_depth else ()), *mask)
        return out if len(out) > 1 else rgb

    def _render_image_grad(self, model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth):
        shape = self._validate(model)
        if self._needs_gen(shape, model) and not self._use_gen_train(shape, model):
            self._gen_training_unsupported(shape, model)          # before any device work, as forward() raises it
        from .training import camera_leaves
        leaves = [model.encoder.latent, *camera_leaves(model, None)[1:], *model.mlp_fine.parameters()]
        H, W = int(H), int(W)
        rgb, depth = _RenderImageFn.apply(self, model, shape, (H, W), target_extrinsics, target_intrinsics, z_near, z_far, *leaves)
        SB = rgb.shape[0]
        rgb = rgb.view(SB, H, W, 3).permute(0, 3, 1, 2)
        if return_depth:
            return rgb, depth.view(SB, H, W, 1).permute(0, 3, 1, 2)
        return rgb

    def _render_image(self, model, target_extrinsics, target_intrinsics, H, W, z_near, z_far, return_depth=False, saved=None):
        """render_image's inference launch.  ``saved`` (a dict): the forward of an autograd frame, which is the training path's -- exact
        fp32 on a shape-general route, the ctypes binding (the torch op gives no access to its workspace) -- and fills it (``_launch``)."""
        route = self._resolve(model, f16_ok=saved is None, stacklevel=5)
        H, W = int(H), int(W)
        with torch.no_grad():
            dev = target_extrinsics.device
            SB = target_extrinsics.shape[0]
            E, Ki = _f32c(target_extrinsics), _f32c(target_intrinsics)
            zn = torch.as_tensor(z_near, dtype=torch.float32, device=dev).expand(SB).contiguous()
            zf = torch.as_tensor(z_far, dtype=torch.float32, device=dev).expand(SB).contiguous()
            # examined once per frame: a NaN image never leaves this function
            rgb, depth, _ = self._launch(model, route, cam=(E, Ki, zn, zf, H, W), saved=saved, sync=self.finite_check != "off")
            rgb = rgb.view(SB, H, W, 3).permute(0, 3, 1, 2)
            if return_depth:
                return rgb, depth.view(SB, H, W, 1).permute(0, 3, 1, 2)
            return rgb

    def _train_prelude(self, model, rays, noise, z_samples, d_latent):
        """what both training paths start with -> (z, scene, the tensors it points into): the samples (injected, or drawn under no_grad
        as src/models/nerf_renderer.py:65 does) and the scene without a packed latent, ``encoder.latent``'s own shape written into it"""
        r = self._check_rays(rays)
        with torch.no_grad():
            if z_samples is not None:
                z = _f32c(z_samples)
            else:
                z = self._sample(r, model, int(self.n_samples), self.n_depth_candidates, self.n_gaussian, 0.05, noise, None)["z"]
            sc, keep = self._scene(model, need_latent=False)
        assert r.shape[0] == sc.SB
        lat = model.encoder.latent
        assert lat.shape[:2] == (sc.SB, sc.NV) and lat.shape[2] == d_latent
        sc.C, sc.h, sc.w = int(lat.shape[2]), int(lat.shape[3]), int(lat.shape[4])
        return z, sc, keep

    def _forward_train(self, model, rays, want_weights, noise=None, z_samples=None):
        """Training path (reference DINER.calc_losses, src/models/diner.py:217-290): sampler under no_grad, then the differentiable
        point evaluation + compositing of diner_amd/training.py (HIP building blocks; gradients to the MLP parameters, encoder.latent,
        the rays, the source cameras and encoder.depths)."""
        from . import training
        z, sc, keep = self._train_prelude(model, rays, noise, z_samples, 512)
        rgb, depth, weights = training.render_with_grad(self, model, rays, z, sc, keep=keep)
        return RenderOutput(fine=self._format_outputs(weights, rgb, depth, want_weights=want_weights))

    def _forward_train_gen(self, model, rays, want_weights, shape: MlpShape, noise=None, z_samples=None):
        """_forward_train for a model of any shape of the envelope (train_any_shape): the path of diner_amd/training_gen.py, in exact fp32
        or (train_f16x3_any_shape) in f16x3"""
        from . import training_gen
        f16 = self._use_gen_train_f16(shape, model)
        if f16:
            self.effective_precision = "f16x3"
        else:
            self._settle_fp32(shape, stacklevel=4)
        z, sc, keep = self._train_prelude(model, rays, noise, z_samples, shape.d_latent)
        kw = dict(f16=True) if f16 else {}   # (the fp32 call keeps the argument list it had)
        rgb, depth, weights = training_gen.render_with_grad(self, model, rays, z, sc, shape, keep=keep, **kw)
        self.last_route, self.last_binding = ("train_gen_f16" if f16 else "train_gen"), "ctypes"
        return RenderOutput(fine=self._format_outputs(weights, rgb, depth, want_weights=want_weights))

    # alias asked for by the north_star text; the reference itself has no render_rays
    render_rays = forward

    def _format_outputs(self, weights, rgb, depth, want_weights):
        out = RenderOutput(rgb=rgb, depth=depth)
        if want_weights:
            out.weights = weights
        return out


class _RenderImageFn(torch.autograd.Function):
    """(target_extrinsics, target_intrinsics, z_near, z_far, encoder.latent, poses, focal, c, image_shape, encoder.depths, *MLP parameters)
    -> rgb [SB,H*W,3], depth [SB,H*W] of ``NeRFRendererDGS.render_image``.

    forward: the inference entry point of the model's route (the no-grad frame, bit for bit), keeping the generated rays and the samples.
    backward: the training path -- what ``forward(model, rays, z_samples=z)`` runs under autograd -- re-run on the saved rays and samples in
    chunks of ``renderer.grad_chunk_rays`` rays; ``torch.autograd.grad`` of each chunk against its slice of the incoming gradient, summed in
    chunk order; then the rays' gradient through ``diner_gen_rays_backward`` to the target cameras.  The gradients are those of ``forward()``
    under autograd (the training path's arithmetic), not of the inference kernel's rounding.  The samples are constants, as in the training
    path: z_near gets 0 and z_far only the delta_inf term."""

    @staticmethod
    def forward(ctx, renderer, model, shape, HW, E, Kt, z_near, z_far, *leaves):
        H, W = HW
        saved = {}
        renderer._render_image(model, E, Kt, H, W, z_near, z_far, return_depth=True, saved=saved)
        ctx.renderer, ctx.model, ctx.shape, ctx.HW, ctx.precision = renderer, model, shape, HW, renderer.precision
        ctx.rays, ctx.z = saved["rays"], saved["z"]
        ctx.tcams, ctx.e32, ctx.k32 = (E, Kt, z_near, z_far), _f32c(E), _f32c(Kt)
        ctx.leaves = leaves
        # backward() re-reads all of these: an in-place update between forward and backward is an error, as in training._RenderFn
        ctx.versions = [(t, t._version) for t in (E, Kt, z_near, z_far, *leaves) if isinstance(t, torch.Tensor)]
        return saved["rgb"], saved["depth"]

    @staticmethod
    def backward(ctx, d_rgb, d_depth):
        r, model, shape = ctx.renderer, ctx.model, ctx.shape
        from .training import camera_leaves
        current = [model.encoder.latent, *camera_leaves(model, None)[1:], *model.mlp_fine.parameters()]
        if (any(t._version != v for t, v in ctx.versions) or len(current) != len(ctx.leaves)
                or any(a is not b for a, b in zip(current, ctx.leaves))):
            raise RuntimeError("diner_amd.NeRFRendererDGS.render_image: one of the variables needed for gradient computation (a target "
                               "camera, an MLP parameter, encoder.latent, or a source camera / depth-map tensor) has been modified by an "
                               "inplace operation, or re-bound on the model, between forward and backward")
        want_t = any(ctx.needs_input_grad[4:8])
        idx = [i for i in range(len(ctx.leaves)) if ctx.needs_input_grad[8 + i]]
        leaves = [ctx.leaves[i] for i in idx]
        cot = [(i, g) for i, g in ((0, d_rgb), (1, d_depth)) if g is not None]
        rays, z = ctx.rays, ctx.z
        SB, NR, _ = rays.shape
        acc = [None] * len(idx)
        d_rays = torch.zeros_like(rays) if want_t else None
        step = max(1, int(r.grad_chunk_rays))
        gen = r._use_gen_train(shape, model)
        prec, r.precision = r.precision, ctx.precision
        try:
            with torch.enable_grad():
                for a in range(0, NR if cot and (leaves or want_t) else 0, step):
                    b = min(NR, a + step)
                    rc = rays[:, a:b].contiguous().requires_grad_(want_t)
                    zc = z[:, a:b].contiguous()
                    fine = (r._forward_train_gen(model, rc, False, shape, z_samples=zc) if gen else
                            r._forward_train(model, rc, False, z_samples=zc)).fine
                    outs = [(fine.rgb, fine.depth)[i] for i, _ in cot]
                    gs = torch.autograd.grad(outs, leaves + ([rc] if want_t else []), [g[:, a:b] for _, g in cot], allow_unused=True)
                    for j in range(len(leaves)):
                        if gs[j] is not None:
                            acc[j] = gs[j] if acc[j] is None else acc[j].add_(gs[j])
                    if want_t and gs[-1] is not None:
                        d_rays[:, a:b] = gs[-1]
        finally:
            r.precision = prec
        t_grads = [None] * 4
        if want_t:
            from .glue import _like, gen_rays_backward
            H, W = ctx.HW
            for i, g in enumerate(gen_rays_backward(ctx.e32, ctx.k32, d_rays, H, W)):
                if ctx.needs_input_grad[4 + i]:
                    t_grads[i] = _like(g, ctx.tcams[i])
        leaf_grads = [None] * len(ctx.leaves)
        for j, i in enumerate(idx):
            leaf_grads[i] = acc[j] if acc[j] is not None else torch.zeros_like(ctx.leaves[i])
        return (None, None, None, None, *t_grads, *leaf_grads)
