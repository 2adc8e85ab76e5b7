"""ctypes binding of ``libdiner_hip.so`` (the C ABI declared in ``include/diner_hip.h``).

There is NO fallback: if the HIP library is missing the import of the product path fails loudly
(build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C diner_amd/csrc``).
``torch`` is imported first on purpose: its bundled ``libamdhip64.so`` (soname ``libamdhip64.so.7``)
is then the HIP runtime our library binds to, so torch's streams and device pointers are valid
inside our launches.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch  # noqa: F401  (must be loaded before libdiner_hip.so, see above)

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libdiner_hip.so"
_FP = C.c_void_p  # device pointers travel as integers

N_BLOCKS, COMBINE = 5, 3
# the ABI version THIS binding (the argument lists in SYMBOLS below) is written against = DINER_ABI_VERSION of include/diner_hip.h
ABI_VERSION = 3
PRECISIONS = {"fp32": 0, "f16x3": 1}
# DINER_ROUND_* of include/diner_hip.h (diner_frames_u8)
ROUNDINGS = {"save_image": 0, "video": 1}
# DINER_BG_* of include/diner_hip.h (diner_decode_image_u8)
BG_RULES = {"none": 0, "below_half": 1, "below_one": 2}
# DINER_RESIZE_* of include/diner_hip.h (diner_resize_table)
RESIZE_MODES = {"bilinear_aa": 1, "bilinear": 2, "bicubic_u8": 3}
# DINER_ACT_* of include/diner_hip.h (diner_train_gemm_act)
ACT_NONE, ACT_RELU, ACT_SOFTPLUS = 0, 1, 2


class DinerScene(C.Structure):
    _fields_ = [("SB", C.c_int32), ("NV", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("C", C.c_int32), ("num_freqs", C.c_int32),
                ("image_w", C.c_float), ("image_h", C.c_float), ("feature_padding", C.c_float),
                ("freq_factor", C.c_float),
                ("poses", _FP), ("focal", _FP), ("c", _FP), ("maps", _FP), ("latent", _FP), ("linz_maps", _FP)]


class DinerMlpRaw(C.Structure):
    _fields_ = [("lin_in_w", _FP), ("lin_in_b", _FP),
                ("lin_z_w", _FP * COMBINE), ("lin_z_b", _FP * COMBINE),
                ("fc0_w", _FP * N_BLOCKS), ("fc0_b", _FP * N_BLOCKS),
                ("fc1_w", _FP * N_BLOCKS), ("fc1_b", _FP * N_BLOCKS),
                ("lin_out_w", _FP), ("lin_out_b", _FP)]


class DinerTargetCam(C.Structure):
    _fields_ = [("extrinsics", _FP), ("intrinsics", _FP), ("z_near", _FP), ("z_far", _FP), ("H", C.c_int32), ("W", C.c_int32)]


class DinerSamplerCfg(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("n_samples", C.c_int32), ("n_gaussian", C.c_int32),
                ("depth_diff_max", C.c_float)]


class DinerMlpShape(C.Structure):
    _fields_ = [("d_in", C.c_int32), ("d_latent", C.c_int32), ("d_hidden", C.c_int32), ("n_blocks", C.c_int32),
                ("combine_layer", C.c_int32), ("num_freqs", C.c_int32), ("beta", C.c_float), ("d_out", C.c_int32),
                ("combine_type", C.c_int32)]


class DinerMlpGenRaw(C.Structure):
    _fields_ = [("lin_in_w", _FP), ("lin_in_b", _FP),
                ("lin_z_w", C.POINTER(_FP)), ("lin_z_b", C.POINTER(_FP)),
                ("fc0_w", C.POINTER(_FP)), ("fc0_b", C.POINTER(_FP)),
                ("fc1_w", C.POINTER(_FP)), ("fc1_b", C.POINTER(_FP)),
                ("lin_out_w", _FP), ("lin_out_b", _FP)]


class DinerLatentIndex(C.Structure):
    _fields_ = [("interp", C.c_int32), ("padding", C.c_int32)]


class DinerNovelGen(C.Structure):
    _fields_ = [("latent", _FP), ("h", C.c_int32), ("w", C.c_int32), ("C", C.c_int32), ("_pad", C.c_int32),
                ("poses", _FP), ("focal", _FP), ("c", _FP), ("image_w", C.c_float), ("image_h", C.c_float)]


class DinerNovelPe(C.Structure):
    _fields_ = [("map", _FP), ("head", _FP), ("src_pe", _FP), ("src_h", C.c_int32), ("src_w", C.c_int32),
                ("tgt_pe", _FP), ("tgt_h", C.c_int32), ("tgt_w", C.c_int32),
                ("poses", _FP), ("focal", _FP), ("c", _FP), ("image_w", C.c_float), ("image_h", C.c_float)]


class DinerLatentLevel(C.Structure):
    _fields_ = [("data", _FP), ("C", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


LATENT_MAX_LEVELS = 5   # DINER_LATENT_MAX_LEVELS


class DinerLatentLevels(C.Structure):
    _fields_ = [("level", DinerLatentLevel * LATENT_MAX_LEVELS)]


# SpatialEncoder's index_interp / index_padding (reference src/models/image_encoder.py:24-25) -> DINER_INDEX_* of include/diner_hip.h
INDEX_INTERP = {"bilinear": 0, "nearest": 1}
INDEX_PADDING = {"border": 0, "zeros": 1, "reflection": 2}


# every symbol include/diner_hip.h declares: name -> (restype, argtypes)
_I64, _I32, _U64, _P, _F32, _F64 = C.c_int64, C.c_int32, C.c_uint64, C.c_void_p, C.c_float, C.c_double
SYMBOLS = {
    "diner_last_error": (C.c_char_p, []),
    "diner_version": (C.c_int, []),
    "diner_gen_rays": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "diner_gen_rays_backward_workspace_floats": (_I64, [_I32, _I32, _I32]),
    "diner_gen_rays_backward": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "diner_depth2normal": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "diner_pack_maps": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P]),
    "diner_pack_maps_from_depth": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P]),
    "diner_pack_latent": (C.c_int, [_P, _I64, _I32, _I32, _I32, _P, _P]),
    "diner_mlp_packed_floats": (_I64, []),
    "diner_pack_mlp": (C.c_int, [C.POINTER(DinerMlpRaw), _P, _P]),
    "diner_pack_linz_maps": (C.c_int, [_P, _I64, _I32, _I32, _P, _P, _P]),
    "diner_sample_coarse": (C.c_int, [_P, _I64, _I32, _P, _U64, _P, _P]),
    "diner_sample_depthguided": (C.c_int, [C.POINTER(DinerScene), _P, _I64, C.POINTER(DinerSamplerCfg),
                                           _P, _P, _P, _P, _U64, _P, _P, _P, _P]),
    "diner_fill_up_uniform_samples": (C.c_int, [_P, _P, _I64, _I32, _P, _U64, _P, _P]),
    "diner_render_points_scratch_floats": (_I64, [_I64, _I32, _I32]),
    "diner_render_points": (C.c_int, [C.POINTER(DinerScene), _P, _P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "diner_composite": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P]),
    "diner_decode_depth_u16": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _I32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         _P, _P, _P, _P]),
    "diner_train_gemm": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _I32, _I32, _I64,
                                   _I32, _P, _P, _I32, _I32, _P]),
    "diner_train_amax": (C.c_int, [_P, _I64, _P, _P]),
    "diner_train_colsum_amax": (C.c_int, [_P, _I64, _I32, _I64, _P, _P, _P]),
    "diner_train_split_panel": (C.c_int, [_P, _I32, _I64, _I32, _I32, _P, _P, _P]),
    "diner_train_pack_core": (C.c_int, [_P, _I64, _I32, _I32, _P, _P]),
    "diner_train_gemm_core": (C.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _I64, _I64, _I32, _P, _I32, _I32, _P, _P, _P]),
    "diner_train_gemm_panel": (C.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _I64, _I32, _I32, _P, _I32, _I32, _P]),
    "diner_train_colsum": (C.c_int, [_P, _I64, _I32, _I64, _P, _P]),
    "diner_train_point_inputs": (C.c_int, [C.POINTER(DinerScene), _P, _I32, _P, _P, _I64, _I32, _I32, _P, _P, _P, _P]),
    "diner_train_bilinear_scatter": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "diner_train_nhwc_to_nchw": (C.c_int, [_P, _I64, _I32, _I32, _I32, _P, _P]),
    "diner_train_view_mean": (C.c_int, [_P, _I64, _I32, _P, _I32, _P]),
    "diner_train_head": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _P]),
    "diner_composite_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P, _P]),
    "diner_render_workspace_floats": (_I64, [_I64, _I64, _I32, _I32, _I32]),
    "diner_render_image_workspace_floats": (_I64, [_I64, _I32, _I32, _I32, _I32, _I32]),
    "diner_render_image": (C.c_int, [C.POINTER(DinerScene), _P, C.POINTER(DinerTargetCam), C.POINTER(DinerSamplerCfg), _I32, _I32, _U64,
                                     _P, _P, _P, _P, _P, _P, _P]),
    "diner_render": (C.c_int, [C.POINTER(DinerScene), _P, _P, _I64, C.POINTER(DinerSamplerCfg), _I32, _I32,
                               _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_mlp_gen_packed_floats": (_I64, [C.POINTER(DinerMlpShape)]),
    "diner_pack_mlp_gen": (C.c_int, [C.POINTER(DinerMlpShape), C.POINTER(DinerMlpGenRaw), _P, _P]),
    "diner_render_points_gen": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, _P, _P, _I64, _I32, _P, _P]),
    "diner_render_gen": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, _P, _I64, C.POINTER(DinerSamplerCfg), _I32,
                                   _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_gen": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, C.POINTER(DinerTargetCam),
                                         C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P, _P]),
    # the latent lookup modes (DinerLatentIndex; NULL = bilinear / border)
    "diner_linz_maps_floats": (_I64, [_I64, _I32, _I32, C.POINTER(DinerLatentIndex)]),
    "diner_pack_linz_maps_ix": (C.c_int, [_P, _I64, _I32, _I32, _P, C.POINTER(DinerLatentIndex), _P, _P]),
    "diner_render_points_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, _P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "diner_render_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, _P, _I64, C.POINTER(DinerSamplerCfg), _I32, _I32,
                                  _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, C.POINTER(DinerTargetCam),
                                        C.POINTER(DinerSamplerCfg), _I32, _I32, _U64, _P, _P, _P, _P, _P, _P, _P]),
    "diner_render_points_gen_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P, _P, _P,
                                             _I64, _I32, _P, _P]),
    "diner_render_gen_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P, _P, _I64,
                                      C.POINTER(DinerSamplerCfg), _I32, _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_gen_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P,
                                            C.POINTER(DinerTargetCam), C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P, _P]),
    # the shape-general f16x3 inference path: the argument lists of the *_gen functions (the ABI version stays 3: new entry points only)
    "diner_mlp_gen_f16_packed_floats": (_I64, [C.POINTER(DinerMlpShape)]),
    "diner_pack_mlp_gen_f16": (C.c_int, [C.POINTER(DinerMlpShape), C.POINTER(DinerMlpGenRaw), _P, _P]),
    "diner_render_points_gen_f16": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, _P, _P, _I64, _I32, _P, _P]),
    "diner_render_gen_f16": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, _P, _I64, C.POINTER(DinerSamplerCfg), _I32,
                                       _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_gen_f16": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, C.POINTER(DinerTargetCam),
                                             C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P, _P]),
    "diner_render_points_gen_f16_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P, _P, _P,
                                                 _I64, _I32, _P, _P]),
    "diner_render_gen_f16_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P, _P, _I64,
                                          C.POINTER(DinerSamplerCfg), _I32, _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_gen_f16_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P,
                                                C.POINTER(DinerTargetCam), C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P,
                                                _P]),
    "diner_train_point_inputs_ix": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, _I32, _P, _P, _I64, _I32, _I32, _P,
                                              _P, _P, _P]),
    # camera / ray / depth-map gradients of the training path
    "diner_composite_backward_far": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "diner_train_camera_workspace_floats": (_I64, [_I64, _I32, _I32]),
    "diner_train_point_inputs_backward": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, _P, _P, _I64, _I32, _I32, _P,
                                                    _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # the shape-general training path (DINER_ACT_*; the ABI version stays 3: new entry points only)
    "diner_train_gemm_act": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _I32, C.c_float,
                                       _I32, _I32, _I64, _P]),
    "diner_train_point_inputs_gen": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, _P, _P, _I64, _I32, _I32, _P, _I64,
                                               _P, _P, _P]),
    "diner_train_point_inputs_backward_gen": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, _P, _P, _I64, _I32, _I32,
                                                        _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # the shape-general f16x3 training GEMM (train_gen_f16.hip; the ABI version stays 3: new entry points only)
    "diner_train_gemm_act_f16x3": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _I32,
                                             C.c_float, _I32, _I32, _I64, _P, _P, _I32, _I32, _P]),
    "diner_train_split_weight_halfs": (_I64, [_I32, _I32]),
    "diner_train_split_weight": (C.c_int, [_P, _I32, _I32, _I64, _I32, _I32, _P, _P, _P]),
    "diner_train_gemm_act_f16x3_w": (C.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _I64, _I32, _I32, _I32, _I32, C.c_float, _I32, _P,
                                               _I32, _I32, _P]),
    # the bicubic latent lookup (index_interp="bicubic"): the *_gen_ix argument lists with an int32 padding (INDEX_PADDING) in place of the
    # DinerLatentIndex pointer (the ABI version stays 3: new entry points only; INDEX_INTERP and DinerLatentIndex do not carry bicubic)
    "diner_render_points_gen_bc": (C.c_int, [C.POINTER(DinerScene), _I32, C.POINTER(DinerMlpShape), _P, _P, _P, _I64, _I32, _P, _P]),
    "diner_render_gen_bc": (C.c_int, [C.POINTER(DinerScene), _I32, C.POINTER(DinerMlpShape), _P, _P, _I64, C.POINTER(DinerSamplerCfg), _I32,
                                      _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_gen_bc": (C.c_int, [C.POINTER(DinerScene), _I32, C.POINTER(DinerMlpShape), _P, C.POINTER(DinerTargetCam),
                                            C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P, _P]),
    "diner_render_points_gen_f16_bc": (C.c_int, [C.POINTER(DinerScene), _I32, C.POINTER(DinerMlpShape), _P, _P, _P, _I64, _I32, _P, _P]),
    "diner_render_gen_f16_bc": (C.c_int, [C.POINTER(DinerScene), _I32, C.POINTER(DinerMlpShape), _P, _P, _I64, C.POINTER(DinerSamplerCfg),
                                          _I32, _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "diner_render_image_gen_f16_bc": (C.c_int, [C.POINTER(DinerScene), _I32, C.POINTER(DinerMlpShape), _P, C.POINTER(DinerTargetCam),
                                                C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P, _P]),
    "diner_train_point_inputs_gen_bc": (C.c_int, [C.POINTER(DinerScene), _I32, _P, _P, _P, _I64, _I32, _I32, _P, _I64, _P, _P, _P]),
    "diner_train_point_inputs_backward_gen_bc": (C.c_int, [C.POINTER(DinerScene), _I32, _P, _P, _P, _I64, _I32, _I32, _P, _I64, _P, _P, _P, _P,
                                                           _P, _P, _P, _P, _P, _P]),
    "diner_train_bicubic_scatter": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    # the latent assembled from the encoder's feature pyramid in diner_pack_latent's layout, and its adjoint (csrc/latent_assemble.hip;
    # the ABI version stays 3: new entry points only)
    "diner_assemble_latent": (C.c_int, [C.POINTER(DinerLatentLevels), _I32, _I64, _I32, _I32, _P, _P]),
    "diner_assemble_latent_backward": (C.c_int, [_P, _I32, _I64, _I32, _I32, C.POINTER(DinerLatentLevels), _P]),
    "diner_assemble_latent_bicubic": (C.c_int, [C.POINTER(DinerLatentLevels), _I32, _I64, _I32, _I32, _P, _P]),
    "diner_assemble_latent_bicubic_backward": (C.c_int, [_P, _I32, _I64, _I32, _I32, C.POINTER(DinerLatentLevels), _P]),
    # conv1's input (the head of the encoder: normalise, replicate pad, the padding's positional encoding) and its adjoint to the images
    # (csrc/encoder_input.hip; the ABI version stays 3: new entry points only)
    "diner_encoder_input": (C.c_int, [_P, _I64, _I32, _I32, _I32, _I32, _P, _P, _F32, _F32, _F32, _F32, _F32, _F32, _P, _P]),
    "diner_encoder_input_backward": (C.c_int, [_P, _I64, _I32, _I32, _I32, _I32, _F32, _F32, _F32, _P, _P]),
    # a training step's ray selection and photometric losses (csrc/train_glue.hip; the ABI version stays 3: new entry points only)
    "diner_gen_rays_at": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "diner_gen_rays_at_backward_workspace_floats": (_I64, [_I32, _I32]),
    "diner_gen_rays_at_backward": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "diner_photo_loss_workspace_floats": (_I64, [_I32, _I32, _I32, _I32]),
    "diner_photo_loss": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "diner_photo_loss_backward": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    # frame output and image scores: depth range, colour map, frames as bytes, l1 / l2 / psnr / ssim (csrc/frame_out.hip; the ABI version
    # stays 3: new entry points only)
    "diner_depth_range_workspace_floats": (_I64, [_I64, _I32, _I32]),
    "diner_depth_range": (C.c_int, [_P, _I64, _I32, _I32, _P, _P, _P]),
    "diner_depth_cmap": (C.c_int, [_P, _I64, _I32, _I32, _P, _F64, _F64, _I32, _I32, _P, _I32, _P, _P]),
    "diner_frames_u8": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _P, _F64, _F64, _I32, _I32, _P, _I32, _P, _P, _P]),
    "diner_image_scores_workspace_floats": (_I64, [_I64, _I32, _I32]),
    "diner_image_scores": (C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P]),
    # lin_z hoisted into per-texel maps on the shape-general kernels: the *_gen_ix argument lists, then precision (PRECISIONS), the bicubic
    # padding (-1: not bicubic, else INDEX_PADDING) and the maps of diner_pack_linz_maps_gen (the ABI version stays 3: new entry points only)
    "diner_linz_maps_gen_floats": (_I64, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape)]),
    "diner_pack_linz_maps_gen": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerMlpShape), _P, _P, _P]),
    "diner_render_points_gen_lz": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P, _P, _P,
                                             _I64, _I32, _P, _P, _I32, _I32, _P]),
    "diner_render_gen_lz": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P, _P, _I64,
                                      C.POINTER(DinerSamplerCfg), _I32, _P, _P, _P, _U64, _P, _P, _P, _P, _P, _P, _I32, _I32, _P]),
    "diner_render_image_gen_lz": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerMlpShape), _P,
                                            C.POINTER(DinerTargetCam), C.POINTER(DinerSamplerCfg), _I32, _U64, _P, _P, _P, _P, _P, _P, _P,
                                            _I32, _I32, _P]),
    # rendering inside a scene bounding box: hit pixels with the box's near / far, the compact rays, the frame from the compact results
    # (csrc/ray_box.hip; the ABI version stays 3: new entry points only)
    "diner_ray_box_select_workspace_floats": (_I64, [_I32, _I32, _I32]),
    "diner_ray_box_select": (C.c_int, [C.POINTER(DinerTargetCam), _I32, _P, _F32, _F32, _P, _P, _P, _P, _P, _P]),
    "diner_gen_rays_box": (C.c_int, [C.POINTER(DinerTargetCam), _I32, _P, _F32, _F32, _P, _P, C.POINTER(C.c_int32), _I32, _P, _P]),
    "diner_frame_from_hits": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    # the datasets' image bytes and Multiface's depth planes (csrc/image_wire.hip; the ABI version stays 3: new entry points only)
    "diner_decode_image_u8": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _F32, _I32, _I32, _P, _P, _P]),
    "diner_decode_depth_u16_mf": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _F32, _F32, _F32, _F32, _P, _P, _P, _P]),
    "diner_encoder_input_u8": (C.c_int, [_P, _P, _I32, _I32, _F32, _I32, _I32, _I64, _I32, _I32, _I32, _I32, _P, _P, _F32, _F32, _F32, _F32,
                                         _F32, _F32, _P, _P]),
    # the image resizes fused with the byte decode (csrc/image_resize.hip; the ABI version stays 3: new entry points only); the tables
    # of diner_resize_table are host arrays
    "diner_resize_taps": (C.c_int, [_I32, _I32, _I32]),
    "diner_resize_table": (C.c_int, [_I32, _I32, _I32, _I32, _P, _P]),
    "diner_decode_image_u8_resized": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _F32, _I32, _I32, _I32, _I32, _P, _P, _I32, _P, _P,
                                                _I32, _P, _P, _P, _P]),
    "diner_resize_u8": (C.c_int, [_P, _I64, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32, _P, _P, _I32, _P, _P, _P]),
    "diner_decode_depth_u16_mf_nearest": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _F32, _F32, _F32, _F32, _P, _P, _P, _P]),
    # nearest mesh vertex and the deformation built on it (csrc/nearest_vertex.hip; the ABI version stays 3: new entry points only)
    "diner_nearest_vertex_workspace_floats": (_I64, [_I32, _I32]),
    "diner_nearest_vertex_keys": (C.c_int, [_P, _I32, _I32, _P, _P]),
    "diner_nearest_vertex_build": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "diner_nearest_vertex": (C.c_int, [_P, _P, _P, _I32, _I64, _I32, _P, _P, _P]),
    "diner_deform_points": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I64, _I32, _P, _P, _P]),
    "diner_deform_ray_points": (C.c_int, [_P, _P, _P, _P, _P, _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P]),
    # the depth-guided sampler on given candidate points (csrc/sampler_points.hip; the ABI version stays 3: a new entry point only)
    "diner_sample_depthguided_points": (C.c_int, [C.POINTER(DinerScene), _P, _P, _P, _I64, C.POINTER(DinerSamplerCfg), _P, _P, _U64,
                                                  _P, _P, _P, _P]),
    # the NOVEL point model on the shape-general kernels: given points, a second (general) latent lookup (csrc/points_mlp_gen_nv.hip,
    # points_mlp_gen_f16_nv.hip; the ABI version stays 3: a new entry point only)
    "diner_render_points_novel": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerNovelGen),
                                            C.POINTER(DinerMlpShape), _P, _P, _P, _P, _I64, _I32, _P, _P]),
    # the NOVEL_PE point model: a third point set, two pos-encoding lookups, the deformation layer hoisted onto the latent's texels
    # (csrc/points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip, novel_pe_map.hip; new entry points only)
    "diner_novel_pe_map_floats": (_I64, [C.POINTER(DinerScene)]),
    "diner_pack_novel_pe_map": (C.c_int, [C.POINTER(DinerScene), _P, _P, _P]),
    "diner_render_points_novel_pe": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), C.POINTER(DinerNovelGen),
                                               C.POINTER(DinerNovelPe), C.POINTER(DinerMlpShape), _P, _P, _P, _P, _P, _I64, _I32, _P, _P]),
    # the NOVEL point model's training path: the point inputs at given points with the general lookup added, and the general latent's
    # scatter (csrc/train_novel.hip; the ABI version stays 3: new entry points only)
    "diner_train_point_inputs_novel": (C.c_int, [C.POINTER(DinerScene), C.POINTER(DinerLatentIndex), _P, C.POINTER(DinerNovelGen), _P, _P, _P,
                                                 _I64, _I32, _P, _I64, _P, _P, _P, _P]),
    "diner_train_novel_gen_scatter": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _I32, _P, _P]),
}

_lib = None


class DinerHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """The loaded library with typed entry points; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} is missing: the MI355X render path has no CPU or PyTorch fallback. "
                "Build it with `make -C diner_amd/csrc` (hipcc --offload-arch=gfx950).")
        l = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the ABI and the header drift apart
            fn.restype, fn.argtypes = res, args
        if l.diner_version() != ABI_VERSION:   # a stale .so (e.g. a git-ignored build from before an ABI change): never call into it
            raise ImportError(f"{LIB_PATH} has ABI version {l.diner_version()}, this binding needs {ABI_VERSION}: rebuild it "
                              "(`make -C diner_amd/csrc`)")
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().diner_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        if rc == -3:
            raise NotImplementedError(f"{what}: {msg}")
        raise DinerHipError(f"{what}: {msg} (rc={rc})")
