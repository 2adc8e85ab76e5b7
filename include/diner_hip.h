/*
 * diner_hip.h -- C ABI of the MI355X-native DINER render path (libdiner_hip.so).
 *
 * The reference (tancredeguillou/diner) implements this path in pure Python/PyTorch and has no
 * FFI; each entry point below therefore names the reference *Python* function it replaces
 * (paths relative to the reference root).  The Python plug-in class
 * diner_amd.NeRFRendererDGS (drop-in for src/models/nerf_renderer.py:12 NeRFRendererDGS, selected
 * by the YAML key renderer.module, src/models/diner.py:48) binds these with ctypes; the binding a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless stated otherwise; plain pointers and sizes
 *    only, no torch types;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); nothing synchronises;
 *  - every function returns 0 on success, <0 on error (DINER_E_*), never aborts the process;
 *    diner_last_error() returns a thread-local message for the last failure;
 *  - tensors use the reference's own shapes: SB scenes, NV source views, NR rays per scene,
 *    NC candidates, K samples, G gaussian samples; rays [SB,NR,8] = origin(3) dir(3) near far.
 */
#ifndef DINER_HIP_H
#define DINER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINER_OK 0
#define DINER_E_INVALID (-1)  /* bad argument (NULL pointer, unsupported size) */
#define DINER_E_LAUNCH (-2)   /* HIP launch / runtime failure */
#define DINER_E_UNSUPPORTED (-3)

#define DINER_D_LATENT 512 /* SpatialEncoder.latent_size, num_layers=4 (src/models/image_encoder.py:56) */
#define DINER_D_HIDDEN 512 /* configs/train_diner_facescape.yaml:57 */
#define DINER_D_IN 55      /* PE3 39 + viewdir 3 + PE1 13 (src/models/pixelnerf.py:18) */
#define DINER_N_BLOCKS 5
#define DINER_COMBINE_LAYER 3
#define DINER_MAP_TEXEL 8  /* floats per packed map texel: nx ny nz depth sigma 0 0 0 */

/* Arithmetic of the fusion-MLP GEMMs (everything else is fp32 in both modes):
 *  FP32  : v_mfma_f32_32x32x2_f32, bit-identical to a k-ordered fmaf chain;
 *  F16X3 : every fp32 operand split into fp16 hi+lo, 3 fp16 MFMAs per product, fp32 accumulate
 *          (fp32-grade: operand error <= 2^-23 relative, dropped lo*lo term <= 2^-22). */
#define DINER_PRECISION_FP32 0
#define DINER_PRECISION_F16X3 1

/* Per-scene state the renderer reads from the model:
 * PixelNeRF buffers (src/models/pixelnerf.py:27-30,47-51) and SpatialEncoder state
 * (src/models/image_encoder.py:92-95,214-218,271-272), with the maps re-packed once per
 * encode() by diner_pack_maps / diner_pack_latent. */
typedef struct DinerScene {
    int32_t SB, NV;          /* scenes in the batch, source views */
    int32_t H, W;            /* size of the depth / sigma / normal maps */
    int32_t h, w, C;         /* latent map size and channels (C must be DINER_D_LATENT) */
    int32_t num_freqs;       /* positional-encoding octaves (6) */
    float image_w, image_h;  /* model.image_shape = (W, H) */
    float feature_padding;   /* encoder.feature_padding in latent texels (32) */
    float freq_factor;       /* 6.28 (configs/train_diner_facescape.yaml:51) */
    const float *poses;      /* [SB,NV,4,4] world->camera */
    const float *focal;      /* [SB,NV,2] */
    const float *c;          /* [SB,NV,2] */
    const float *maps;       /* [SB,NV,H,W,8] packed by diner_pack_maps */
    const float *latent;     /* [SB,NV,h,w,C] packed by diner_pack_latent (may be NULL for the sampler) */
    const float *linz_maps;  /* [3][SB,NV,h,w,C] from diner_pack_linz_maps, or NULL: the F16X3 kernel then
                                evaluates lin_z per point like the FP32 kernel does */
} DinerScene;

/* ResnetFC parameters in the reference's nn.Linear layout, weight [out,in]
 * (src/models/resnetfc.py:72-127); input of diner_pack_mlp. */
typedef struct DinerMlpRaw {
    const float *lin_in_w, *lin_in_b;                  /* [512,55], [512] */
    const float *lin_z_w[DINER_COMBINE_LAYER], *lin_z_b[DINER_COMBINE_LAYER]; /* [512,512] */
    const float *fc0_w[DINER_N_BLOCKS], *fc0_b[DINER_N_BLOCKS];
    const float *fc1_w[DINER_N_BLOCKS], *fc1_b[DINER_N_BLOCKS];
    const float *lin_out_w, *lin_out_b;                /* [4,512], [4] */
} DinerMlpRaw;

typedef struct DinerSamplerCfg {
    int32_t n_candidates;    /* NC  (n_depth_candidates, 1000) */
    int32_t n_samples;       /* K   (n_samples, 40) */
    int32_t n_gaussian;      /* G   (n_gaussian, 15), 0 <= G <= K */
    float depth_diff_max;    /* 0.05 (src/models/nerf_renderer.py:67) */
} DinerSamplerCfg;

/* Target cameras for diner_render_image: the sampler generates each ray from its pixel instead of reading a rays tensor
 * (gen_rays fused into the sampler; src/util/cam_geometry.py:36-79). */
typedef struct DinerTargetCam {
    const float *extrinsics; /* [SB,4,4] world->camera */
    const float *intrinsics; /* [SB,3,3] */
    const float *z_near;     /* [SB] */
    const float *z_far;      /* [SB] */
    int32_t H, W;            /* target image size: rays per scene = H*W, ray r = pixel (r / W, r % W) */
} DinerTargetCam;

/* SpatialEncoder.index's grid_sample settings (src/models/image_encoder.py:24-25,119-125: align_corners=False, mode=index_interp,
 * padding_mode=index_padding), the lookup of the latent features of every point.  Every mode is a footprint of at most 4 texels with
 * weights, evaluated like ATen's grid_sample after the feature_padding rescale of the coordinate:
 *   border     (default): ix clipped to [0, w-1];
 *   reflection: ix reflected over [-0.5, w-0.5] (ATen's reflect_coordinates), then clipped to [0, w-1];
 *   zeros:      ix not clipped; a tap outside the map has weight 0 (the others are not renormalised);
 *   nearest:    one tap of weight 1 at rint(ix), rint(iy) (half to even) of the padded coordinate (zeros: 0 outside the map).
 * The entry points without the _ix suffix are the bilinear / border case of their _ix form.  Unknown values: DINER_E_INVALID. */
#define DINER_INDEX_BILINEAR 0
#define DINER_INDEX_NEAREST 1
#define DINER_INDEX_PAD_BORDER 0
#define DINER_INDEX_PAD_ZEROS 1
#define DINER_INDEX_PAD_REFLECTION 2
typedef struct DinerLatentIndex {
    int32_t interp;          /* DINER_INDEX_BILINEAR | DINER_INDEX_NEAREST */
    int32_t padding;         /* DINER_INDEX_PAD_BORDER | _ZEROS | _REFLECTION */
} DinerLatentIndex;

/* Version of THIS ABI (argument lists, struct layouts).  Bumped by every incompatible change; a binding compiled or written
 * against another value must refuse to call in: diner_version() returns the value the loaded library was built with, the
 * torch-ops extension checks it at every op entry, diner_amd/_lib.py at load time.  (2: diner_render / diner_composite gained
 * `status`.  3: the shape-general inference path, the *_gen entry points below.)  New entry points that leave every existing argument
 * list and struct layout as it was do not bump it (the shape-general training blocks, diner_train_gemm_act and
 * diner_train_point_inputs(_backward)_gen, and the shape-general f16x3 inference path, the *_gen_f16 entry points, came under 3).
 * The shape-general f16x3 training GEMM (diner_train_gemm_act_f16x3, _f16x3_w, diner_train_split_weight(_halfs)) adds symbols only and
 * changes no struct: it came under 3 as well. */
#define DINER_ABI_VERSION 3

const char *diner_last_error(void);
int diner_version(void);

/* ---- adjacent per-image producers, one thread per pixel ---------- */
/* gen_rays (src/util/cam_geometry.py:36-79): extrinsics [B,4,4] world->camera, intrinsics [B,3,3],
 * z_near/z_far [B] -> rays [B,H,W,8] (pixel-centre rays: origin, unit direction, near, far). */
int diner_gen_rays(const float *extrinsics, const float *intrinsics, const float *z_near, const float *z_far,
                   int32_t B, int32_t H, int32_t W, float *rays_out, void *stream);
/* Backward of diner_gen_rays (the reference's gen_rays under autograd): d_rays [B,H,W,8] -> d_extrinsics [B,4,4] (row 3: 0),
 * d_intrinsics [B,3,3] (only fx, fy, cx, cy, i.e. [0,0], [1,1], [0,2], [1,2], are non-zero: the entries gen_rays reads), d_near [B],
 * d_far [B] (sums of d_rays[..., 6] and [..., 7]).  Every output is written (not accumulated).  Per-block partial sums go to the
 * workspace (diner_gen_rays_backward_workspace_floats(B, H, W) floats, 8-byte aligned) and are added in a fixed order, in fp64: the
 * result is bitwise reproducible.  The workspace query returns -1 for bad sizes. */
int64_t diner_gen_rays_backward_workspace_floats(int32_t B, int32_t H, int32_t W);
int diner_gen_rays_backward(const float *extrinsics, const float *intrinsics, const float *d_rays, int32_t B, int32_t H, int32_t W,
                            float *d_extrinsics, float *d_intrinsics, float *d_near, float *d_far, float *workspace, void *stream);
/* depth2normal (src/util/depth2normal.py:7-87): dmap [N,1,H,W], K [N,3,3] -> normals [N,3,H,W]
 * (central differences of the re-projected depth map + the reference's hole clean-up). */
int diner_depth2normal(const float *dmap, const float *intrinsics, int32_t N, int32_t H, int32_t W,
                       float *normals_out, void *stream);

/* ---- once per encode(): re-pack the model's maps for the kernels ----------------------- */
/* depths, depths_std [N,1,H,W], normals [N,3,H,W] (N = SB*NV) -> maps [N,H,W,8] */
int diner_pack_maps(const float *depths, const float *depths_std, const float *normals,
                    int64_t N, int32_t H, int32_t W, float *maps_out, void *stream);
/* the same with depth2normal (src/util/depth2normal.py:7-87, called at src/models/pixelnerf.py:45) fused in:
 * depths, depths_std [N,1,H,W], intrinsics [N,3,3] -> maps [N,H,W,8]; no NCHW normal tensor is materialised */
int diner_pack_maps_from_depth(const float *depths, const float *depths_std, const float *intrinsics,
                               int64_t N, int32_t H, int32_t W, float *maps_out, void *stream);
/* Upstream wire format: TransMVSNet's uint16 depth / confidence planes [N,H,W] ->
 * depth_out, std_out (and mask_out = depth > 0, optional) [N,H/stride,W/stride] fp32, nearest-subsampled by
 * `stride` (src/data/dtu.py:113-117):  depth = ((u16 * mul0) / div) * mul1,  std = std_a * conf + std_b with the
 * confidence decoded like the depth (src/data/dtu.py:100-119,220-223; src/data/facescape.py:54-56,80-91,266).
 * mesh (optional): Facescape's mesh-rendered depth for depth_type "merge" (src/data/facescape.py:96-104). */
int diner_decode_depth_u16(const uint16_t *depth, const uint16_t *conf, const uint16_t *mesh, int64_t N, int32_t H,
                           int32_t W, int32_t stride, float mul0, float div, float mul1, float std_a, float std_b,
                           float *depth_out, float *std_out, float *mask_out, void *stream);
/* latent [N,C,h,w] (NCHW, src/models/image_encoder.py:271) -> [N,h,w,C] with the channel order
 * the MLP kernel stages into LDS (C = 512; any other multiple of 8 up to 1024 for the shape-general path) */
int diner_pack_latent(const float *latent_nchw, int64_t N, int32_t C, int32_t h, int32_t w,
                      float *latent_out, void *stream);
/* ---- the latent assembled from the encoder's feature pyramid, directly in diner_pack_latent's layout ----
 * Replaces the tail of SpatialEncoder.forward (src/models/image_encoder.py:262-272): every level upsampled to the first level's size
 * with F.interpolate(mode="bilinear", align_corners=True), then torch.cat along the channels -- and the diner_pack_latent that followed.
 * A level: NCHW [N, C, h, w], contiguous; C a multiple of 8; a level may be larger or smaller than the output.  The output has
 * C = sum of the levels' C (at most 1024, diner_pack_latent's limit), N = SB * NV images; element offsets are 64-bit.
 *   out[n, y, x, off_l + c] = bilinear(level_l[n, c])(y, x) with ATen's align_corners=True taps: scale = (in - 1) / (out - 1) in fp32
 *   (0 when out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1,
 *   value = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d): a level of the output's size comes out bit-identical.
 * diner_assemble_latent_backward is the exact adjoint in gather form: every coarse texel sums weight * d_out over the fine pixels whose
 * i0 or i1 is that texel, in a fixed order (no atomics: run-to-run deterministic), with the taps of the same device function as the
 * forward.  levels_grad: the levels' shapes with `data` = the gradient buffers, NCHW, every element of which is WRITTEN (no pre-zeroing;
 * the descriptor is shared by both directions, hence the const of the field).
 * Before any launch: DINER_E_INVALID for a NULL pointer, n_levels outside 1..DINER_LATENT_MAX_LEVELS or a non-positive size;
 * DINER_E_UNSUPPORTED for a channel count outside the envelope (or N > 65535 images). */
#define DINER_LATENT_MAX_LEVELS 5
typedef struct DinerLatentLevel {
    const float *data;       /* [N, C, h, w] */
    int32_t C, h, w;
} DinerLatentLevel;
typedef struct DinerLatentLevels {
    DinerLatentLevel level[DINER_LATENT_MAX_LEVELS];   /* the first n_levels are read */
} DinerLatentLevels;
int diner_assemble_latent(const DinerLatentLevels *levels, int32_t n_levels, int64_t N, int32_t h, int32_t w, float *out_nhwc,
                          void *stream);
int diner_assemble_latent_backward(const float *d_out_nhwc, int32_t n_levels, int64_t N, int32_t h, int32_t w,
                                   const DinerLatentLevels *levels_grad, void *stream);
/* The same tail for SpatialEncoder's upsample_interp = "bicubic" (src/models/image_encoder.py:262-272 with
 * F.interpolate(mode="bicubic", align_corners=True); "bilinear" and "bicubic" are the two modes torch accepts there): the same level
 * descriptors, envelope (1..5 levels, every C_l a multiple of 8, C <= 1024, N <= 65535), output layout and refusals as the pair above, with
 * messages that start with "assemble_latent_bicubic".  ATen's upsample_bicubic2d, per axis:
 *   scale = (in - 1) / (out - 1) in fp32 (0 when out == 1);  src = scale * dst;  i = min((int)src, in - 1);  t = src - i;
 *   taps i - 1, i, i + 1, i + 2, each clamped to [0, in - 1];  A = -0.75;
 *   w0 = ((A (t + 1) - 5 A) (t + 1) + 8 A) (t + 1) - 4 A       w1 = ((A + 2) t - (A + 3)) t t + 1
 *   w3 = ((A (2 - t) - 5 A) (2 - t) + 8 A) (2 - t) - 4 A       w2 = ((A + 2) (1 - t) - (A + 3)) (1 - t) (1 - t) + 1
 *   out[n, y, x, off_l + c] = sum_i wy_i * (sum_j wx_j * level_l[n, c, iy_i, ix_j])   (rows inside, then columns; sums left to right).
 * The four cubics are evaluated in their factored forms, w0 = A t (1 - t)^2, w1 = (1 - t) (1 + t - (A + 2) t^2), w2 = w1(1 - t),
 * w3 = w0(1 - t): the same polynomials, each coefficient within a few ulp of itself (the Horner forms above leave up to 12 * 2^-24
 * absolute on coefficients as small as 0.02, which the gradient of a level larger than the output would show).
 * A level of the output's size is copied: bit-identical whatever it holds (t = 0 gives the weights (0, 1, 0, 0), but 0 * inf never occurs).
 * diner_assemble_latent_bicubic_backward is the exact adjoint in gather form: every coarse texel sums weight * d_out over the fine pixels
 * that have at least one clamped tap on it, rows outside, columns inside, ascending (no atomics: run-to-run deterministic); per axis the
 * weight is the sum of the coefficients whose clamped tap is the texel (at a border several taps of one fine pixel land on it), from the
 * same device function as the forward.  Every element of every level's gradient is WRITTEN. */
int diner_assemble_latent_bicubic(const DinerLatentLevels *levels, int32_t n_levels, int64_t N, int32_t h, int32_t w, float *out_nhwc,
                                  void *stream);
int diner_assemble_latent_bicubic_backward(const float *d_out_nhwc, int32_t n_levels, int64_t N, int32_t h, int32_t w,
                                           const DinerLatentLevels *levels_grad, void *stream);
/* ---- once per encode(): conv1's input, the head of the encoder ----------------------------- */
/* Replaces PixelNeRF.encode's Normalize (src/models/pixelnerf.py:44) and the head of SpatialEncoder.forward (pad_layer, linspace /
 * meshgrid / PositionalEncoding / interior zeroing / expand / cat, src/models/image_encoder.py:222-232) in one launch (New symbols only:
 * DINER_ABI_VERSION stays 3).  images [N,3,H,W] -> out [N, 3 + Cpe, Hp, Wp], Hp = H + 2 pad, Wp = W + 2 pad (pad = image_padding):
 *   channels 0..2:  (images[n, c, clamp(y - pad, 0, H - 1), clamp(x - pad, 0, W - 1)] - mean[c]) / std[c] -- an fp32 subtract and a true
 *                   fp32 divide, bit-equal to Normalize + ReplicationPad2d; pad may exceed H or W;
 *   channels 3..:   present iff pe_freqs >= 0 && pad > 0 (the reference's padding_pe >= 0 and feature_padding > 0), Cpe = 2 (1 + 2F),
 *                   F = pe_freqs (-1: none; 0: the two raw coordinates only).  0 where pad <= y < Hp - pad && pad <= x < Wp - pad;
 *                   elsewhere, with v = (xs[x], ys[y]): [v_0, v_1, e_0, ...], e[2 j + i] = sin(phi_j + v_i f_(j / 2)), j = 0..2F-1,
 *                   f_k = fp32(pi) 2^k, phi_j = 0 (j even) / fp32(pi / 2) (j odd): PositionalEncoding(F, freq_factor = pi, d_in = 2)
 *                   (src/models/positional_encoding.py:14-53).  The same values for every n: computed once per pixel.
 * xs [Wp], ys [Hp]: the pixel coordinates, torch.linspace(-1, 1, Wp) / (.., Hp) made by the caller (read only with the encoding on, may be
 * NULL otherwise).  mean / std: the three channel constants by value.  `out` 16-byte aligned with Wp % 4 == 0 takes 16-byte stores.
 * diner_encoder_input_backward is the adjoint to the images: d_images[n,c,y,x] = (sum of d_out[n,c,y',x'] over every (y',x') whose clamp
 * lands on (y,x)) / std[c], a gather with a fixed summation order (no atomics: two runs agree bit for bit); the encoding's channels of
 * d_out [N, 3 + Cpe, Hp, Wp] carry no gradient and are not read.  Every element of d_images [N,3,H,W] is written.
 * Before any launch: DINER_E_INVALID for a NULL pointer, N / H / W <= 0, pad < 0, pe_freqs < -1, Hp or Wp below 2, or a std of 0;
 * DINER_E_UNSUPPORTED for pe_freqs > 30, a padded size of 2^30 or more, N > 65535 images (forward) or pad > 4095 (backward only). */
int diner_encoder_input(const float *images, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, const float *xs,
                        const float *ys, float mean0, float mean1, float mean2, float std0, float std1, float std2, float *out,
                        void *stream);
int diner_encoder_input_backward(const float *d_out, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, float std0, float std1,
                                 float std2, float *d_images, void *stream);
/* ---- once per training step: ray selection and the photometric losses (csrc/train_glue.hip) ---- */
/* The two stretches of DINER.calc_losses (src/models/diner.py:217-290) around renderer.forward (New symbols only: DINER_ABI_VERSION stays
 * 3).  pix_idcs [SB,B]: the selected pixels, idx = x + y W (diner.py:246), int64 (idx_is_int64 != 0) or int32; an index outside
 * [0, H W) is clamped into it -- nothing is read or written out of bounds, the result for such an index is unspecified.
 *
 * diner_gen_rays_at replaces gen_rays + the selection rays.view(SB, H*W, -1)[batch_idx_helper, pix_idcs] (diner.py:224-227, :257-258):
 * rays_out [SB,B,8], ray (b, j) = diner_gen_rays' ray of camera b at pixel pix_idcs[b, j], bit for bit (one device function computes
 * both).  diner_gen_rays_at_backward: d_rays [SB,B,8] -> the outputs of diner_gen_rays_backward (every one written, not accumulated);
 * reads d_rays and the indices only, a pixel selected twice is two terms.  The same 18 per-camera sums in fp64: per-block partials in the
 * workspace (diner_gen_rays_at_backward_workspace_floats(SB, B) floats, 8-byte aligned; -1 for bad sizes), a block count that depends on
 * B only, added in block order -- no atomics, bitwise reproducible.
 * Before any launch: DINER_E_INVALID for a NULL pointer, SB or B < 0, H or W <= 0, H W >= 2^31; DINER_E_UNSUPPORTED for SB > 65535 or
 * SB B >= 2^31. */
int diner_gen_rays_at(const float *extrinsics, const float *intrinsics, const float *z_near, const float *z_far, const void *pix_idcs,
                      int32_t idx_is_int64, int32_t SB, int32_t B, int32_t H, int32_t W, float *rays_out, void *stream);
int64_t diner_gen_rays_at_backward_workspace_floats(int32_t SB, int32_t B);
int diner_gen_rays_at_backward(const float *extrinsics, const float *intrinsics, const float *d_rays, const void *pix_idcs,
                               int32_t idx_is_int64, int32_t SB, int32_t B, int32_t H, int32_t W, float *d_extrinsics, float *d_intrinsics,
                               float *d_near, float *d_far, float *workspace, void *stream);
/* diner_photo_loss replaces the ground-truth gather target_rgb.view(SB, 3, -1).permute(0, 2, 1)[batch_idx_helper, pix_idcs]
 * (diner.py:265), MSELoss (:267) and AntibiasLoss on the two patches (:280-282, src/losses/antibiasloss.py: AvgPool2d(pool) of both, then
 * L1Loss).  pred [SB,B,3] (the renderer's fine.rgb), target_rgb [SB,3,H,W] ->
 *   gt_colors_out [SB,B,3]   = target_rgb[b, :, y, x] at pixel pix_idcs[b, j], bit for bit;
 *   losses_out[0]            = sum (pred - gt)^2 / (SB B 3);
 *   losses_out[1]            = with patch = s > 0 (B == s s, ray j = row j / s, column j % s, as view(SB, s, s, 3)) and pool = p = 2^n:
 *                              sum |avg_cell(pred) - avg_cell(gt)| / (SB 3 nc^2) over the nc = s / p (floor) cells per side and channel
 *                              (AvgPool2d's floor semantics: trailing rows / columns that fill no cell are ignored); 0 with patch = 0;
 *   cell_sign_out [SB,3,nc,nc] = sign of that pooled difference (-1, 0, 1), kept for the backward (not read with patch = 0, may be NULL).
 * Prediction and ground truth of a cell are pooled separately, in the same order, then subtracted: equal cells give an exact 0.  One
 * workgroup per (scene, cell row, chunk of cells) -- or 1024 rays without a patch -- writes an fp64 partial pair to the workspace
 * (diner_photo_loss_workspace_floats floats, 8-byte aligned; -1 for bad sizes), a one-block pass adds them in block order: no atomics,
 * bitwise reproducible.
 * diner_photo_loss_backward: d_pred_out [SB,B,3] = g_mse 2 (pred - gt) / (SB B 3) + g_ab cell_sign / (p^2 SB 3 nc^2), formed in fp64 and
 * rounded once; a pixel outside every cell gets the first term only.  g_mse, g_ab: device scalars (NULL: 0).  target_rgb and the indices
 * get no gradient.
 * Before any launch: DINER_E_INVALID for a NULL pointer, SB or B <= 0, B != s s, pool not a power of two, s < pool;
 * DINER_E_UNSUPPORTED for pool > 32 (a cell row is pooled from LDS) and the limits of diner_gen_rays_at. */
int64_t diner_photo_loss_workspace_floats(int32_t SB, int32_t B, int32_t patch, int32_t pool);
int diner_photo_loss(const float *pred, const float *target_rgb, const void *pix_idcs, int32_t idx_is_int64, int32_t SB, int32_t B, int32_t H,
                     int32_t W, int32_t patch, int32_t pool, float *gt_colors_out, float *losses_out, float *cell_sign_out, float *workspace,
                     void *stream);
int diner_photo_loss_backward(const float *pred, const float *gt_colors, const float *cell_sign, const float *g_mse, const float *g_ab,
                              int32_t SB, int32_t B, int32_t patch, int32_t pool, float *d_pred_out, void *stream);
/* ---- once per weight version: MFMA-fragment-ordered copies of the fusion MLP (one image per
 * precision mode, both in the same buffer) ------------------------------------------------ */
int64_t diner_mlp_packed_floats(void);
int diner_pack_mlp(const DinerMlpRaw *raw, float *packed_out, void *stream);
/* ---- once per (encode, weight version): G_b = lin_z[b](latent), b = 0..2, as feature maps ----
 * lin_z (src/models/resnetfc.py:152) is linear and SpatialEncoder.index (src/models/image_encoder.py:97-127)
 * is a 4-texel convex combination, so lin_z[b](index(uv)) == bilerp(G_b)(uv) up to fp32 rounding.
 * latent_packed [N,h,w,512] from diner_pack_latent, mlp_packed from diner_pack_mlp -> out [3][N,h,w,512]. */
int diner_pack_linz_maps(const float *latent_packed, int64_t N, int32_t h, int32_t w, const float *mlp_packed,
                         float *out, void *stream);
/* The maps for a lookup mode.  With DINER_INDEX_PAD_ZEROS the convex-combination argument above fails near the border (the weights
 * of the in-map taps sum to less than 1, and the folded biases would shrink with them), so the maps get a one-texel ring of texels
 * that hold lin_z[b](0) + the folded biases, i.e. the biases alone: out [3][N,h+2,w+2,512], the interior at (y+1, x+1).  The F16X3
 * kernel then sends the taps outside the map to the ring with their full weight, and the weights again sum to 1.  Every other
 * mode: exactly diner_pack_linz_maps.  diner_linz_maps_floats gives the size of `out`. */
int64_t diner_linz_maps_floats(int64_t N, int32_t h, int32_t w, const DinerLatentIndex *index);
int diner_pack_linz_maps_ix(const float *latent_packed, int64_t N, int32_t h, int32_t w, const float *mlp_packed,
                            const DinerLatentIndex *index, float *out, void *stream);

/* ---- the hot path ---------------------------------------------------------------------- */
/* Stage entry points with the reference's stage boundaries (for stage-level parity tests and for
 * callers that use the stages on their own): */
/* NeRFRendererDGS.sample_coarse (src/models/nerf_renderer.py:39-63): rays [N,8] -> z [N,NC];
 * u_coarse [N,NC] or NULL (Philox keyed on seed). */
int diner_sample_coarse(const float *rays, int64_t N, int32_t NC, const float *u_coarse, uint64_t seed,
                        float *z_out, void *stream);
/* NeRFRendererDGS.fill_up_uniform_samples (src/models/nerf_renderer.py:367-397): z_in [N,K] with
 * 0 = empty slot -> z_out [N,K] filled and sorted; u_fill [N,K] (column i feeds the i-th empty
 * slot) or NULL. */
int diner_fill_up_uniform_samples(const float *rays, const float *z_in, int64_t N, int32_t K,
                                  const float *u_fill, uint64_t seed, float *z_out, void *stream);

/* Replaces NeRFRendererDGS.sample_coarse + sample_depthguided + fill_up_uniform_samples
 * (src/models/nerf_renderer.py:39-63, 65-284, 367-397).  One ray per wavefront.
 *   noise (parity mode, any may be NULL -> in-kernel Philox keyed on `seed`):
 *     u_coarse [SB,NR,NC] U[0,1);  n_gauss [SB,NR,G] N(0,1), row used iff the ray has a hit;
 *     u_fill [SB,NR,K] U[0,1), column i feeds the i-th empty slot of the ray.
 *   z_cand  [SB,NR,NC] optional: inject the candidates instead of computing them (tests).
 *   z_out   [SB,NR,K] sorted samples (what composite() consumes).
 *   z_dg_out [SB,NR,K] optional: samples BEFORE fill-up, kept candidates first (0 = empty),
 *            gaussian draws in the last G slots (the return value of sample_depthguided).
 *   lik_out [SB,NR,NC] optional: per-candidate likelihood max over views (:129). */
int diner_sample_depthguided(const DinerScene *scene, const float *rays, int64_t NR,
                             const DinerSamplerCfg *cfg, const float *u_coarse,
                             const float *n_gauss, const float *u_fill, const float *z_cand,
                             uint64_t seed, float *z_out, float *z_dg_out, float *lik_out,
                             void *stream);

/* Replaces the model evaluation inside composite(): points = o + z*d (:304-307) and
 * PixelNeRF.forward (src/models/pixelnerf.py:55-145) incl. PositionalEncoding.forward,
 * SpatialEncoder.index / index_depth and ResnetFC.forward.  z [SB,NR,K] -> rgbsigma [SB,NR,K,4].
 * mlp_packed from diner_pack_mlp.  scratch: device buffer of diner_render_points_scratch_floats()
 * floats (the F16X3 kernel parks per-view hidden states there until the mean over views; may be
 * NULL when that is 0); one buffer per concurrently running launch. */
int64_t diner_render_points_scratch_floats(int64_t SB, int32_t NV, int32_t precision);
int diner_render_points(const DinerScene *scene, const float *mlp_packed, const float *rays,
                        const float *z, int64_t NR, int32_t K, int32_t precision, float *scratch,
                        float *rgbsigma_out, void *stream);
/* with the latent lookup `index` (NULL = bilinear / border).
 * F16X3 with scene->linz_maps and DINER_INDEX_PAD_ZEROS: linz_maps MUST be the ringed maps of diner_pack_linz_maps_ix for that mode
 * ([3][SB,NV,h+2,w+2,C], diner_linz_maps_floats); the kernel reads that many texels.  DinerScene does not record the layout: a
 * buffer whose allocation ends before the ringed size is refused (DINER_E_INVALID), plain maps inside a larger allocation would be
 * read as ringed ones (wrong values).  Every other mode reads the plain maps of diner_pack_linz_maps. */
int diner_render_points_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *mlp_packed, const float *rays,
                           const float *z, int64_t NR, int32_t K, int32_t precision, float *scratch, float *rgbsigma_out,
                           void *stream);

/* Replaces the alpha compositing of composite() (src/models/nerf_renderer.py:299-301,341-360).
 * N rays (= SB*NR).  weights_out [N,K] optional.
 * status (optional): one device word, OR-ed with DINER_STATUS_NONFINITE when any rgb-sigma sample is inf/NaN
 * (the reference would hand NaN images on silently; in f16x3 mode it means an activation left the fp16 range,
 * |x| >= ~1e6, and the frame must be re-rendered with DINER_PRECISION_FP32).  Sticky: the caller clears it. */
#define DINER_STATUS_NONFINITE 1u
int diner_composite(const float *rays, const float *z, const float *rgbsigma, int64_t N, int32_t K,
                    int32_t white_bkgd, float *rgb_out, float *depth_out, float *weights_out,
                    uint32_t *status, void *stream);

/* Replaces NeRFRendererDGS.forward (src/models/nerf_renderer.py:399-424): the three stages
 * back to back on `stream`.  workspace: device buffer of diner_render_workspace_floats(...)
 * floats (holds z, rgbsigma and the point kernel's scratch). */
int64_t diner_render_workspace_floats(int64_t SB, int64_t NR, int32_t K, int32_t NV, int32_t precision);
int diner_render(const DinerScene *scene, const float *mlp_packed, const float *rays, int64_t NR,
                 const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, const float *u_coarse,
                 const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace,
                 float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);
int diner_render_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *mlp_packed, const float *rays, int64_t NR,
                    const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, const float *u_coarse,
                    const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace,
                    float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);

/* Replaces the render half of DINER.predict_imgs_from_batch (src/models/diner.py:75-97): gen_rays
 * (src/util/cam_geometry.py:36-79) is evaluated INSIDE the sampler kernel -- a wave computes its ray from the pixel index and
 * the target camera, and stores it once for the two later stages -- then the three stages run as in diner_render.
 * workspace: diner_render_image_workspace_floats(...) floats (rays | z | rgbsigma | scratch).  Outputs [SB,H*W,3], [SB,H*W],
 * [SB,H*W,K]|NULL; rays_out [SB,H*W,8]|NULL also hands the generated rays to the caller. */
int64_t diner_render_image_workspace_floats(int64_t SB, int32_t H, int32_t W, int32_t K, int32_t NV, int32_t precision);
int diner_render_image(const DinerScene *scene, const float *mlp_packed, const DinerTargetCam *cam,
                       const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, uint64_t seed,
                       float *workspace, float *rays_out, float *rgb_out, float *depth_out, float *weights_out,
                       uint32_t *status, void *stream);
int diner_render_image_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *mlp_packed, const DinerTargetCam *cam,
                          const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, uint64_t seed, float *workspace,
                          float *rays_out, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);

/* ---- shape-general inference path ----------------------------------------------------------------------------------------
 * The entry points above serve the one model the configs ship (DINER_D_* above).  The reference renders any ResnetFC /
 * PositionalEncoding its constructors accept (src/models/pixelnerf.py:14-24, src/models/resnetfc.py:72-127,
 * src/models/positional_encoding.py:9-31); these entry points take the shape at run time and evaluate it with exact fp32 MFMA
 * (the arithmetic of DINER_PRECISION_FP32) in a second point/MLP kernel.  Envelope (anything else: DINER_E_UNSUPPORTED with
 * the reason in diner_last_error()):
 *   d_hidden a multiple of 32 in [32, 512]; d_latent a multiple of 8 in [8, 1024]; n_blocks in [1, 64]; combine_layer >= 0
 *   (>= n_blocks: no mean over views, which the reference supports for NV = 1 only, src/models/pixelnerf.py:137);
 *   num_freqs F >= 1 with d_in = 7 + 8F <= 512 (both encodings, include_input); activation ReLU (beta = 0) or
 *   Softplus(beta) (beta > 0); d_out = 4; combine_type average. */
#define DINER_COMBINE_AVERAGE 0
typedef struct DinerMlpShape {
    int32_t d_in, d_latent, d_hidden, n_blocks, combine_layer, num_freqs;
    float beta;              /* Softplus beta; 0 = ReLU (resnetfc.py:124-127) */
    int32_t d_out;           /* must be 4 */
    int32_t combine_type;    /* must be DINER_COMBINE_AVERAGE */
} DinerMlpShape;

/* ResnetFC parameters of any shape, nn.Linear layout weight [out,in].  The per-block members are HOST arrays of device pointers:
 * lin_z_*: min(combine_layer, n_blocks) entries ([d_hidden,d_latent], [d_hidden]); fc0_*, fc1_*: n_blocks entries
 * ([d_hidden,d_hidden], [d_hidden]). */
typedef struct DinerMlpGenRaw {
    const float *lin_in_w, *lin_in_b;                  /* [d_hidden,d_in], [d_hidden] */
    const float *const *lin_z_w, *const *lin_z_b;
    const float *const *fc0_w, *const *fc0_b;
    const float *const *fc1_w, *const *fc1_b;
    const float *lin_out_w, *lin_out_b;                /* [4,d_hidden], [4] */
} DinerMlpGenRaw;

/* floats of the packed image of a shape (< 0: the DINER_E_* code of an unsupported shape) */
int64_t diner_mlp_gen_packed_floats(const DinerMlpShape *shape);
int diner_pack_mlp_gen(const DinerMlpShape *shape, const DinerMlpGenRaw *raw, float *packed_out, void *stream);
/* diner_render_points for a shape: mlp_packed from diner_pack_mlp_gen; scene->C must be d_latent and scene->num_freqs F */
int diner_render_points_gen(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const float *rays,
                            const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream);
/* diner_render / diner_render_image for a shape (workspace: diner_render_workspace_floats / diner_render_image_workspace_floats
 * with DINER_PRECISION_FP32) */
int diner_render_gen(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const float *rays, int64_t NR,
                     const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse, const float *n_gauss, const float *u_fill,
                     uint64_t seed, float *workspace, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status,
                     void *stream);
int diner_render_image_gen(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const DinerTargetCam *cam,
                           const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed, float *workspace, float *rays_out,
                           float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);
/* the same with a latent lookup mode (NULL = bilinear / border) */
int diner_render_points_gen_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,
                               const float *mlp_packed, const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out,
                               void *stream);
int diner_render_gen_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                        const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,
                        const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                        float *weights_out, uint32_t *status, void *stream);
int diner_render_image_gen_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                              const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed, float *workspace,
                              float *rays_out, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);

/* ---- shape-general inference path in split fp16 (points_mlp_gen_f16.hip) -----------------------------------------------------
 * The *_gen entry points above with the arithmetic of DINER_PRECISION_F16X3 (three fp16 MFMAs per product on hi / lo operand halves,
 * fp32 accumulation, the hidden state carried * 2^-4; an activation beyond the fp16 range makes the sample non-finite and
 * diner_composite raises DINER_STATUS_NONFINITE): same envelope, same DinerMlpShape / DinerMlpGenRaw, same argument lists, inference
 * only.  The packed image is another one: fp16 hi / lo weight fragments followed by fp32 biases and lin_out, 16-byte aligned.
 * diner_mlp_gen_f16_packed_floats / diner_pack_mlp_gen_f16 replace what ResnetFC.__init__ / load_state_dict leave in nn.Linear
 * layout (src/models/resnetfc.py:72-127), as diner_pack_mlp_gen does. */
int64_t diner_mlp_gen_f16_packed_floats(const DinerMlpShape *shape);   /* < 0: the DINER_E_* code of an unsupported shape */
int diner_pack_mlp_gen_f16(const DinerMlpShape *shape, const DinerMlpGenRaw *raw, float *packed_out, void *stream);
/* Replaces PixelNeRF.forward + ResnetFC.forward per point (src/models/pixelnerf.py:55-145, src/models/resnetfc.py:129-159), as
 * diner_render_points_gen does; mlp_packed from diner_pack_mlp_gen_f16 */
int diner_render_points_gen_f16(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const float *rays,
                                const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream);
/* Replace NeRFRendererDGS.forward (src/models/nerf_renderer.py:399-424) and the render half of DINER.predict_imgs_from_batch
 * (src/models/diner.py:75-97), as diner_render_gen / diner_render_image_gen do.  workspace: diner_render_workspace_floats /
 * diner_render_image_workspace_floats with DINER_PRECISION_FP32 (this kernel needs no scratch beyond z and rgbsigma; the
 * DINER_PRECISION_F16X3 size is that of the standard kernel's view-sum slabs and is not needed here) */
int diner_render_gen_f16(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const float *rays, int64_t NR,
                         const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse, const float *n_gauss,
                         const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out, float *weights_out,
                         uint32_t *status, void *stream);
int diner_render_image_gen_f16(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const DinerTargetCam *cam,
                               const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed, float *workspace, float *rays_out,
                               float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);
/* the same with a latent lookup mode (NULL = bilinear / border; SpatialEncoder.index, src/models/image_encoder.py:97-127) */
int diner_render_points_gen_f16_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,
                                   const float *mlp_packed, const float *rays, const float *z, int64_t NR, int32_t K,
                                   float *rgbsigma_out, void *stream);
int diner_render_gen_f16_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                            const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,
                            const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out,
                            float *depth_out, float *weights_out, uint32_t *status, void *stream);
int diner_render_image_gen_f16_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,
                                  const float *mlp_packed, const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd,
                                  uint64_t seed, float *workspace, float *rays_out, float *rgb_out, float *depth_out,
                                  float *weights_out, uint32_t *status, void *stream);

/* ---- the bicubic latent lookup: SpatialEncoder.index with index_interp="bicubic" (src/models/image_encoder.py:119-125:
 * F.grid_sample(mode="bicubic", align_corners=False, padding_mode=index_padding) at the feature_padding-rescaled uv of :113-114) on the
 * shape-general kernels (points_mlp_gen_bc.hip, points_mlp_gen_f16_bc.hip).  ATen's semantics: the centre coordinate
 * ix = ((u sxl + 1) w - 1) / 2 is neither clipped nor reflected; x0 = floor(ix), tx = ix - x0; four cubic-convolution weights per axis
 * (A = -0.75) at distances tx + 1, tx, 1 - tx, 2 - tx; the 16 taps sit at (x0 - 1 + i, y0 - 1 + j) and every integer tap position goes
 * through the padding on its own (border: clamped; reflection: reflected over [-0.5, size - 0.5], then clamped; zeros: a tap outside
 * the map contributes 0); result = sum_j cy_j (sum_i cx_i texel_ij).  Every index is clamped into the map, whatever the coordinate.
 * Bicubic does not travel in DinerLatentIndex (the _ix entry points keep rejecting interp = 2): these entry points take the argument
 * lists of their _gen_ix forms with `padding` (DINER_INDEX_PAD_*) in place of the DinerLatentIndex pointer; any other padding value:
 * DINER_E_INVALID.  New symbols only: DINER_ABI_VERSION stays 3.  The 512-wide kernels and the lin_z maps do not serve bicubic. */
/* Replaces PixelNeRF.forward + ResnetFC.forward per point (src/models/pixelnerf.py:55-145, src/models/resnetfc.py:129-159) with the
 * encoder's index() of src/models/image_encoder.py:97-127 in bicubic mode; mlp_packed from diner_pack_mlp_gen / _gen_f16 */
int diner_render_points_gen_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,
                               const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream);
int diner_render_points_gen_f16_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,
                                   const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream);
/* Replace NeRFRendererDGS.forward (src/models/nerf_renderer.py:399-424) for such a model, as diner_render_gen_ix does */
int diner_render_gen_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed, const float *rays,
                        int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse, const float *n_gauss,
                        const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out, float *weights_out,
                        uint32_t *status, void *stream);
int diner_render_gen_f16_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,
                            const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,
                            const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                            float *weights_out, uint32_t *status, void *stream);
/* Replace the render half of DINER.predict_imgs_from_batch (src/models/diner.py:75-97), as diner_render_image_gen_ix does */
int diner_render_image_gen_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,
                              const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed, float *workspace,
                              float *rays_out, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream);
int diner_render_image_gen_f16_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,
                                  const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed,
                                  float *workspace, float *rays_out, float *rgb_out, float *depth_out, float *weights_out,
                                  uint32_t *status, void *stream);

/* ---- lin_z hoisted into per-texel maps on the shape-general kernels (linz_maps_gen.hip, points_mlp_gen_lz.hip,
 * points_mlp_gen_f16_lz.hip and their _bc twins).  ResnetFC.forward's `x = x + self.lin_z[blkid](z)` (src/models/resnetfc.py:152-153) is
 * linear and z = SpatialEncoder.index (src/models/image_encoder.py:97-127) a weighted sum of texels, so
 * lin_z[b](z) = sum_i w_i (W_b F_i) + bias_b.  A map is M_b[sb, v, y, x, :] = W_z[b] . F[sb, v, y, x, :]: d_hidden floats per latent
 * texel, NHWC fp32, layout [nlz][SB, NV, h, w, d_hidden], nlz = min(combine_layer, n_blocks), WITHOUT lin_z[b].bias (unlike
 * diner_pack_linz_maps): exactly linear in the taps, so the same maps serve every lookup mode -- bilinear / nearest, border / zeros /
 * reflection, and bicubic -- with no ring of extra texels.  Memory: nlz * d_hidden / d_latent times the latent.  The point kernels
 * gather d_hidden channels of M_b through the lookup's taps and add them to the fp32 accumulator in place of the per-point lin_z GEMM;
 * everything else is the arithmetic of the *_gen / *_gen_f16 entry points.  New symbols only: DINER_ABI_VERSION stays 3; the other
 * *_gen* entry points keep ignoring scene->linz_maps. */
/* floats of the maps of a scene (SB, NV, h, w are read): 0 when nlz = 0; < 0: DINER_E_INVALID, or the DINER_E_* code of an unsupported
 * shape (that of diner_mlp_gen_packed_floats) */
int64_t diner_linz_maps_gen_floats(const DinerScene *scene, const DinerMlpShape *shape);
/* Replaces the lin_z[b](z) Linear layers of ResnetFC.forward (src/models/resnetfc.py:152-153), per texel instead of per point: an exact
 * fp32 MFMA GEMM of scene->latent (NHWC, diner_pack_latent) with each lin_z[b] of mlp_packed = the image of diner_pack_mlp_gen (the fp32
 * one, for both precisions).  Writes diner_linz_maps_gen_floats floats; nlz = 0: nothing. */
int diner_pack_linz_maps_gen(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, float *maps_out, void *stream);
/* Replace PixelNeRF.forward + ResnetFC.forward per point (src/models/pixelnerf.py:55-145, src/models/resnetfc.py:129-159),
 * NeRFRendererDGS.forward (src/models/nerf_renderer.py:399-424) and the render half of DINER.predict_imgs_from_batch
 * (src/models/diner.py:75-97), as their _gen_ix forms do.  One family for both precisions and every lookup: the argument lists of the
 * _gen_ix forms, then precision (DINER_PRECISION_FP32: mlp_packed from diner_pack_mlp_gen; DINER_PRECISION_F16X3: from
 * diner_pack_mlp_gen_f16), bicubic_padding (-1: the lookup of `index`, NULL = bilinear / border; otherwise DINER_INDEX_PAD_* of the
 * bicubic lookup, `index` is then ignored) and linz_maps_gen (diner_pack_linz_maps_gen's output; with nlz = 0 it is not read and the
 * call is that of the _gen_ix / _gen_bc form).  DINER_E_INVALID: NULL maps with nlz > 0, precision or bicubic_padding out of range. */
int diner_render_points_gen_lz(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                               const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream,
                               int32_t precision, int32_t bicubic_padding, const float *linz_maps_gen);
int diner_render_gen_lz(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                        const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,
                        const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                        float *weights_out, uint32_t *status, void *stream, int32_t precision, int32_t bicubic_padding,
                        const float *linz_maps_gen);
int diner_render_image_gen_lz(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                              const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed, float *workspace,
                              float *rays_out, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream,
                              int32_t precision, int32_t bicubic_padding, const float *linz_maps_gen);

/* ---- training path: building blocks of the forward-with-saved-activations and
 * the backward of composite (src/models/nerf_renderer.py:286-365) + PixelNeRF.forward
 * (src/models/pixelnerf.py:55-145) + ResnetFC.forward (src/models/resnetfc.py:129-159), orchestrated by
 * diner_amd/training.py exactly like autograd orchestrates the reference's ATen ops.  Gradients: MLP
 * parameters and encoder.latent (NCHW); the sampler is @torch.no_grad in the reference. ------------------ */
/* C[m][n] (+)= sum_k opA(A[m*sam + k*sak]) * opB(B[k*sbk + n*sbn]) (+ bias[n]) (* [S[m*lds + n] > 0]).
 * Each operand must be contiguous along one of its two indices, with that index's extent and the other
 * index's stride multiples of 4 (as diner_train_gemm_act); N % 4 == 0; k_chunk (0 = no split, else a
 * multiple of 32) splits the contraction over blockIdx.z (use with atomic = 1).
 * precision DINER_PRECISION_FP32: exact fp32 MFMA (amax / exp arguments ignored).
 * precision DINER_PRECISION_F16X3: each operand element is multiplied by a power of two, split into fp16
 * hi + lo, three fp16 MFMAs per product, fp32 accumulate (the arithmetic of diner_render_points' default
 * mode).  The power of two is 2^exp_a (2^exp_b), or, when amax_a (amax_b) is not NULL, the one that maps the
 * value stored there by diner_train_amax into [2^13, 2^14) -- meant for gradients, whose magnitude is
 * arbitrary while fp16 has an absolute floor of 2^-24.  C is divided by the product of the two scales. */
int diner_train_gemm(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M,
                     int32_t N, int32_t K, int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc,
                     int64_t lds, int32_t relu_a, int32_t relu_b, int32_t accumulate, int32_t atomic,
                     int64_t k_chunk, int32_t precision, const void *amax_a, const void *amax_b, int32_t exp_a,
                     int32_t exp_b, void *stream);
/* *amax_out (one 32-bit device word) = bit pattern of max |x[i]|, i < n (0 for an empty or all-zero tensor) */
int diner_train_amax(const float *x, int64_t n, void *amax_out, void *stream);
/* Both reductions of a gradient matrix in one pass: db[n] += sum_m dY[m*ld + n] (skipped if db is NULL) and
 * *amax_out as diner_train_amax (skipped if NULL).  N % 4 == 0 and N/4 must divide 256. */
int diner_train_colsum_amax(const float *dY, int64_t M, int32_t N, int64_t ld, float *db, void *amax_out, void *stream);
/* Weight operand of diner_train_gemm_panel: B[n][k] = (transpose ? W[k*ld + n] : W[n*ld + k]) * 2^exp, n < 512,
 * k < K, as fp16 hi / lo planes of 512 * ceil32(K) halfs each, laid out [k/32][512][32] (one k-step of the GEMM
 * is one contiguous 32-KiB piece per plane), zero-padded in k. */
int diner_train_split_panel(const float *W, int32_t K, int64_t ld, int32_t transpose, int32_t exp, void *hi, void *lo,
                            void *stream);
/* C[m][n] = addend[m*ldadd + n] + (sum_k opA(A[m*sam + k]) * B[n][k] + bias[n]) * [S[m*lds + n] > 0], n < 512:
 * the forward and dX GEMMs of the training path in f16x3 arithmetic (see diner_train_gemm) with the weights
 * arriving pre-split (no conversion work for them in the GEMM) and A split twice instead of four times.  opA = relu if relu_a,
 * scaled by 2^exp_a or by *amax_a like diner_train_gemm; exp_b must be the exponent given to
 * diner_train_split_panel.  bias, S, addend may be NULL; addend may alias C. */
int diner_train_gemm_panel(const float *A, int64_t sam, const void *Bhi, const void *Blo, const float *bias,
                           const float *S, int64_t lds, const float *addend, int64_t ldadd, float *C, int64_t ldc,
                           int64_t M, int32_t K, int32_t relu_a, const void *amax_a, int32_t exp_a, int32_t exp_b,
                           void *stream);
/* Weight operand of diner_train_gemm_core: B[n][k] = (transpose ? W[k*ld + n] : W[n*ld + k]) * 2^exp, n, k < 512, fp16 hi/lo in the
 * stream layout of the inference kernel's GEMM core (points_mlp_f16.hip, "packed weight image"): out = 512*512*2 halfs. */
int diner_train_pack_core(const float *W, int64_t ld, int32_t transpose, int32_t exp, void *out, void *stream);
/* diner_train_gemm_panel for K = 512 on the inference kernel's assembly GEMM core (same f16x3 arithmetic; A read and split once per
 * 64-row tile, the weights L2 -> registers, no workgroup barrier in the loop).  Optionally folds the two reductions of
 * diner_train_colsum_amax over the RESULT into the epilogue: colsum[n] += sum_m C[m][n], *amax_out = max(*amax_out, bits of max|C|)
 * (either may be NULL).  Reference: the Linear layers of ResnetFC (src/models/resnetfc.py:62-69) and their autograd transposes. */
int diner_train_gemm_core(const float *A, int64_t sam, const void *Wcore, const float *bias, const float *S, int64_t lds,
                          const float *addend, int64_t ldadd, float *C, int64_t ldc, int64_t M, int32_t relu_a, const void *amax_a,
                          int32_t exp_a, int32_t exp_b, float *colsum, void *amax_out, void *stream);
/* db[n] += sum_m dY[m*ld + n] */
int diner_train_colsum(const float *dY, int64_t M, int32_t N, int64_t ld, float *db, void *stream);
/* per (view, point) row = v*P + p of scene sb: in56 [R,56] (55 inputs of pixelnerf.py:128 + 0), z [R,512]
 * (bilinear latent, image_encoder.py:97-127), taps [R,8] (4 texel indices, 4 weights).  latent: the reference's
 * NCHW tensor [SB,NV,512,h,w], or (latent_is_nhwc) its diner_pack_latent copy [SB,NV,h,w,512] -- same values, a
 * wave then reads whole 256-byte pieces of a texel instead of 64 planes */
int diner_train_point_inputs(const DinerScene *scene, const float *latent, int32_t latent_is_nhwc, const float *rays,
                             const float *z, int64_t NR, int32_t K, int32_t sb, float *in56, float *zlat, float *taps,
                             void *stream);
/* the same with a latent lookup mode (NULL = bilinear / border): taps then hold that mode's footprint (nearest: one texel, weight 1;
 * zeros: weight 0 outside the map), which is also where grid_sample's input gradient goes -- diner_train_bilinear_scatter serves
 * every mode unchanged */
int diner_train_point_inputs_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *latent, int32_t latent_is_nhwc,
                                const float *rays, const float *z, int64_t NR, int32_t K, int32_t sb, float *in56, float *zlat,
                                float *taps, void *stream);
/* dlatent_nhwc[sb][v][texel][ch] += dz[row][ch] * weight (float atomics on 256-byte contiguous rows; the
 * caller zeroes the [SB,NV,h,w,C] buffer), then diner_train_nhwc_to_nchw gives encoder.latent's layout */
int diner_train_bilinear_scatter(const float *dz, const float *taps, int64_t P, int32_t C, int32_t h, int32_t w,
                                 int32_t NV, int32_t sb, float *dlatent_nhwc, void *stream);
int diner_train_nhwc_to_nchw(const float *nhwc, int64_t N, int32_t C, int32_t h, int32_t w, float *nchw_out,
                             void *stream);
/* forward: x [NV,PC] -> mean [PC] (resnetfc.py:146-149); backward: d_mean [PC] -> dx [NV,PC] */
int diner_train_view_mean(const float *x, int64_t PC, int32_t NV, float *out, int32_t backward, void *stream);
/* forward: out [n4] -> sigmoid/relu head (pixelnerf.py:139-143); backward: d_out from d_rgbsigma */
int diner_train_head(const float *out, const float *rgbsigma, const float *d_rgbsigma, int64_t n4, float *result,
                     int32_t backward, void *stream);
/* backward of diner_composite: d_rgb [N,3], d_depth [N]|NULL, d_weights [N,K]|NULL -> d_rgbsigma [N,K,4] */
int diner_composite_backward(const float *rays, const float *z, const float *rgbsigma, const float *d_rgb,
                             const float *d_depth, const float *d_weights, int64_t N, int32_t K,
                             int32_t white_bkgd, float *d_rgbsigma, void *stream);
/* diner_composite_backward, and d_far [N]: the gradient of rays[..., 7] through delta_inf = far - z_K (nerf_renderer.py:300-301, the
 * transpose of alpha_K = 1 - exp(-delta_inf relu(sigma_K)), :344).  d_far must not be NULL. */
int diner_composite_backward_far(const float *rays, const float *z, const float *rgbsigma, const float *d_rgb,
                                 const float *d_depth, const float *d_weights, int64_t N, int32_t K, int32_t white_bkgd,
                                 float *d_rgbsigma, float *d_far, void *stream);
/* floats of the workspace diner_train_point_inputs_backward needs (-1 for bad arguments) */
int64_t diner_train_camera_workspace_floats(int64_t NR, int32_t K, int32_t NV);
/* Backward of diner_train_point_inputs(_ix) (index NULL = bilinear / border) to the geometric leaves, for scene sb: the transpose of
 * nerf_renderer.py:304-305 (points = o + z d, viewdirs = d), pixelnerf.py:92-101 (x_cam = R x + t, R d), :105-108 (uv),
 * image_encoder.py:97-127 (grid_sample's gradient with respect to the grid: ATen's, align_corners=False, every DINER_INDEX_* mode;
 * nearest: 0), image_encoder.py:129-151 + pixelnerf.py:116-117 (depth_dist = depth[nearest(uv)] - x_cam.z: to the depth texel only) and
 * the positional encodings (positional_encoding.py:45-49).
 *   d_in56 [R,56]: gradient of the MLP inputs (lin_in's input gradient);  d_zlat [R,512]: gradient of the latent lookup;
 *   d_far [SB*NR] | NULL: diner_composite_backward_far's, copied to d_rays[..., 7] (0 when NULL);  latent_nhwc: diner_pack_latent's copy.
 * Outputs, each NULL when not wanted:
 *   d_rays [SB,NR,8]: rows of sb written (origin, direction summed over the K samples and NV views; near: 0; far: d_far);
 *   d_poses [SB,NV,4,4]: rows 0..2 of sb's views written (row 3 untouched: the caller zeroes it);  d_focal, d_c [SB,NV,2]: sb's written;
 *   d_image_shape [2]: += (summed over every view; the caller zeroes it before sb 0);
 *   d_depths [SB,NV,H,W]: += at each row's nearest depth texel (float atomics; the caller zeroes it).
 * The reductions run in a fixed order; workspace: diner_train_camera_workspace_floats(NR, K, NV) floats. */
int diner_train_point_inputs_backward(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc,
                                      const float *rays, const float *z, int64_t NR, int32_t K, int32_t sb, const float *d_in56,
                                      const float *d_zlat, const float *d_far, float *workspace, float *d_rays, float *d_poses,
                                      float *d_focal, float *d_c, float *d_image_shape, float *d_depths, void *stream);

/* ---- shape-general training path: building blocks of diner_amd/training_gen.py, which trains any shape of the shape-general
 * inference envelope above in exact fp32 (v_mfma_f32_32x32x2_f32).  The shape-agnostic entry points above (view mean, head,
 * colsum, bilinear scatter, nhwc_to_nchw, composite backward) serve it unchanged. ------------------------------------------- */
#define DINER_ACT_NONE 0
#define DINER_ACT_RELU 1
#define DINER_ACT_SOFTPLUS 2     /* Softplus(beta, threshold 20): beta*x > 20 ? x : log1p(exp(beta*x)) / beta */
/* C[m][n] (+)= sum_k actA(A[m*sam + k*sak]) * actB(B[k*sbk + n*sbn]) (+ bias[n]), then * act_s'(S[m*lds + n]) when S is not NULL:
 * diner_train_gemm's fp32 mode with activation codes (DINER_ACT_*) in place of the relu flags.  act_a / act_b transform an operand
 * while it is staged (forward: act(X) W^T; weight gradient: dY^T act(X)); act_s' is the activation's derivative as autograd
 * evaluates it at the saved pre-activation S (ReLU: [S > 0]; Softplus: z / (z + 1) with z = exp(beta S), 1 where beta S > 20).
 * beta: the Softplus beta (> 0 when any code is DINER_ACT_SOFTPLUS).  Each operand must be contiguous along one of its two indices,
 * with the contiguous extent a multiple of 4; N % 4 == 0; k_chunk (0 = no split, else a multiple of 32) splits the contraction over
 * blockIdx.z (use with atomic = 1); accumulate = 1 adds to C. */
int diner_train_gemm_act(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M, int32_t N, int32_t K,
                         int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc, int64_t lds, int32_t act_a, int32_t act_b,
                         int32_t act_s, float beta, int32_t accumulate, int32_t atomic, int64_t k_chunk, void *stream);
/* diner_train_point_inputs_ix for any num_freqs F = scene->num_freqs (1..63) and latent width C = scene->C (a multiple of 8 in
 * [8, 1024]): in_out [R, ld_in] = the 7 + 8F inputs of pixelnerf.py:128 in diner_train_point_inputs' column order, zero-padded to
 * ld_in (>= 7 + 8F, a multiple of 4) columns; zlat [R, C]; taps [R, 8].  The encodings use sinf (the shape-general inference
 * kernel's arithmetic).  latent_nhwc: diner_pack_latent's copy; index NULL = bilinear / border. */
int diner_train_point_inputs_gen(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc, const float *rays,
                                 const float *z, int64_t NR, int32_t K, int32_t sb, float *in_out, int64_t ld_in, float *zlat, float *taps,
                                 void *stream);
/* diner_train_point_inputs_backward for diner_train_point_inputs_gen: d_in [R, ld_in] (columns >= 7 + 8F ignored), d_zlat [R, C];
 * same outputs, same workspace (diner_train_camera_workspace_floats), same fixed-order reductions. */
int diner_train_point_inputs_backward_gen(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc,
                                          const float *rays, const float *z, int64_t NR, int32_t K, int32_t sb, const float *d_in,
                                          int64_t ld_in, const float *d_zlat, const float *d_far, float *workspace, float *d_rays,
                                          float *d_poses, float *d_focal, float *d_c, float *d_image_shape, float *d_depths,
                                          void *stream);

/* The same three steps for the bicubic lookup (train_gen_bc.hip; see "the bicubic latent lookup" above; padding: DINER_INDEX_PAD_*).
 * diner_train_point_inputs_gen_bc replaces SpatialEncoder.index (src/models/image_encoder.py:97-127) next to the inputs of
 * pixelnerf.py:128, as diner_train_point_inputs_gen does: in_out [R, ld_in], zlat [R, C], and taps [R, 16] = the footprint's 4 columns
 * and 4 rows (int bits), then the weights cx[4], cy[4] (zeros padding: 0 for a column / row outside the map). */
int diner_train_point_inputs_gen_bc(const DinerScene *scene, int32_t padding, const float *latent_nhwc, const float *rays, const float *z,
                                    int64_t NR, int32_t K, int32_t sb, float *in_out, int64_t ld_in, float *zlat, float *taps,
                                    void *stream);
/* diner_train_point_inputs_backward_gen for the bicubic lookup: grid_sample's gradient with respect to the grid (autograd of
 * image_encoder.py:119-125) is sum_ij dcx_i cy_j texel_ij (and cx_i dcy_j) with the cubic weights' derivatives in tx, ty, times
 * w/2 sxl and h/2 syl; the padding puts no factor on it.  Same 24-column row records, reductions, outputs and workspace. */
int diner_train_point_inputs_backward_gen_bc(const DinerScene *scene, int32_t padding, const float *latent_nhwc, const float *rays,
                                             const float *z, int64_t NR, int32_t K, int32_t sb, const float *d_in, int64_t ld_in,
                                             const float *d_zlat, const float *d_far, float *workspace, float *d_rays, float *d_poses,
                                             float *d_focal, float *d_c, float *d_image_shape, float *d_depths, void *stream);
/* diner_train_bilinear_scatter for the 16-tap records of diner_train_point_inputs_gen_bc (grid_sample's input gradient, autograd of
 * image_encoder.py:119-125): dlatent_nhwc[sb][v][y_j][x_i][ch] += dz[row][ch] * cx_i * cy_j, float atomics, consecutive rows with the
 * same footprint summed in registers first; the caller zeroes the [SB,NV,h,w,C] buffer. */
int diner_train_bicubic_scatter(const float *dz, const float *taps, int64_t P, int32_t C, int32_t h, int32_t w, int32_t NV, int32_t sb,
                                float *dlatent_nhwc, void *stream);

/* ---- shape-general training path in f16x3 (train_gen_f16.hip; renderer.train_f16x3_any_shape) ------------------------------- */
/* diner_train_gemm_act in the arithmetic of diner_train_gemm's DINER_PRECISION_F16X3 mode: the activation is applied in fp32, then each
 * operand element is multiplied by a power of two -- 2^exp_a / 2^exp_b, or, when amax_a / amax_b is not NULL, the one that maps the
 * max|.| its device word holds (diner_train_amax, diner_train_colsum_amax) into [2^13, 2^14) -- and split into fp16 hi + lo; three fp16
 * MFMAs per product (hi*hi, hi*lo, lo*hi), fp32 accumulation, C divided by the two scales; act_s' in fp32 as diner_train_gemm_act
 * evaluates it.  Same operand rules as diner_train_gemm_act, A and B 16-byte aligned, and a split contraction (0 < k_chunk < K) only
 * with atomic = 1.  A scaled element beyond the fp16 range
 * becomes +-inf in its hi half and the products it enters are non-finite (never clamped), as in diner_train_gemm. */
int diner_train_gemm_act_f16x3(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M, int32_t N, int32_t K,
                               int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc, int64_t lds, int32_t act_a, int32_t act_b,
                               int32_t act_s, float beta, int32_t accumulate, int32_t atomic, int64_t k_chunk, const void *amax_a,
                               const void *amax_b, int32_t exp_a, int32_t exp_b, void *stream);
/* Pre-split form of a weight operand B[k][n] (n < N, k < K) for diner_train_gemm_act_f16x3_w: two fp16 planes hi, lo of
 * diner_train_split_weight_halfs(N, K) = roundup(N, 128) * roundup(K, 32) halfs each, plane[n][k] = the hi / lo half of
 * B[k][n] * 2^exp, zero in the padding.  B[k][n] = W[n*ld + k] (transpose 0: the forward's W of [N, K]) or W[k*ld + n] (transpose 1:
 * the input-gradient GEMM's operand, W of [K, N]).  Made once per parameter version (diner_amd/training_gen.py caches it). */
int64_t diner_train_split_weight_halfs(int32_t N, int32_t K);
int diner_train_split_weight(const float *W, int32_t N, int32_t K, int64_t ld, int32_t transpose, int32_t exp, void *hi, void *lo,
                             void *stream);
/* C[m][n] (+)= sum_k actA(A[m*sam + k]) * B[k][n] (+ bias[n]), then * act_s'(S[m*lds + n]) when S is not NULL, B given by
 * diner_train_split_weight's planes made with 2^exp_b: diner_train_gemm_act_f16x3 for a row-major A (K % 4 == 0, sam % 4 == 0) without
 * the in-kernel split of the weight.  amax_a / exp_a as above. */
int diner_train_gemm_act_f16x3_w(const float *A, int64_t sam, const void *Bhi, const void *Blo, const float *bias, const float *S,
                                 int64_t lds, float *C, int64_t ldc, int64_t M, int32_t N, int32_t K, int32_t act_a, int32_t act_s,
                                 float beta, int32_t accumulate, const void *amax_a, int32_t exp_a, int32_t exp_b, void *stream);

/* ---- frame output and image scores (frame_out.hip; glue.torch_cmap, glue.frames_u8, glue.image_scores): what the reference's
 * evaluation path does with a rendered frame -- create_prediction_folder (src/models/diner.py:100-136), create_cam_sweep (:138-215) and
 * the scoring loop of evaluate_folder (src/evaluation/eval_suite.py:62-73) -- without leaving the device.  New symbols only:
 * DINER_ABI_VERSION stays 3.  Every function: N images of H x W pixels, contiguous; before any launch DINER_E_INVALID for a NULL
 * pointer or a non-positive size, DINER_E_UNSUPPORTED for H W >= 2^31 or N > 65535.  None synchronises with the host. ------------- */
/* np.min / np.max per image (src/util/torch_helpers.py:64-65): depth [N,1,H,W] fp32 -> range_out [N,2] = (min, max) as doubles, exact;
 * a NaN anywhere in an image makes both of its values NaN.  Two stages: (min, max) per workgroup into `workspace`
 * (diner_depth_range_workspace_floats floats; -1 for bad sizes), then one thread per image walks them in block order. */
int64_t diner_depth_range_workspace_floats(int64_t N, int32_t H, int32_t W);
int diner_depth_range(const float *depth, int64_t N, int32_t H, int32_t W, double *range_out, float *workspace, void *stream);
/* torch_cmap (src/util/torch_helpers.py:43-76): out [N,3,H,W] float64 = rows of `table` [ncolors + 3, 3] float64 (the colours, then
 * under, over, bad: matplotlib's Colormap._lut without alpha), picked in double as numpy and matplotlib 3.10
 * (Colormap._get_rgba_and_mask) do: t = ((double) d - vmin) / (vmax - vmin), xa = t ncolors, xa == ncolors counts as ncolors - 1,
 * row ncolors if xa < 0, else ncolors + 1 if xa >= ncolors, else ncolors + 2 if xa is NaN, else (int) xa.  A flat image gives 0 / 0 =
 * NaN: the bad row (black), as the reference does.  vmin / vmax: the scalar when has_vmin / has_vmax, else image n's range[n][0] /
 * range[n][1] (diner_depth_range's output, read on the device; range may be NULL when both are given). */
int diner_depth_cmap(const float *depth, int64_t N, int32_t H, int32_t W, const double *range, double vmin, double vmax, int32_t has_vmin,
                     int32_t has_vmax, const double *table, int32_t ncolors, double *out, void *stream);
/* Frames as bytes in one pass: rgb [N,3,H,W] fp32 and optionally depth [N,1,H,W] fp32 (NULL: none) -> HWC uint8.  stacked = 0:
 * rgb_out [N,H,W,3] and depth_out [N,H,W,3]; stacked = 1 (needs a depth; depth_out is not read): rgb_out [N,2H,W,3] with the colour
 * above the depth, create_cam_sweep's cat((rgbs, depths), dim=-2) (diner.py:209).  rounding:
 *   DINER_ROUND_SAVE_IMAGE  (uint8) clamp(x 255 + 0.5, 0, 255), multiply and add two fp32 roundings (torchvision save_image, diner.py:129-133)
 *   DINER_ROUND_VIDEO       (uint8) ((double) x 255.0)   (save_torch_video, torch_helpers.py:91, on frames the float64 colour map promoted)
 * Our own definition where numpy's / torch's cast is undefined: the value saturates to [0, 255] and NaN gives 0.
 * The depth half is the byte row table_u8 [ncolors + 3, 3] of diner_depth_cmap's index (vmin / vmax / range as there): the caller
 * quantises the float64 table once by the same rule, in double.  16-byte loads and 12 bytes stored per lane when W % 4 == 0 and the
 * pointers are aligned (inputs 16, outputs 4 bytes), else one pixel per lane. */
#define DINER_ROUND_SAVE_IMAGE 0
#define DINER_ROUND_VIDEO 1
int diner_frames_u8(const float *rgb, const float *depth, int64_t N, int32_t H, int32_t W, int32_t rounding, int32_t stacked,
                    const double *range, double vmin, double vmax, int32_t has_vmin, int32_t has_vmax, const uint8_t *table_u8,
                    int32_t ncolors, uint8_t *rgb_out, uint8_t *depth_out, void *stream);
/* The scores of evaluate_folder (eval_suite.py:63-68) for N pairs of HWC uint8 images [N,H,W,3], as it computes them from the PNG pair
 * (uint8 / 255, data_range = 1, channel_axis = -1): scores_out [4,N] doubles = ssim, psnr, l2, l1.
 *   l1 = sum |d| / (255 3 H W), l2 = sum d^2 / (255^2 3 H W), psnr = 10 log10(1 / l2) (+inf for equal images);
 *   ssim: skimage's structural_similarity with its defaults -- uniform 7 x 7 window, sample covariance (cov_norm = 49 / 48), K1 = 0.01,
 *   K2 = 0.03, S = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)), the mean over the (H - 6)(W - 6) whole windows
 *   (its crop by 3) per channel, then the mean of the three channel means.
 * All sums are exact integers; each window's S is formed in fp64 from them (equal images give exactly 1).  One fp64 partial set per
 * workgroup in `workspace` (diner_image_scores_workspace_floats floats, 8-byte aligned; -1 for bad sizes), added in block order: no
 * atomics, two runs agree bit for bit.  H < 7 or W < 7: DINER_E_INVALID (skimage raises ValueError there). */
int64_t diner_image_scores_workspace_floats(int64_t N, int32_t H, int32_t W);
int diner_image_scores(const uint8_t *pred, const uint8_t *gt, int64_t N, int32_t H, int32_t W, double *scores_out, float *workspace,
                       void *stream);

/* ---- rendering inside a scene bounding box (ray_box.hip; glue.ray_box, glue.box_rays, glue.frame_from_hits;
 * NeRFRendererDGS.render_image(bounds=)): the rays of a target camera that meet an axis-aligned box, each with the box's own depth
 * interval, compacted in pixel order, and the way back from the compact results to a frame.  The device form of
 * FacescapeDataSet.get_near_far / get_mask_at_box (src/data/facescape.py:128-185) on gen_rays' rays (pixel centres, unit directions).
 * New symbols only: DINER_ABI_VERSION stays 3.
 *   box      b_min = bounds[sb][0] + box_lo, b_max = bounds[sb][1] + box_hi (bounds [SB,2,3] fp32 on the device; the reference's
 *            boffset is (-0.01, 0.01))
 *   faces    a direction component with |d| < 1e-5 becomes 1e-5; per face plane t = (b - o) / d, SIGNED; the face counts when the point
 *            t d + o lies within eps = 1e-6 of the box in the two other axes; t0 / t1 = the smallest / largest t of the faces that count
 *   result   near = max(t0, z_near), far = min(t1, z_far); a hit: two or more faces count and far > near
 * Two deliberate differences from get_near_far, which takes the unsigned distances |p - o| and their min / max:
 *   - a box behind the camera is a miss (the reference mirrors it to the front);
 *   - a camera inside the box gets near = z_near (the reference takes the nearer face, which may be the one behind the camera).
 * A ray through an edge or a corner meets more than two faces within eps: a hit here, a miss for the reference's "exactly two" count.
 * Every function, before any launch: DINER_E_INVALID for a NULL pointer, a negative size or a misaligned buffer, DINER_E_UNSUPPORTED for
 * H W >= 2^31 or SB > 65535; SB = 0 or H W = 0: DINER_OK, nothing is launched.  No atomics: two runs give the same bytes. ------------- */
/* Every pixel of the SB cameras (cam->H x cam->W) against its scene's box.
 *   near_far [SB,H W,2]  optional (NULL: not written; 8-byte aligned): a miss holds the camera's z_near, z_far
 *   idx      [SB,H W]    the first count[sb] entries: the hit pixels x + y W, ascending; the others -1
 *   slot     [SB,H W]    the rank of the pixel among its scene's hits (idx[sb][slot] = pixel), or -1
 *   count    [SB]
 * Three passes: each workgroup of 256 pixels ranks its hits and stores their number in `workspace`
 * (diner_ray_box_select_workspace_floats 4-byte words, 4-byte aligned; -1 for bad sizes), one workgroup per scene scans the numbers,
 * the third pass adds the offsets. */
int64_t diner_ray_box_select_workspace_floats(int32_t SB, int32_t H, int32_t W);
int diner_ray_box_select(const DinerTargetCam *cam, int32_t SB, const float *bounds, float box_lo, float box_hi, float *near_far,
                         int32_t *idx, int32_t *slot, int32_t *count, float *workspace, void *stream);
/* The compact rays [SB,B,8] (16-byte aligned) from diner_ray_box_select's idx and count (on the device): entry j < count[sb] is
 * gen_rays' ray at pixel idx[sb][j] -- origin and direction those of the full image, bit for bit -- with components 6, 7 = that ray's
 * near, far of the box.  Entries from count[sb] on are padding: they repeat the scene's last hit; a scene without hits repeats pixel 0
 * with the camera's z_near, z_far.  count_host (optional, [SB] on the HOST): DINER_E_INVALID when B is below one of them. */
int diner_gen_rays_box(const DinerTargetCam *cam, int32_t SB, const float *bounds, float box_lo, float box_hi, const int32_t *idx,
                       const int32_t *count, const int32_t *count_host, int32_t B, float *rays, void *stream);
/* The frame from the compact results rgb_c [SB,B,3], depth_c [SB,B] (NULL allowed when B = 0), one thread per pixel:
 * rgb_out [SB,H W,3] = slot >= 0 ? rgb_c[sb][slot] : (white_bkgd ? 1 : 0), depth_out [SB,H W] = slot >= 0 ? depth_c[sb][slot] : 0,
 * mask_out [SB,H W] bytes (optional) = slot >= 0.  Every output element is written: nothing needs clearing first. */
int diner_frame_from_hits(const float *rgb_c, const float *depth_c, const int32_t *slot, int32_t SB, int32_t B, int32_t H, int32_t W,
                          int32_t white_bkgd, float *rgb_out, float *depth_out, uint8_t *mask_out, void *stream);

/* ---- the datasets' image bytes and Multiface's depth planes, decoded on the device (csrc/image_wire.hip) ------------------------------
 * The other half of the upstream wire format (PNG decoding stays on the host).  New symbols only:
 * DINER_ABI_VERSION stays 3.  pixels [N,H,W,C] uint8, interleaved as np.asarray(PIL.Image) gives them, C = 3 or 4; alpha (optional)
 * [N,H,W] uint8, a plane of its own that wins over a fourth channel (Multiface keeps alpha in a file of its own).  Replaces
 * FacescapeDataSet.read_rgba (src/data/facescape.py:59-66), DTUDataSet.read_rgb after its PIL resize (src/data/dtu.py:83-88), and
 * MultiFaceDataset.read_img / read_alpha / gammaCorrect (src/data/multiface.py:65-95) with the white fill of :322-323.
 * Per pixel, one fp32 rounding per operation, in this order:
 *   1. v = (float)byte / 255.0f, a = (float)alpha_byte / 255.0f   (true divisions)
 *   2. gamma != 0 (gammaCorrect + the clip(0, 1) of multiface.py:68), per channel c with s = (1.4f, 1.1f, 1.6f):
 *        t = (v s_c) / 1.1f;  t = clamp(t - float(3/255), 0, 2);  t = float((1 / (1 - 3/255)) 0.95) t;  t = sqrt(t) (correctly rounded);
 *        t = clamp(t - float(15/255), 0, 2);  v = clamp(t, 0, 1)
 *   3. symmetric_range != 0: v = v 2 - 1 (two operations)
 *   4. the background fill, written last with `bg` as given (it is NOT mapped to the symmetric range, as in the reference):
 *        DINER_BG_BELOW_HALF (facescape.py:65): the three channels = bg where a < 0.5f;  DINER_BG_BELOW_ONE (multiface.py:322-323): where
 *        a < 1.0f;  DINER_BG_NONE: no fill.
 * rgb_out [N,3,H,W], alpha_out [N,1,H,W] = a (optional) fp32; every element is written, no atomics.  With W % 4 == 0, pixels 16-byte
 * (C = 4) or 4-byte (C = 3) aligned, alpha 4-byte and the outputs 16-byte aligned a thread takes 4 pixels (16- / 4-byte loads, 16-byte
 * stores); otherwise one: the same bits either way.
 * Before any launch: DINER_E_INVALID for a NULL pixels / rgb_out, C not 3 or 4, an unknown rule, a rule other than DINER_BG_NONE or
 * an alpha_out without any alpha (neither C == 4 nor a plane), N / H / W <= 0; DINER_E_UNSUPPORTED for H W >= 2^31, N > 65535 or more
 * workgroups than one launch's grid holds (2^31 - 1 of 256 threads). */
#define DINER_BG_NONE 0
#define DINER_BG_BELOW_HALF 1
#define DINER_BG_BELOW_ONE 2
int diner_decode_image_u8(const uint8_t *pixels, const uint8_t *alpha, int64_t N, int32_t H, int32_t W, int32_t C, int32_t bg_rule, float bg,
                          int32_t gamma, int32_t symmetric_range, float *rgb_out, float *alpha_out, void *stream);
/* Multiface's depth planes: MultiFaceDataset.read_depth (src/data/multiface.py:103-109) and the std of :305-311.  depth, conf
 * (optional) uint16 [N,H,W] -> depth_out, std_out (and mask_out = depth > 0, optional) [N,H/stride,W/stride] fp32, nearest-subsampled
 * by `stride` as diner_decode_depth_u16:  depth = u16 * mul0 (the reference: 1e-4f);  std = max(std_a * (conf * mul0) + std_b, 0), a
 * multiplication and an addition (:309-310, std_a = -1.582e-2, std_b = 1.649e-2), or const_std without a confidence plane (:307,
 * 1e-3f);  std = 0 where depth == 0 (:311).
 * Before any launch: DINER_E_INVALID for a NULL depth / depth_out / std_out, N < 0, H / W / stride <= 0 or a stride that does not
 * divide H and W; DINER_E_UNSUPPORTED for H W >= 2^31, N > 65535 or more workgroups than one launch's grid holds.  N = 0: DINER_OK,
 * nothing is launched. */
int diner_decode_depth_u16_mf(const uint16_t *depth, const uint16_t *conf, int64_t N, int32_t H, int32_t W, int32_t stride, float mul0,
                              float std_a, float std_b, float const_std, float *depth_out, float *std_out, float *mask_out, void *stream);
/* conv1's input straight from the bytes: diner_encoder_input (above; src/models/pixelnerf.py:44, src/models/image_encoder.py:222-232)
 * applied to diner_decode_image_u8's rgb, bit for bit, without the fp32 images in between -- the same kernel with a loader that decodes
 * the pixel (steps 1..4) where the fp32 one reads it.  The arguments of diner_decode_image_u8's source and format, then those of
 * diner_encoder_input; both functions' refusals.  No adjoint: bytes carry no gradient. */
int diner_encoder_input_u8(const uint8_t *pixels, const uint8_t *alpha, int32_t C, int32_t bg_rule, float bg, int32_t gamma,
                           int32_t symmetric_range, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, const float *xs,
                           const float *ys, float mean0, float mean1, float mean2, float std0, float std1, float std2, float *out,
                           void *stream);

/* ---- the datasets' image resizes, fused with the byte decode (csrc/image_resize.hip) -------------------------------------------------
 * New symbols only: DINER_ABI_VERSION stays 3.  Three resamplers, each defined by the library call it replaces:
 *   nearest                    F.interpolate(mode="nearest"): src = min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out,
 *                              the product in fp32 (Multiface's alphas, depths and stds, src/data/multiface.py:349-354)
 *   DINER_RESIZE_BILINEAR_AA   F.interpolate(mode="bilinear", align_corners=False, antialias=True), what current torchvision's resize
 *                              runs on a float tensor (multiface.py:347-348): per axis scale = in / out, support = max(scale, 1),
 *                              center = scale (i + 0.5), xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support +
 *                              0.5), in) - xmin, w_j = max(0, 1 - |(j + xmin - center + 0.5) / max(scale, 1)|) / their sum
 *   DINER_RESIZE_BILINEAR      the same call with antialias=False (torchvision 0.12 on tensors): src = max(scale (i + 0.5) - 0.5, 0),
 *                              i0 = (int)src, taps i0 and i0 + (i0 < in - 1) with 1 - (src - i0) and src - i0
 *   DINER_RESIZE_BICUBIC_U8    PIL's Image.resize on 8-bit pixels (src/data/dtu.py:79-83): support = 2 max(scale, 1), the window as
 *                              above, k_j = bicubic((j + xmin - center + 0.5) / max(scale, 1)) with a = -0.5 / their sum, then to fixed
 *                              point with 22 fractional bits, (int)(+-0.5 + k 2^22)
 * The filters are separable.  diner_resize_table tabulates one axis on the HOST, in double: bounds [out][2] = (xmin, n) and weights
 * [out][taps] (fp32, or int32 for DINER_RESIZE_BICUBIC_U8; zero beyond n), taps >= diner_resize_taps(in, out, mode) = the longest
 * window.  The caller copies the tables to the device and may keep them per (in, out, mode).  The kernels only multiply and add, in the
 * order of the taps (fp32: one fused multiply-add per tap), so two runs give the same bits; what a table says is clamped into the
 * source before it addresses anything; no atomics; every output element is written.
 * Both: DINER_E_INVALID for in / out <= 0, an unknown mode, NULL pointers or taps below diner_resize_taps. */
#define DINER_RESIZE_BILINEAR_AA 1
#define DINER_RESIZE_BILINEAR 2
#define DINER_RESIZE_BICUBIC_U8 3
int diner_resize_taps(int32_t in, int32_t out, int32_t mode);
int diner_resize_table(int32_t in, int32_t out, int32_t mode, int32_t taps, int32_t *bounds, void *weights);
/* diner_decode_image_u8 at the size (h, w): the pixels are decoded at full size (steps 1..4 above: a filled pixel enters the filter as
 * the fill, the reference's order), filtered along x into tmp [N,3,H,w] fp32 (the decoded values of a row segment staged in LDS once
 * per workgroup) and along y into rgb_out [N,3,h,w]; alpha_out [N,1,h,w] (optional) is the NEAREST resample of alpha / 255.  The tables
 * (device pointers) are those of a float mode for (W, w) and (H, h).
 * Before any launch: diner_decode_image_u8's refusals, DINER_E_INVALID for a NULL tmp or table, taps or h / w <= 0;
 * DINER_E_UNSUPPORTED for H W, H w or h w >= 2^31, N > 65535, N H >= 2^31 or w > 256 x 65535. */
int diner_decode_image_u8_resized(const uint8_t *pixels, const uint8_t *alpha, int64_t N, int32_t H, int32_t W, int32_t C, int32_t bg_rule,
                                  float bg, int32_t gamma, int32_t symmetric_range, int32_t h, int32_t w, const int32_t *bounds_x,
                                  const float *weights_x, int32_t taps_x, const int32_t *bounds_y, const float *weights_y, int32_t taps_y,
                                  float *tmp, float *rgb_out, float *alpha_out, void *stream);
/* PIL's Image.resize((w, h)) with its default filter on N images [N,H,W,C] uint8, C = 1 or 3 interleaved -> out [N,h,w,C] uint8:
 * pixel = clip((2^21 + sum byte k) >> 22, 0, 255) in integer arithmetic, the horizontal pass first into tmp [N,H,w,C] uint8, the
 * vertical pass second; a pass whose size does not change is skipped (its table and, unless both run, tmp may be NULL).  The tables are
 * DINER_RESIZE_BICUBIC_U8's.  Before any launch: DINER_E_INVALID for a NULL pointer, a non-positive size or taps, C not 1 or 3 (PIL
 * premultiplies RGBA: not served); DINER_E_UNSUPPORTED as above. */
int diner_resize_u8(const uint8_t *pixels, int64_t N, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, const int32_t *bounds_x,
                    const int32_t *weights_x, int32_t taps_x, const int32_t *bounds_y, const int32_t *weights_y, int32_t taps_y,
                    uint8_t *tmp, uint8_t *out, void *stream);
/* diner_decode_depth_u16_mf at the size (h, w): its arithmetic, the zero-depth rule included, on the texel the nearest resample
 * selects -> depth_out, std_out (, mask_out) [N,h,w].  Its refusals, with h / w <= 0 in place of the stride's; N <= 0 is refused. */
int diner_decode_depth_u16_mf_nearest(const uint16_t *depth, const uint16_t *conf, int64_t N, int32_t H, int32_t W, int32_t h, int32_t w,
                                      float mul0, float std_a, float std_b, float const_std, float *depth_out, float *std_out,
                                      float *mask_out, void *stream);

/* ---- nearest mesh vertex and the deformation built on it (csrc/nearest_vertex.hip; glue.nearest_vertex, glue.deform_points,
 * glue.deform_ray_points; diner_amd.compat.pytorch3d_knn) --------------------------------------------------------------------------------
 * What the fork's NOVEL / NOVEL_PE renderers do to every candidate and sample (src/models/novel/nerf_novel_renderer.py:40-50):
 * knn_points(points, target_vertices, K=1) and points + offsets[nearest].  New symbols only: DINER_ABI_VERSION stays 3.
 * Arithmetic contract, for an fp32 point p and vertex v:
 *   d2      = ((px - vx)^2 + (py - vy)^2) + (pz - vz)^2, every operation rounded once to fp32, nothing contracted
 *   winner  the vertex of smallest (d2, original index), lexicographic, among those with d2 < +inf: a tie goes to the lowest index, a
 *           NaN d2 never wins; a point without such a vertex gets idx = 0, d2 = +inf
 * points [SB,N,3], vertices [SB,V,3] (every scene its own set, the same V), idx [SB,N] int32, d2 [SB,N], offsets [SB,V,3], all fp32 and
 * on the device.  No array index is derived from a point's coordinates; what is derived from vertex coordinates (the Morton keys) is
 * clamped before the conversion to int.  No atomics; every output element is written; two runs give the same bits.
 * Two routes with the same results, bit for bit, for every input:
 *   workspace == NULL  brute force: the vertices pass through LDS in SoA tiles, ascending, strict `<`
 *   workspace != NULL  the cluster structure of diner_nearest_vertex_build (16-byte aligned): per cluster of 64 vertices, consecutive in
 *                      Morton order, lb = (ex^2 + ey^2) + ez^2 with e = max(lo - p, p - hi, 0) per axis, in the operation order of d2.
 *                      fp32 subtraction, squaring of non-negatives and addition are monotone, so lb <= d2 of every member; a cluster is
 *                      scanned iff lb <= best (not strict: a tie with a lower index may sit in it), starting from the cluster of smallest
 *                      lb, which is not scanned again.
 * Envelope: 0 < V <= 2^24, 0 <= N < 2^31, 0 <= SB <= 65535.  Before any launch: DINER_E_INVALID for a NULL pointer, V <= 0 or a
 * negative size, DINER_E_UNSUPPORTED outside the envelope; N = 0 or SB = 0: DINER_OK, nothing is launched. */
/* floats of the cluster structure: per scene ceil(V / 64) clusters of 64 (x, y, z, original index) and 6 AABB floats; -1 for bad sizes */
int64_t diner_nearest_vertex_workspace_floats(int32_t SB, int32_t V);
/* keys [SB,V] int32: the 30-bit Morton key of every vertex over the bounding box of its scene's finite coordinates, 10 bits per axis,
 * q = (int)min(max((v - lo) (1024 / extent), 0), 1023); an axis of zero extent contributes 0.  One workgroup per scene. */
int diner_nearest_vertex_keys(const float *vertices, int32_t SB, int32_t V, int32_t *keys, void *stream);
/* order [SB,V] int32: the vertices of each scene in the STABLE order of their keys (the sort is the caller's; entries are clamped into
 * [0, V - 1]) -> workspace: the permuted copy with each vertex's original index, the ragged last cluster padded with NaN vertices, and
 * one AABB [lo, hi] per cluster (NaN coordinates bound nothing).  The order decides the time of a query, never its result. */
int diner_nearest_vertex_build(const float *vertices, const int32_t *order, int32_t SB, int32_t V, float *workspace, void *stream);
int diner_nearest_vertex(const float *points, const float *vertices, const float *workspace, int32_t SB, int64_t N, int32_t V, int32_t *idx,
                         float *d2, void *stream);
/* out [SB,N,3] = points + offsets[idx], in one pass; offsets2 / out2 (optional, together): a second offset set over the same vertices,
 * served by the same search. */
int diner_deform_points(const float *points, const float *vertices, const float *workspace, const float *offsets, const float *offsets2,
                        int32_t SB, int64_t N, int32_t V, float *out, float *out2, void *stream);
/* The same with the points formed from rays [SB,B,8] and z [SB,B,K] as the reference forms them (:412): p = o + z d, a multiplication
 * and an addition; N = B K, point b K + k.  points_out [SB,B K,3] (optional): the undeformed points. */
int diner_deform_ray_points(const float *rays, const float *z, const float *vertices, const float *workspace, const float *offsets,
                            const float *offsets2, int32_t SB, int64_t B, int32_t K, int32_t V, float *out, float *out2, float *points_out,
                            void *stream);

/* ---- the depth-guided sampler on given candidate points (sampler_points.hip) ------------------------------------------------------
 * The sampler of the NOVEL / NOVEL_PE renderers (reference src/models/novel/nerf_novel_renderer.py:79-167): diner_sample_depthguided
 * with the position of candidate j of a ray read from xyz_cand [SB,NR,NC,3] (e.g. diner_deform_ray_points of diner_sample_coarse's
 * depths) instead of formed as o + z d.  z_cand [SB,NR,NC] are the candidates' depths: the moments, the short-list and every output
 * are depths.  The ray's direction still gives raydirs_cam, near / far give the likelihood's half step and the fill-up.  No candidate
 * noise is drawn; n_gauss / u_fill (optional) replace Philox streams 1 / 2 of `seed` as in diner_sample_depthguided, whose outputs
 * z_out [SB,NR,K] (filled and sorted), z_dg_out [SB,NR,K] and lik_out [SB,NR,NC] (both optional) these are.  The likelihood is the
 * same device function: on xyz = o + z d the two entry points return the same bits.  NC <= 4096 (DINER_E_UNSUPPORTED beyond). */
int diner_sample_depthguided_points(const DinerScene *scene, const float *rays, const float *z_cand, const float *xyz_cand,
                                    int64_t NR, const DinerSamplerCfg *cfg, const float *n_gauss, const float *u_fill,
                                    uint64_t seed, float *z_out, float *z_dg_out, float *lik_out, void *stream);

/* ---- the NOVEL point model on the shape-general point/MLP kernels (points_mlp_gen_nv.hip, points_mlp_gen_f16_nv.hip) ---------------
 * The fork's NOVEL PixelNeRF (reference src/models/novel/novel_pixelnerf.py:143-242): diner_render_points_gen at points that are
 * given instead of formed as o + z d, with a second, learned latent added to the encoder's.  New symbols only: DINER_ABI_VERSION stays 3.
 *   xyz_in   [SB,P,3]  goes to the source cameras, the positional code, the depth feature and the encoder's latent lookup
 *   xyz_gen  [SB,P,3]  is projected by scene sb's general camera; gen->latent is looked up there with the scene's feature_padding
 *                      (scaled by the general latent's own size) and the lookup mode of `index`, and added to the encoder's lookup in
 *                      every view before lin_z: final_latent = gen_latent + latent (:196)
 *   viewdirs [SB,P,3]  replace the ray direction
 * index: NULL = bilinear / border; every 4-tap DinerLatentIndex mode is served and applies to both lookups (bicubic and the lin_z-map
 * forms are not).  precision: DINER_PRECISION_FP32 with mlp_packed from diner_pack_mlp_gen, DINER_PRECISION_F16X3 with mlp_packed from
 * diner_pack_mlp_gen_f16.  Any shape of the shape-general envelope, the standard one included.  No atomics: two runs agree bit for
 * bit.  Before any launch: DINER_E_INVALID for a NULL pointer, an unknown index or precision, P < 0, h or w < 1, C != d_latent for
 * either latent; DINER_E_UNSUPPORTED for a shape outside the envelope; P = 0 or SB = 0: DINER_OK, nothing is launched. */
typedef struct DinerNovelGen {
    const float *latent;     /* [h, w, C] NHWC: diner_pack_latent of gen_latent [C,h,w] with N = 1; not read when combine_layer = 0 */
    int32_t h, w, C;         /* its size (need not be the encoder latent's) and channels (= d_latent) */
    int32_t _pad;
    const float *poses;      /* [SB,4,4] world -> general camera, one per scene */
    const float *focal;      /* [SB,2] */
    const float *c;          /* [SB,2] */
    float image_w, image_h;  /* gen_image_shape (W, H) */
} DinerNovelGen;
int diner_render_points_novel(const DinerScene *scene, const DinerLatentIndex *index, const DinerNovelGen *gen, const DinerMlpShape *shape,
                              const float *mlp_packed, const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P,
                              int32_t precision, float *rgbsigma_out, void *stream);

/* ---- the NOVEL_PE point model on the shape-general point/MLP kernels (points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip) --------
 * The fork's NOVEL_PE PixelNeRF (reference src/models/novel_pe/pe_novel_pixelnerf.py:200-292): diner_render_points_novel with
 * C = encoder.latent_size, a fusion MLP of d_latent = C + 6, and
 *   xyz_tgt [SB,P,3]   the undeformed points, projected by scene sb's target camera (pe->poses / focal / c / image_w, image_h)
 *   src_pe = lookup(pe->src_pe[sb, v], uv) per view, tgt_pe = lookup(pe->tgt_pe[sb], tgt_uv) per point: 3 channels each, with the
 *            scene's feature_padding (scaled by that map's own size) and the lookup mode of `index`
 *   conditioned = deformation_layer(cat(latent(uv), src_pe, tgt_pe)); final_latent = gen_latent(gen_uv) + conditioned (:265-268)
 *   the MLP's latent input is cat(final_latent, src_pe, tgt_pe) (:275)
 * deformation_layer is linear and every 4-tap lookup a weighted sum of texels, so its latent part is applied to the texels once per
 * encode: diner_pack_novel_pe_map writes D[sb,v,y,x,:] = W_d[:, :C] . latent[sb,v,y,x,:] (exact fp32 MFMA, no bias; the layout and
 * size of scene->latent, diner_novel_pe_map_floats floats), and the kernel adds b_d[c] + sum_j W_d[c, C + j] pe6[j] from the head table.
 * `shape` is the fusion MLP with d_latent = C + 8: lin_z[b].weight [d_hidden, C + 6] padded with two zero columns before
 * diner_pack_mlp_gen / diner_pack_mlp_gen_f16 (mlp_packed).  scene->latent is not read; scene->C, h, w describe D.
 * New symbols only: DINER_ABI_VERSION stays 3.  No atomics: two runs agree bit for bit.  Before any launch: DINER_E_INVALID for a NULL
 * pointer, an unknown index or precision, P < 0, a map size < 1, scene->C or gen->C != shape->d_latent - 8; DINER_E_UNSUPPORTED for a
 * shape outside the envelope (C + 8 > 1024 included); P = 0 or SB = 0: DINER_OK, nothing is launched.  With combine_layer = 0 no
 * latent, map or pos-encoding is read. */
typedef struct DinerNovelPe {
    const float *map;        /* [SB,NV,h,w,C]: diner_pack_novel_pe_map */
    const float *head;       /* [C][8]: W_d[c, C:C+6] | b_d[c] | 0 */
    const float *src_pe;     /* [SB,NV,src_h,src_w,4]: pos_encodings, NHWC, the 4th channel padding */
    int32_t src_h, src_w;
    const float *tgt_pe;     /* [SB,tgt_h,tgt_w,4]: tgt_pos_encoding, likewise */
    int32_t tgt_h, tgt_w;
    const float *poses;      /* [SB,4,4] world -> target camera, one per scene */
    const float *focal;      /* [SB,2] */
    const float *c;          /* [SB,2] */
    float image_w, image_h;  /* tgt_image_shape (W, H) */
} DinerNovelPe;
int64_t diner_novel_pe_map_floats(const DinerScene *scene);
int diner_pack_novel_pe_map(const DinerScene *scene, const float *w_latent_part, float *map_out, void *stream);
int diner_render_points_novel_pe(const DinerScene *scene, const DinerLatentIndex *index, const DinerNovelGen *gen, const DinerNovelPe *pe,
                                 const DinerMlpShape *shape, const float *mlp_packed, const float *xyz_in, const float *xyz_gen,
                                 const float *xyz_tgt, const float *viewdirs, int64_t P, int32_t precision, float *rgbsigma_out,
                                 void *stream);

/* ---- the NOVEL point model's training path (train_novel.hip; diner_amd/training_novel.py) ------------------------------------------
 * Training the fork's NOVEL PixelNeRF (reference src/models/novel/novel_pixelnerf.py:143-242) on the shape-general training path's
 * staged schedule (diner_train_gemm_act and its f16x3 forms, view mean, head): only the first and the last stage differ from the plain
 * model's.  New symbols only: DINER_ABI_VERSION stays 3.  Both: before any launch DINER_E_INVALID for a NULL pointer, an unknown index
 * mode, P < 0, gen->C != scene->C, gen->h or gen->w < 1; P = 0: DINER_OK, nothing is launched.
 *
 * diner_train_point_inputs_novel replaces :159-200 (projection of xyz into the source views, viewdirs rotated, the encoder's lookup
 * and PixelNeRF.index :108-141 of gen_latent at the general camera, final_latent = gen_latent + latent :196, the depth feature) and the
 * positional code of :225: diner_train_point_inputs_gen at GIVEN points.  Same rows (row = v*P + p), same in_out [R, ld_in] columns
 * with the same sinf expressions, same taps [R,8] record of the encoder's lookup; the world point is xyz_in[sb][p], the direction
 * viewdirs[sb][p] ([SB,P,3] each).  zlat [R, C] = lookup(latent[sb, v], uv) + lookup(gen->latent, gen_uv), with gen_uv from
 * xyz_gen[sb][p] through scene sb's general camera, the scene's feature_padding scaled by the general map's own size and the lookup
 * mode of `index` (NULL = bilinear / border; every 4-tap mode is served; interp = 2, bicubic: DINER_E_UNSUPPORTED).  gen_taps [P,8]:
 * the general footprint in the taps format (4 texel indices as int bits, 4 weights), written once per point.  With gen->latent = 0,
 * xyz_gen = xyz_in = o + z d and viewdirs = d the three outputs equal diner_train_point_inputs_gen's bit for bit.  zlat = NULL
 * (combine_layer = 0): neither latent is read, taps and gen_taps are not written and may be NULL. */
int diner_train_point_inputs_novel(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc, const DinerNovelGen *gen,
                                   const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P, int32_t sb, float *in_out,
                                   int64_t ld_in, float *zlat, float *taps, float *gen_taps, void *stream);
/* grid_sample's input gradient for the general lookup (autograd of :126-137, where index() repeats the one map over SB * NV):
 * d_gen_nhwc[texel][ch] += (sum_v d_zlat[v*P + p][ch]) * weight, the view sum formed in registers in the order v = 0 .. NV-1, then
 * diner_train_bilinear_scatter's scheme (runs of consecutive points merged while the footprint stays, one float atomic per used tap on
 * 256-byte contiguous rows, a tap of weight 0 never flushed).  The caller zeroes d_gen_nhwc [h,w,C] once per backward; every scene
 * accumulates into it; diner_train_nhwc_to_nchw with N = 1 then gives gen_latent's [C,h,w] layout.  The encoder latent's gradient
 * goes through diner_train_bilinear_scatter unchanged (taps has its format). */
int diner_train_novel_gen_scatter(const float *d_zlat, const float *gen_taps, int64_t P, int32_t C, int32_t h, int32_t w, int32_t NV,
                                  float *d_gen_nhwc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DINER_HIP_H */
