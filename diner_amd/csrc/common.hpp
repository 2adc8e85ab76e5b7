// Shared device helpers of the gfx950 DINER kernels.
//
// Arithmetic contract: every helper performs the reference's fp32 operations in the reference's
// order, one rounding per op (the library is compiled with -ffp-contract=off; fused multiply-adds
// appear only where written as __builtin_fmaf, at the places where ATen's own kernels contract --
// pinned bit-exact against the reference by tests/test_oracle_golden.py on the CPU restatement).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diner_hip.h"

#define DINER_WAVE 64
#define DINER_SIGMA_PAD 100  // exponential padding of the sigma map (image_encoder.py:173)

namespace diner {

void set_error(const char *fmt, ...);
int check_launch(const char *what);

// Launch state that belongs to the DEVICE, not the process (a process may render on cuda:1 after cuda:0): the CU count that sizes the
// persistent grids, and the raised dynamic-LDS limit of a kernel (hipFuncSetAttribute acts on the current device's copy of the function).
// Both are cached per device ordinal (api.hip); thread-safe (atomics; a race only repeats an idempotent call).
int device_cus();                                                    // CUs of the current device (256 on MI355X)
enum LdsSlot { LDS_SLOT_F16_LINZ = 0, LDS_SLOT_F16_LATENT = 2, LDS_SLOT_F16_TRACE = 4, LDS_SLOT_TRAIN_CORE0 = 6, LDS_SLOT_DW512 = 10,
               LDS_SLOT_F16_GIX = 12, LDS_SLOT_COUNT = 16 };   // (the f16 slots come in pairs: view-sequential / views-in-tile; + LDS_SLOT_F16_GIX: the any-lookup-mode twins)
int ensure_dynamic_lds(const void *kernel, int bytes, int slot);    // DINER_OK, or DINER_E_LAUNCH with the error set

// --------------------------------------------------------------------------------------------
// camera of one source view, held in registers (SGPRs once the compiler sees it is uniform)
// --------------------------------------------------------------------------------------------
struct View {
    float r[9];  // rotation rows
    float t[3];
    float fx, fy, cx, cy;
};

__device__ __forceinline__ View load_view(const DinerScene &s, int sb, int v)
{
    View o;
    const float *P = s.poses + ((int64_t)sb * s.NV + v) * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.r[i * 3 + 0] = P[i * 4 + 0];
        o.r[i * 3 + 1] = P[i * 4 + 1];
        o.r[i * 3 + 2] = P[i * 4 + 2];
        o.t[i] = P[i * 4 + 3];
    }
    const float *f = s.focal + ((int64_t)sb * s.NV + v) * 2, *c = s.c + ((int64_t)sb * s.NV + v) * 2;
    o.fx = f[0]; o.fy = f[1]; o.cx = c[0]; o.cy = c[1];
    return o;
}

// the one camera per scene of the NOVEL models (general, target): poses [SB,4,4], focal [SB,2], c [SB,2]
__device__ __forceinline__ View view_of(const float *poses, const float *focal, const float *c, int sb)
{
    View v;
    const float *Pm = poses + (int64_t)sb * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v.r[i * 3 + 0] = Pm[i * 4 + 0]; v.r[i * 3 + 1] = Pm[i * 4 + 1]; v.r[i * 3 + 2] = Pm[i * 4 + 2];
        v.t[i] = Pm[i * 4 + 3];
    }
    v.fx = focal[sb * 2]; v.fy = focal[sb * 2 + 1]; v.cx = c[sb * 2]; v.cy = c[sb * 2 + 1];
    return v;
}

// R*x as torch.matmul evaluates it (BLAS: k-ordered FMA chain) -- nerf_renderer.py:100,103
__device__ __forceinline__ void rotate(const View &v, float x, float y, float z, float &ox, float &oy, float &oz)
{
    ox = __builtin_fmaf(v.r[2], z, __builtin_fmaf(v.r[1], y, v.r[0] * x));
    oy = __builtin_fmaf(v.r[5], z, __builtin_fmaf(v.r[4], y, v.r[3] * x));
    oz = __builtin_fmaf(v.r[8], z, __builtin_fmaf(v.r[7], y, v.r[6] * x));
}

// world point -> camera point + NDC uv -- nerf_renderer.py:99-110 == pixelnerf.py:91-108
__device__ __forceinline__ void project(const View &v, float iw, float ih, float x, float y, float z,
                                        float &px, float &py, float &pz, float &u, float &w)
{
    rotate(v, x, y, z, px, py, pz);
    px = px + v.t[0]; py = py + v.t[1]; pz = pz + v.t[2];
    u = px / pz; w = py / pz;
    u = u * v.fx; w = w * v.fy;
    u = u + v.cx; w = w + v.cy;
    u = u / iw * 2.0f - 1.0f;
    w = w / ih * 2.0f - 1.0f;
}

// One ray of gen_rays (reference src/util/cam_geometry.py:36-79) at pixel (x, y): E [4,4] world->cam, Kk [3,3] -> o[8] = origin(3), unit
// direction(3), near, far; pixel centres, OpenCV convention.  The only place that computes a ray: gen_rays_kernel (encode_glue.hip, every
// pixel) and gen_rays_at_kernel (train_glue.hip, selected pixels) both call it, so a selected ray is the full image's ray bit for bit.
__device__ __forceinline__ void gen_ray(const float *__restrict__ E, const float *__restrict__ Kk, int x, int y, float near, float far,
                                        float *__restrict__ o)
{
    const float fx = Kk[0], fy = Kk[4], cx = Kk[2], cy = Kk[5];
    float dx = (((float)x + 0.5f) - cx) / fx, dy = (((float)y + 0.5f) - cy) / fy, dz = 1.0f;  // :62-63
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);                                        // :64 pow(2).sum().sqrt()
    dx = dx / n; dy = dy / n; dz = dz / n;
    // world direction = R^T d (bmm: k-ordered FMA chain), origin = -R^T t (:67-72)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[3 + r] = __builtin_fmaf(E[2 * 4 + r], dz, __builtin_fmaf(E[1 * 4 + r], dy, E[0 * 4 + r] * dx));
        o[r] = __builtin_fmaf(-1.0f * E[2 * 4 + r], E[2 * 4 + 3], __builtin_fmaf(-1.0f * E[1 * 4 + r], E[1 * 4 + 3], (-1.0f * E[0 * 4 + r]) * E[0 * 4 + 3]));
    }
    o[6] = near;
    o[7] = far;
}

// sin() of the positional encodings.  The argument is the reference's fp32 value (one fma, positional_encoding.py:45-49); its sine comes
// from the hardware's v_sin_f32 (sin(2 pi x) of an argument in revolutions) behind a compensated reduction: r1 = RN(a * C_HI),
// r2 = the part of a / 2pi that r1 lost (exact by fma) + a * C_LO, sin(2 pi (fract(r1) + r2)) -- accurate for every finite a.  Measured
// over the encodings' range (tools/sin_probe.hip, 1.7e7 arguments up to 705 rad): max |error| 4.2e-7 against 6.8e-8 for sinf -- below
// the 2^-22 x 16 granularity of the fp16 hi/lo operand split the value goes through next -- for 6 instructions instead of the ~90 of
// the inlined sinf (with its Payne-Hanek path), 48 times per point and view.  Used by the default (f16x3) inference kernel
// (points_mlp_f16.hip) and by the training path's point_inputs_kernel (train.hip); the exact-fp32 inference kernel (points_mlp.hip)
// keeps sinf.  (Tried sinf in the f16x3 paths too: measured 0.5 % slower, not kept.)
__device__ __forceinline__ float pe_sin(float a)
{
    const float C_HI = 0.15915494f;                                             // fp32(1 / 2pi)
    const float C_LO = (float)(0.15915494309189535 - (double)0.15915494f);
    const float r1 = a * C_HI;
    const float r2 = __builtin_fmaf(a, C_HI, -r1) + a * C_LO;
    return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r1) + r2);
}

// grid_sample(align_corners=False) un-normalisation, contracted as ATen compiles it
__device__ __forceinline__ float unnorm(float u, float half_size) { return __builtin_fmaf(u + 1.0f, half_size, -0.5f); }

// clamp_max(size-1, clamp_min(0, x)); NaN -> 0
__device__ __forceinline__ float clipf(float x, float hi)
{
    float y = (x > 0.0f) ? x : 0.0f;
    return (y < hi) ? y : hi;
}

// float pixel index -> int in [0,size-1] (callers have already range-checked finite values; the
// clamp makes every address safe for NaN/inf inputs as well)
__device__ __forceinline__ int safe_idx(float f, int size)
{
    int i = (int)f;  // v_cvt_i32_f32 saturates, NaN -> 0
    return i < 0 ? 0 : (i > size - 1 ? size - 1 : i);
}

// --------------------------------------------------------------------------------------------
// the input stage of the shape-general point models (render: points_mlp_gen*; training: train_gen_points.hpp, train_novel.hip)
// --------------------------------------------------------------------------------------------
// depth of view (sb, v) at the texel (ddx, ddy) nearest to uv (pixelnerf.py:114)
__device__ __forceinline__ float nearest_depth(const DinerScene &s, int sb, int v, float u, float w, int &ddx, int &ddy)
{
    const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
    ddx = safe_idx(__builtin_rintf(clipf(unnorm(u, (float)s.W / 2.0f), (float)(s.W - 1))), s.W);
    ddy = safe_idx(__builtin_rintf(clipf(unnorm(w, (float)s.H / 2.0f), (float)(s.H - 1))), s.H);
    return tex[((int64_t)ddy * s.W + ddx) * 2].w;
}

// world point (wx, wy, wz) and direction (dwx, dwy, dwz) in source view (sb, v): camera point, NDC uv, camera direction and
// delta = depth - z (pixelnerf.py:91-115).  Scalars in and out: a record selected from by index would live in scratch memory.
__device__ __forceinline__ void view_geometry(const DinerScene &s, int sb, int v, float wx, float wy, float wz, float dwx, float dwy,
                                              float dwz, float &px, float &py, float &pz, float &u, float &w, float &dcx, float &dcy,
                                              float &dcz, float &delta)
{
    const View vw = load_view(s, sb, v);
    project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);
    rotate(vw, dwx, dwy, dwz, dcx, dcy, dcz);
    int ddx, ddy;
    delta = nearest_depth(s, sb, v, u, w, ddx, ddy) - pz;
}

// column e of the MLP's 7 + 8F inputs (pixelnerf.py:128; positional_encoding.py:45-49), 0 past them:
//   [x_cam 3 | sin(f_j x_cam + phi_j) 6F | R d_w 3 | depth_dist 1 | sin(f_j depth_dist + phi_j) 2F]
// The one place that states the layout and the sinf expressions for the render and the training kernels alike.
__device__ __forceinline__ float input_element(int e, float px, float py, float pz, float dcx, float dcy, float dcz, float delta, int F,
                                               float freq_factor)
{
    const int e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1;
    const float half_pi = 1.5707963267948966f;
    float val;
    if (e < 3) val = e == 0 ? px : e == 1 ? py : pz;
    else if (e < e_pe3) {
        const int j = (e - 3) / 3, i = (e - 3) % 3;
        val = sinf(__builtin_fmaf(i == 0 ? px : i == 1 ? py : pz, ldexpf(freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f));
    } else if (e < e_dir) val = e == e_pe3 ? dcx : e == e_pe3 + 1 ? dcy : dcz;
    else if (e == e_dir) val = delta;
    else if (e < e_pe1 + 2 * F) {
        const int j = e - e_pe1;
        val = sinf(__builtin_fmaf(delta, ldexpf(freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f));
    } else val = 0.0f;
    return val;
}

// XCD-aware order of the point tiles (workgroups go round-robin to the 8 XCDs): consecutive tiles -- neighbouring samples of a ray,
// then neighbouring rays, so neighbouring latent texels -- stay on one XCD's L2.  Bijective for any grid size.  (train_blocks.hpp's
// tile_of is another function: it deals the column blocks of a 2-D GEMM tile grid, not a 1-D run of tiles.)
__device__ __forceinline__ int64_t xcd_tile(int64_t nwg, int64_t b)
{
    const int64_t q = nwg / 8, r = nwg % 8, xcd = b % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
}

// a wave's [RB][CT] block of 16-float MFMA accumulators (V = f32x16 of either family): cleared, and summed over the views
template <class V, int RB, int CT>
__device__ __forceinline__ void acc_zero(V (&acc)[RB][CT])
{
#pragma unroll
    for (int tm = 0; tm < RB; ++tm)
#pragma unroll
        for (int tn = 0; tn < CT; ++tn)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tm][tn][i] = 0.0f;
}

template <class V, int RB, int CT>
__device__ __forceinline__ void acc_add(V (&acc)[RB][CT], const V (&x)[RB][CT])
{
#pragma unroll
    for (int tm = 0; tm < RB; ++tm)
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) acc[tm][tn] += x[tm][tn];
}

// --------------------------------------------------------------------------------------------
// latent lookup: SpatialEncoder.index (image_encoder.py:97-127) = grid_sample(align_corners=False, mode=index_interp,
// padding_mode=index_padding) of the latent map at the feature_padding-rescaled uv.  Every mode is a footprint of at most 4 texels
// (x0|x1) x (y0|y1) with the weights nw ne sw se, consumed in ATen's accumulation order by the gathers and by the training path's
// scatter.  Indices are always inside the map, so every tap is readable.
// --------------------------------------------------------------------------------------------
struct LatentFoot {
    int x0, x1, y0, y1;
    float nw, ne, sw, se;
};

// ATen's reflect_coordinates(in, -1, 2 size - 1): reflect over [-0.5, size - 0.5]
__device__ __forceinline__ float reflect_coord(float x, int size)
{
    const float span = (float)size;
    const float in = fabsf(x + 0.5f);
    const float extra = fmodf(in, span);
    const int flips = (int)floorf(in / span);
    return (flips & 1) ? span - extra - 0.5f : extra - 0.5f;
}

// GIX = false: bilinear / border, the instruction sequence every kernel had before the other modes existed.  GIX = true: any mode
// (DINER_INDEX_*, uniform).  ring = 1: the map has a one-texel ring around its lw x lh interior (the zeros-padded lin_z maps,
// diner_pack_linz_maps_ix): taps outside the interior then go to the ring with their full weight instead of weight 0; the indices
// are those of the (lw + 2) x (lh + 2) map.
template <bool GIX>
__device__ __forceinline__ LatentFoot latent_footprint(float u, float w, float sxl, float syl, int lw, int lh, int interp = 0,
                                                       int padding = 0, int ring = 0)
{
    LatentFoot f;
    if (!GIX) {
        const float ix = clipf(unnorm(u * sxl, (float)lw / 2.0f), (float)(lw - 1));
        const float iy = clipf(unnorm(w * syl, (float)lh / 2.0f), (float)(lh - 1));
        const float x0f = floorf(ix), y0f = floorf(iy);
        const float fx = ix - x0f, ex = 1.0f - fx, fy = iy - y0f, ey = 1.0f - fy;
        const int x0 = safe_idx(x0f, lw), y0 = safe_idx(y0f, lh);
        const bool x1ok = x0 + 1 <= lw - 1, y1ok = y0 + 1 <= lh - 1;
        f.x0 = x0; f.y0 = y0;
        f.x1 = x1ok ? x0 + 1 : x0; f.y1 = y1ok ? y0 + 1 : y0;
        f.nw = ey * ex; f.ne = x1ok ? ey * fx : 0.0f;   // a tap outside the map has its weight forced to 0
        f.sw = y1ok ? fy * ex : 0.0f; f.se = (x1ok && y1ok) ? fy * fx : 0.0f;
        return f;
    }
    float ix = unnorm(u * sxl, (float)lw / 2.0f), iy = unnorm(w * syl, (float)lh / 2.0f);
    if (padding == DINER_INDEX_PAD_REFLECTION) { ix = reflect_coord(ix, lw); iy = reflect_coord(iy, lh); }
    if (padding != DINER_INDEX_PAD_ZEROS) { ix = clipf(ix, (float)(lw - 1)); iy = clipf(iy, (float)(lh - 1)); }
    float xa, ya, nw, ne, sw, se;
    if (interp == DINER_INDEX_NEAREST) {
        xa = __builtin_rintf(ix); ya = __builtin_rintf(iy);   // round half to even, like ATen's nearbyint
        nw = 1.0f; ne = sw = se = 0.0f;
    } else {
        xa = floorf(ix); ya = floorf(iy);
        const float fx = ix - xa, ex = 1.0f - fx, fy = iy - ya, ey = 1.0f - fy;
        nw = ey * ex; ne = ey * fx; sw = fy * ex; se = fy * fx;
    }
    const float xb = interp == DINER_INDEX_NEAREST ? xa : xa + 1.0f, yb = interp == DINER_INDEX_NEAREST ? ya : ya + 1.0f;
    // in-map tests on the float positions (NaN: outside)
    const bool xa_in = xa >= 0.0f && xa <= (float)(lw - 1), xb_in = xb >= 0.0f && xb <= (float)(lw - 1);
    const bool ya_in = ya >= 0.0f && ya <= (float)(lh - 1), yb_in = yb >= 0.0f && yb <= (float)(lh - 1);
    if (!ring) {
        f.nw = (xa_in && ya_in) ? nw : 0.0f; f.ne = (xb_in && ya_in) ? ne : 0.0f;
        f.sw = (xa_in && yb_in) ? sw : 0.0f; f.se = (xb_in && yb_in) ? se : 0.0f;
    } else {   // (a NaN position reads the ring with weight 0 instead: the result is the biases, lin_z of grid_sample's 0)
        const bool ok = ix == ix && iy == iy;
        f.nw = ok ? nw : 0.0f; f.ne = ok ? ne : 0.0f; f.sw = ok ? sw : 0.0f; f.se = ok ? se : 0.0f;
        if (!ok) f.nw = 1.0f;
    }
    // indices clamped into [-ring, size - 1 + ring], then shifted by ring (v_cvt_i32_f32 saturates, NaN -> 0)
    auto idx = [&](float p, int size) {
        int i = (int)p;
        i = i < -ring ? -ring : (i > size - 1 + ring ? size - 1 + ring : i);
        return ring ? (p == p ? i + ring : 0) : i;
    };
    f.x0 = idx(xa, lw); f.x1 = idx(xb, lw); f.y0 = idx(ya, lh); f.y1 = idx(yb, lh);
    return f;
}

// uv scale of feature_padding along an axis of `size` texels (image_encoder.py:113-114): every map scales it by its own size
__device__ __forceinline__ float pad_scale(int size, float feature_padding) { return ((float)size - feature_padding * 2.0f) / (float)size; }

// footprint, in a [mh, mw] map, of world point x seen by the scene's one camera `cam` of image shape (iw, ih): the NOVEL models'
// index() of gen_latent
__device__ __forceinline__ LatentFoot camera_footprint(const View &cam, float iw, float ih, const float *x, int mh, int mw,
                                                       float feature_padding, int interp, int padding)
{
    float px, py, pz, u, w;
    project(cam, iw, ih, x[0], x[1], x[2], px, py, pz, u, w);
    return latent_footprint<true>(u, w, pad_scale(mw, feature_padding), pad_scale(mh, feature_padding), mw, mh, interp, padding);
}

// one channel of a 4-tap lookup: the texel values a b c d under the weights nw ne sw se of t (a LatentFoot or a kernel's tap record),
// in ATen's accumulation order nw, ne, sw, se with contracted FMAs
template <class TapRec>
__device__ __forceinline__ float tap_sum(float a, float b, float c, float d, const TapRec &t)
{
    return __builtin_fmaf(d, t.se, __builtin_fmaf(c, t.sw, __builtin_fmaf(b, t.ne, a * t.nw)));
}

// --------------------------------------------------------------------------------------------
// bicubic latent lookup: grid_sample(mode="bicubic", align_corners=False) of SpatialEncoder.index (image_encoder.py:119-125) with
// index_interp="bicubic".  The centre coordinate is NOT clipped or reflected; the 4 x 4 taps sit at (floor(ix) - 1 + i,
// floor(iy) - 1 + j) and each integer tap position goes through the padding on its own (ATen's get_value_bounded): border clamps it,
// reflection reflects it over [-0.5, size - 0.5] and clamps, zeros drops a tap outside the map.  The footprint is separable:
// result = sum_j cy[j] * (sum_i cx[i] * texel(x[i], y[j])); with zeros padding the weight of a column / row outside the map is
// folded to 0 per axis.  Indices are always inside the map (NaN / inf coordinates included), so every tap is readable.
// --------------------------------------------------------------------------------------------
struct BicubicFoot {
    int x[4], y[4];        // texel columns / rows of the taps
    float cx[4], cy[4];    // cubic-convolution weights (A = -0.75) at distances t + 1, t, 1 - t, 2 - t
};

// one axis: indices, weights and the weights' derivative in the fractional position t (d ic / d t = 1; the padding acts on the
// integer tap positions and carries no gradient)
__device__ __forceinline__ void bicubic_axis(float ic, int size, int padding, int (&idx)[4], float (&c)[4], float (&dc)[4])
{
    const float A = -0.75f;
    const float c0f = floorf(ic), t = ic - c0f;
    float d = t + 1.0f;                                     // ATen get_cubic_upsample_coefficients
    c[0] = ((A * d - 5.0f * A) * d + 8.0f * A) * d - 4.0f * A;
    dc[0] = (3.0f * A * d - 10.0f * A) * d + 8.0f * A;
    c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    dc[1] = (3.0f * (A + 2.0f) * t - 2.0f * (A + 3.0f)) * t;
    d = 1.0f - t;
    c[2] = ((A + 2.0f) * d - (A + 3.0f)) * d * d + 1.0f;
    dc[2] = -((3.0f * (A + 2.0f) * d - 2.0f * (A + 3.0f)) * d);
    d = d + 1.0f;
    c[3] = ((A * d - 5.0f * A) * d + 8.0f * A) * d - 4.0f * A;
    dc[3] = -((3.0f * A * d - 10.0f * A) * d + 8.0f * A);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float p = c0f + (float)(i - 1);
        const bool in = p >= 0.0f && p <= (float)(size - 1);   // NaN: outside
        if (padding == DINER_INDEX_PAD_REFLECTION) p = reflect_coord(p, size);
        idx[i] = safe_idx(clipf(p, (float)(size - 1)), size);
        if (padding == DINER_INDEX_PAD_ZEROS && !in) { c[i] = 0.0f; dc[i] = 0.0f; }
    }
}

__device__ __forceinline__ BicubicFoot bicubic_footprint(float u, float w, float sxl, float syl, int lw, int lh, int padding)
{
    BicubicFoot f;
    float dcx[4], dcy[4];
    bicubic_axis(unnorm(u * sxl, (float)lw / 2.0f), lw, padding, f.x, f.cx, dcx);
    bicubic_axis(unnorm(w * syl, (float)lh / 2.0f), lh, padding, f.y, f.cy, dcy);
    return f;
}

// --------------------------------------------------------------------------------------------
// Philox4x32-10 counter RNG (perf mode: statistically equivalent to torch.rand/randn, not
// bit-matching any torch generator -- parity tests against the reference inject explicit noise
// instead).  What the sampler draws from it is a fixed function of (call seed, ray, index), the
// stream contract of DESIGN.md section 2: key = (seed_lo, seed_hi), counter = (x, stream, gray_lo,
// gray_hi).  tests/philox_ref.py restates it on the host and tests/test_gpu_philox.py holds the
// kernels to that restatement (uniform streams bit for bit): a change here or to a counter in
// sampler.hip changes every frame rendered at a fixed seed.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32(uint4 ctr, uint2 key)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
        uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += 0x9E3779B9u; key.y += 0xBB67AE85u;
    }
    return ctr;
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }  // [0,1)

// --------------------------------------------------------------------------------------------
// wave-level primitives (64 lanes)
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scans over the 64 lanes
__device__ __forceinline__ float wave_scan_mul(float v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        float n = __shfl_up(v, o, 64);
        if (lane >= o) v = n * v;
    }
    return v;
}
__device__ __forceinline__ int wave_scan_add_i(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}

}  // namespace diner
