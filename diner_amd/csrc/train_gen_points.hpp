// The point-input kernels of the shape-general training path (train_gen.hip has the description), forward and backward, as templates on
// the lookup: BC = false, the 4-tap lookup of any DINER_INDEX_* mode (instantiated by train_gen.hip); BC = true, the 16-tap bicubic
// lookup (common.hpp bicubic_footprint) and its gradient with respect to the grid (instantiated by train_gen_bc.hip, next to
// bicubic_scatter_kernel, in a code object of their own).
#pragma once
#include "train_blocks.hpp"

namespace diner {

namespace train_gen {

using namespace train_blocks;

// ---- per-(view, point) MLP inputs of any num_freqs F and latent width C ---------------------------------------------------------
// rows are view-major: row = v*P + p.  in [R, ld_in]: pixelnerf.py:128's 7 + 8F inputs in point_inputs_kernel's column order
//   [x_cam 3 | sin(f_j x_cam + phi_j) 6F | R d_w 3 | depth_dist 1 | sin(f_j depth_dist + phi_j) 2F | 0 ...]
// from common.hpp's input_element, the shape-general inference kernels' (points_mlp_gen.hip); zlat [R, C]: the latent lookup of the
// scene's DINER_INDEX_* mode from the NHWC latent; taps [R, 8]: its 4 texel indices (int bits) and weights.
// BC: taps [R, 16] = the 4 columns and 4 rows of the footprint (int bits), then cx[4], cy[4].
template <bool BC>
__global__ __launch_bounds__(64) void point_inputs_gen_kernel(DinerScene s, const float *__restrict__ latent_nhwc,
                                                              const float *__restrict__ rays, const float *__restrict__ zsamp,
                                                              int64_t NR, int K, int sb, int ix_interp, int ix_padding,
                                                              float *__restrict__ in, int64_t ld_in, float *__restrict__ zlat,
                                                              float *__restrict__ taps_out)
{
    const int64_t P = NR * (int64_t)K, row = blockIdx.x;
    const int v = (int)(row / P);
    const int64_t p = row - (int64_t)v * P;
    const int lane = threadIdx.x;
    const float *rp = rays + ((int64_t)sb * NR + p / K) * 8;
    const float zz = zsamp[(int64_t)sb * P + p];
    const float dwx = rp[3], dwy = rp[4], dwz = rp[5];
    const float wx = rp[0] + zz * dwx, wy = rp[1] + zz * dwy, wz = rp[2] + zz * dwz;  // nerf_renderer.py:304
    float px, py, pz, u, w, dcx, dcy, dcz, delta;
    view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);   // pixelnerf.py:91-115
    for (int e = lane; e < ld_in; e += 64) in[row * ld_in + e] = input_element(e, px, py, pz, dcx, dcy, dcz, delta, s.num_freqs, s.freq_factor);
    // footprint of the lookup mode in the latent map (image_encoder.py:97-127; common.hpp)
    const float sxl = pad_scale(s.w, s.feature_padding), syl = pad_scale(s.h, s.feature_padding);
    if constexpr (BC) {
        const BicubicFoot f = bicubic_footprint(u, w, sxl, syl, s.w, s.h, ix_padding);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                taps_out[row * 16 + i] = __int_as_float(f.x[i]); taps_out[row * 16 + 4 + i] = __int_as_float(f.y[i]);
                taps_out[row * 16 + 8 + i] = f.cx[i]; taps_out[row * 16 + 12 + i] = f.cy[i];
            }
        }
        const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
        for (int ch = lane; ch < s.C; ch += 64) {   // sum_j cy[j] * (sum_i cx[i] * texel_ij): the inference kernels' order and contraction
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float *lr = lat + (int64_t)f.y[j] * s.w * s.C + ch;
                float t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = lr[(int64_t)f.x[i] * s.C];
                const float rowv = __builtin_fmaf(t[3], f.cx[3], __builtin_fmaf(t[2], f.cx[2], __builtin_fmaf(t[1], f.cx[1], t[0] * f.cx[0])));
                acc = j == 0 ? rowv * f.cy[0] : __builtin_fmaf(rowv, f.cy[j], acc);
            }
            zlat[row * s.C + ch] = acc;
        }
    } else {
        const LatentFoot f = latent_footprint<true>(u, w, sxl, syl, s.w, s.h, ix_interp, ix_padding);
        const int o[4] = {f.y0 * s.w + f.x0, f.y0 * s.w + f.x1, f.y1 * s.w + f.x0, f.y1 * s.w + f.x1};
        const float wt[4] = {f.nw, f.ne, f.sw, f.se};
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { taps_out[row * 8 + i] = __int_as_float(o[i]); taps_out[row * 8 + 4 + i] = wt[i]; }
        }
        const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
        for (int ch = lane; ch < s.C; ch += 64) {
            float t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = lat[(int64_t)o[i] * s.C + ch];
            zlat[row * s.C + ch] = tap_sum(t[0], t[1], t[2], t[3], f);
        }
    }
}

// ---- the transpose of point_inputs_gen_kernel to the geometric leaves (train.hip point_inputs_bwd_kernel for any F, ld_in, C) ---
template <bool BC>
__global__ __launch_bounds__(64) void point_inputs_bwd_gen_kernel(DinerScene s, const float *__restrict__ latent_nhwc,
                                                                  const float *__restrict__ rays, const float *__restrict__ zsamp,
                                                                  int64_t NR, int K, int sb, int ix_interp, int ix_padding,
                                                                  const float *__restrict__ d_in, int64_t ld_in,
                                                                  const float *__restrict__ d_zlat, float *__restrict__ rowg,
                                                                  float *__restrict__ d_depths)
{
    const int64_t P = NR * (int64_t)K, row = blockIdx.x;
    const int v = (int)(row / P);
    const int64_t p = row - (int64_t)v * P;
    const int lane = threadIdx.x;
    const float *rp = rays + ((int64_t)sb * NR + p / K) * 8;
    const float zz = zsamp[(int64_t)sb * P + p];
    const float dwx = rp[3], dwy = rp[4], dwz = rp[5];
    const float wx = rp[0] + zz * dwx, wy = rp[1] + zz * dwy, wz = rp[2] + zz * dwz;  // nerf_renderer.py:304
    const View vw = load_view(s, sb, v);
    float px, py, pz, u, w;
    project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);                  // pixelnerf.py:91-93,105-108
    int ddx, ddy;   // view_geometry's pieces: the camera and the depth texel are needed below
    const float delta = nearest_depth(s, sb, v, u, w, ddx, ddy) - pz;

    // positional encodings: d sin(f a + phi) / d a = f cos(f a + phi) (positional_encoding.py:45-49); lanes stride the inputs,
    // each lane sums its own in a fixed order before the wave sums
    const float *gin = d_in + row * ld_in;
    const int F = s.num_freqs, e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1, d_in_n = e_pe1 + 2 * F;
    const float half_pi = 1.5707963267948966f;
    float t_p[4] = {0.f, 0.f, 0.f, 0.f};   // -> x_cam.x, x_cam.y, x_cam.z, depth_dist
    for (int e = lane; e < d_in_n; e += 64) {
        const float g = gin[e];
        if (e < 3) t_p[e] += g;
        else if (e < e_pe3) {
            const int j = (e - 3) / 3, i = (e - 3) % 3;
            const float f = ldexpf(s.freq_factor, j >> 1), a = i == 0 ? px : i == 1 ? py : pz;
            t_p[i] += g * cosf(__builtin_fmaf(a, f, (j & 1) ? half_pi : 0.0f)) * f;
        } else if (e == e_dir) t_p[3] += g;
        else if (e > e_dir) {
            const int j = e - e_pe1;
            const float f = ldexpf(s.freq_factor, j >> 1);
            t_p[3] += g * cosf(__builtin_fmaf(delta, f, (j & 1) ? half_pi : 0.0f)) * f;
        }
    }

    // grid_sample's gradient with respect to the grid (ATen, align_corners=False; nearest: 0)
    float gix = 0.f, giy = 0.f, mx = 0.f, my = 0.f;
    if constexpr (BC) {
        // bicubic: d/d ix = sum_ij dcx[i] cy[j] texel_ij, d/d iy = sum_ij cx[i] dcy[j] texel_ij; the padding acts on the integer tap
        // positions and puts no factor on the gradient (zeros: a tap outside the map has weight and derivative 0)
        const float sxl = pad_scale(s.w, s.feature_padding), syl = pad_scale(s.h, s.feature_padding);
        int xi[4], yi[4];
        float cx[4], cy[4], dcx[4], dcy[4];
        bicubic_axis(unnorm(u * sxl, (float)s.w / 2.0f), s.w, ix_padding, xi, cx, dcx);
        bicubic_axis(unnorm(w * syl, (float)s.h / 2.0f), s.h, ix_padding, yi, cy, dcy);
        mx = ((float)s.w / 2.0f) * sxl;   // d ix / d u
        my = ((float)s.h / 2.0f) * syl;
        const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
        const float *dz = d_zlat + row * s.C;
        for (int ch = lane * 4; ch < s.C; ch += 256) {   // C % 4 == 0
            const float4 g = *(const float4 *)(dz + ch);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float rx = 0.f, rd = 0.f;   // sum_i cx[i] <g, texel_ij>, sum_i dcx[i] <g, texel_ij>
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 t = *(const float4 *)(lat + ((int64_t)yi[j] * s.w + xi[i]) * s.C + ch);
                    const float d = g.x * t.x + g.y * t.y + g.z * t.z + g.w * t.w;
                    rx += cx[i] * d; rd += dcx[i] * d;
                }
                gix += cy[j] * rd; giy += dcy[j] * rx;
            }
        }
    } else if (ix_interp == DINER_INDEX_BILINEAR) {
        const float sxl = pad_scale(s.w, s.feature_padding), syl = pad_scale(s.h, s.feature_padding);
        float gx, gy;
        const float ix = pad_coord_grad(unnorm(u * sxl, (float)s.w / 2.0f), s.w, ix_padding, gx);
        const float iy = pad_coord_grad(unnorm(w * syl, (float)s.h / 2.0f), s.h, ix_padding, gy);
        mx = gx * ((float)s.w / 2.0f) * sxl;   // d ix / d u
        my = gy * ((float)s.h / 2.0f) * syl;
        const float x0f = floorf(ix), y0f = floorf(iy);
        const float fx = ix - x0f, ex = 1.0f - fx, fy = iy - y0f, ey = 1.0f - fy;
        const bool xa = x0f >= 0.0f && x0f <= (float)(s.w - 1), xb = x0f + 1.0f >= 0.0f && x0f + 1.0f <= (float)(s.w - 1);
        const bool ya = y0f >= 0.0f && y0f <= (float)(s.h - 1), yb = y0f + 1.0f >= 0.0f && y0f + 1.0f <= (float)(s.h - 1);
        const int x0 = safe_idx(x0f, s.w), x1 = safe_idx(x0f + 1.0f, s.w), y0 = safe_idx(y0f, s.h), y1 = safe_idx(y0f + 1.0f, s.h);
        const float kx[4] = {(xa && ya) ? -ey : 0.f, (xb && ya) ? ey : 0.f, (xa && yb) ? -fy : 0.f, (xb && yb) ? fy : 0.f};
        const float ky[4] = {(xa && ya) ? -ex : 0.f, (xb && ya) ? -fx : 0.f, (xa && yb) ? ex : 0.f, (xb && yb) ? fx : 0.f};
        const bool inm[4] = {xa && ya, xb && ya, xa && yb, xb && yb};
        const int o[4] = {y0 * s.w + x0, y0 * s.w + x1, y1 * s.w + x0, y1 * s.w + x1};
        const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
        const float *dz = d_zlat + row * s.C;
        for (int ch = lane * 4; ch < s.C; ch += 256) {   // C % 4 == 0
            const float4 g = *(const float4 *)(dz + ch);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!inm[i]) continue;   // (wave-uniform)
                const float4 t = *(const float4 *)(lat + (int64_t)o[i] * s.C + ch);
                const float d = g.x * t.x + g.y * t.y + g.z * t.z + g.w * t.w;
                gix += kx[i] * d; giy += ky[i] * d;
            }
        }
    }
    const float S0 = wave_sum(t_p[0]), S1 = wave_sum(t_p[1]), S2 = wave_sum(t_p[2]), Sd = wave_sum(t_p[3]);
    gix = wave_sum(gix); giy = wave_sum(giy);
    if (lane != 0) return;

    if (d_depths) atomicAdd(d_depths + (((int64_t)sb * s.NV + v) * s.H + ddy) * s.W + ddx, Sd);   // the nearest depth texel
    float gpx = S0, gpy = S1, gpz = S2 - Sd;                 // depth_dist = depth - x_cam.z
    const float qu = px / pz, qw = py / pz;
    const float Uu = qu * vw.fx + vw.cx, Uw = qw * vw.fy + vw.cy;
    const float gu = gix * mx, gw = giy * my;
    const float gUu = gu * 2.0f / s.image_w, gUw = gw * 2.0f / s.image_h;
    const float g_iw = -gu * 2.0f * Uu / (s.image_w * s.image_w), g_ih = -gw * 2.0f * Uw / (s.image_h * s.image_h);
    const float gqu = gUu * vw.fx, gqw = gUw * vw.fy;
    gpx += gqu / pz; gpy += gqw / pz; gpz -= (gqu * qu + gqw * qw) / pz;
    // x_cam = R x_w + t, dir_cam = R d_w (pixelnerf.py:92-101), x_w = o + z d (nerf_renderer.py:304-305)
    const float gp[3] = {gpx, gpy, gpz}, gd[3] = {gin[e_pe3], gin[e_pe3 + 1], gin[e_pe3 + 2]}, xw[3] = {wx, wy, wz}, dw[3] = {dwx, dwy, dwz};
    float *out = rowg + row * CAMG_COLS;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float gx = vw.r[j] * gp[0] + vw.r[3 + j] * gp[1] + vw.r[6 + j] * gp[2];
        const float gdd = vw.r[j] * gd[0] + vw.r[3 + j] * gd[1] + vw.r[6 + j] * gd[2];
        out[j] = gx;                      // d_o
        out[3 + j] = gdd + zz * gx;       // d_d
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[6 + i * 3 + j] = gp[i] * xw[j] + gd[i] * dw[j];
        out[15 + i] = gp[i];
    }
    out[18] = gUu * qu; out[19] = gUw * qw;   // focal
    out[20] = gUu; out[21] = gUw;             // c
    out[22] = g_iw; out[23] = g_ih;           // image_shape
}

}  // namespace train_gen
}  // namespace diner
