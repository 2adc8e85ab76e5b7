// The two kernels the NOVEL point model's training path adds to the shape-general one (diner_amd/training_novel.py; train_gen.hip has the
// GEMMs and the description of the staged schedule).  The fork's NOVEL PixelNeRF (reference src/models/novel/novel_pixelnerf.py:143-242)
// is PixelNeRF.forward with GIVEN points, per-point viewdirs, and a learned latent gen_latent [h_g, w_g, C] that is looked up at one
// general camera per scene and added to the encoder's lookup in every view before lin_z (:196).  Under autograd d(final_latent) goes to
// both maps, and index() (:108-141) repeats the one general map over the views, so its gradient sums over them.
//   point_inputs_novel   point_inputs_gen_kernel<false> (train_gen_points.hpp) at given points: the same rows (row = v*P + p), the same
//                        in [R, ld_in] columns with the same sinf expressions, the same taps [R,8] record of the encoder's lookup;
//                        zlat [R, C] = lookup(latent[sb, v], uv) + lookup(gen_latent, gen_uv), each an fma chain in ATen's order
//                        nw, ne, sw, se and the sum formed last, as points_mlp_gen_nv.hip forms it (gen_latent = 0: the encoder's
//                        lookup bit for bit); gen_taps [P,8]: the general footprint, which no view changes, written by view 0's rows.
//   novel_gen_scatter    grid_sample's input gradient of the general lookup: per point and channel the sum of d_zlat over the NV view
//                        rows in registers (fixed order v = 0 .. NV-1), then train.hip's bilinear_scatter_kernel scheme -- one wave
//                        walks SCATTER_RUN consecutive points, 64 channels per pass, merges contributions while the footprint stays,
//                        and flushes one float atomicAdd per used tap on 256-byte contiguous NHWC rows; a tap of weight 0 is never
//                        flushed.  All scenes accumulate into the one map.
// The encoder latent's gradient needs nothing new: taps has bilinear_scatter_kernel's format.
// latent_footprint, project, rotate, load_view: common.hpp's, shared with every other kernel.
#include "train_blocks.hpp"

namespace diner {
namespace train_novel {

using namespace train_blocks;

struct GenIn {              // what a validated diner_train_point_inputs_novel call hands to the kernel of DinerNovelGen
    const float *glat;      // [gh, gw, C] NHWC
    int gh, gw;
    const float *gposes, *gfocal, *gc;   // [SB,4,4], [SB,2], [SB,2]
    float giw, gih;         // the general cameras' image shape (W, H)
};

__global__ __launch_bounds__(64) void point_inputs_novel_kernel(DinerScene s, const float *__restrict__ latent_nhwc, GenIn n,
                                                                const float *__restrict__ xyz_in, const float *__restrict__ xyz_gen,
                                                                const float *__restrict__ viewdirs, int64_t P, int sb, int ix_interp,
                                                                int ix_padding, float *__restrict__ in, int64_t ld_in,
                                                                float *__restrict__ zlat, float *__restrict__ taps_out,
                                                                float *__restrict__ gen_taps)
{
    const int64_t row = blockIdx.x;
    const int v = (int)(row / P);
    const int64_t p = row - (int64_t)v * P;
    const int lane = threadIdx.x;
    const float *xp = xyz_in + ((int64_t)sb * P + p) * 3, *dp = viewdirs + ((int64_t)sb * P + p) * 3;
    const float wx = xp[0], wy = xp[1], wz = xp[2];        // novel_pixelnerf.py:159
    const float dwx = dp[0], dwy = dp[1], dwz = dp[2];     // :171
    const View vw = load_view(s, sb, v);
    float px, py, pz, u, w, dcx, dcy, dcz;
    project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);                  // :160-161, :177-180
    rotate(vw, dwx, dwy, dwz, dcx, dcy, dcz);                                           // :172-173
    const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
    const int ddx = safe_idx(__builtin_rintf(clipf(unnorm(u, (float)s.W / 2.0f), (float)(s.W - 1))), s.W);
    const int ddy = safe_idx(__builtin_rintf(clipf(unnorm(w, (float)s.H / 2.0f), (float)(s.H - 1))), s.H);
    const float delta = tex[((int64_t)ddy * s.W + ddx) * 2].w - pz;                    // :199-200
    const int F = s.num_freqs, e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1;
    const float half_pi = 1.5707963267948966f;
    for (int e = lane; e < ld_in; e += 64) {               // point_inputs_gen_kernel's columns and expressions
        float val;
        if (e < 3) val = e == 0 ? px : e == 1 ? py : pz;
        else if (e < e_pe3) { const int j = (e - 3) / 3, i = (e - 3) % 3;    // positional_encoding.py:45-49
            val = sinf(__builtin_fmaf(i == 0 ? px : i == 1 ? py : pz, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
        else if (e < e_dir) val = e == e_pe3 ? dcx : e == e_pe3 + 1 ? dcy : dcz;
        else if (e == e_dir) val = delta;
        else if (e < e_pe1 + 2 * F) { const int j = e - e_pe1;
            val = sinf(__builtin_fmaf(delta, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
        else val = 0.0f;
        in[row * ld_in + e] = val;
    }
    if (!zlat) return;   // combine_layer 0: no lin_z, neither latent is read (wave-uniform)

    // the encoder's footprint (image_encoder.py:97-127) and the general one (novel_pixelnerf.py:163-165, :183-186, index() :126-137):
    // the scene's feature_padding scaled by each map's own size, one lookup mode for both
    const float sxl = ((float)s.w - s.feature_padding * 2.0f) / (float)s.w, syl = ((float)s.h - s.feature_padding * 2.0f) / (float)s.h;
    const LatentFoot f = latent_footprint<true>(u, w, sxl, syl, s.w, s.h, ix_interp, ix_padding);
    const int o[4] = {f.y0 * s.w + f.x0, f.y0 * s.w + f.x1, f.y1 * s.w + f.x0, f.y1 * s.w + f.x1};
    const float wt[4] = {f.nw, f.ne, f.sw, f.se};
    const float *gx = xyz_gen + ((int64_t)sb * P + p) * 3;
    View gv;
    const float *Pm = n.gposes + (int64_t)sb * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gv.r[i * 3 + 0] = Pm[i * 4 + 0]; gv.r[i * 3 + 1] = Pm[i * 4 + 1]; gv.r[i * 3 + 2] = Pm[i * 4 + 2];
        gv.t[i] = Pm[i * 4 + 3];
    }
    gv.fx = n.gfocal[sb * 2]; gv.fy = n.gfocal[sb * 2 + 1]; gv.cx = n.gc[sb * 2]; gv.cy = n.gc[sb * 2 + 1];
    float gpx, gpy, gpz, gu, gw;
    project(gv, n.giw, n.gih, gx[0], gx[1], gx[2], gpx, gpy, gpz, gu, gw);
    const float sxg = ((float)n.gw - s.feature_padding * 2.0f) / (float)n.gw, syg = ((float)n.gh - s.feature_padding * 2.0f) / (float)n.gh;
    const LatentFoot fg = latent_footprint<true>(gu, gw, sxg, syg, n.gw, n.gh, ix_interp, ix_padding);
    const int og[4] = {fg.y0 * n.gw + fg.x0, fg.y0 * n.gw + fg.x1, fg.y1 * n.gw + fg.x0, fg.y1 * n.gw + fg.x1};
    const float wg[4] = {fg.nw, fg.ne, fg.sw, fg.se};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { taps_out[row * 8 + i] = __int_as_float(o[i]); taps_out[row * 8 + 4 + i] = wt[i]; }
        if (v == 0) {   // the general lookup does not depend on the view
#pragma unroll
            for (int i = 0; i < 4; ++i) { gen_taps[p * 8 + i] = __int_as_float(og[i]); gen_taps[p * 8 + 4 + i] = wg[i]; }
        }
    }
    const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
    for (int ch = lane; ch < s.C; ch += 64) {
        float t[4], g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { t[i] = lat[(int64_t)o[i] * s.C + ch]; g[i] = n.glat[(int64_t)og[i] * s.C + ch]; }
        const float zl = __builtin_fmaf(t[3], wt[3], __builtin_fmaf(t[2], wt[2], __builtin_fmaf(t[1], wt[1], t[0] * wt[0])));
        const float zg = __builtin_fmaf(g[3], wg[3], __builtin_fmaf(g[2], wg[2], __builtin_fmaf(g[1], wg[1], g[0] * wg[0])));
        zlat[row * s.C + ch] = zg + zl;                                                 // novel_pixelnerf.py:196
    }
}

__global__ __launch_bounds__(64) void novel_gen_scatter_kernel(const float *__restrict__ dz, const float *__restrict__ gen_taps, int64_t P,
                                                               int C, int NV, float *__restrict__ d_gen_nhwc)
{
    const int64_t p0 = (int64_t)blockIdx.x * SCATTER_RUN;
    const int64_t p1 = p0 + SCATTER_RUN < P ? p0 + SCATTER_RUN : P;
    const int lane = threadIdx.x;
    for (int ch = lane; ch < C; ch += 64) {
        int cur[4] = {-1, -1, -1, -1};
        bool have = false;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        bool used[4] = {false, false, false, false};
        for (int64_t p = p0; p < p1; ++p) {
            int o[4];
            float wt[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { o[i] = __float_as_int(gen_taps[p * 8 + i]); wt[i] = gen_taps[p * 8 + 4 + i]; }
            if (!have || o[0] != cur[0] || o[1] != cur[1] || o[2] != cur[2] || o[3] != cur[3]) {  // wave-uniform
                if (have) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (used[i]) atomicAdd(d_gen_nhwc + (int64_t)cur[i] * C + ch, acc[i]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) { cur[i] = o[i]; acc[i] = 0.f; used[i] = false; }
                have = true;
            }
            float g = dz[p * C + ch];                      // the view sum: index() repeats the one map over the views
            for (int v = 1; v < NV; ++v) g += dz[((int64_t)v * P + p) * C + ch];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (wt[i] != 0.0f) { acc[i] += g * wt[i]; used[i] = true; }
        }
        if (have) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (used[i]) atomicAdd(d_gen_nhwc + (int64_t)cur[i] * C + ch, acc[i]);
        }
    }
}

}  // namespace train_novel

// calls api.hip has validated (diner_train_point_inputs_novel, diner_train_novel_gen_scatter): P > 0, the row / run count fits a grid
int launch_train_point_inputs_novel(const DinerScene &s, const DinerLatentIndex &ix, const float *latent_nhwc, const DinerNovelGen &g,
                                    const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P, int sb, float *in,
                                    int64_t ld_in, float *zlat, float *taps, float *gen_taps, hipStream_t st)
{
    const int64_t R = P * s.NV;
    const train_novel::GenIn n{g.latent, g.h, g.w, g.poses, g.focal, g.c, g.image_w, g.image_h};
    hipLaunchKernelGGL(train_novel::point_inputs_novel_kernel, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, n, xyz_in, xyz_gen, viewdirs, P,
                       sb, ix.interp, ix.padding, in, ld_in, zlat, taps, gen_taps);
    return check_launch("train_novel::point_inputs_novel_kernel");
}

int launch_train_novel_gen_scatter(const float *dz, const float *gen_taps, int64_t P, int C, int NV, float *d_gen_nhwc, hipStream_t st)
{
    using namespace train_novel;
    hipLaunchKernelGGL(novel_gen_scatter_kernel, dim3((unsigned)((P + SCATTER_RUN - 1) / SCATTER_RUN)), dim3(64), 0, st, dz, gen_taps, P, C, NV,
                       d_gen_nhwc);
    return check_launch("train_novel::novel_gen_scatter_kernel");
}

}  // namespace diner
