// The two kernels the NOVEL point model's training path adds to the shape-general one (diner_amd/training_novel.py; train_gen.hip has the
// GEMMs and the description of the staged schedule).  The fork's NOVEL PixelNeRF (reference src/models/novel/novel_pixelnerf.py:143-242)
// is PixelNeRF.forward with GIVEN points, per-point viewdirs, and a learned latent gen_latent [h_g, w_g, C] that is looked up at one
// general camera per scene and added to the encoder's lookup in every view before lin_z (:196).  Under autograd d(final_latent) goes to
// both maps, and index() (:108-141) repeats the one general map over the views, so its gradient sums over them.
//   point_inputs_novel   point_inputs_gen_kernel<false> (train_gen_points.hpp) at given points: the same rows (row = v*P + p), the same
//                        in [R, ld_in] columns (common.hpp's input_element), the same taps [R,8] record of the encoder's lookup;
//                        zlat [R, C] = lookup(latent[sb, v], uv) + lookup(gen_latent, gen_uv), each an fma chain in ATen's order
//                        nw, ne, sw, se and the sum formed last, as points_mlp_gen_nv.hip forms it (gen_latent = 0: the encoder's
//                        lookup bit for bit); gen_taps [P,8]: the general footprint, which no view changes, written by view 0's rows.
//   novel_gen_scatter    grid_sample's input gradient of the general lookup: per point and channel the sum of d_zlat over the NV view
//                        rows in registers (fixed order v = 0 .. NV-1), then train.hip's bilinear_scatter_kernel scheme -- one wave
//                        walks SCATTER_RUN consecutive points, 64 channels per pass, merges contributions while the footprint stays,
//                        and flushes one float atomicAdd per used tap on 256-byte contiguous NHWC rows; a tap of weight 0 is never
//                        flushed.  All scenes accumulate into the one map.
// The encoder latent's gradient needs nothing new: taps has bilinear_scatter_kernel's format.
// view_geometry, input_element, latent_footprint, camera_footprint: common.hpp's, shared with the render kernels.
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
    float px, py, pz, u, w, dcx, dcy, dcz, delta;
    view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);   // :160-161, :172-180, :199-200
    for (int e = lane; e < ld_in; e += 64) in[row * ld_in + e] = input_element(e, px, py, pz, dcx, dcy, dcz, delta, s.num_freqs, s.freq_factor);
    if (!zlat) return;   // combine_layer 0: no lin_z, neither latent is read (wave-uniform)

    // the encoder's footprint (image_encoder.py:97-127) and the general one (novel_pixelnerf.py:163-165, :183-186, index() :126-137):
    // the scene's feature_padding scaled by each map's own size, one lookup mode for both
    const LatentFoot f = latent_footprint<true>(u, w, pad_scale(s.w, s.feature_padding), pad_scale(s.h, s.feature_padding), s.w, s.h,
                                                ix_interp, ix_padding);
    const int o[4] = {f.y0 * s.w + f.x0, f.y0 * s.w + f.x1, f.y1 * s.w + f.x0, f.y1 * s.w + f.x1};
    const float wt[4] = {f.nw, f.ne, f.sw, f.se};
    const LatentFoot fg = camera_footprint(view_of(n.gposes, n.gfocal, n.gc, sb), n.giw, n.gih, xyz_gen + ((int64_t)sb * P + p) * 3, n.gh,
                                           n.gw, s.feature_padding, ix_interp, ix_padding);
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
        zlat[row * s.C + ch] = tap_sum(g[0], g[1], g[2], g[3], fg) + tap_sum(t[0], t[1], t[2], t[3], f);   // novel_pixelnerf.py:196
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
