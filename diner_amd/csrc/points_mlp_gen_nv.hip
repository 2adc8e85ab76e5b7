// The "novel" form of the shape-general fp32 point/MLP kernel (points_mlp_gen.hip, points_mlp_gen_kernel.hpp): the point model of the
// fork's NOVEL configuration, reference src/models/novel/novel_pixelnerf.py:143-242.  It is PixelNeRF.forward with two differences:
//   * the points are GIVEN: xyz_in [SB,P,3] goes to the source cameras, the positional code, the depth feature and the encoder's
//     latent exactly as o + z d does in points_mlp_gen_kernel; viewdirs [SB,P,3] arrive per point; xyz_gen [SB,P,3] is projected by one
//     general camera per scene (:163-165, :183-186);
//   * a learned latent gen_latent [h_g, w_g, C] (NHWC, one map for every scene and view) is looked up at the general camera's uv with
//     the encoder's feature_padding and lookup mode (index(), :108-141) and ADDED to the encoder's latent before the MLP (:196).
// The general footprint does not depend on the view: it is computed once per point into a second tap record, and every gather of
// lin_z's input row -- every view, every lin_z block, every 512-column piece -- loads the four general texels beside the encoder's four
// and stores lookup(latent) + lookup(gen_latent): the sum is formed BEFORE lin_z, as in the reference.  The two lookups are fma chains
// in ATen's order nw, ne, sw, se; with gen_latent = 0 the sum is the encoder's lookup bit for bit.
//
// This unit holds what is the NOVEL model's own: the given points, the general tap record and the gather of the sum.  The packed weight
// image (diner_pack_mlp_gen), the input stage, lin_in, the ResNet blocks and the finish are points_mlp_gen_kernel.hpp's building blocks.
// The footprint is always common.hpp's latent_footprint<true> (any 4-tap lookup, bilinear / border included: the same taps and weights
// as the written-out form for every finite coordinate).  Bicubic and the lin_z-map forms are not served.  LDS: the 128-KiB A image +
// two Taps per row.
#include "points_mlp_gen_kernel.hpp"

namespace diner {
namespace gen {

struct NovelIn {            // what a validated diner_render_points_novel call hands to the kernel
    const float *xyz_in, *xyz_gen, *viewdirs;   // [SB,P,3] each
    int64_t P;
    const float *glat;      // [gh, gw, C] NHWC, C = d_latent
    int gh, gw;
    const float *gposes, *gfocal, *gc;          // [SB,4,4], [SB,2], [SB,2]
    float giw, gih;         // the general cameras' image shape (W, H)
    int ix_interp, ix_padding;                  // DINER_INDEX_* of both lookups
};

template <int RB, int CT>
__global__ __launch_bounds__(NWAVES * 64) void points_mlp_gen_nv_kernel(DinerScene s, Layout L, const float *__restrict__ Wp, NovelIn n,
                                                                        float *__restrict__ rgbsigma)
{
    __shared__ f32x4 lds[A_F4 + 2 * TILE_P * (sizeof(Tap) / sizeof(f32x4))];  // A image + the encoder's Tap + the general Tap per row
    f32x4 *A4 = lds;
    float *A = (float *)lds;
    Tap *taps = (Tap *)(lds + A_F4);
    Tap *gtaps = taps + TILE_P;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT;
    const int sb = blockIdx.y;
    const int64_t P = n.P;
    const int64_t tile = xcd_tile(gridDim.x, blockIdx.x);
    const float *bias = Wp + L.off_bias;

    // ---- this thread's point: given ----------
    const int row = tid & 63;
    int64_t p = tile * TILE_P + row;
    if (p > P - 1) p = P - 1;  // tail tile: duplicate the last point, masked at the store
    const float *xp = n.xyz_in + ((int64_t)sb * P + p) * 3, *dp = n.viewdirs + ((int64_t)sb * P + p) * 3;
    const float wx = xp[0], wy = xp[1], wz = xp[2];        // novel_pixelnerf.py:159
    const float dwx = dp[0], dwy = dp[1], dwz = dp[2];     // :171

    f32x16 x[RB][CT], xsum[RB][CT];
    acc_zero(xsum);

    const float sxl = pad_scale(s.w, s.feature_padding), syl = pad_scale(s.h, s.feature_padding);
    const int F = L.F, din_pad = 8 * L.njb_in;
    const int c4 = L.dlat / 4;   // float4 per texel of either latent

    if (L.nvb > 0 && wave == 0)
        // ---- the general footprint, once per point (:163-165, :183-186, index() :126-137): its own map size in the footprint and in
        // the feature-padding scale.  The first barrier of the view loop publishes it.
        gtaps[row] = tap_of(camera_footprint(view_of(n.gposes, n.gfocal, n.gc, sb), n.giw, n.gih, n.xyz_gen + ((int64_t)sb * P + p) * 3,
                                             n.gh, n.gw, s.feature_padding, n.ix_interp, n.ix_padding), n.gw, c4);
    const f32x4 *glat = (const f32x4 *)n.glat;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> A[:, 0:din_pad] (:160-161, :172-180, :199-200; input layout :225, after the latent);
        // the encoder's footprint -> taps ----------
        {
            float px, py, pz, u, w, dcx, dcy, dcz, delta;
            view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);
            for (int e = wave; e < din_pad; e += NWAVES)
                A[a_off(row, e)] = input_element(e, px, py, pz, dcx, dcy, dcz, delta, F, s.freq_factor);
            if (wave == 0)   // footprint of the lookup mode in the encoder's latent map (image_encoder.py:97-127; common.hpp)
                taps[row] = tap_of(latent_footprint<true>(u, w, sxl, syl, s.w, s.h, n.ix_interp, n.ix_padding), s.w, c4);
        }
        __syncthreads();
        acc_bias(x, bias + L.bias_lin_in(), false, ct0, NT, lane);
        gemm(x, A4, (const f32x4 *)(Wp + L.off_in), L.njb_in, 0, L.njb_in, rb0, ct0, NT, lane);   // resnetfc.py:139
        __syncthreads();

        const f32x4 *lat = (const f32x4 *)s.latent + ((int64_t)sb * s.NV + v) * s.h * s.w * c4;
        for (int b = 0; b < L.nvb; ++b) {
            acc_bias(x, bias + L.bias_lin_z(b), true, ct0, NT, lane);                               // :152-153 x = x + lin_z(z)
            for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
                // ---- z[:, k0 : k0 + kc] = lookup(latent_v) + lookup(gen_latent) of the 64 points -> A (each wave gathers 8 rows) ----
                const int kc4 = (L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX) / 4;
                for (int rr = 0; rr < TILE_P / NWAVES; ++rr) {
                    const int r = wave * (TILE_P / NWAVES) + rr;
                    const Tap t = taps[r], g = gtaps[r];
                    for (int q = lane; q < kc4; q += 64) {
                        const int qq = k0 / 4 + q;
                        const f32x4 a = lat[t.o00 + qq], bb = lat[t.o01 + qq], c = lat[t.o10 + qq], d = lat[t.o11 + qq];
                        const f32x4 ga = glat[g.o00 + qq], gb = glat[g.o01 + qq], gc = glat[g.o10 + qq], gd = glat[g.o11 + qq];
#pragma unroll
                        for (int i = 0; i < 4; ++i)                                                 // novel_pixelnerf.py:196
                            A[a_off(r, 4 * q + i)] = tap_sum(ga[i], gb[i], gc[i], gd[i], g) + tap_sum(a[i], bb[i], c[i], d[i], t);
                    }
                }
                __syncthreads();
                gemm(x, A4, (const f32x4 *)(Wp + L.off_z + b * L.w_z), L.njb_lat, k0 / 8, kc4 / 2, rb0, ct0, NT, lane);
                __syncthreads();
            }
            resnet_block(x, A, Wp, L, b, rb0, ct0, lane);
        }
        acc_add(xsum, x);                                                                           // :146-149
    }
    finish(xsum, A, Wp, L, s.NV, rb0, ct0, lane, wave, sb, tile, P, rgbsigma);                 // head: novel_pixelnerf.py:236-240
}

// a call api.hip has validated (diner_render_points_novel): P > 0, SB > 0, the tile count fits a grid
int launch_points_mlp_novel(const DinerScene &s, const DinerLatentIndex &ix, const DinerNovelGen &g, const DinerMlpShape &m,
                            const float *mlp_packed, const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P,
                            float *rgbsigma, hipStream_t st)
{
    const Layout L = layout_of(m);
    const NovelIn n{xyz_in, xyz_gen, viewdirs, P, g.latent, g.h, g.w, g.poses, g.focal, g.c, g.image_w, g.image_h, ix.interp, ix.padding};
    const dim3 grid((unsigned)((P + TILE_P - 1) / TILE_P), (unsigned)s.SB), block(NWAVES * 64);
    void (*const kernel)(DinerScene, Layout, const float *, NovelIn, float *) =
        L.H <= 128 ? points_mlp_gen_nv_kernel<1, 1> : L.H <= 256 ? points_mlp_gen_nv_kernel<2, 1> : points_mlp_gen_nv_kernel<2, 2>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, s, L, mlp_packed, n, rgbsigma);
    return check_launch("points_mlp_gen_nv_kernel");
}

}  // namespace gen
}  // namespace diner
