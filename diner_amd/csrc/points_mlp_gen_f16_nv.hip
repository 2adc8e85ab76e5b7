// The "novel" form of the shape-general f16x3 point/MLP kernel (points_mlp_gen_f16.hip, points_mlp_gen_f16_kernel.hpp): the point model
// of the fork's NOVEL configuration, reference src/models/novel/novel_pixelnerf.py:143-242, in the split-fp16 arithmetic of that header.
// What differs from PixelNeRF.forward is described in points_mlp_gen_nv.hip, the fp32 twin: given points xyz_in / xyz_gen and per-point
// viewdirs, and lookup(gen_latent) at the general camera's uv added to the encoder's lookup before lin_z.  The general footprint is
// computed once per point into a second tap record; both records carry their weights * 2^-4, the two fma chains are added in fp32 and
// the hi / lo split takes the SUM, so the operand is split once, as the encoder's lookup alone is in the parent kernel.
//
// This unit holds what is the NOVEL model's own: the given points, the general tap record and the gather of the sum.  The packed weight
// image (diner_pack_mlp_gen_f16), the input stage, lin_in, the ResNet blocks and the finish are points_mlp_gen_f16_kernel.hpp's building
// blocks.  The footprint is always common.hpp's latent_footprint<true>.  Bicubic and the lin_z-map forms are not served.  LDS: the
// 128-KiB A image + two Taps per point.
#include "points_mlp_gen_f16_kernel.hpp"

namespace diner {
namespace genf16 {

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
__global__ __launch_bounds__(NWAVES * 64) void points_mlp_gen_f16_nv_kernel(DinerScene s, Layout L, const float *__restrict__ Wp, NovelIn n,
                                                                            float *__restrict__ rgbsigma)
{
    __shared__ u32x4 lds[A_H8 + 2 * TILE_P * (sizeof(Tap) / sizeof(u32x4))];  // A image + the encoder's Tap + the general Tap per point
    u32x4 *A = lds;
    const h8 *A8 = (const h8 *)lds;
    Tap *taps = (Tap *)(lds + A_H8);
    Tap *gtaps = taps + TILE_P;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT, H = L.H;
    const int sb = blockIdx.y;
    const int64_t P = n.P;
    const int64_t tile = xcd_tile(gridDim.x, blockIdx.x);
    const h8 *Wh = (const h8 *)Wp;
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
    const int F = L.F;
    const int c4 = L.dlat / 4;   // float4 per texel of either latent

    if (L.nvb > 0 && wave == 0)
        // ---- the general footprint, once per point (:163-165, :183-186, index() :126-137): its own map size in the footprint and in
        // the feature-padding scale.  The first barrier of the view loop publishes it.
        gtaps[row] = tap_of(camera_footprint(view_of(n.gposes, n.gfocal, n.gc, sb), n.giw, n.gih, n.xyz_gen + ((int64_t)sb * P + p) * 3,
                                             n.gh, n.gw, s.feature_padding, n.ix_interp, n.ix_padding), n.gw, c4);
    const f32x4 *glat = (const f32x4 *)n.glat;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> planes 0 .. 2 nkb_in of A (a wave writes whole planes; :160-161, :172-180, :199-200;
        // input layout :225, after the latent); footprint -> taps ----------
        {
            float px, py, pz, u, w, dcx, dcy, dcz, delta;
            view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);
            for (int pl = wave; pl < 2 * L.nkb_in; pl += NWAVES)
                store_input_plane(A, pl, row, px, py, pz, dcx, dcy, dcz, delta, F, s.freq_factor);
            if (wave == 0)   // footprint of the lookup mode in the encoder's latent map (image_encoder.py:97-127; common.hpp)
                taps[row] = tap_of(latent_footprint<true>(u, w, sxl, syl, s.w, s.h, n.ix_interp, n.ix_padding), s.w, c4);
        }
        __syncthreads();
        acc_bias(x, bias + L.bias_lin_in(), false, ct0, NT, lane);
        gemm(x, A8, Wh + L.off_in / 8, L.nkb_in, 0, L.nkb_in, rb0, ct0, NT, lane);                  // resnetfc.py:139
        __syncthreads();

        const f32x4 *lat = (const f32x4 *)s.latent + ((int64_t)sb * s.NV + v) * s.h * s.w * c4;
        for (int b = 0; b < L.nvb; ++b) {
            acc_bias(x, bias + L.bias_lin_z(b), true, ct0, NT, lane);                               // :152-153 x = x + lin_z(z)
            for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
                // ---- z[:, k0 : k0 + kc] / 16 = (lookup(latent_v) + lookup(gen_latent)) / 16 of the 64 points -> A: a wave gathers 8
                // points, a lane 8 columns of one ----
                const int kc = L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX;
                const int npl = (kc + 15) / 16 * 2;   // planes the GEMM reads (the last one zero when kc % 16 == 8)
                const int r = wave * (TILE_P / NWAVES) + (lane & 7);
                const Tap t = taps[r], g = gtaps[r];
                for (int pl = lane >> 3; pl < npl; pl += 8) {
                    u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
                    if (pl * 8 < kc) {
                        unsigned ph[4], plo[4];
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            const int qq = k0 / 4 + pl * 2 + half;
                            const f32x4 a = lat[t.o00 + qq], bb = lat[t.o01 + qq], c = lat[t.o10 + qq], d = lat[t.o11 + qq];
                            const f32x4 ga = glat[g.o00 + qq], gb = glat[g.o01 + qq], gc = glat[g.o10 + qq], gd = glat[g.o11 + qq];
                            _Float16 hi[4], lo[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i)                                             // novel_pixelnerf.py:196
                                split(tap_sum(ga[i], gb[i], gc[i], gd[i], g) + tap_sum(a[i], bb[i], c[i], d[i], t), hi[i], lo[i]);
                            ph[2 * half] = pack2(hi[0], hi[1]); ph[2 * half + 1] = pack2(hi[2], hi[3]);
                            plo[2 * half] = pack2(lo[0], lo[1]); plo[2 * half + 1] = pack2(lo[2], lo[3]);
                        }
                        vh = u32x4{ph[0], ph[1], ph[2], ph[3]}; vl = u32x4{plo[0], plo[1], plo[2], plo[3]};
                    }
                    A[a_slot(pl, 0, r)] = vh;
                    A[a_slot(pl, 1, r)] = vl;
                }
                __syncthreads();
                gemm(x, A8, Wh + (L.off_z + b * L.w_z) / 8, L.nkb_lat, k0 / 16, npl / 2, rb0, ct0, NT, lane);
                __syncthreads();
            }
            f32x16 net[RB][CT];   // resnet_block(), written out: through the helper <2,2> spills one VGPR more and all three more SGPRs
            store_act(x, A, L.beta, rb0, ct0, NT, lane);                                            // :62 fc_0(act(x))
            __syncthreads();
            acc_bias(net, bias + L.bias_fc0(b), false, ct0, NT, lane);
            gemm(net, A8, Wh + (L.off_fc0 + b * L.w_h) / 8, H / 16, 0, H / 16, rb0, ct0, NT, lane);
            __syncthreads();
            store_act(net, A, L.beta, rb0, ct0, NT, lane);                                          // :63 fc_1(act(net))
            __syncthreads();
            acc_bias(x, bias + L.bias_fc1(b), true, ct0, NT, lane);                                 // :69 x + dx
            gemm(x, A8, Wh + (L.off_fc1 + b * L.w_h) / 8, H / 16, 0, H / 16, rb0, ct0, NT, lane);
            __syncthreads();
        }
        acc_add(xsum, x);                                                                           // :146-149
    }
    finish(xsum, A, Wp, L, s.NV, rb0, ct0, tid, sb, tile, P, rgbsigma);                             // head: novel_pixelnerf.py:236-240
}

// a call api.hip has validated (diner_render_points_novel): P > 0, SB > 0, the tile count fits a grid, mlp_packed 16-byte aligned
int launch_points_mlp_novel(const DinerScene &s, const DinerLatentIndex &ix, const DinerNovelGen &g, const DinerMlpShape &m,
                            const float *mlp_packed, const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P,
                            float *rgbsigma, hipStream_t st)
{
    const Layout L = layout_of(m);
    const NovelIn n{xyz_in, xyz_gen, viewdirs, P, g.latent, g.h, g.w, g.poses, g.focal, g.c, g.image_w, g.image_h, ix.interp, ix.padding};
    const dim3 grid((unsigned)((P + TILE_P - 1) / TILE_P), (unsigned)s.SB), block(NWAVES * 64);
    void (*const kernel)(DinerScene, Layout, const float *, NovelIn, float *) =
        L.H <= 128   ? points_mlp_gen_f16_nv_kernel<1, 1>
        : L.H <= 256 ? points_mlp_gen_f16_nv_kernel<2, 1>
                     : points_mlp_gen_f16_nv_kernel<2, 2>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, s, L, mlp_packed, n, rgbsigma);
    return check_launch("points_mlp_gen_f16_nv_kernel");
}

}  // namespace genf16
}  // namespace diner
