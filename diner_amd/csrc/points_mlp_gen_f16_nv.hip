// The "novel" form of the shape-general f16x3 point/MLP kernel (points_mlp_gen_f16.hip, points_mlp_gen_f16_kernel.hpp): the point model
// of the fork's NOVEL configuration, reference src/models/novel/novel_pixelnerf.py:143-242, in the split-fp16 arithmetic of that header.
// What differs from PixelNeRF.forward is described in points_mlp_gen_nv.hip, the fp32 twin: given points xyz_in / xyz_gen and per-point
// viewdirs, and lookup(gen_latent) at the general camera's uv added to the encoder's lookup before lin_z.  The general footprint is
// computed once per point into a second tap record; both records carry their weights * 2^-4, the two fma chains are added in fp32 and
// the hi / lo split takes the SUM, so the operand is split once, as the encoder's lookup alone is in the parent kernel.
//
// Layout, gemm(), acc_bias(), act(), store_act(), the Tap record and the packed weight image (diner_pack_mlp_gen_f16) are those of
// points_mlp_gen_f16_kernel.hpp, unchanged; the kernel below is that header's template without its mode parameter: the footprint is
// always common.hpp's latent_footprint<true>.  Bicubic and the lin_z-map forms are not served.  LDS: the 128-KiB A image + two Taps
// per point.
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

__device__ __forceinline__ Tap tap_of(const LatentFoot &f, int lw, int c4)   // the weights * 2^-4
{
    Tap t;
    t.o00 = (f.y0 * lw + f.x0) * c4; t.o01 = (f.y0 * lw + f.x1) * c4;
    t.o10 = (f.y1 * lw + f.x0) * c4; t.o11 = (f.y1 * lw + f.x1) * c4;
    t.nw = f.nw * ACT_SCALE; t.ne = f.ne * ACT_SCALE; t.sw = f.sw * ACT_SCALE; t.se = f.se * ACT_SCALE;
    return t;
}

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
    int64_t tile;   // XCD-aware tile order (points_mlp.hip)
    {
        const int64_t nwg = gridDim.x, b = blockIdx.x, q = nwg / 8, r = nwg % 8, xcd = b % 8;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
    }
    const h8 *Wh = (const h8 *)Wp;
    const float *bias = Wp + L.off_bias;

    const int row = tid & 63;
    int64_t p = tile * TILE_P + row;
    if (p > P - 1) p = P - 1;  // tail tile: duplicate the last point, masked at the store
    const float *xp = n.xyz_in + ((int64_t)sb * P + p) * 3, *dp = n.viewdirs + ((int64_t)sb * P + p) * 3;
    const float wx = xp[0], wy = xp[1], wz = xp[2];        // novel_pixelnerf.py:159
    const float dwx = dp[0], dwy = dp[1], dwz = dp[2];     // :171

    f32x16 x[RB][CT], net[RB][CT], xsum[RB][CT];
#pragma unroll
    for (int tm = 0; tm < RB; ++tm)
#pragma unroll
        for (int tn = 0; tn < CT; ++tn)
#pragma unroll
            for (int i = 0; i < 16; ++i) xsum[tm][tn][i] = 0.0f;

    const float sxl = ((float)s.w - s.feature_padding * 2.0f) / (float)s.w;  // image_encoder.py:113-114
    const float syl = ((float)s.h - s.feature_padding * 2.0f) / (float)s.h;
    const int F = L.F, e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1;
    const int c4 = L.dlat / 4;   // float4 per texel of either latent

    if (L.nvb > 0 && wave == 0) {
        // ---- the general footprint, once per point (:163-165, :183-186, index() :126-137): its own map size in the footprint and in
        // the feature-padding scale.  The first barrier of the view loop publishes it.
        const float *gx = n.xyz_gen + ((int64_t)sb * P + p) * 3;
        View gv;
        const float *Pm = n.gposes + (int64_t)sb * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gv.r[i * 3 + 0] = Pm[i * 4 + 0]; gv.r[i * 3 + 1] = Pm[i * 4 + 1]; gv.r[i * 3 + 2] = Pm[i * 4 + 2];
            gv.t[i] = Pm[i * 4 + 3];
        }
        gv.fx = n.gfocal[sb * 2]; gv.fy = n.gfocal[sb * 2 + 1]; gv.cx = n.gc[sb * 2]; gv.cy = n.gc[sb * 2 + 1];
        float px, py, pz, u, w;
        project(gv, n.giw, n.gih, gx[0], gx[1], gx[2], px, py, pz, u, w);
        const float sxg = ((float)n.gw - s.feature_padding * 2.0f) / (float)n.gw;
        const float syg = ((float)n.gh - s.feature_padding * 2.0f) / (float)n.gh;
        gtaps[row] = tap_of(latent_footprint<true>(u, w, sxg, syg, n.gw, n.gh, n.ix_interp, n.ix_padding), n.gw, c4);
    }
    const f32x4 *glat = (const f32x4 *)n.glat;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> planes 0 .. 2 nkb_in of A (a wave writes whole planes); footprint -> taps ----------
        {
            const View vw = load_view(s, sb, v);
            float px, py, pz, u, w;
            project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);   // :160-161, :177-180
            float dcx, dcy, dcz;
            rotate(vw, dwx, dwy, dwz, dcx, dcy, dcz);                            // :172-173
            const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
            const int ddx = safe_idx(__builtin_rintf(clipf(unnorm(u, (float)s.W / 2.0f), (float)(s.W - 1))), s.W);
            const int ddy = safe_idx(__builtin_rintf(clipf(unnorm(w, (float)s.H / 2.0f), (float)(s.H - 1))), s.H);
            const float delta = tex[((int64_t)ddy * s.W + ddx) * 2].w - pz;     // :199-200
            const float half_pi = 1.5707963267948966f;
            for (int pl = wave; pl < 2 * L.nkb_in; pl += NWAVES) {              // input layout :225 (after the latent)
                unsigned ph[4], plo[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    _Float16 hi[2], lo[2];
#pragma unroll
                    for (int j2 = 0; j2 < 2; ++j2) {
                        const int e = pl * 8 + jj * 2 + j2;
                        float val;
                        if (e < 3) val = e == 0 ? px : e == 1 ? py : pz;
                        else if (e < e_pe3) { const int j = (e - 3) / 3, i = (e - 3) % 3;    // positional_encoding.py:45-49
                            val = sinf(__builtin_fmaf(i == 0 ? px : i == 1 ? py : pz, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
                        else if (e < e_dir) val = e == e_pe3 ? dcx : e == e_pe3 + 1 ? dcy : dcz;
                        else if (e == e_dir) val = delta;
                        else if (e < e_pe1 + 2 * F) { const int j = e - e_pe1;
                            val = sinf(__builtin_fmaf(delta, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
                        else val = 0.0f;
                        split(val * ACT_SCALE, hi[j2], lo[j2]);
                    }
                    ph[jj] = pack2(hi[0], hi[1]); plo[jj] = pack2(lo[0], lo[1]);
                }
                const u32x4 vh = {ph[0], ph[1], ph[2], ph[3]}, vl = {plo[0], plo[1], plo[2], plo[3]};
                A[a_slot(pl, 0, row)] = vh;
                A[a_slot(pl, 1, row)] = vl;
            }
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
                            for (int i = 0; i < 4; ++i) {  // each lookup in ATen's accumulation order nw,ne,sw,se with contracted FMAs
                                const float zl = __builtin_fmaf(d[i], t.se, __builtin_fmaf(c[i], t.sw, __builtin_fmaf(bb[i], t.ne, a[i] * t.nw)));
                                const float zg = __builtin_fmaf(gd[i], g.se, __builtin_fmaf(gc[i], g.sw, __builtin_fmaf(gb[i], g.ne, ga[i] * g.nw)));
                                split(zg + zl, hi[i], lo[i]);                                       // novel_pixelnerf.py:196
                            }
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
#pragma unroll
        for (int tm = 0; tm < RB; ++tm)
#pragma unroll
            for (int tn = 0; tn < CT; ++tn) xsum[tm][tn] += x[tm][tn];                              // :146-149
    }
    {   // combine(): mean over views (combine_layer >= n_blocks: NV = 1 and this divides by 1, i.e. is exact)
        const float nv = (float)s.NV;
#pragma unroll
        for (int tm = 0; tm < RB; ++tm)
#pragma unroll
            for (int tn = 0; tn < CT; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) xsum[tm][tn][i] = xsum[tm][tn][i] / nv;
    }
    for (int b = L.nvb; b < L.nb; ++b) {
        store_act(xsum, A, L.beta, rb0, ct0, NT, lane);
        __syncthreads();
        acc_bias(net, bias + L.bias_fc0(b), false, ct0, NT, lane);
        gemm(net, A8, Wh + (L.off_fc0 + b * L.w_h) / 8, H / 16, 0, H / 16, rb0, ct0, NT, lane);
        __syncthreads();
        store_act(net, A, L.beta, rb0, ct0, NT, lane);
        __syncthreads();
        acc_bias(xsum, bias + L.bias_fc1(b), true, ct0, NT, lane);
        gemm(xsum, A8, Wh + (L.off_fc1 + b * L.w_h) / 8, H / 16, 0, H / 16, rb0, ct0, NT, lane);
        __syncthreads();
    }
    // ---- lin_out(act(x)) (:158) in fp32 on the VALU: every lane's partial dot products over its own features -> LDS (the A image is
    // free: the barrier above), [slot = 2 (tile group) + h][point][4]; a tile group past NT contributes zeros ----------------------
    {
        float *red = (float *)lds;
        const float *wout = Wp + L.off_wout;
        const int h = lane >> 5, grp = RB == 2 ? wave : (wave >> 1);
#pragma unroll
        for (int tm = 0; tm < RB; ++tm) {
            float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int tn = 0; tn < CT; ++tn) {
                if (ct0 + tn >= NT) continue;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float a[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[j] = act(xsum[tm][tn][4 * g + j], L.beta);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const f32x4 wq = *(const f32x4 *)(wout + c * H + (ct0 + tn) * 32 + 8 * g + 4 * h);
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[c] = __builtin_fmaf(a[j], wq[j], o[c]);
                    }
                }
            }
            const f32x4 ov = {o[0], o[1], o[2], o[3]};
            ((f32x4 *)red)[(grp * 2 + h) * TILE_P + (rb0 + tm) * 32 + (lane & 31)] = ov;
        }
        __syncthreads();
        if (tid < TILE_P * 4) {
            const int r = tid >> 2, c = tid & 3;
            const int ngrp = RB == 2 ? NWAVES : NWAVES / 2;   // <1,1>: the point block of r was written by the waves of its parity only
            float sum = 0.0f;
            for (int g = 0; g < 2 * ngrp; ++g) sum += red[(g * TILE_P + r) * 4 + c];
            const int64_t pp = tile * TILE_P + r;
            if (pp < P) {
                const float val = (sum + bias[L.bias_lin_out() + c]) * (1.0f / ACT_SCALE);          // novel_pixelnerf.py:236-240
                rgbsigma[((int64_t)sb * P + pp) * 4 + c] = c < 3 ? 1.0f / (1.0f + expf(-val)) : (val < 0.0f ? 0.0f : val);
            }
        }
    }
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
