// The "novel_pe" form of the shape-general f16x3 point/MLP kernel: the point model of the fork's NOVEL_PE configuration, reference
// src/models/novel_pe/pe_novel_pixelnerf.py:200-292, in the split-fp16 arithmetic of points_mlp_gen_f16_kernel.hpp.  What the model
// computes and how the deformation layer is hoisted onto the latent's texels is described in points_mlp_gen_nvpe.hip, the fp32 twin:
//   A[r, c] = zg + (zd + head_c) for c < C;  A[r, C .. C + 5] = src_pe | tgt_pe;  A[r, C + 6 .. C + 7] = 0
// with zd the lookup of the map D = W_d[:, :C] . latent, zg the lookup of gen_latent and head_c = b_d[c] + sum_j W_d[c, C + j] pe6[j].
// Everything is carried * 2^-4: both tap records carry their weights scaled, the pe values are stored scaled and the head's bias is
// scaled where it enters; the sum is formed in fp32 and split hi / lo once.  The GEMM's K is d_latent = C + 8, the texel stride of D
// and gen_latent C / 4 float4.
//
// The packed weight image (diner_pack_mlp_gen_f16), the tap records and the input stage are points_mlp_gen_f16_kernel.hpp's and
// common.hpp's building blocks.  The ResNet blocks and the finish are written out here, not taken from that header's resnet_block() /
// finish(): through either one alone <2,1> spills 104 to 105 VGPRs instead of 80.  LDS: the 128-KiB A image + two Taps per point + 8 floats per point.  No atomics.
#include "points_mlp_gen_f16_kernel.hpp"
#include "points_mlp_gen_nvpe.hpp"

namespace diner {
namespace genf16 {

constexpr int NVPE_LDS_SLOTS = A_H8 + 2 * TILE_P * (int)(sizeof(Tap) / sizeof(u32x4)) + 2 * TILE_P;

template <int RB, int CT>
__global__ __launch_bounds__(NWAVES * 64) void points_mlp_gen_f16_nvpe_kernel(DinerScene s, Layout L, const float *__restrict__ Wp, NovelPeIn n,
                                                                            float *__restrict__ rgbsigma)
{
    __shared__ u32x4 lds[NVPE_LDS_SLOTS];   // A image + the encoder's Tap + the general Tap + two float4 of pe per point
    u32x4 *A = lds;
    const h8 *A8 = (const h8 *)lds;
    Tap *taps = (Tap *)(lds + A_H8);
    Tap *gtaps = taps + TILE_P;
    f32x4 *pe4 = (f32x4 *)(gtaps + TILE_P);   // [point][2], * 2^-4: src_pe xyz, tgt_pe x | tgt_pe yz, 0, 0

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT, H = L.H;
    const int sb = blockIdx.y;
    const int64_t P = n.P;
    const int64_t tile = xcd_tile(gridDim.x, blockIdx.x);
    const h8 *Wh = (const h8 *)Wp;
    const float *bias = Wp + L.off_bias;

    const int row = tid & 63;
    int64_t p = tile * TILE_P + row;
    if (p > P - 1) p = P - 1;  // tail tile: duplicate the last point, masked at the store
    const float *xp = n.xyz_in + ((int64_t)sb * P + p) * 3, *dp = n.viewdirs + ((int64_t)sb * P + p) * 3;
    const float wx = xp[0], wy = xp[1], wz = xp[2];        // pe_novel_pixelnerf.py:216-218
    const float dwx = dp[0], dwy = dp[1], dwz = dp[2];     // :232-234

    f32x16 x[RB][CT], net[RB][CT], xsum[RB][CT];
    acc_zero(xsum);

    const float sxl = pad_scale(s.w, s.feature_padding), syl = pad_scale(s.h, s.feature_padding);
    const int F = L.F;
    const int Cl = L.dlat - 8, c4 = Cl / 4;   // the latents' channels; float4 per texel of D and gen_latent: C / 4, NOT the GEMM's K / 4

    if (L.nvb > 0 && wave == 0)
        // ---- the general footprint, once per point (:220-222, :243-246, index() :117-128).  The first barrier of the view loop
        // publishes it.
        gtaps[row] = tap_of(camera_footprint(view_of(n.gposes, n.gfocal, n.gc, sb), n.giw, n.gih, n.xyz_gen + ((int64_t)sb * P + p) * 3,
                                             n.gh, n.gw, s.feature_padding, n.ix_interp, n.ix_padding), n.gw, c4);
    float tpx = 0.0f, tpy = 0.0f, tpz = 0.0f;   // wave 1: this point's tgt_pe
    if (L.nvb > 0 && wave == 1) {
        // ---- tgt_pe, once per point (:224-226, :248-251, :262): the same in every view
        const float4 t = pe_lookup_at((const float4 *)n.tpe + (int64_t)sb * n.tph * n.tpw, n.tph, n.tpw, view_of(n.tposes, n.tfocal, n.tc, sb),
                                      n.tiw, n.tih, n.xyz_tgt + ((int64_t)sb * P + p) * 3, s.feature_padding, n.ix_interp, n.ix_padding);
        tpx = t.x * ACT_SCALE; tpy = t.y * ACT_SCALE; tpz = t.z * ACT_SCALE;
    }
    const f32x4 *glat = (const f32x4 *)n.glat;
    const f32x4 *head = (const f32x4 *)n.head;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> planes 0 .. 2 nkb_in of A (a wave writes whole planes); footprint -> taps ----------
        {
            float px, py, pz, u, w, dcx, dcy, dcz, delta;
            view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);
            for (int pl = wave; pl < 2 * L.nkb_in; pl += NWAVES)
                store_input_plane(A, pl, row, px, py, pz, dcx, dcy, dcz, delta, F, s.freq_factor);
            if (wave == 0)   // footprint of the lookup mode in the encoder's latent map = in D (image_encoder.py:97-127; common.hpp)
                taps[row] = tap_of(latent_footprint<true>(u, w, sxl, syl, s.w, s.h, n.ix_interp, n.ix_padding), s.w, c4);
            if (L.nvb > 0 && wave == 1) {   // src_pe at the encoder lookup's uv, in this view's own map (:134-165, :260)
                const float4 sp = pe_lookup((const float4 *)n.spe + ((int64_t)sb * s.NV + v) * n.sph * n.spw, n.sph, n.spw, u, w,
                                            s.feature_padding, n.ix_interp, n.ix_padding);
                pe4[row * 2] = f32x4{sp.x * ACT_SCALE, sp.y * ACT_SCALE, sp.z * ACT_SCALE, tpx};
                pe4[row * 2 + 1] = f32x4{tpy, tpz, 0.0f, 0.0f};
            }
        }
        __syncthreads();
        acc_bias(x, bias + L.bias_lin_in(), false, ct0, NT, lane);
        gemm(x, A8, Wh + L.off_in / 8, L.nkb_in, 0, L.nkb_in, rb0, ct0, NT, lane);                  // resnetfc.py:139
        __syncthreads();

        const f32x4 *dm = (const f32x4 *)n.dmap + ((int64_t)sb * s.NV + v) * s.h * s.w * c4;
        for (int b = 0; b < L.nvb; ++b) {
            acc_bias(x, bias + L.bias_lin_z(b), true, ct0, NT, lane);                               // :152-153 x = x + lin_z(z)
            for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
                // ---- z[:, k0 : k0 + kc] / 16 of the 64 points -> A: a wave gathers 8 points, a lane 8 columns of one: a plane of the
                // latents' C columns, or the pe plane behind them ----
                const int kc = L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX;
                const int npl = (kc + 15) / 16 * 2;   // planes the GEMM reads (the last one zero when kc % 16 == 8)
                const int r = wave * (TILE_P / NWAVES) + (lane & 7);
                const Tap t = taps[r], g = gtaps[r];
                const f32x4 p0 = pe4[r * 2], p1 = pe4[r * 2 + 1];
                for (int pl = lane >> 3; pl < npl; pl += 8) {
                    u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
                    if (pl * 8 < kc) {
                        unsigned ph[4], plo[4];
                        const bool tail = k0 + pl * 8 >= Cl;   // columns C .. C + 7: the pe values (:275)
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            _Float16 hi[4], lo[4];
                            if (tail) {
                                const f32x4 pv = half ? p1 : p0;
#pragma unroll
                                for (int i = 0; i < 4; ++i) split(pv[i], hi[i], lo[i]);
                            } else {
                                const int qq = k0 / 4 + pl * 2 + half;
                                const f32x4 a = dm[t.o00 + qq], bb = dm[t.o01 + qq], c = dm[t.o10 + qq], d = dm[t.o11 + qq];
                                const f32x4 ga = glat[g.o00 + qq], gb = glat[g.o01 + qq], gc = glat[g.o10 + qq], gd = glat[g.o11 + qq];
#pragma unroll
                                for (int i = 0; i < 4; ++i) {  // each lookup in ATen's accumulation order nw,ne,sw,se with contracted FMAs
                                    const f32x4 h0 = head[(4 * qq + i) * 2], h1 = head[(4 * qq + i) * 2 + 1];
                                    const float zd = tap_sum(a[i], bb[i], c[i], d[i], t), zg = tap_sum(ga[i], gb[i], gc[i], gd[i], g);
                                    float hd = h1[2] * ACT_SCALE;                                   // b_d[c], then the six pe terms
                                    hd = __builtin_fmaf(h0[0], p0[0], hd); hd = __builtin_fmaf(h0[1], p0[1], hd);
                                    hd = __builtin_fmaf(h0[2], p0[2], hd); hd = __builtin_fmaf(h0[3], p0[3], hd);
                                    hd = __builtin_fmaf(h1[0], p1[0], hd); hd = __builtin_fmaf(h1[1], p1[1], hd);
                                    split(zg + (zd + hd), hi[i], lo[i]);                            // pe_novel_pixelnerf.py:266, :268
                                }
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
        acc_add(xsum, x);                                                                           // :146-149
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
                const float val = (sum + bias[L.bias_lin_out() + c]) * (1.0f / ACT_SCALE);          // pe_novel_pixelnerf.py:286-290
                rgbsigma[((int64_t)sb * P + pp) * 4 + c] = c < 3 ? 1.0f / (1.0f + expf(-val)) : (val < 0.0f ? 0.0f : val);
            }
        }
    }
}

// a call api.hip has validated (diner_render_points_novel_pe): P > 0, SB > 0, the tile count fits a grid, mlp_packed 16-byte aligned,
// scene C = d_latent - 8
int launch_points_mlp_novel_pe(const DinerScene &s, const DinerLatentIndex &ix, const DinerNovelGen &g, const DinerNovelPe &pe,
                               const DinerMlpShape &m, const float *mlp_packed, const float *xyz_in, const float *xyz_gen,
                               const float *xyz_tgt, const float *viewdirs, int64_t P, float *rgbsigma, hipStream_t st)
{
    const Layout L = layout_of(m);
    const NovelPeIn n{xyz_in, xyz_gen, xyz_tgt, viewdirs, P, g.latent, g.h, g.w, g.poses, g.focal, g.c, g.image_w, g.image_h,
                      pe.map, pe.head, pe.src_pe, pe.src_h, pe.src_w, pe.tgt_pe, pe.tgt_h, pe.tgt_w, pe.poses, pe.focal, pe.c,
                      pe.image_w, pe.image_h, ix.interp, ix.padding};
    const dim3 grid((unsigned)((P + TILE_P - 1) / TILE_P), (unsigned)s.SB), block(NWAVES * 64);
    void (*const kernel)(DinerScene, Layout, const float *, NovelPeIn, float *) =
        L.H <= 128   ? points_mlp_gen_f16_nvpe_kernel<1, 1>
        : L.H <= 256 ? points_mlp_gen_f16_nvpe_kernel<2, 1>
                     : points_mlp_gen_f16_nvpe_kernel<2, 2>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, s, L, mlp_packed, n, rgbsigma);
    return check_launch("points_mlp_gen_f16_nvpe_kernel");
}

}  // namespace genf16
}  // namespace diner
