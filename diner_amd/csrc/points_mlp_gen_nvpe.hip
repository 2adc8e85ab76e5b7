// The "novel_pe" form of the shape-general fp32 point/MLP kernel: the point model of the fork's NOVEL_PE configuration, reference
// src/models/novel_pe/pe_novel_pixelnerf.py:200-292.  It is the NOVEL model of points_mlp_gen_nv.hip (given points xyz_in / xyz_gen,
// per-point viewdirs, gen_latent looked up at the general camera) with C = encoder.latent_size, d_latent = C + 6, and:
//   * a third point set xyz_tgt [SB,P,3] (the undeformed samples), projected by one target camera per scene (:224-226, :248-251);
//   * two 3-channel lookups with the encoder's lookup mode and feature_padding (each scaled by its map's own size):
//     src_pe = lookup(pos_encodings[sb, v], uv) per view (:260), tgt_pe = lookup(tgt_pos_encoding[sb], tgt_uv) once per point (:262);
//   * conditioned = deformation_layer(cat(latent(uv), src_pe, tgt_pe)) (:265-266), final_latent = gen_latent(gen_uv) + conditioned (:268);
//   * the MLP's latent input is cat(final_latent, src_pe, tgt_pe) (:275).
// deformation_layer is linear and latent(uv) a weighted sum of texels, so its latent part is hoisted onto the texels: the gather reads
// the map D = W_d[:, :C] . latent (novel_pe_map.hip; no bias in it, so zeros padding's missing taps stay exact) where the NOVEL kernel
// reads the latent, and adds head_c = b_d[c] + sum_j W_d[c, C + j] pe6[j] per row from the [C][8] head table:
//   A[r, c] = zg + (zd + head_c) for c < C;  A[r, C .. C + 5] = pe6;  A[r, C + 6 .. C + 7] = 0
// The GEMM's K is d_latent = C + 8 (lin_z padded with two zero columns by the caller); the texel stride of D and gen_latent is C / 4
// float4.  With W_d = [I | 0], b_d = 0 and zero pe columns in lin_z the output is the NOVEL kernel's bit for bit.
//
// The packed weight image, the tap records, the input stage and the per-view ResNet block are points_mlp_gen_kernel.hpp's and
// common.hpp's building blocks.  What follows the view loop is written out here, not taken from that header's finish(): through
// finish() <2,1> spills one VGPR more (27 -> 28).  LDS: the 128-KiB A image + two Taps per row + 8 floats per row (src_pe | tgt_pe | 0 0).  No atomics.
#include "points_mlp_gen_kernel.hpp"
#include "points_mlp_gen_nvpe.hpp"

namespace diner {
namespace gen {

constexpr int NVPE_LDS_F4 = A_F4 + 2 * TILE_P * (int)(sizeof(Tap) / sizeof(f32x4)) + 2 * TILE_P;

template <int RB, int CT>
__global__ __launch_bounds__(NWAVES * 64) void points_mlp_gen_nvpe_kernel(DinerScene s, Layout L, const float *__restrict__ Wp, NovelPeIn n,
                                                                          float *__restrict__ rgbsigma)
{
    __shared__ f32x4 lds[NVPE_LDS_F4];   // A image + the encoder's Tap + the general Tap + two float4 of pe per row
    f32x4 *A4 = lds;
    float *A = (float *)lds;
    Tap *taps = (Tap *)(lds + A_F4);
    Tap *gtaps = taps + TILE_P;
    f32x4 *pe4 = (f32x4 *)(gtaps + TILE_P);   // [row][2]: src_pe xyz, tgt_pe x | tgt_pe yz, 0, 0

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT, H = L.H;
    const int sb = blockIdx.y;
    const int64_t P = n.P;
    const int64_t tile = xcd_tile(gridDim.x, blockIdx.x);
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
    const int F = L.F, din_pad = 8 * L.njb_in;
    const int c4 = (L.dlat - 8) / 4;   // float4 per texel of D and gen_latent: C / 4, NOT the GEMM's K / 4

    if (L.nvb > 0 && wave == 0)
        // ---- the general footprint, once per point (:220-222, :243-246, index() :117-128).  The first barrier of the view loop
        // publishes it.
        gtaps[row] = tap_of(camera_footprint(view_of(n.gposes, n.gfocal, n.gc, sb), n.giw, n.gih, n.xyz_gen + ((int64_t)sb * P + p) * 3,
                                             n.gh, n.gw, s.feature_padding, n.ix_interp, n.ix_padding), n.gw, c4);
    float tpx = 0.0f, tpy = 0.0f, tpz = 0.0f;   // wave 1: this row's tgt_pe
    if (L.nvb > 0 && wave == 1) {
        // ---- tgt_pe, once per point (:224-226, :248-251, :262): the same in every view
        const float4 t = pe_lookup_at((const float4 *)n.tpe + (int64_t)sb * n.tph * n.tpw, n.tph, n.tpw, view_of(n.tposes, n.tfocal, n.tc, sb),
                                      n.tiw, n.tih, n.xyz_tgt + ((int64_t)sb * P + p) * 3, s.feature_padding, n.ix_interp, n.ix_padding);
        tpx = t.x; tpy = t.y; tpz = t.z;
    }
    const f32x4 *glat = (const f32x4 *)n.glat;
    const f32x4 *head = (const f32x4 *)n.head;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> A[:, 0:din_pad]; the encoder's footprint -> taps; src_pe | tgt_pe -> pe4 ----------
        {
            float px, py, pz, u, w, dcx, dcy, dcz, delta;
            view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);
            for (int e = wave; e < din_pad; e += NWAVES)
                A[a_off(row, e)] = input_element(e, px, py, pz, dcx, dcy, dcz, delta, F, s.freq_factor);
            if (wave == 0)   // footprint of the lookup mode in the encoder's latent map = in D (image_encoder.py:97-127; common.hpp)
                taps[row] = tap_of(latent_footprint<true>(u, w, sxl, syl, s.w, s.h, n.ix_interp, n.ix_padding), s.w, c4);
            if (L.nvb > 0 && wave == 1) {   // src_pe at the encoder lookup's uv, in this view's own map (:134-165, :260)
                const float4 sp = pe_lookup((const float4 *)n.spe + ((int64_t)sb * s.NV + v) * n.sph * n.spw, n.sph, n.spw, u, w,
                                            s.feature_padding, n.ix_interp, n.ix_padding);
                pe4[row * 2] = f32x4{sp.x, sp.y, sp.z, tpx};
                pe4[row * 2 + 1] = f32x4{tpy, tpz, 0.0f, 0.0f};
            }
        }
        __syncthreads();
        acc_bias(x, bias + L.bias_lin_in(), false, ct0, NT, lane);
        gemm(x, A4, (const f32x4 *)(Wp + L.off_in), L.njb_in, 0, L.njb_in, rb0, ct0, NT, lane);   // resnetfc.py:139
        __syncthreads();

        const f32x4 *dm = (const f32x4 *)n.dmap + ((int64_t)sb * s.NV + v) * s.h * s.w * c4;
        for (int b = 0; b < L.nvb; ++b) {
            acc_bias(x, bias + L.bias_lin_z(b), true, ct0, NT, lane);                               // :152-153 x = x + lin_z(z)
            for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
                // ---- z[:, k0 : k0 + kc] of the 64 points -> A: a wave gathers 8 rows; a lane holds the head table's rows of its 4
                // channels across those 8 rows ----
                const int kc4 = (L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX) / 4;
                for (int q = lane; q < kc4; q += 64) {
                    const int qq = k0 / 4 + q;
                    if (qq < c4) {
                        f32x4 h0[4], h1[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) { h0[i] = head[(4 * qq + i) * 2]; h1[i] = head[(4 * qq + i) * 2 + 1]; }
                        for (int rr = 0; rr < TILE_P / NWAVES; ++rr) {
                            const int r = wave * (TILE_P / NWAVES) + rr;
                            const Tap t = taps[r], g = gtaps[r];
                            const f32x4 p0 = pe4[r * 2], p1 = pe4[r * 2 + 1];
                            const f32x4 a = dm[t.o00 + qq], bb = dm[t.o01 + qq], c = dm[t.o10 + qq], d = dm[t.o11 + qq];
                            const f32x4 ga = glat[g.o00 + qq], gb = glat[g.o01 + qq], gc = glat[g.o10 + qq], gd = glat[g.o11 + qq];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {  // each lookup in ATen's accumulation order nw,ne,sw,se with contracted FMAs
                                const float zd = tap_sum(a[i], bb[i], c[i], d[i], t), zg = tap_sum(ga[i], gb[i], gc[i], gd[i], g);
                                float hd = h1[i][2];                                                // b_d[c], then the six pe terms
                                hd = __builtin_fmaf(h0[i][0], p0[0], hd); hd = __builtin_fmaf(h0[i][1], p0[1], hd);
                                hd = __builtin_fmaf(h0[i][2], p0[2], hd); hd = __builtin_fmaf(h0[i][3], p0[3], hd);
                                hd = __builtin_fmaf(h1[i][0], p1[0], hd); hd = __builtin_fmaf(h1[i][1], p1[1], hd);
                                A[a_off(r, 4 * q + i)] = zg + (zd + hd);                            // pe_novel_pixelnerf.py:266, :268
                            }
                        }
                    } else {   // the pe tail: columns C .. C + 7 (:275)
                        for (int rr = 0; rr < TILE_P / NWAVES; ++rr) {
                            const int r = wave * (TILE_P / NWAVES) + rr;
                            const f32x4 pv = pe4[r * 2 + (qq - c4)];
#pragma unroll
                            for (int i = 0; i < 4; ++i) A[a_off(r, 4 * q + i)] = pv[i];
                        }
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
        gemm(net, A4, (const f32x4 *)(Wp + L.off_fc0 + b * L.w_h), H / 8, 0, H / 8, rb0, ct0, NT, lane);
        __syncthreads();
        store_act(net, A, L.beta, rb0, ct0, NT, lane);
        __syncthreads();
        acc_bias(xsum, bias + L.bias_fc1(b), true, ct0, NT, lane);
        gemm(xsum, A4, (const f32x4 *)(Wp + L.off_fc1 + b * L.w_h), H / 8, 0, H / 8, rb0, ct0, NT, lane);
        __syncthreads();
    }
    store_act(xsum, A, L.beta, rb0, ct0, NT, lane);                                                 // :158 lin_out(act(x))
    __syncthreads();
    if (wave < 2) {  // lin_out: one 32-column tile (4 real outputs), wave w = rows 32w..32w+31
        f32x16 o;
        const float bo = bias[L.bias_lin_out() + (lane & 31)];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = bo;
        const f32x4 *ap = A4 + (lane >> 5) * TILE_P + wave * 32 + (lane & 31);
        const f32x4 *bp = (const f32x4 *)(Wp + L.off_out) + lane;
#pragma unroll 4
        for (int jb = 0; jb < H / 8; ++jb) {
            const f32x4 a = ap[jb * 2 * TILE_P], bq = bp[jb * 64];
#pragma unroll
            for (int ji = 0; ji < 4; ++ji) o = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ji], bq[ji], o, 0, 0, 0);
        }
        const int c = lane & 31, h = lane >> 5;
        if (c < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = wave * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                const int64_t pp = tile * TILE_P + r;
                if (pp < P) {
                    const float val = o[i];                                                         // pe_novel_pixelnerf.py:286-290
                    rgbsigma[((int64_t)sb * P + pp) * 4 + c] = c < 3 ? 1.0f / (1.0f + expf(-val)) : (val < 0.0f ? 0.0f : val);
                }
            }
        }
    }
}

// a call api.hip has validated (diner_render_points_novel_pe): P > 0, SB > 0, the tile count fits a grid, scene C = d_latent - 8
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
        L.H <= 128 ? points_mlp_gen_nvpe_kernel<1, 1> : L.H <= 256 ? points_mlp_gen_nvpe_kernel<2, 1> : points_mlp_gen_nvpe_kernel<2, 2>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, s, L, mlp_packed, n, rgbsigma);
    return check_launch("points_mlp_gen_nvpe_kernel");
}

}  // namespace gen
}  // namespace diner
