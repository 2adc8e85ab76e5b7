// The lin_z maps of the shape-general point/MLP kernels' lin_z-map forms (points_mlp_gen_lz.hip, points_mlp_gen_f16_lz.hip):
//   M_b[sb, v, y, x, :] = W_z[b] . F[sb, v, y, x, :]      b < nlz = min(combine_layer, n_blocks)      (ResnetFC.forward, resnetfc.py:152-153)
// d_hidden floats per latent texel, NHWC fp32, [nlz][SB, NV, h, w, d_hidden], WITHOUT lin_z[b].bias: a map without the bias is exactly
// linear in the taps of a lookup, so one set of maps serves every index_interp / index_padding (SpatialEncoder.index,
// image_encoder.py:97-127), bicubic's negative weights and zeros padding's missing taps included, and needs no ring of extra texels.
//
// An exact fp32 GEMM (v_mfma_f32_32x32x2_f32) of the NHWC latent [texels, d_latent] with each lin_z[b] of the image diner_pack_mlp_gen
// writes: 64 texels per workgroup, the A operand in the 128-KiB LDS image of points_mlp_gen.hip, d_latent above 512 in 512-column pieces,
// the device gemm() and the <RB, CT> instantiations of points_mlp_gen_kernel.hpp.  One builder serves both precisions.
#include "points_mlp_gen_kernel.hpp"   // the layout and gemm() only

namespace diner {
namespace gen {

int check_shape(const DinerMlpShape &);   // points_mlp_gen.hip

template <int RB, int CT>
__global__ __launch_bounds__(NWAVES * 64) void linz_maps_gen_kernel(const float *__restrict__ latent, int64_t T, Layout L,
                                                                    const float *__restrict__ Wp, float *__restrict__ out)
{
    __shared__ f32x4 lds[A_F4];
    const f32x4 *A4 = lds;
    float *A = (float *)lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT, H = L.H, c4 = L.dlat / 4;
    const int64_t t0 = (int64_t)blockIdx.x * TILE_P;
    const f32x4 *lat = (const f32x4 *)latent;
    const bool one_piece = L.dlat <= KMAX;

    for (int b = 0; b < L.nlz; ++b) {
        f32x16 acc[RB][CT];
#pragma unroll
        for (int tm = 0; tm < RB; ++tm)
#pragma unroll
            for (int tn = 0; tn < CT; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[tm][tn][i] = 0.0f;
        for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
            const int kc4 = (L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX) / 4;
            if (!one_piece || b == 0) {   // F[t0 .. t0 + 64, k0 : k0 + 4 kc4] -> A (a wave copies 8 texels; the last tile repeats texel T - 1)
                for (int rr = 0; rr < TILE_P / NWAVES; ++rr) {
                    const int r = wave * (TILE_P / NWAVES) + rr;
                    const int64_t t = t0 + r < T ? t0 + r : T - 1;
                    for (int q = lane; q < kc4; q += 64) {
                        const f32x4 val = lat[t * c4 + k0 / 4 + q];
#pragma unroll
                        for (int i = 0; i < 4; ++i) A[a_off(r, 4 * q + i)] = val[i];
                    }
                }
                __syncthreads();
            }
            gemm(acc, A4, (const f32x4 *)(Wp + L.off_z + b * L.w_z), L.njb_lat, k0 / 8, kc4 / 2, rb0, ct0, NT, lane);
            if (!one_piece) __syncthreads();
        }
        // C/D layout of the 32x32 MFMA: register i of lane (c = lane & 31, half) is row 8 (i / 4) + 4 half + i % 4, column c of the tile
        float *ob = out + (int64_t)b * T * H;
        const int c = lane & 31, half = lane >> 5;
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) {
            if (ct0 + tn >= NT) continue;
#pragma unroll
            for (int tm = 0; tm < RB; ++tm)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t t = t0 + (rb0 + tm) * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
                    if (t < T) ob[t * H + (ct0 + tn) * 32 + c] = acc[tm][tn][i];
                }
        }
    }
}

int64_t linz_maps_floats(const DinerMlpShape &m, int64_t texels)
{
    const Layout L = layout_of(m);
    return (int64_t)L.nlz * texels * L.H;
}

// out[nlz][T][d_hidden] from latent [T][d_latent] (NHWC) and the packed image of diner_pack_mlp_gen
int launch_linz_maps(const DinerMlpShape &m, const float *latent, int64_t T, const float *mlp_packed, float *out, hipStream_t st)
{
    int rc;
    if ((rc = check_shape(m))) return rc;
    const Layout L = layout_of(m);
    if (L.nlz == 0 || T == 0) return DINER_OK;
    const int64_t tiles = (T + TILE_P - 1) / TILE_P;
    if (tiles > 0x7fffffffLL) { set_error("pack_linz_maps_gen: too many texels (%lld)", (long long)T); return DINER_E_INVALID; }
    const dim3 grid((unsigned)tiles), block(NWAVES * 64);
    if (m.d_hidden <= 128)
        hipLaunchKernelGGL((linz_maps_gen_kernel<1, 1>), grid, block, 0, st, latent, T, L, mlp_packed, out);
    else if (m.d_hidden <= 256)
        hipLaunchKernelGGL((linz_maps_gen_kernel<2, 1>), grid, block, 0, st, latent, T, L, mlp_packed, out);
    else
        hipLaunchKernelGGL((linz_maps_gen_kernel<2, 2>), grid, block, 0, st, latent, T, L, mlp_packed, out);
    return check_launch("linz_maps_gen_kernel");
}

}  // namespace gen
}  // namespace diner
