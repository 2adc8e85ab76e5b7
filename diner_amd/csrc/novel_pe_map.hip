// The deformation map of the NOVEL_PE point kernels (points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip):
//   D[sb, v, y, x, :] = W_d[:, :C] . F[sb, v, y, x, :]       (deformation_layer's latent part, pe_novel_pixelnerf.py:265-266)
// C floats per latent texel, NHWC fp32, the layout and size of the packed latent, WITHOUT the layer's bias and pe part: a map without
// them is exactly linear in the taps of a lookup, so one map serves every 4-tap index_interp / index_padding, zeros padding's missing
// taps included.  This is linz_maps_gen.hip's argument with a C x C matrix read row-major as the caller holds it.
//
// An exact fp32 GEMM (v_mfma_f32_32x32x2_f32) of the NHWC latent [texels, C] with W [C, C]: 64 texels per workgroup, the A operand in
// the 128-KiB LDS image of points_mlp_gen_kernel.hpp (its a_off), C above 512 in 512-column pieces; a wave owns the 32-column output
// tiles wave, wave + 8, ... and both 32-row blocks of each.  With W = I the map is the latent bit for bit.  One builder serves both
// precisions.  No atomics.
#include "points_mlp_gen_kernel.hpp"   // the A image and its index map only

namespace diner {
namespace gen {

__global__ __launch_bounds__(NWAVES * 64) void novel_pe_map_kernel(const float *__restrict__ latent, int64_t T, int C,
                                                                   const float *__restrict__ W, float *__restrict__ out)
{
    __shared__ f32x4 lds[A_F4];
    const f32x4 *A4 = lds;
    float *A = (float *)lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c4 = C / 4, NTc = (C + 31) / 32;
    const int64_t t0 = (int64_t)blockIdx.x * TILE_P;
    const f32x4 *lat = (const f32x4 *)latent;
    const bool one_piece = C <= KMAX;
    const int col = lane & 31, half = lane >> 5;

    for (int g = 0; g * NWAVES < NTc; ++g) {          // every wave makes every trip: the barriers below are the workgroup's
        const int ct = g * NWAVES + wave;
        const int n = ct * 32 + col;                  // this lane's output column = row of W
        const bool live = n < C;
        const float *wr = W + (int64_t)(live ? n : C - 1) * C + half;
        f32x16 acc[2];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tm][i] = 0.0f;
        for (int k0 = 0; k0 < C; k0 += KMAX) {
            const int kc4 = (C - k0 < KMAX ? C - k0 : KMAX) / 4;
            if (!one_piece || g == 0) {   // F[t0 .. t0 + 64, k0 : k0 + 4 kc4] -> A (a wave copies 8 texels; the last tile repeats texel T - 1)
                if (!one_piece) __syncthreads();      // the previous piece's readers are done
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
            // lane (half, col) holds W[n][k0 + 8 jb + 2 ji + half], ji = 0..3, of k-block jb: the B operand of points_mlp_gen_kernel.hpp's gemm()
            const f32x4 *ap = A4 + half * TILE_P + col;
            const float *wk = wr + k0;
            for (int jb = 0; jb < kc4 / 2; ++jb) {
                float b[4];
#pragma unroll
                for (int ji = 0; ji < 4; ++ji) { const float w = wk[8 * jb + 2 * ji]; b[ji] = live ? w : 0.0f; }
                const f32x4 a0 = ap[jb * 2 * TILE_P], a1 = ap[jb * 2 * TILE_P + 32];
#pragma unroll
                for (int ji = 0; ji < 4; ++ji) {
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[ji], b[ji], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[ji], b[ji], acc[1], 0, 0, 0);
                }
            }
        }
        // C/D layout of the 32x32 MFMA: register i of lane (col, half) is row 8 (i / 4) + 4 half + i % 4, column col of the tile
        if (live) {
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t t = t0 + tm * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
                    if (t < T) out[t * C + n] = acc[tm][i];
                }
        }
    }
}

// out [T][C] from latent [T][C] (NHWC) and W [C][C] row-major; api.hip has validated C (a multiple of 8 in [8, 1016]) and the pointers
int launch_novel_pe_map(const float *latent, int64_t T, int C, const float *W, float *out, hipStream_t st)
{
    if (T == 0) return DINER_OK;
    const int64_t tiles = (T + TILE_P - 1) / TILE_P;
    if (tiles > 0x7fffffffLL) { set_error("pack_novel_pe_map: too many texels (%lld)", (long long)T); return DINER_E_INVALID; }
    hipLaunchKernelGGL(novel_pe_map_kernel, dim3((unsigned)tiles), dim3(NWAVES * 64), 0, st, latent, T, C, W, out);
    return check_launch("novel_pe_map_kernel");
}

}  // namespace gen
}  // namespace diner
