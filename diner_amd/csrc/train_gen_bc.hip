// The shape-general training path's point inputs for the bicubic latent lookup (index_interp "bicubic", any index_padding):
// point_inputs_gen_kernel<true> / point_inputs_bwd_gen_kernel<true> (train_gen_points.hpp) + bicubic_scatter_kernel, in a translation
// unit of its own so that train_gen.hip's code object holds exactly the kernels it always held.
#include "train_gen_points.hpp"

namespace diner {

namespace train_gen {

// d_lat_nhwc[v][texel (x[i], y[j])][ch] += dz[row][ch] * cx[i] * cy[j] over the 16 taps of each row's record (grid_sample's input
// gradient; float atomics on 256-byte contiguous rows, as train.hip's bilinear_scatter_kernel).  One wave walks SCATTER_RUN consecutive
// rows (consecutive samples of a ray in one view, whose footprints move by a fraction of a texel per sample): contributions are summed
// in registers while the 4 columns and 4 rows stay the same and flushed with one atomic per tap when they change.  A tap of weight 0
// (zeros padding outside the map) adds nothing and is never flushed.  Several taps of one footprint may be the same texel (border /
// reflection at the rim, maps smaller than the footprint): the atomics add them up.
__global__ __launch_bounds__(64) void bicubic_scatter_kernel(const float *__restrict__ dz, const float *__restrict__ taps, int64_t P, int C,
                                                             int h, int w, int NV, int sb, float *__restrict__ dlatent_nhwc)
{
    const int64_t R = P * NV, row0 = (int64_t)blockIdx.x * SCATTER_RUN;
    const int64_t row1 = row0 + SCATTER_RUN < R ? row0 + SCATTER_RUN : R;
    const int lane = threadIdx.x;
    for (int ch = lane; ch < C; ch += 64) {
        int cur[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // x[4], y[4] of the open run
        int64_t cur_v = -1;
        float acc[16];
        unsigned used = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.f;
        for (int64_t row = row0; row <= row1; ++row) {
            const bool last = row == row1;
            const int64_t v = last ? -1 : row / P;
            int o[8];
            bool same = !last && v == cur_v;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                o[i] = last ? -1 : __float_as_int(taps[row * 16 + i]);
                if (!last) { const int hi = (i < 4 ? w : h) - 1; o[i] = o[i] < 0 ? 0 : (o[i] > hi ? hi : o[i]); }   // never outside the map
                same = same && o[i] == cur[i];
            }
            if (!same) {  // wave-uniform
                if (cur_v >= 0 && used) {
                    float *lat = dlatent_nhwc + ((int64_t)sb * NV + cur_v) * h * w * C + ch;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (used >> (j * 4 + i) & 1u) atomicAdd(lat + ((int64_t)cur[4 + j] * w + cur[i]) * C, acc[j * 4 + i]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) cur[i] = o[i];
#pragma unroll
                for (int t = 0; t < 16; ++t) acc[t] = 0.f;
                used = 0;
                cur_v = v;
            }
            if (last) break;
            const float g = dz[row * C + ch];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gy = g * taps[row * 16 + 12 + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float wx = taps[row * 16 + 8 + i];
                    if (wx != 0.0f && taps[row * 16 + 12 + j] != 0.0f) { acc[j * 4 + i] += gy * wx; used |= 1u << (j * 4 + i); }
                }
            }
        }
    }
}

}  // namespace train_gen

int launch_train_point_inputs_gen_bc(const DinerScene &s, int padding, const float *latent_nhwc, const float *rays, const float *z, int64_t NR,
                                     int K, int sb, float *in, int64_t ld_in, float *zlat, float *taps, hipStream_t st)
{
    const int64_t R = NR * (int64_t)K * s.NV;
    if (R == 0) return DINER_OK;
    hipLaunchKernelGGL(train_gen::point_inputs_gen_kernel<true>, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, 0, padding,
                       in, ld_in, zlat, taps);
    return check_launch("train_gen::point_inputs_gen_kernel<true>");
}

int launch_train_point_inputs_bwd_gen_bc(const DinerScene &s, int padding, const float *latent_nhwc, const float *rays, const float *z,
                                         int64_t NR, int K, int sb, const float *d_in, int64_t ld_in, const float *d_zlat, const float *d_far,
                                         float *workspace, float *d_rays, float *d_poses, float *d_focal, float *d_c, float *d_image_shape,
                                         float *d_depths, hipStream_t st)
{
    using namespace train_gen;
    const int64_t P = NR * (int64_t)K, R = P * s.NV;
    if (R == 0) return DINER_OK;
    float *rowg = workspace, *partial = workspace + R * CAMG_COLS;   // diner_train_camera_workspace_floats' layout
    hipLaunchKernelGGL(point_inputs_bwd_gen_kernel<true>, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, 0, padding, d_in,
                       ld_in, d_zlat, rowg, d_depths);
    const int rc = check_launch("train_gen::point_inputs_bwd_gen_kernel<true>");
    if (rc) return rc;
    return launch_train_camg_reduce(rowg, partial, NR, K, s.NV, sb, d_far, d_rays, d_poses, d_focal, d_c, d_image_shape, st);
}

int launch_train_bicubic_scatter(const float *dz, const float *taps, int64_t P, int C, int h, int w, int NV, int sb, float *dlatent_nhwc,
                                 hipStream_t st)
{
    using namespace train_gen;
    if (P * NV == 0) return DINER_OK;
    hipLaunchKernelGGL(bicubic_scatter_kernel, dim3((unsigned)((P * NV + SCATTER_RUN - 1) / SCATTER_RUN)), dim3(64), 0, st, dz, taps, P, C, h, w, NV,
                       sb, dlatent_nhwc);
    return check_launch("train_gen::bicubic_scatter_kernel");
}

}  // namespace diner
