// The any-lookup-mode twin of the exact-fp32 point/MLP kernel: points_mlp_kernel<int, int> (index_interp / index_padding other than
// bilinear / border; common.hpp latent_footprint).  Compiled in a translation unit of its own, so that points_mlp.hip's code object
// holds exactly the default kernel it always held (instantiated next to it, the twin changed the default kernel's spills).
#define DINER_FP32_KERNEL_ONLY
#include "points_mlp.hip"

namespace diner {

int launch_points_mlp_ix_kernel(const DinerScene &s, int interp, int padding, const float *mlp_packed, const float *rays, const float *z,
                                int64_t NR, int K, int64_t tiles, float *rgbsigma, hipStream_t st)
{
    hipLaunchKernelGGL((points_mlp_kernel<int, int>), dim3((unsigned)tiles, (unsigned)s.SB), dim3(NWAVES * 64), 0, st, s, mlp_packed, rays,
                       z, NR, K, rgbsigma, interp, padding);
    return check_launch("points_mlp_kernel<ix>");
}

}  // namespace diner
