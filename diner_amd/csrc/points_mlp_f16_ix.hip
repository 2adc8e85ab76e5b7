// The any-lookup-mode twins of the default point/MLP kernel: points_mlp_f16_kernel<LINZ, false, VIT, int, int> (index_interp /
// index_padding other than bilinear / border; common.hpp latent_footprint).  They differ from the product instantiations only in the
// footprint glue (and, for LINZ with zeros padding, in the size of a lin_z map: the ringed maps of diner_pack_linz_maps_ix), and are
// compiled in a translation unit of their own, so points_mlp_f16.hip's code object holds exactly the default kernels it always held.
#define DINER_F16_KERNEL_ONLY
#include "points_mlp_f16.hip"

namespace diner {

const void *points_mlp_f16_gix_kernel(bool linz, bool vit)
{
    using namespace f16x3;
    return linz ? (vit ? (const void *)points_mlp_f16_kernel<true, false, true, int, int> : (const void *)points_mlp_f16_kernel<true, false, false, int, int>)
                : (vit ? (const void *)points_mlp_f16_kernel<false, false, true, int, int> : (const void *)points_mlp_f16_kernel<false, false, false, int, int>);
}

}  // namespace diner
