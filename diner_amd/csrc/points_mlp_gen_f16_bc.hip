// The shape-general f16x3 point/MLP kernel for the bicubic latent lookup (index_interp "bicubic", any index_padding):
// points_mlp_gen_f16.hip compiled a third time as points_mlp_gen_f16_bc_kernel, in a translation unit of its own so that the code
// objects of points_mlp_gen_f16.hip and points_mlp_gen_f16_ix.hip hold exactly the kernels they always held.  DINER_GENF16_IX leaves
// the packers to points_mlp_gen_f16.hip; BC_ROW_UNROLL: rows of the 4 x 4 footprint whose loads are in flight together in the gather.
#define DINER_GENF16_IX
#define DINER_GENF16_BC
#define BC_ROW_UNROLL 2
#include "points_mlp_gen_f16.hip"
