// The lin_z-map form of the shape-general f16x3 point/MLP kernel for the bicubic latent lookup: points_mlp_gen_f16.hip compiled as
// points_mlp_gen_f16_lz_bc_kernel (see points_mlp_gen_f16_lz.hip and points_mlp_gen_f16_bc.hip), in a translation unit of its own.
#define DINER_GENF16_IX
#define DINER_GENF16_BC
#define DINER_GENF16_LZ
#define BC_ROW_UNROLL 2
#include "points_mlp_gen_f16.hip"
