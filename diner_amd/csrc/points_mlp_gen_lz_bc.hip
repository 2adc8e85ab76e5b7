// The lin_z-map form of the shape-general fp32 point/MLP kernel for the bicubic latent lookup: points_mlp_gen.hip compiled as
// points_mlp_gen_lz_bc_kernel (see points_mlp_gen_lz.hip and points_mlp_gen_bc.hip), in a translation unit of its own.
#define DINER_GEN_IX
#define DINER_GEN_BC
#define DINER_GEN_LZ
#define BC_ROW_UNROLL 2
#include "points_mlp_gen.hip"
