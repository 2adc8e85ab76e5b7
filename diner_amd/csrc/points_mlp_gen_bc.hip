// The shape-general point/MLP kernel for the bicubic latent lookup (index_interp "bicubic", any index_padding): points_mlp_gen.hip
// compiled a third time as points_mlp_gen_bc_kernel, in a translation unit of its own so that the code objects of points_mlp_gen.hip
// and points_mlp_gen_ix.hip hold exactly the kernels they always held.  DINER_GEN_IX leaves the packers and check_shape to
// points_mlp_gen.hip; BC_ROW_UNROLL: rows of the 4 x 4 footprint whose loads are in flight together in the gather.
#define DINER_GEN_IX
#define DINER_GEN_BC
#define BC_ROW_UNROLL 2
#include "points_mlp_gen.hip"
