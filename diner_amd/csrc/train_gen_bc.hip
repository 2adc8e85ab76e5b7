// The shape-general training path's point inputs for the bicubic latent lookup (index_interp "bicubic", any index_padding):
// train_gen.hip compiled a second time as point_inputs_gen_bc_kernel / point_inputs_bwd_gen_bc_kernel + bicubic_scatter_kernel, in a
// translation unit of its own so that train_gen.hip's code object holds exactly the kernels it always held.
#define DINER_TRAIN_GEN_BC
#include "train_gen.hip"
