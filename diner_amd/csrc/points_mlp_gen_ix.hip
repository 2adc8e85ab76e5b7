// The shape-general point/MLP kernel for every latent lookup mode other than bilinear / border (index_interp nearest, index_padding
// zeros / reflection): points_mlp_gen.hip compiled again as points_mlp_gen_ix_kernel, in a translation unit of its own so that
// points_mlp_gen.hip's code object holds exactly the three default kernels it always held.
#define DINER_GEN_IX
#include "points_mlp_gen.hip"
