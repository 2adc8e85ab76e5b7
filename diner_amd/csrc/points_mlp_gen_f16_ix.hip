// The shape-general f16x3 point/MLP kernel for every latent lookup mode other than bilinear / border (index_interp nearest,
// index_padding zeros / reflection): points_mlp_gen_f16.hip compiled again as points_mlp_gen_f16_ix_kernel, in a translation unit of
// its own so that points_mlp_gen_f16.hip's code object holds exactly the three default kernels.
#define DINER_GENF16_IX
#include "points_mlp_gen_f16.hip"
