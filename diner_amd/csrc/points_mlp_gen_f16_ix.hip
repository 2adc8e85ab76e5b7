// The shape-general f16x3 point/MLP kernel for every latent lookup mode other than bilinear / border (index_interp nearest, index_padding
// zeros / reflection): points_mlp_gen_f16_kernel<Ix, RB, CT>, instantiated in a translation unit of its own so that points_mlp_gen_f16.hip's code
// object holds exactly the three default kernels it always held.
#include "points_mlp_gen_f16_kernel.hpp"

template int diner::genf16::launch_mode<diner::genf16::Ix>(const diner::genf16::Launch &);
