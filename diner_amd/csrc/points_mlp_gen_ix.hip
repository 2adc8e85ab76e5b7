// The shape-general point/MLP kernel for every latent lookup mode other than bilinear / border (index_interp nearest, index_padding
// zeros / reflection): points_mlp_gen_kernel<Ix, RB, CT>, instantiated in a translation unit of its own so that points_mlp_gen.hip's code
// object holds exactly the three default kernels it always held.
#include "points_mlp_gen_kernel.hpp"

template int diner::gen::launch_mode<diner::gen::Ix>(const diner::gen::Launch &);
