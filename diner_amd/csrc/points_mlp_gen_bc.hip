// The shape-general point/MLP kernel for the bicubic latent lookup (index_interp "bicubic", any index_padding):
// points_mlp_gen_kernel<Bc, RB, CT>, instantiated in a translation unit of its own so that the code objects of points_mlp_gen.hip and
// points_mlp_gen_ix.hip hold exactly the kernels they always held.
#include "points_mlp_gen_kernel.hpp"

template int diner::gen::launch_mode<diner::gen::Bc>(const diner::gen::Launch &);
