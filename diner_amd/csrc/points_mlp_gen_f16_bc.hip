// The shape-general f16x3 point/MLP kernel for the bicubic latent lookup (index_interp "bicubic", any index_padding):
// points_mlp_gen_f16_kernel<Bc, RB, CT>, instantiated in a translation unit of its own so that the code objects of points_mlp_gen_f16.hip and
// points_mlp_gen_f16_ix.hip hold exactly the kernels they always held.
#include "points_mlp_gen_f16_kernel.hpp"

template int diner::genf16::launch_mode<diner::genf16::Bc>(const diner::genf16::Launch &);
