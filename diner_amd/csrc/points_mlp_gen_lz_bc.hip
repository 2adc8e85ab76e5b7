// The lin_z-map form of the shape-general fp32 point/MLP kernel for the bicubic latent lookup: points_mlp_gen_kernel<LzBc, RB, CT> (see
// points_mlp_gen_lz.hip and points_mlp_gen_bc.hip), instantiated in a translation unit of its own.
#include "points_mlp_gen_kernel.hpp"

template int diner::gen::launch_mode<diner::gen::LzBc>(const diner::gen::Launch &);
