// The lin_z-map form of the shape-general f16x3 point/MLP kernel for the bicubic latent lookup: points_mlp_gen_f16_kernel<LzBc, RB, CT> (see
// points_mlp_gen_f16_lz.hip and points_mlp_gen_f16_bc.hip), instantiated in a translation unit of its own.
#include "points_mlp_gen_f16_kernel.hpp"

template int diner::genf16::launch_mode<diner::genf16::LzBc>(const diner::genf16::Launch &);
