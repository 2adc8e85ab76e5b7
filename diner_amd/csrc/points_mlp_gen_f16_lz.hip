// The lin_z-map form of the shape-general f16x3 point/MLP kernel: points_mlp_gen_f16_kernel<Lz, RB, CT>, which reads the per-texel fp32 maps
// M_b = W_z[b] F of linz_maps_gen.hip instead of gathering the latent and multiplying by lin_z[b] per point, view and block.  One
// lookup-general instantiation (the footprint code of points_mlp_gen_f16_ix.hip: bilinear / nearest, border / zeros / reflection), in a
// translation unit of its own so that the other code objects hold exactly the kernels they always held.
#include "points_mlp_gen_f16_kernel.hpp"

template int diner::genf16::launch_mode<diner::genf16::Lz>(const diner::genf16::Launch &);
