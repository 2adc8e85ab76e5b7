// The lin_z-map form of the shape-general fp32 point/MLP kernel: points_mlp_gen_kernel<Lz, RB, CT>, which reads the per-texel maps
// M_b = W_z[b] F of linz_maps_gen.hip instead of gathering the latent and multiplying by lin_z[b] per point, view and block.  One
// lookup-general instantiation (the footprint code of points_mlp_gen_ix.hip: bilinear / nearest, border / zeros / reflection), in a
// translation unit of its own so that the other code objects hold exactly the kernels they always held.
#include "points_mlp_gen_kernel.hpp"

template int diner::gen::launch_mode<diner::gen::Lz>(const diner::gen::Launch &);
