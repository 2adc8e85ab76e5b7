// The lin_z-map form of the shape-general fp32 point/MLP kernel: points_mlp_gen.hip compiled as points_mlp_gen_lz_kernel, which reads the
// per-texel maps M_b = W_z[b] F of linz_maps_gen.hip instead of gathering the latent and multiplying by lin_z[b] per point, view and
// block.  One lookup-general compilation (the footprint code of points_mlp_gen_ix.hip: bilinear / nearest, border / zeros / reflection),
// in a translation unit of its own so that the other code objects hold exactly the kernels they always held.  DINER_GEN_IX leaves the
// packers and check_shape to points_mlp_gen.hip.
#define DINER_GEN_IX
#define DINER_GEN_LZ
#include "points_mlp_gen.hip"
