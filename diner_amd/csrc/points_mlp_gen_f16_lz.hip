// The lin_z-map form of the shape-general f16x3 point/MLP kernel: points_mlp_gen_f16.hip compiled as points_mlp_gen_f16_lz_kernel, which
// reads the per-texel fp32 maps M_b = W_z[b] F of linz_maps_gen.hip instead of gathering the latent and multiplying by lin_z[b] per
// point, view and block.  One lookup-general compilation (the footprint code of points_mlp_gen_f16_ix.hip), in a translation unit of
// its own so that the other code objects hold exactly the kernels they always held.  DINER_GENF16_IX leaves the packers to
// points_mlp_gen_f16.hip.
#define DINER_GENF16_IX
#define DINER_GENF16_LZ
#include "points_mlp_gen_f16.hip"
