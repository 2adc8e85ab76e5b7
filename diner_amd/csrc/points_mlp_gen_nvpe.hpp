// What both precisions of the NOVEL_PE point kernels share (points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip): the argument record
// a validated diner_render_points_novel_pe call hands to the kernel, and the 3-channel lookup of a positional-encoding map (the camera
// record of a [SB,4,4] pose, view_of, is common.hpp's).
#pragma once
#include "common.hpp"

namespace diner {

struct NovelPeIn {
    const float *xyz_in, *xyz_gen, *xyz_tgt, *viewdirs;   // [SB,P,3] each
    int64_t P;
    const float *glat;      // [gh, gw, C] NHWC
    int gh, gw;
    const float *gposes, *gfocal, *gc;          // [SB,4,4], [SB,2], [SB,2]
    float giw, gih;         // the general cameras' image shape (W, H)
    const float *dmap;      // [SB, NV, h, w, C]: W_d[:, :C] . latent per texel (novel_pe_map.hip), no bias
    const float *head;      // [C][8]: W_d[c, C:C+6] | b_d[c] | 0
    const float *spe;       // [SB, NV, sph, spw, 4]: the source views' pos-encoding maps, NHWC padded to 4 channels
    int sph, spw;
    const float *tpe;       // [SB, tph, tpw, 4]: the target view's
    int tph, tpw;
    const float *tposes, *tfocal, *tc;          // [SB,4,4], [SB,2], [SB,2]
    float tiw, tih;         // the target cameras' image shape (W, H)
    int ix_interp, ix_padding;                  // DINER_INDEX_* of all four lookups
};

// lookup of one [mh, mw, 4] map at uv with the encoder's feature_padding (scaled by the map's own size, as index() scales gen_latent's)
// and lookup mode; .w is the padding channel
__device__ __forceinline__ float4 pe_lookup(const float4 *__restrict__ map, int mh, int mw, float u, float w, float feature_padding,
                                            int interp, int padding)
{
    const LatentFoot f = latent_footprint<true>(u, w, pad_scale(mw, feature_padding), pad_scale(mh, feature_padding), mw, mh, interp, padding);
    const float4 a = map[f.y0 * mw + f.x0], b = map[f.y0 * mw + f.x1], c = map[f.y1 * mw + f.x0], d = map[f.y1 * mw + f.x1];
    return make_float4(tap_sum(a.x, b.x, c.x, d.x, f), tap_sum(a.y, b.y, c.y, d.y, f), tap_sum(a.z, b.z, c.z, d.z, f), 0.0f);
}

// the same lookup at a world point x seen by the scene's one camera `cam` of image shape (iw, ih): NOVEL_PE's tgt_pe
__device__ __forceinline__ float4 pe_lookup_at(const float4 *__restrict__ map, int mh, int mw, const View &cam, float iw, float ih,
                                               const float *x, float feature_padding, int interp, int padding)
{
    float px, py, pz, u, w;
    project(cam, iw, ih, x[0], x[1], x[2], px, py, pz, u, w);
    return pe_lookup(map, mh, mw, u, w, feature_padding, interp, padding);
}

}  // namespace diner
