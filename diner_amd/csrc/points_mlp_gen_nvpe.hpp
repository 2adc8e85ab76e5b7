// What both precisions of the NOVEL_PE point kernels share (points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip): the argument record
// a validated diner_render_points_novel_pe call hands to the kernel, and the 3-channel lookup of a positional-encoding map.
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

__device__ __forceinline__ View view_of(const float *poses, const float *focal, const float *c, int sb)
{
    View v;
    const float *Pm = poses + (int64_t)sb * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v.r[i * 3 + 0] = Pm[i * 4 + 0]; v.r[i * 3 + 1] = Pm[i * 4 + 1]; v.r[i * 3 + 2] = Pm[i * 4 + 2];
        v.t[i] = Pm[i * 4 + 3];
    }
    v.fx = focal[sb * 2]; v.fy = focal[sb * 2 + 1]; v.cx = c[sb * 2]; v.cy = c[sb * 2 + 1];
    return v;
}

// lookup of one [mh, mw, 4] map at uv with the encoder's feature_padding (scaled by the map's own size, as index() scales gen_latent's)
// and lookup mode: ATen's accumulation order nw, ne, sw, se with contracted FMAs; .w is the padding channel
__device__ __forceinline__ float4 pe_lookup(const float4 *__restrict__ map, int mh, int mw, float u, float w, float feature_padding,
                                            int interp, int padding)
{
    const float sx = ((float)mw - feature_padding * 2.0f) / (float)mw, sy = ((float)mh - feature_padding * 2.0f) / (float)mh;
    const LatentFoot f = latent_footprint<true>(u, w, sx, sy, mw, mh, interp, padding);
    const float4 a = map[f.y0 * mw + f.x0], b = map[f.y0 * mw + f.x1], c = map[f.y1 * mw + f.x0], d = map[f.y1 * mw + f.x1];
    float4 o;
    o.x = __builtin_fmaf(d.x, f.se, __builtin_fmaf(c.x, f.sw, __builtin_fmaf(b.x, f.ne, a.x * f.nw)));
    o.y = __builtin_fmaf(d.y, f.se, __builtin_fmaf(c.y, f.sw, __builtin_fmaf(b.y, f.ne, a.y * f.nw)));
    o.z = __builtin_fmaf(d.z, f.se, __builtin_fmaf(c.z, f.sw, __builtin_fmaf(b.z, f.ne, a.z * f.nw)));
    o.w = 0.0f;
    return o;
}

}  // namespace diner
