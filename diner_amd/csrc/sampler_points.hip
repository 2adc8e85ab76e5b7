// Depth-guided ray sampler on GIVEN candidate points, one ray per wavefront -- the sampler of the fork's NOVEL / NOVEL_PE
// renderers (reference src/models/novel/nerf_novel_renderer.py:79-167), whose candidates are deformed by their nearest mesh vertex
// before they are projected into the source views (:105-108):
//   z_cand   [SB,NR,NC]    the stratified depths (diner_sample_coarse): the moments, the short-list and the outputs are depths
//   xyz_cand [SB,NR,NC,3]  the points those depths stand for (diner_deform_ray_points): what the source views see
// The kernel is sampler_kernel (sampler.hip) with the candidate's position read instead of formed as o + z d; it draws no
// candidate noise.  The ray's direction still gives raydirs_cam (:115), near / far still give half_step (:104) and the fill-up.
// The per-view likelihood and the fill-up are sampler_blocks.hpp's definitions, shared with sampler_kernel; the decisions between
// them (shortlist_gauss_fill) are a copy of sampler_kernel's statements, held bit-equal to them by a GPU test.
//
// The candidate's point is RELOADED in every view, by the lane's own 12-byte load (one global_load_dwordx3 at a stride of 12 B
// across the wave; the NV - 1 repeats are served by the caches), and never kept across the view loop.  A one-off record of that
// choice -- only the first form is in the tree, the others cannot be rebuilt from it -- measured on an MI355X at 4096 rays x 1000
// candidates, 4 views (tools/bench_novel_sampler.py; sampler_kernel on the same depths: 0.094 ms):
//   reloaded per view, 12-byte loads                                  0.092 ms    90 VGPRs at CPL = 16
//   reloaded per view, a chunk's 768 B loaded as coalesced dwords
//     and exchanged through LDS (two barriers per chunk)              0.136 ms    92
//   loaded once through that exchange, kept in 3 CPL registers        0.142 ms   208
//   loaded once by 12-byte loads, kept                                not run: 512 VGPRs and scratch at CPL = 16 and 32
// The exchange saves nothing that matters (49 MB over 256 CUs is about a microsecond of L1 throughput however the lanes are laid
// out) and its barriers put a chunk's memory latency between the chunks; keeping the points costs occupancy.  With the reload the
// instantiations take 52 / 90 / 154 / 225 VGPRs against sampler_kernel's 75 / 168 / 294 / 202, and CPL = 64 takes 272 B of scratch
// against its 528 B.
#include "common.hpp"
#include "sampler_blocks.hpp"

namespace diner {

template <int CPL>  // candidates per lane: NC <= 64*CPL
__global__ __launch_bounds__(64) void sampler_points_kernel(
    DinerScene s, const float *__restrict__ rays, const float *__restrict__ z_cand, const float *__restrict__ xyz_cand, int64_t NR,
    DinerSamplerCfg cfg, const float *__restrict__ n_gauss, const float *__restrict__ u_fill, uint64_t seed,
    float *__restrict__ z_out, float *__restrict__ z_dg_out, float *__restrict__ lik_out)
{
    extern __shared__ float zs[];  // n2 = pow2 >= K floats
    const int lane = threadIdx.x;
    const int sb = blockIdx.y;
    const int64_t ray = blockIdx.x, gray = (int64_t)sb * NR + ray;
    const int NC = cfg.n_candidates, K = cfg.n_samples, G = cfg.n_gaussian;
    const float *rp = rays + gray * 8;
    const float dx = rp[3], dy = rp[4], dz = rp[5], near = rp[6], far = rp[7];
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const float *ray_xyz = xyz_cand + gray * NC * 3;

    float z[CPL], L[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = c * 64 + lane;
        L[c] = 0.0f;
        z[c] = j < NC ? z_cand[gray * NC + j] : 0.0f;
    }

    // ---- per-view surface likelihood of the given points, max over views (:110-141) -------------
    const MapGeo g = map_geo(s);
    const float half_step = ((far - near) / (float)NC) / 2.0f;  // :104, :138
    for (int v = 0; v < s.NV; ++v) {
        const View vw = load_view(s, sb, v);
        float dcx, dcy, dcz;
        rotate(vw, dx, dy, dz, dcx, dcy, dcz);  // raydirs_cam (:115)
        const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = c * 64 + lane;
            if (j < NC) {
                const float *p = ray_xyz + (int64_t)j * 3;   // :105-108, in place of o + z d
                const float l = view_likelihood(tex, vw, g, s.image_w, s.image_h, dcx, dcy, dcz, p[0], p[1], p[2], half_step,
                                                cfg.depth_diff_max);
                L[c] = l > L[c] ? l : L[c];
            }
        }
    }
    if (lik_out) {
#pragma unroll
        for (int c = 0; c < CPL; ++c)
            if (c * 64 + lane < NC) lik_out[gray * NC + c * 64 + lane] = L[c];
    }

    shortlist_gauss_fill<CPL>(z, L, zs, K, G, near, far, n_gauss, u_fill, gray, key, lane, z_out, z_dg_out);
}

int launch_sampler_points(const DinerScene &s, const float *rays, const float *z_cand, const float *xyz_cand, int64_t NR,
                          const DinerSamplerCfg &cfg, const float *n_gauss, const float *u_fill, uint64_t seed, float *z_out,
                          float *z_dg_out, float *lik_out, hipStream_t st)
{
    const int NC = cfg.n_candidates;
    if (NC > 64 * 64) { set_error("sampler_points: n_candidates=%d > 4096 unsupported", NC); return DINER_E_UNSUPPORTED; }
    if (NR == 0 || s.SB == 0) return DINER_OK;
    int n2 = 1;
    while (n2 < cfg.n_samples) n2 <<= 1;
    const size_t lds = sizeof(float) * (size_t)n2;
    const dim3 grid((unsigned)NR, (unsigned)s.SB), block(64);
#define DINER_LAUNCH_SAMPLER_POINTS(CPL)                                                                                       \
    hipLaunchKernelGGL(sampler_points_kernel<CPL>, grid, block, lds, st, s, rays, z_cand, xyz_cand, NR, cfg, n_gauss, u_fill, seed, \
                       z_out, z_dg_out, lik_out)
    if (NC <= 64 * 4) DINER_LAUNCH_SAMPLER_POINTS(4);
    else if (NC <= 64 * 16) DINER_LAUNCH_SAMPLER_POINTS(16);
    else if (NC <= 64 * 32) DINER_LAUNCH_SAMPLER_POINTS(32);
    else DINER_LAUNCH_SAMPLER_POINTS(64);
#undef DINER_LAUNCH_SAMPLER_POINTS
    return check_launch("sampler_points_kernel");
}

}  // namespace diner
