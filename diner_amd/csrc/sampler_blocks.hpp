// Device functions of the two depth-guided samplers: sampler.hip (candidates on the ray, o + z d) and sampler_points.hip
// (candidates given as points, the NOVEL renderers' deformed candidates).
//   shared, one definition:   MapGeo, view_likelihood (the per-view likelihood), fill_up_and_sort
//   sampler_points.hip only:  map_geo and shortlist_gauss_fill -- COPIES of statements that sampler_kernel carries in place.
// sampler_kernel does not call the copies: routing it through shortlist_gauss_fill changes its generated code (226 against
// 202 VGPRs at CPL = 64, for one), and that kernel is on the benchmarked path.  An edit to
// either copy must be made to the other; tests/test_gpu_novel_sampler.py holds the two kernels' z_dg and z bit-equal on
// xyz = o + z d for one NC per instantiation, so a copy that drifts fails there.
#pragma once
#include "common.hpp"

namespace diner {

struct MapGeo {
    int H, W;
    float halfW, halfH, Wm1, Hm1;          // depth / normal maps
    float sfx, sfy, halfWp, halfHp, Wpm1, Hpm1;  // sigma map extended by DINER_SIGMA_PAD
};

// Likelihood of one candidate under one source view -- nerf_renderer.py:107-128.
// tex: the view's packed map, 2 float4 per texel = {nx,ny,nz,depth},{sigma,0,0,0}.
__device__ __forceinline__ float view_likelihood(const float4 *__restrict__ tex, const View &vw, const MapGeo &g,
                                                 float iw, float ih, float dcx, float dcy, float dcz,
                                                 float x, float y, float z, float half_step, float ddmax)
{
    float px, py, pz, u, w;
    project(vw, iw, ih, x, y, z, px, py, pz, u, w);
    // depth: nearest, border (image_encoder.py:129-151)
    const float ux = unnorm(u, g.halfW), uy = unnorm(w, g.halfH);
    const int dx = safe_idx(__builtin_rintf(clipf(ux, g.Wm1)), g.W), dy = safe_idx(__builtin_rintf(clipf(uy, g.Hm1)), g.H);
    const float depth = tex[((int64_t)dy * g.W + dx) * 2].w;
    if (!(fabsf(depth - pz) < ddmax)) return 0.0f;                      // depth_dist_mask (:122)
    // sigma: nearest in the exponentially padded map, zeros outside (image_encoder.py:153-180,
    // torch_helpers.py:100-160): ring at Chebyshev distance d>=1 = border * exp((d-1)/12 * ln 2)
    const float jx = __builtin_rintf(unnorm(u * g.sfx, g.halfWp)), jy = __builtin_rintf(unnorm(w * g.sfy, g.halfHp));
    if (!(jx >= 0.0f && jx <= g.Wpm1 && jy >= 0.0f && jy <= g.Hpm1)) return 0.0f;
    const int sx = (int)jx - DINER_SIGMA_PAD, sy = (int)jy - DINER_SIGMA_PAD;
    const int ox = sx < 0 ? -sx : (sx > g.W - 1 ? sx - (g.W - 1) : 0);
    const int oy = sy < 0 ? -sy : (sy > g.H - 1 ? sy - (g.H - 1) : 0);
    const int cheb = ox > oy ? ox : oy;
    const int cx = sx < 0 ? 0 : (sx > g.W - 1 ? g.W - 1 : sx), cy = sy < 0 ? 0 : (sy > g.H - 1 ? g.H - 1 : sy);
    float sigma = tex[((int64_t)cy * g.W + cx) * 2 + 1].x;
    if (cheb > 1) sigma = sigma * expf((float)(cheb - 1) / 12.0f * 0.6931471805599453f);
    if (sigma == 0.0f) return 0.0f;                                      // bg_mask (:123)
    // normal: nearest, zeros (image_encoder.py:182-204)
    const float nxf = __builtin_rintf(ux), nyf = __builtin_rintf(uy);
    float cosd = 0.0f;
    if (nxf >= 0.0f && nxf <= g.Wm1 && nyf >= 0.0f && nyf <= g.Hm1) {
        const float4 n = tex[((int64_t)(int)nyf * g.W + (int)nxf) * 2];
        cosd = dcx * n.x + dcy * n.y + dcz * n.z;                        // :119
    }
    if (!(cosd <= 0.0f)) return 0.0f;                                    // :121
    const float den = sigma * 1.4142135623730951f;
    const float a = erff((pz + half_step - depth) / den), b = erff((pz - half_step - depth) / den);
    return fabsf(0.5f * (a - b));                                        // :125-128
}

// fill_up_uniform_samples (:376-396) on the K values of one ray held in LDS (one wave):
// after the reference's first sort the m zeros sit in columns n_neg .. n_neg+m-1 (n_neg = number of
// negative samples, normally 0), so the i-th empty slot becomes near + (n_neg+i)*step + u_i*step;
// then one ascending bitonic sort (:396) over n2 = pow2 >= K with +inf padding.
__device__ __forceinline__ void fill_up_and_sort(float *zs, int K, float near, float far, const float *u_fill_row,
                                                 int64_t gray, uint2 key, int lane)
{
    int m = 0, n_neg = 0;
    for (int i0 = 0; i0 < K; i0 += 64) {
        const int i = i0 + lane;
        const float v = i < K ? zs[i] : 1.0f;
        m += __popcll(__ballot(v == 0.0f));
        n_neg += __popcll(__ballot(v < 0.0f));
    }
    if (m > 0) {
        const float step = (far - near) / (float)m;                   // :388
        int seen = 0;
        for (int i0 = 0; i0 < K; i0 += 64) {
            const int i = i0 + lane;
            const bool zero = i < K && zs[i] == 0.0f;
            const unsigned long long zm = __ballot(zero);
            if (zero) {
                const int rank = seen + __popcll(zm & ((1ull << lane) - 1ull));
                float u;
                if (u_fill_row) u = u_fill_row[rank];
                else u = u01(philox4x32(make_uint4((uint32_t)rank, 2u, (uint32_t)gray, (uint32_t)(gray >> 32)), key).x);
                const float zmiss = near + (float)(n_neg + rank) * step;  // :389
                zs[i] = zmiss + u * step;                                  // :390
            }
            seen += __popcll(zm);
        }
    }
    int n2 = 1;
    while (n2 < K) n2 <<= 1;
    for (int i = K + lane; i < n2; i += 64) zs[i] = __builtin_inff();
    __syncthreads();
    for (int kk = 2; kk <= n2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n2 >> 1); t += 64) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i + j;
                const float a = zs[i], b = zs[l];
                const bool asc = (i & kk) == 0;
                if ((a > b) == asc) { zs[i] = b; zs[l] = a; }
            }
            __syncthreads();
        }
    }
}

// the map geometry view_likelihood reads, from the scene: a copy of the assignments sampler_kernel states in place
__device__ __forceinline__ MapGeo map_geo(const DinerScene &s)
{
    MapGeo g;
    g.H = s.H; g.W = s.W;
    g.halfW = (float)s.W / 2.0f; g.halfH = (float)s.H / 2.0f; g.Wm1 = (float)(s.W - 1); g.Hm1 = (float)(s.H - 1);
    const int Wp = s.W + 2 * DINER_SIGMA_PAD, Hp = s.H + 2 * DINER_SIGMA_PAD;
    g.sfx = (float)s.W / (float)Wp; g.sfy = (float)s.H / (float)Hp;
    g.halfWp = (float)Wp / 2.0f; g.halfHp = (float)Hp / 2.0f; g.Wpm1 = (float)(Wp - 1); g.Hpm1 = (float)(Hp - 1);
    return g;
}

// A COPY of everything sampler_kernel does after the likelihood, statement for statement (see the head of this file; keep the
// two alike): the occlusion product and its moments (:131-132, :181-185), the top-(K-G) short-list by a bisection on
// the bit pattern with ties to the lower index (:172-178), the gaussian slots (:186-190, Philox stream 1 unless n_gauss), z_dg_out,
// the fill-up (stream 2 unless u_fill) and the sort.  z / L: candidate j = 64*c + lane, both 0 for j >= NC.  zs: n2 = pow2 >= K
// floats of LDS.  One wave.
template <int CPL>
__device__ __forceinline__ void shortlist_gauss_fill(const float (&z)[CPL], const float (&L)[CPL], float *zs, int K, int G, float near,
                                                     float far, const float *__restrict__ n_gauss, const float *__restrict__ u_fill,
                                                     int64_t gray, uint2 key, int lane, float *__restrict__ z_out,
                                                     float *__restrict__ z_dg_out)
{
    const int keep = K - G;
    float wsum = 0.0f;
    float O[CPL];
    {
        float carry = 1.0f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const float incl = wave_scan_mul(1.0f - L[c], lane);
            float excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 1.0f;
            O[c] = L[c] * (carry * excl);
            carry = carry * __shfl(incl, 63, 64);
            wsum += O[c];
        }
    }
    bool hit = false;
#pragma unroll
    for (int c = 0; c < CPL; ++c) hit |= (O[c] != 0.0f);
    hit = __any(hit);
    float gmean = 0.0f, gstd = 0.0f;
    if (G > 0 && hit) {  // weighted_mean_n_std, torch_helpers.py:294-302
        wsum = wave_sum(wsum);
        float m = 0.0f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) m += z[c] * (O[c] / wsum);
        gmean = wave_sum(m);
        float var = 0.0f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) { const float d = z[c] - gmean; var += d * d * (O[c] / wsum); }
        gstd = sqrtf(wave_sum(var));
    }

    int n_kept = 0;
    if (keep > 0) {
        uint32_t T = 0;
        int n_nz = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) n_nz += __popcll(__ballot(L[c] > 0.0f));
        // fewer non-zero likelihoods than slots: everything non-zero is kept, no threshold to search for
        for (int b = (n_nz <= keep) ? -1 : 29; b >= 0; --b) {
            const uint32_t cand = T | (1u << b);
            int cnt = 0;
#pragma unroll
            for (int c = 0; c < CPL; ++c) cnt += __popcll(__ballot(__float_as_uint(L[c]) >= cand));
            if (cnt >= keep) T = cand;
        }
        // T = bit pattern of the keep-th largest likelihood, or 0 if fewer than `keep` are non-zero
        int n_gt = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) n_gt += __popcll(__ballot(__float_as_uint(L[c]) > T));
        const int n_eq = (T == 0) ? 0 : keep - n_gt;  // ties at the cut that are still kept
        int seen_eq = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const uint32_t k = __float_as_uint(L[c]);
            const unsigned long long eqm = __ballot(k == T && T != 0);
            const int my_eq_rank = seen_eq + __popcll(eqm & ((1ull << lane) - 1ull));
            const bool kept = (k > T) || (k == T && T != 0 && my_eq_rank < n_eq);
            const unsigned long long km = __ballot(kept);
            if (kept) zs[n_kept + __popcll(km & ((1ull << lane) - 1ull))] = z[c];  // z=0 where L==0: not kept
            n_kept += __popcll(km);
            seen_eq += __popcll(eqm);
        }
    }
    for (int i = n_kept + lane; i < keep; i += 64) zs[i] = 0.0f;     // empty slots (:176-178)
    for (int i = lane; i < G; i += 64) {                              // gaussian slots (:186-190)
        float val = 0.0f;
        if (hit) {
            float n;
            if (n_gauss) n = n_gauss[gray * G + i];
            else {
                const uint4 r = philox4x32(make_uint4((uint32_t)i, 1u, (uint32_t)gray, (uint32_t)(gray >> 32)), key);
                n = sqrtf(-2.0f * logf(1.0f - u01(r.x))) * cosf(6.283185307179586f * u01(r.y));
            }
            val = n * gstd + gmean;
        }
        zs[keep + i] = val;
    }
    __syncthreads();
    if (z_dg_out)
        for (int i = lane; i < K; i += 64) z_dg_out[gray * K + i] = zs[i];

    fill_up_and_sort(zs, K, near, far, u_fill ? u_fill + gray * K : nullptr, gray, key, lane);
    for (int i = lane; i < K; i += 64) z_out[gray * K + i] = zs[i];
}

}  // namespace diner
