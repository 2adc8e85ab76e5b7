// Shape-general training path: the building blocks that let diner_amd/training_gen.py train any ResnetFC / PositionalEncoding
// shape of the inference envelope (include/diner_hip.h, "shape-general inference path") in exact fp32:
//   gemm_act_kernel        the fp32 MFMA GEMM of train.hip (v_mfma_f32_32x32x2_f32, 128 x 128 x 16 tiles, double-buffered LDS;
//                          the tile loads and the block -> tile map are the shared ones of train_blocks.hpp)
//                          with activation codes instead of relu flags:
//                            C[m][n] (+)= sum_k actA(A[m][k]) * actB(B[k][n])  (+ bias[n]) (* act'(S[m][n]))
//                          act = identity | ReLU | Softplus(beta, threshold 20) (resnetfc.py:49-52,124-127), act' its derivative
//                          as autograd evaluates it (ReLU: [S > 0]; Softplus: torch's softplus_backward)
//   point_inputs_gen       the 7 + 8F MLP inputs of pixelnerf.py:128 (zero-padded to ld_in columns), the latent lookup of any
//                          DINER_INDEX_* mode and its 4-tap footprint, for any num_freqs F and latent width C
//   point_inputs_bwd_gen   the transpose of point_inputs_gen to the rays, cameras and depth maps (point_inputs_bwd_kernel of
//                          train.hip for any F, ld_in and C), same per-row records and fixed-order reductions
// The fixed-order reductions of the per-row records (camg_* kernels, launch_train_camg_reduce) are here for both training paths:
// train.hip's point_inputs_bwd_kernel writes the same records and ends in the same call.
// The point-input kernels are templates on the lookup (train_gen_points.hpp): this file instantiates the 4-tap forms, train_gen_bc.hip the
// 16-tap bicubic ones next to bicubic_scatter_kernel, in a code object of their own; the GEMM and the reductions are here.
#include "train_gen_points.hpp"

namespace diner {

namespace train_gen {

constexpr int BM = 128, BN = 128, BK = 16, LDT = 132;  // block tile; LDS tile row stride (floats, 16-byte aligned rows)

struct GemmArgs {
    const float *A, *B, *bias, *S;
    float *C;
    int64_t M;
    int N, K;
    int64_t sam, sak, sbk, sbn;  // element strides of the logical A[m][k], B[k][n]
    int64_t ldc, lds_;           // row strides of C and of S
    int act_a, act_b, act_s;     // DINER_ACT_* of the A operand, the B operand and the epilogue derivative
    float beta;                  // Softplus beta (any DINER_ACT_SOFTPLUS code)
    int accumulate, atomic;
    int64_t k_chunk;             // split-K: blockIdx.z handles k in [z*k_chunk, (z+1)*k_chunk)
};

// the operand transform happens here, once per staged element; out-of-range pieces are 0 (not act(0): Softplus(0) != 0)
template <bool KC>
__device__ __forceinline__ void tile_store(float (*T)[LDT], const f32x4 (&v)[2], unsigned ok, int act, float beta, int tid)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        f32x4 x = v[i];
        const bool in = (ok >> i) & 1u;
        if (act == DINER_ACT_SOFTPLUS) {
            for (int j = 0; j < 4; ++j) x[j] = in ? softplus(x[j], beta) : 0.0f;
        } else {
            const float lo = act == DINER_ACT_RELU ? 0.f : -__builtin_inff();
            for (int j = 0; j < 4; ++j) x[j] = in ? (x[j] < lo ? lo : x[j]) : 0.f;  // NaN-keeping floor
        }
        if (KC) {
            const int l = idx >> 2, kq = (idx & 3) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) T[kq + j][l] = x[j];
        } else {
            const int k = idx >> 5, lq = (idx & 31) * 4;
            *(f32x4 *)&T[k][lq] = x;
        }
    }
}

// This kernel's own epilogue, not train_blocks.hpp's epilogue<PA, PB>: it forms the row index in 64-bit steps (m0 + mbl + ...), the shared one
// in 32-bit ones before adding m0, and hipcc allocates this kernel's registers differently around the other form.
// C layout of the 32x32 MFMA accumulators: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)
__device__ __forceinline__ void epilogue(const GemmArgs &g, const f32x16 (&acc)[2][2], int64_t m0, int n0, int wm, int wn, int lane)
{
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const int n = n0 + wn + tb * 32 + (lane & 31);
        if (n >= g.N) continue;
        const float bias = (g.bias && blockIdx.z == 0) ? g.bias[n] : 0.0f;
#pragma unroll
        for (int ta = 0; ta < 2; ++ta) {
            const int mbl = wm + ta * 32 + 4 * (lane >> 5);
            float old[16], msk[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { old[i] = 0.0f; msk[i] = 1.0f; }
            if (g.accumulate && !g.atomic) {  // uniform branches, unconditional loads from clamped rows
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t m = m0 + mbl + (i & 3) + 8 * (i >> 2);
                    old[i] = g.C[(m < g.M ? m : g.M - 1) * g.ldc + n];
                }
            }
            if (g.S) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t m = m0 + mbl + (i & 3) + 8 * (i >> 2);
                    msk[i] = g.S[(m < g.M ? m : g.M - 1) * g.lds_ + n];
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t m = m0 + mbl + (i & 3) + 8 * (i >> 2);
                if (m >= g.M) continue;
                float v = acc[ta][tb][i] + bias;
                if (g.S) v = act_bwd(v, msk[i], g.act_s, g.beta);
                float *c = g.C + m * g.ldc + n;
                if (g.atomic) atomicAdd(c, v);
                else *c = old[i] + v;
            }
        }
    }
}

// AK: A contiguous along k (sak == 1) else along m (sam == 1).  BNC: B contiguous along n (sbn == 1) else along k.
// 4 waves as 2 x 2, each a 64 x 64 output (2 x 2 MFMA tiles); the global loads of tile t+1 are in flight while tile t is
// multiplied out of LDS (double-buffered, one barrier per k-step) -- train.hip's gemm_kernel.
template <bool AK, bool BNC>
__global__ __launch_bounds__(256) void gemm_act_kernel(GemmArgs g)
{
    __shared__ float As[2][BK][LDT], Bs[2][BK][LDT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t m0;
    int n0;
    tile_of(g.M, g.N, BM, BN, blockIdx.x, m0, n0);
    const int64_t kbeg = (int64_t)blockIdx.z * g.k_chunk;
    const int64_t kend = kbeg + g.k_chunk < g.K ? kbeg + g.k_chunk : g.K;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;
    f32x4 ra[2], rb[2];
    unsigned oka = tile_load<AK>(ra, g.A, g.sam, g.sak, m0, g.M, kbeg, kend, tid);
    unsigned okb = tile_load<!BNC>(rb, g.B, g.sbn, g.sbk, n0, g.N, kbeg, kend, tid);
    tile_store<AK>(As[0], ra, oka, g.act_a, g.beta, tid);
    tile_store<!BNC>(Bs[0], rb, okb, g.act_b, g.beta, tid);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = kbeg; k0 < kend; k0 += BK) {
        const bool more = k0 + BK < kend;
        if (more) {
            oka = tile_load<AK>(ra, g.A, g.sam, g.sak, m0, g.M, k0 + BK, kend, tid);
            okb = tile_load<!BNC>(rb, g.B, g.sbn, g.sbk, n0, g.N, k0 + BK, kend, tid);
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const int kr = kk + (lane >> 5), c = lane & 31;
            const float a0 = As[buf][kr][wm + c], a1 = As[buf][kr][wm + 32 + c];
            const float b0 = Bs[buf][kr][wn + c], b1 = Bs[buf][kr][wn + 32 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) {
            tile_store<AK>(As[buf ^ 1], ra, oka, g.act_a, g.beta, tid);
            tile_store<!BNC>(Bs[buf ^ 1], rb, okb, g.act_b, g.beta, tid);
        }
        __syncthreads();
        buf ^= 1;
    }
    epilogue(g, acc, m0, n0, wm, wn, lane);
}

// The fixed-order reductions of the per-row records, for both training paths (train.hip's point_inputs_bwd_kernel writes the same
// records): d_rays[sb][ray] = (sum over views and samples of d_o, d_d;  0 (near: sampler only);  d_far or 0) -- one thread per ray
__global__ __launch_bounds__(256) void camg_ray_reduce_kernel(const float *__restrict__ rowg, int64_t NR, int K, int NV, int sb,
                                                              const float *__restrict__ d_far, float *__restrict__ d_rays)
{
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= NR) return;
    const int64_t P = NR * K;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < NV; ++v)
        for (int k = 0; k < K; ++k) {
            const float *g = rowg + ((int64_t)v * P + ray * K + k) * CAMG_COLS;
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[c] += g[c];
        }
    float *o = d_rays + ((int64_t)sb * NR + ray) * 8;
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = acc[c];
    o[6] = 0.0f;
    o[7] = d_far ? d_far[(int64_t)sb * NR + ray] : 0.0f;
}

// per-view partial sums of the camera columns (6..23) over a contiguous chunk of the view's P rows: grid (blocks, NV)
__global__ __launch_bounds__(256) void camg_view_partial_kernel(const float *__restrict__ rowg, int64_t P, float *__restrict__ partial)
{
    constexpr int NC = CAMG_COLS - 6;
    __shared__ float red[NC][256];
    const int v = blockIdx.y, t = threadIdx.x;
    const int64_t chunk = (P + gridDim.x - 1) / gridDim.x, beg = blockIdx.x * chunk, end = beg + chunk < P ? beg + chunk : P;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    for (int64_t p = beg + t; p < end; p += 256) {
        const float *g = rowg + ((int64_t)v * P + p) * CAMG_COLS + 6;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += g[c];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) red[c][t] = acc[c];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
#pragma unroll
            for (int c = 0; c < NC; ++c) red[c][t] += red[c][t + h];
        __syncthreads();
    }
    if (t < NC) partial[((int64_t)v * gridDim.x + blockIdx.x) * NC + t] = red[t][0];
}

// final sums (fixed order): poses[sb][v] rows 0..2 (d_R | d_t), focal, c; image_shape += over all views (the caller zeroes it once)
__global__ __launch_bounds__(256) void camg_view_final_kernel(const float *__restrict__ partial, int NV, int nblk, int sb,
                                                              float *__restrict__ d_poses, float *__restrict__ d_focal,
                                                              float *__restrict__ d_c, float *__restrict__ d_ishape)
{
    constexpr int NC = CAMG_COLS - 6;
    for (int t = threadIdx.x; t < NV * NC; t += blockDim.x) {
        const int v = t / NC, c = t - v * NC;
        float sum = 0.f;
        for (int b = 0; b < nblk; ++b) sum += partial[((int64_t)v * nblk + b) * NC + c];
        const int64_t sv = (int64_t)sb * NV + v;
        if (c < 9) { if (d_poses) d_poses[sv * 16 + (c / 3) * 4 + c % 3] = sum; }
        else if (c < 12) { if (d_poses) d_poses[sv * 16 + (c - 9) * 4 + 3] = sum; }
        else if (c < 14) { if (d_focal) d_focal[sv * 2 + c - 12] = sum; }
        else if (c < 16) { if (d_c) d_c[sv * 2 + c - 14] = sum; }
        else if (v == 0 && d_ishape) {
            float tot = sum;
            for (int u = 1; u < NV; ++u) {
                float su = 0.f;
                for (int b = 0; b < nblk; ++b) su += partial[((int64_t)u * nblk + b) * NC + c];
                tot += su;
            }
            d_ishape[c - 16] += tot;
        }
    }
}

}  // namespace train_gen

int launch_train_gemm_act(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M, int N, int K, int64_t sam,
                          int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc, int64_t lds, int act_a, int act_b, int act_s, float beta,
                          int accumulate, int atomic, int64_t k_chunk, hipStream_t st)
{
    using namespace train_gen;
    if (M == 0 || N == 0) return DINER_OK;
    const int64_t kc = k_chunk > 0 ? k_chunk : K;
    GemmArgs g{A, B, bias, S, C, M, N, K, sam, sak, sbk, sbn, ldc, lds, act_a, act_b, act_s, beta, accumulate, atomic, kc};
    const dim3 grid((unsigned)(((M + BM - 1) / BM) * ((N + BN - 1) / BN)), 1, (unsigned)((K + kc - 1) / kc));
    const bool ak = sak == 1, bnc = sbn == 1;
    if (ak && bnc) hipLaunchKernelGGL((gemm_act_kernel<true, true>), grid, dim3(256), 0, st, g);
    else if (ak && !bnc) hipLaunchKernelGGL((gemm_act_kernel<true, false>), grid, dim3(256), 0, st, g);
    else if (!ak && bnc) hipLaunchKernelGGL((gemm_act_kernel<false, true>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((gemm_act_kernel<false, false>), grid, dim3(256), 0, st, g);
    return check_launch("train_gen::gemm_act_kernel");
}

int launch_train_point_inputs_gen(const DinerScene &s, const DinerLatentIndex &ix, const float *latent_nhwc, const float *rays, const float *z,
                                  int64_t NR, int K, int sb, float *in, int64_t ld_in, float *zlat, float *taps, hipStream_t st)
{
    const int64_t R = NR * (int64_t)K * s.NV;
    if (R == 0) return DINER_OK;
    hipLaunchKernelGGL(train_gen::point_inputs_gen_kernel<false>, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, ix.interp,
                       ix.padding, in, ld_in, zlat, taps);
    return check_launch("train_gen::point_inputs_gen_kernel<false>");
}

int launch_train_point_inputs_bwd_gen(const DinerScene &s, const DinerLatentIndex &ix, const float *latent_nhwc, const float *rays,
                                      const float *z, int64_t NR, int K, int sb, const float *d_in, int64_t ld_in, const float *d_zlat,
                                      const float *d_far, float *workspace, float *d_rays, float *d_poses, float *d_focal, float *d_c,
                                      float *d_image_shape, float *d_depths, hipStream_t st)
{
    using namespace train_gen;
    const int64_t P = NR * (int64_t)K, R = P * s.NV;
    if (R == 0) return DINER_OK;
    float *rowg = workspace, *partial = workspace + R * CAMG_COLS;   // diner_train_camera_workspace_floats' layout
    hipLaunchKernelGGL(point_inputs_bwd_gen_kernel<false>, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, ix.interp,
                       ix.padding, d_in, ld_in, d_zlat, rowg, d_depths);
    int rc = check_launch("train_gen::point_inputs_bwd_gen_kernel<false>");
    if (rc) return rc;
    return launch_train_camg_reduce(rowg, partial, NR, K, s.NV, sb, d_far, d_rays, d_poses, d_focal, d_c, d_image_shape, st);
}

// (behind every point-input backward: this file's, train_gen_bc.hip's and train.hip's)
int launch_train_camg_reduce(const float *rowg, float *partial, int64_t NR, int K, int NV, int sb, const float *d_far, float *d_rays,
                             float *d_poses, float *d_focal, float *d_c, float *d_image_shape, hipStream_t st)
{
    using namespace train_gen;
    const int64_t P = NR * (int64_t)K;
    int rc;
    if (d_rays) {
        hipLaunchKernelGGL(camg_ray_reduce_kernel, dim3((unsigned)((NR + 255) / 256)), dim3(256), 0, st, rowg, NR, K, NV, sb, d_far, d_rays);
        if ((rc = check_launch("train_gen::camg_ray_reduce_kernel"))) return rc;
    }
    if (d_poses || d_focal || d_c || d_image_shape) {
        const int64_t per = (P + 255) / 256;
        const int nblk = (int)(per < CAMG_BLOCKS ? per : CAMG_BLOCKS);
        hipLaunchKernelGGL(camg_view_partial_kernel, dim3((unsigned)nblk, (unsigned)NV), dim3(256), 0, st, rowg, P, partial);
        if ((rc = check_launch("train_gen::camg_view_partial_kernel"))) return rc;
        hipLaunchKernelGGL(camg_view_final_kernel, dim3(1), dim3(256), 0, st, partial, NV, nblk, sb, d_poses, d_focal, d_c, d_image_shape);
        if ((rc = check_launch("train_gen::camg_view_final_kernel"))) return rc;
    }
    return DINER_OK;
}

}  // namespace diner
