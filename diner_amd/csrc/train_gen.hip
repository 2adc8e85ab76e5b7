// Shape-general training path: the building blocks that let diner_amd/training_gen.py train any ResnetFC / PositionalEncoding
// shape of the inference envelope (include/diner_hip.h, "shape-general inference path") in exact fp32:
//   gemm_act_kernel        the fp32 MFMA GEMM of train.hip (v_mfma_f32_32x32x2_f32, 128 x 128 x 16 tiles, double-buffered LDS)
//                          with activation codes instead of relu flags:
//                            C[m][n] (+)= sum_k actA(A[m][k]) * actB(B[k][n])  (+ bias[n]) (* act'(S[m][n]))
//                          act = identity | ReLU | Softplus(beta, threshold 20) (resnetfc.py:49-52,124-127), act' its derivative
//                          as autograd evaluates it (ReLU: [S > 0]; Softplus: torch's softplus_backward)
//   point_inputs_gen       the 7 + 8F MLP inputs of pixelnerf.py:128 (zero-padded to ld_in columns), the latent lookup of any
//                          DINER_INDEX_* mode and its 4-tap footprint, for any num_freqs F and latent width C
//   point_inputs_bwd_gen   the transpose of point_inputs_gen to the rays, cameras and depth maps (point_inputs_bwd_kernel of
//                          train.hip for any F, ld_in and C), same per-row records and fixed-order reductions
// train.hip is left as it is: its code objects (the standard path's) do not change with this file.
// train_gen_bc.hip compiles this file a second time with DINER_TRAIN_GEN_BC defined: the two point-input kernels are then
// point_inputs_gen_bc_kernel / point_inputs_bwd_gen_bc_kernel, the 16-tap bicubic lookup (common.hpp bicubic_footprint) and its
// gradient with respect to the grid, next to bicubic_scatter_kernel -- in a code object of their own; the GEMM and the reductions stay here.
#include "common.hpp"

namespace diner {

namespace train_gen {

#ifndef DINER_TRAIN_GEN_BC
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// Softplus(beta) as torch evaluates it (x * beta > 20: linear): the formula of points_mlp_gen.hip's helper
__device__ __forceinline__ float softplus(float v, float beta)
{
    const float xb = v * beta;
    return xb > 20.0f ? v : log1pf(expf(xb)) / beta;
}

__device__ __forceinline__ float act_fwd(float x, int act, float beta)
{
    if (act == DINER_ACT_RELU) return x < 0.0f ? 0.0f : x;   // keeps NaN, like torch.relu
    if (act == DINER_ACT_SOFTPLUS) return softplus(x, beta);
    return x;
}

// g * act'(s) as autograd evaluates it: ReLU threshold_backward ([s > 0]); Softplus softplus_backward
// (z = exp(beta s), g * z / (z + 1), g where beta s > 20)
__device__ __forceinline__ float act_bwd(float g, float s, int act, float beta)
{
    if (act == DINER_ACT_RELU) return s > 0.0f ? g : 0.0f;
    if (act == DINER_ACT_SOFTPLUS) {
        const float xb = s * beta;
        if (xb > 20.0f) return g;
        const float z = expf(xb);
        return g * z / (z + 1.0f);
    }
    return g;
}

// One operand tile (128 x 16, as [k][m]) = 512 float4, two per thread (train.hip tile_load).  KC: the operand is contiguous along
// the contraction index, else along the tile's long index.  Loads are unconditional from clamped in-range addresses; `ok` zeroes
// the out-of-range pieces when the tile is stored.
template <bool KC>
__device__ __forceinline__ unsigned tile_load(f32x4 (&v)[2], const float *__restrict__ base, int64_t s_long, int64_t s_k, int64_t l0,
                                              int64_t l_end, int64_t k0, int64_t k_end, int tid)
{
    unsigned ok = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        if (KC) {
            const int64_t l = l0 + (idx >> 2), k = k0 + (idx & 3) * 4;
            const bool in = l < l_end && k < k_end;
            ok |= (unsigned)in << i;
            v[i] = *(const f32x4 *)(base + (l < l_end ? l : l_end - 1) * s_long + (k < k_end ? k : k_end - 4));
        } else {
            const int64_t k = k0 + (idx >> 5), l = l0 + (idx & 31) * 4;
            const bool in = k < k_end && l < l_end;
            ok |= (unsigned)in << i;
            v[i] = *(const f32x4 *)(base + (k < k_end ? k : k_end - 1) * s_k + (l < l_end ? l : l_end - 4));
        }
    }
    return ok;
}

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

// Block -> output tile, XCD-aware (train.hip tile_of): the column blocks of one row tile go to consecutive workgroups of one XCD
__device__ __forceinline__ void tile_of(const GemmArgs &g, int64_t &m0, int &n0)
{
    const int64_t gm = (g.M + BM - 1) / BM, lin = blockIdx.x;
    const int gn = (g.N + BN - 1) / BN;
    const int64_t full = gm / 8 * 8;
    int64_t mt, nb;
    if (lin < full * gn) { const int64_t j = lin / 8; nb = j % gn; mt = j / gn * 8 + lin % 8; }
    else { const int64_t r = lin - full * gn; mt = full + r / gn; nb = r % gn; }
    m0 = mt * BM;
    n0 = (int)nb * BN;
}

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
    tile_of(g, m0, n0);
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
#endif  // DINER_TRAIN_GEN_BC

// ---- per-(view, point) MLP inputs of any num_freqs F and latent width C ---------------------------------------------------------
// rows are view-major: row = v*P + p.  in [R, ld_in]: pixelnerf.py:128's 7 + 8F inputs in point_inputs_kernel's column order
//   [x_cam 3 | sin(f_j x_cam + phi_j) 6F | R d_w 3 | depth_dist 1 | sin(f_j depth_dist + phi_j) 2F | 0 ...]
// with sinf and the expression of the shape-general inference kernel (points_mlp_gen.hip); zlat [R, C]: the latent lookup of the
// scene's DINER_INDEX_* mode from the NHWC latent; taps [R, 8]: its 4 texel indices (int bits) and weights.
// Bicubic (DINER_TRAIN_GEN_BC): taps [R, 16] = the 4 columns and 4 rows of the footprint (int bits), then cx[4], cy[4].
#ifdef DINER_TRAIN_GEN_BC
#define point_inputs_gen_kernel point_inputs_gen_bc_kernel
#define point_inputs_bwd_gen_kernel point_inputs_bwd_gen_bc_kernel
#endif
__global__ __launch_bounds__(64) void point_inputs_gen_kernel(DinerScene s, const float *__restrict__ latent_nhwc,
                                                              const float *__restrict__ rays, const float *__restrict__ zsamp,
                                                              int64_t NR, int K, int sb, int ix_interp, int ix_padding,
                                                              float *__restrict__ in, int64_t ld_in, float *__restrict__ zlat,
                                                              float *__restrict__ taps_out)
{
    const int64_t P = NR * (int64_t)K, row = blockIdx.x;
    const int v = (int)(row / P);
    const int64_t p = row - (int64_t)v * P;
    const int lane = threadIdx.x;
    const float *rp = rays + ((int64_t)sb * NR + p / K) * 8;
    const float zz = zsamp[(int64_t)sb * P + p];
    const float dwx = rp[3], dwy = rp[4], dwz = rp[5];
    const float wx = rp[0] + zz * dwx, wy = rp[1] + zz * dwy, wz = rp[2] + zz * dwz;  // nerf_renderer.py:304
    const View vw = load_view(s, sb, v);
    float px, py, pz, u, w, dcx, dcy, dcz;
    project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);                  // pixelnerf.py:91-93,105-108
    rotate(vw, dwx, dwy, dwz, dcx, dcy, dcz);                                           // :99-101
    const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
    const int ddx = safe_idx(__builtin_rintf(clipf(unnorm(u, (float)s.W / 2.0f), (float)(s.W - 1))), s.W);
    const int ddy = safe_idx(__builtin_rintf(clipf(unnorm(w, (float)s.H / 2.0f), (float)(s.H - 1))), s.H);
    const float delta = tex[((int64_t)ddy * s.W + ddx) * 2].w - pz;                    // :114-115
    const int F = s.num_freqs, e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1;
    const float half_pi = 1.5707963267948966f;
    for (int e = lane; e < ld_in; e += 64) {
        float val;
        if (e < 3) val = e == 0 ? px : e == 1 ? py : pz;
        else if (e < e_pe3) { const int j = (e - 3) / 3, i = (e - 3) % 3;    // positional_encoding.py:45-49
            val = sinf(__builtin_fmaf(i == 0 ? px : i == 1 ? py : pz, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
        else if (e < e_dir) val = e == e_pe3 ? dcx : e == e_pe3 + 1 ? dcy : dcz;
        else if (e == e_dir) val = delta;
        else if (e < e_pe1 + 2 * F) { const int j = e - e_pe1;
            val = sinf(__builtin_fmaf(delta, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
        else val = 0.0f;
        in[row * ld_in + e] = val;
    }
    // footprint of the lookup mode in the latent map (image_encoder.py:97-127; common.hpp)
    const float sxl = ((float)s.w - s.feature_padding * 2.0f) / (float)s.w, syl = ((float)s.h - s.feature_padding * 2.0f) / (float)s.h;
#ifdef DINER_TRAIN_GEN_BC
    const BicubicFoot f = bicubic_footprint(u, w, sxl, syl, s.w, s.h, ix_padding);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            taps_out[row * 16 + i] = __int_as_float(f.x[i]); taps_out[row * 16 + 4 + i] = __int_as_float(f.y[i]);
            taps_out[row * 16 + 8 + i] = f.cx[i]; taps_out[row * 16 + 12 + i] = f.cy[i];
        }
    }
    const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
    for (int ch = lane; ch < s.C; ch += 64) {   // sum_j cy[j] * (sum_i cx[i] * texel_ij): the inference kernels' order and contraction
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *lr = lat + (int64_t)f.y[j] * s.w * s.C + ch;
            float t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] = lr[(int64_t)f.x[i] * s.C];
            const float rowv = __builtin_fmaf(t[3], f.cx[3], __builtin_fmaf(t[2], f.cx[2], __builtin_fmaf(t[1], f.cx[1], t[0] * f.cx[0])));
            acc = j == 0 ? rowv * f.cy[0] : __builtin_fmaf(rowv, f.cy[j], acc);
        }
        zlat[row * s.C + ch] = acc;
    }
#else
    const LatentFoot f = latent_footprint<true>(u, w, sxl, syl, s.w, s.h, ix_interp, ix_padding);
    const int o[4] = {f.y0 * s.w + f.x0, f.y0 * s.w + f.x1, f.y1 * s.w + f.x0, f.y1 * s.w + f.x1};
    const float wt[4] = {f.nw, f.ne, f.sw, f.se};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { taps_out[row * 8 + i] = __int_as_float(o[i]); taps_out[row * 8 + 4 + i] = wt[i]; }
    }
    const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
    for (int ch = lane; ch < s.C; ch += 64) {
        float t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = lat[(int64_t)o[i] * s.C + ch];
        zlat[row * s.C + ch] = __builtin_fmaf(t[3], wt[3], __builtin_fmaf(t[2], wt[2], __builtin_fmaf(t[1], wt[1], t[0] * wt[0])));
    }
#endif
}

// ---- the transpose of point_inputs_gen_kernel to the geometric leaves (train.hip point_inputs_bwd_kernel for any F, ld_in, C) ---
constexpr int CAMG_COLS = 24;   // d_o 3, d_d 3, d_R 9 (row-major), d_t 3, d_focal 2, d_c 2, d_image_shape 2
constexpr int CAMG_BLOCKS = 256;   // per-view partial sums of the pose / intrinsics reduction (at most)

// ATen's clip_coordinates_set_grad + reflect_coordinates_set_grad (align_corners=False)
__device__ __forceinline__ float pad_coord_grad(float x, int size, int padding, float &g)
{
    g = 1.0f;
    if (padding == DINER_INDEX_PAD_REFLECTION) {
        float in = x + 0.5f;                  // reflect over [-0.5, size - 0.5]
        float m = 1.0f;
        if (in < 0.0f) { m = -1.0f; in = -in; }
        const float span = (float)size, extra = fmodf(in, span);
        const int flips = (int)floorf(in / span);
        if (flips % 2 == 0) { g = m; x = extra - 0.5f; }
        else { g = -m; x = span - extra - 0.5f; }
    }
    if (padding != DINER_INDEX_PAD_ZEROS) {
        if (x <= 0.0f || x >= (float)(size - 1)) g = 0.0f;
        x = clipf(x, (float)(size - 1));
    }
    return x;
}

__global__ __launch_bounds__(64) void point_inputs_bwd_gen_kernel(DinerScene s, const float *__restrict__ latent_nhwc,
                                                                  const float *__restrict__ rays, const float *__restrict__ zsamp,
                                                                  int64_t NR, int K, int sb, int ix_interp, int ix_padding,
                                                                  const float *__restrict__ d_in, int64_t ld_in,
                                                                  const float *__restrict__ d_zlat, float *__restrict__ rowg,
                                                                  float *__restrict__ d_depths)
{
    const int64_t P = NR * (int64_t)K, row = blockIdx.x;
    const int v = (int)(row / P);
    const int64_t p = row - (int64_t)v * P;
    const int lane = threadIdx.x;
    const float *rp = rays + ((int64_t)sb * NR + p / K) * 8;
    const float zz = zsamp[(int64_t)sb * P + p];
    const float dwx = rp[3], dwy = rp[4], dwz = rp[5];
    const float wx = rp[0] + zz * dwx, wy = rp[1] + zz * dwy, wz = rp[2] + zz * dwz;  // nerf_renderer.py:304
    const View vw = load_view(s, sb, v);
    float px, py, pz, u, w;
    project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);                  // pixelnerf.py:91-93,105-108
    const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
    const int ddx = safe_idx(__builtin_rintf(clipf(unnorm(u, (float)s.W / 2.0f), (float)(s.W - 1))), s.W);
    const int ddy = safe_idx(__builtin_rintf(clipf(unnorm(w, (float)s.H / 2.0f), (float)(s.H - 1))), s.H);
    const float delta = tex[((int64_t)ddy * s.W + ddx) * 2].w - pz;

    // positional encodings: d sin(f a + phi) / d a = f cos(f a + phi) (positional_encoding.py:45-49); lanes stride the inputs,
    // each lane sums its own in a fixed order before the wave sums
    const float *gin = d_in + row * ld_in;
    const int F = s.num_freqs, e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1, d_in_n = e_pe1 + 2 * F;
    const float half_pi = 1.5707963267948966f;
    float t_p[4] = {0.f, 0.f, 0.f, 0.f};   // -> x_cam.x, x_cam.y, x_cam.z, depth_dist
    for (int e = lane; e < d_in_n; e += 64) {
        const float g = gin[e];
        if (e < 3) t_p[e] += g;
        else if (e < e_pe3) {
            const int j = (e - 3) / 3, i = (e - 3) % 3;
            const float f = ldexpf(s.freq_factor, j >> 1), a = i == 0 ? px : i == 1 ? py : pz;
            t_p[i] += g * cosf(__builtin_fmaf(a, f, (j & 1) ? half_pi : 0.0f)) * f;
        } else if (e == e_dir) t_p[3] += g;
        else if (e > e_dir) {
            const int j = e - e_pe1;
            const float f = ldexpf(s.freq_factor, j >> 1);
            t_p[3] += g * cosf(__builtin_fmaf(delta, f, (j & 1) ? half_pi : 0.0f)) * f;
        }
    }

    // grid_sample's gradient with respect to the grid (ATen, align_corners=False; nearest: 0)
    float gix = 0.f, giy = 0.f, mx = 0.f, my = 0.f;
#ifdef DINER_TRAIN_GEN_BC
    {   // bicubic: d/d ix = sum_ij dcx[i] cy[j] texel_ij, d/d iy = sum_ij cx[i] dcy[j] texel_ij; the padding acts on the integer tap
        // positions and puts no factor on the gradient (zeros: a tap outside the map has weight and derivative 0)
        const float sxl = ((float)s.w - s.feature_padding * 2.0f) / (float)s.w, syl = ((float)s.h - s.feature_padding * 2.0f) / (float)s.h;
        int xi[4], yi[4];
        float cx[4], cy[4], dcx[4], dcy[4];
        bicubic_axis(unnorm(u * sxl, (float)s.w / 2.0f), s.w, ix_padding, xi, cx, dcx);
        bicubic_axis(unnorm(w * syl, (float)s.h / 2.0f), s.h, ix_padding, yi, cy, dcy);
        mx = ((float)s.w / 2.0f) * sxl;   // d ix / d u
        my = ((float)s.h / 2.0f) * syl;
        const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
        const float *dz = d_zlat + row * s.C;
        for (int ch = lane * 4; ch < s.C; ch += 256) {   // C % 4 == 0
            const float4 g = *(const float4 *)(dz + ch);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float rx = 0.f, rd = 0.f;   // sum_i cx[i] <g, texel_ij>, sum_i dcx[i] <g, texel_ij>
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 t = *(const float4 *)(lat + ((int64_t)yi[j] * s.w + xi[i]) * s.C + ch);
                    const float d = g.x * t.x + g.y * t.y + g.z * t.z + g.w * t.w;
                    rx += cx[i] * d; rd += dcx[i] * d;
                }
                gix += cy[j] * rd; giy += dcy[j] * rx;
            }
        }
    }
#else
    if (ix_interp == DINER_INDEX_BILINEAR) {
        const float sxl = ((float)s.w - s.feature_padding * 2.0f) / (float)s.w, syl = ((float)s.h - s.feature_padding * 2.0f) / (float)s.h;
        float gx, gy;
        const float ix = pad_coord_grad(unnorm(u * sxl, (float)s.w / 2.0f), s.w, ix_padding, gx);
        const float iy = pad_coord_grad(unnorm(w * syl, (float)s.h / 2.0f), s.h, ix_padding, gy);
        mx = gx * ((float)s.w / 2.0f) * sxl;   // d ix / d u
        my = gy * ((float)s.h / 2.0f) * syl;
        const float x0f = floorf(ix), y0f = floorf(iy);
        const float fx = ix - x0f, ex = 1.0f - fx, fy = iy - y0f, ey = 1.0f - fy;
        const bool xa = x0f >= 0.0f && x0f <= (float)(s.w - 1), xb = x0f + 1.0f >= 0.0f && x0f + 1.0f <= (float)(s.w - 1);
        const bool ya = y0f >= 0.0f && y0f <= (float)(s.h - 1), yb = y0f + 1.0f >= 0.0f && y0f + 1.0f <= (float)(s.h - 1);
        const int x0 = safe_idx(x0f, s.w), x1 = safe_idx(x0f + 1.0f, s.w), y0 = safe_idx(y0f, s.h), y1 = safe_idx(y0f + 1.0f, s.h);
        const float kx[4] = {(xa && ya) ? -ey : 0.f, (xb && ya) ? ey : 0.f, (xa && yb) ? -fy : 0.f, (xb && yb) ? fy : 0.f};
        const float ky[4] = {(xa && ya) ? -ex : 0.f, (xb && ya) ? -fx : 0.f, (xa && yb) ? ex : 0.f, (xb && yb) ? fx : 0.f};
        const bool inm[4] = {xa && ya, xb && ya, xa && yb, xb && yb};
        const int o[4] = {y0 * s.w + x0, y0 * s.w + x1, y1 * s.w + x0, y1 * s.w + x1};
        const float *lat = latent_nhwc + ((int64_t)sb * s.NV + v) * (int64_t)s.h * s.w * s.C;
        const float *dz = d_zlat + row * s.C;
        for (int ch = lane * 4; ch < s.C; ch += 256) {   // C % 4 == 0
            const float4 g = *(const float4 *)(dz + ch);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!inm[i]) continue;   // (wave-uniform)
                const float4 t = *(const float4 *)(lat + (int64_t)o[i] * s.C + ch);
                const float d = g.x * t.x + g.y * t.y + g.z * t.z + g.w * t.w;
                gix += kx[i] * d; giy += ky[i] * d;
            }
        }
    }
#endif
    const float S0 = wave_sum(t_p[0]), S1 = wave_sum(t_p[1]), S2 = wave_sum(t_p[2]), Sd = wave_sum(t_p[3]);
    gix = wave_sum(gix); giy = wave_sum(giy);
    if (lane != 0) return;

    if (d_depths) atomicAdd(d_depths + (((int64_t)sb * s.NV + v) * s.H + ddy) * s.W + ddx, Sd);   // the nearest depth texel
    float gpx = S0, gpy = S1, gpz = S2 - Sd;                 // depth_dist = depth - x_cam.z
    const float qu = px / pz, qw = py / pz;
    const float Uu = qu * vw.fx + vw.cx, Uw = qw * vw.fy + vw.cy;
    const float gu = gix * mx, gw = giy * my;
    const float gUu = gu * 2.0f / s.image_w, gUw = gw * 2.0f / s.image_h;
    const float g_iw = -gu * 2.0f * Uu / (s.image_w * s.image_w), g_ih = -gw * 2.0f * Uw / (s.image_h * s.image_h);
    const float gqu = gUu * vw.fx, gqw = gUw * vw.fy;
    gpx += gqu / pz; gpy += gqw / pz; gpz -= (gqu * qu + gqw * qw) / pz;
    // x_cam = R x_w + t, dir_cam = R d_w (pixelnerf.py:92-101), x_w = o + z d (nerf_renderer.py:304-305)
    const float gp[3] = {gpx, gpy, gpz}, gd[3] = {gin[e_pe3], gin[e_pe3 + 1], gin[e_pe3 + 2]}, xw[3] = {wx, wy, wz}, dw[3] = {dwx, dwy, dwz};
    float *out = rowg + row * CAMG_COLS;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float gx = vw.r[j] * gp[0] + vw.r[3 + j] * gp[1] + vw.r[6 + j] * gp[2];
        const float gdd = vw.r[j] * gd[0] + vw.r[3 + j] * gd[1] + vw.r[6 + j] * gd[2];
        out[j] = gx;                      // d_o
        out[3 + j] = gdd + zz * gx;       // d_d
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[6 + i * 3 + j] = gp[i] * xw[j] + gd[i] * dw[j];
        out[15 + i] = gp[i];
    }
    out[18] = gUu * qu; out[19] = gUw * qw;   // focal
    out[20] = gUu; out[21] = gUw;             // c
    out[22] = g_iw; out[23] = g_ih;           // image_shape
}

#ifdef DINER_TRAIN_GEN_BC
#undef point_inputs_gen_kernel
#undef point_inputs_bwd_gen_kernel
#endif

#ifndef DINER_TRAIN_GEN_BC
// The fixed-order reductions of the per-row records (train.hip's camg_* kernels, the same sums in the same order)
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
#else
// d_lat_nhwc[v][texel (x[i], y[j])][ch] += dz[row][ch] * cx[i] * cy[j] over the 16 taps of each row's record (grid_sample's input
// gradient; float atomics on 256-byte contiguous rows, as train.hip's bilinear_scatter_kernel).  One wave walks SCATTER_RUN consecutive
// rows (consecutive samples of a ray in one view, whose footprints move by a fraction of a texel per sample): contributions are summed
// in registers while the 4 columns and 4 rows stay the same and flushed with one atomic per tap when they change.  A tap of weight 0
// (zeros padding outside the map) adds nothing and is never flushed.  Several taps of one footprint may be the same texel (border /
// reflection at the rim, maps smaller than the footprint): the atomics add them up.
constexpr int SCATTER_RUN = 16;
__global__ __launch_bounds__(64) void bicubic_scatter_kernel(const float *__restrict__ dz, const float *__restrict__ taps, int64_t P, int C,
                                                             int h, int w, int NV, int sb, float *__restrict__ dlatent_nhwc)
{
    const int64_t R = P * NV, row0 = (int64_t)blockIdx.x * SCATTER_RUN;
    const int64_t row1 = row0 + SCATTER_RUN < R ? row0 + SCATTER_RUN : R;
    const int lane = threadIdx.x;
    for (int ch = lane; ch < C; ch += 64) {
        int cur[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // x[4], y[4] of the open run
        int64_t cur_v = -1;
        float acc[16];
        unsigned used = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.f;
        for (int64_t row = row0; row <= row1; ++row) {
            const bool last = row == row1;
            const int64_t v = last ? -1 : row / P;
            int o[8];
            bool same = !last && v == cur_v;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                o[i] = last ? -1 : __float_as_int(taps[row * 16 + i]);
                if (!last) { const int hi = (i < 4 ? w : h) - 1; o[i] = o[i] < 0 ? 0 : (o[i] > hi ? hi : o[i]); }   // never outside the map
                same = same && o[i] == cur[i];
            }
            if (!same) {  // wave-uniform
                if (cur_v >= 0 && used) {
                    float *lat = dlatent_nhwc + ((int64_t)sb * NV + cur_v) * h * w * C + ch;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (used >> (j * 4 + i) & 1u) atomicAdd(lat + ((int64_t)cur[4 + j] * w + cur[i]) * C, acc[j * 4 + i]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) cur[i] = o[i];
#pragma unroll
                for (int t = 0; t < 16; ++t) acc[t] = 0.f;
                used = 0;
                cur_v = v;
            }
            if (last) break;
            const float g = dz[row * C + ch];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gy = g * taps[row * 16 + 12 + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float wx = taps[row * 16 + 8 + i];
                    if (wx != 0.0f && taps[row * 16 + 12 + j] != 0.0f) { acc[j * 4 + i] += gy * wx; used |= 1u << (j * 4 + i); }
                }
            }
        }
    }
}
#endif  // DINER_TRAIN_GEN_BC

}  // namespace train_gen

#ifndef DINER_TRAIN_GEN_BC
int launch_train_camg_reduce(const float *, float *, int64_t, int, int, int, const float *, float *, float *, float *, float *, float *,
                             hipStream_t);

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
    hipLaunchKernelGGL(train_gen::point_inputs_gen_kernel, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, ix.interp,
                       ix.padding, in, ld_in, zlat, taps);
    return check_launch("train_gen::point_inputs_gen_kernel");
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
    hipLaunchKernelGGL(point_inputs_bwd_gen_kernel, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, ix.interp,
                       ix.padding, d_in, ld_in, d_zlat, rowg, d_depths);
    int rc = check_launch("train_gen::point_inputs_bwd_gen_kernel");
    if (rc) return rc;
    return launch_train_camg_reduce(rowg, partial, NR, K, s.NV, sb, d_far, d_rays, d_poses, d_focal, d_c, d_image_shape, st);
}

// the fixed-order reductions of the rowg records [R, CAMG_COLS] to the rays and the per-view camera gradients (also behind
// train_gen_bc.hip's backward)
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
#else   // DINER_TRAIN_GEN_BC
int launch_train_camg_reduce(const float *, float *, int64_t, int, int, int, const float *, float *, float *, float *, float *, float *,
                             hipStream_t);   // train_gen.hip

int launch_train_point_inputs_gen_bc(const DinerScene &s, int padding, const float *latent_nhwc, const float *rays, const float *z, int64_t NR,
                                     int K, int sb, float *in, int64_t ld_in, float *zlat, float *taps, hipStream_t st)
{
    const int64_t R = NR * (int64_t)K * s.NV;
    if (R == 0) return DINER_OK;
    hipLaunchKernelGGL(train_gen::point_inputs_gen_bc_kernel, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, 0, padding,
                       in, ld_in, zlat, taps);
    return check_launch("train_gen::point_inputs_gen_bc_kernel");
}

int launch_train_point_inputs_bwd_gen_bc(const DinerScene &s, int padding, const float *latent_nhwc, const float *rays, const float *z,
                                         int64_t NR, int K, int sb, const float *d_in, int64_t ld_in, const float *d_zlat, const float *d_far,
                                         float *workspace, float *d_rays, float *d_poses, float *d_focal, float *d_c, float *d_image_shape,
                                         float *d_depths, hipStream_t st)
{
    using namespace train_gen;
    const int64_t P = NR * (int64_t)K, R = P * s.NV;
    if (R == 0) return DINER_OK;
    float *rowg = workspace, *partial = workspace + R * CAMG_COLS;   // diner_train_camera_workspace_floats' layout
    hipLaunchKernelGGL(point_inputs_bwd_gen_bc_kernel, dim3((unsigned)R), dim3(64), 0, st, s, latent_nhwc, rays, z, NR, K, sb, 0, padding, d_in,
                       ld_in, d_zlat, rowg, d_depths);
    const int rc = check_launch("train_gen::point_inputs_bwd_gen_bc_kernel");
    if (rc) return rc;
    return launch_train_camg_reduce(rowg, partial, NR, K, s.NV, sb, d_far, d_rays, d_poses, d_focal, d_c, d_image_shape, st);
}

int launch_train_bicubic_scatter(const float *dz, const float *taps, int64_t P, int C, int h, int w, int NV, int sb, float *dlatent_nhwc,
                                 hipStream_t st)
{
    using namespace train_gen;
    if (P * NV == 0) return DINER_OK;
    hipLaunchKernelGGL(bicubic_scatter_kernel, dim3((unsigned)((P * NV + SCATTER_RUN - 1) / SCATTER_RUN)), dim3(64), 0, st, dz, taps, P, C, h, w, NV,
                       sb, dlatent_nhwc);
    return check_launch("train_gen::bicubic_scatter_kernel");
}
#endif  // DINER_TRAIN_GEN_BC

}  // namespace diner
