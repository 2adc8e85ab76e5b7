// The building blocks the training translation units share (train.hip, train_core.hip, train_gen.hip, train_gen_bc.hip,
// train_gen_f16.hip, train_novel.hip, train_gen_points.hpp): the operand tile loads of the fp32 and the f16x3 GEMMs, the XCD-aware block -> tile map, the
// fp16 hi / lo split and its LDS layout, the power-of-two operand scale, the activations and their derivatives, the GEMM epilogue, and
// the constants of the camera-gradient records.  One definition each: the kernels, their argument structs and the Softplus-aware tile
// stores stay in their units and namespaces.  Everything here is __forceinline__ device code or a constant, so a unit's code object
// holds exactly the kernels it defines.
#pragma once
#include <math.h>

#include "common.hpp"

namespace diner {

// the fixed-order reductions of the rowg records [R, CAMG_COLS] to the rays and the per-view camera gradients (train_gen.hip; behind
// every point-input backward: train.hip's, train_gen.hip's and train_gen_bc.hip's)
int launch_train_camg_reduce(const float *rowg, float *partial, int64_t NR, int K, int NV, int sb, const float *d_far, float *d_rays,
                             float *d_poses, float *d_focal, float *d_c, float *d_image_shape, hipStream_t st);

namespace train_blocks {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ---- camera / ray gradient records and the latent scatter ------------------------------------------------------------------------
constexpr int CAMG_COLS = 24;      // d_o 3, d_d 3, d_R 9 (row-major), d_t 3, d_focal 2, d_c 2, d_image_shape 2
constexpr int CAMG_BLOCKS = 256;   // per-view partial sums of the pose / intrinsics reduction (at most)
constexpr int SCATTER_RUN = 16;    // consecutive rows one wave of a latent scatter kernel walks, merging equal footprints

// ATen's clip_coordinates_set_grad + reflect_coordinates_set_grad (align_corners=False): the source coordinate of one axis after the
// padding mode, and the factor its gradient picks up on the way back (border: 0 where clipped; reflection: the sign flips)
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

// ---- activations (resnetfc.py:49-52,124-127) ---------------------------------------------------------------------------------------
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

// ---- block -> output tile -----------------------------------------------------------------------------------------------------------
// Workgroups are dealt round-robin to the 8 XCDs (id % 8), each with its own L2: the column blocks of one BM-row tile (they all read
// the same A tile, the big streamed operand) are given to consecutive workgroups of ONE XCD, so A leaves HBM once instead of once per
// column block.  lin: the workgroup's linear id (blockIdx.x, or what a split-K kernel re-dealt it to).
__device__ __forceinline__ void tile_of(int64_t M, int N, int bm, int bn, int64_t lin, int64_t &m0, int &n0)
{
    const int64_t gm = (M + bm - 1) / bm;
    const int gn = (N + bn - 1) / bn;
    const int64_t full = gm / 8 * 8;
    int64_t mt, nb;
    if (lin < full * gn) { const int64_t j = lin / 8; nb = j % gn; mt = j / gn * 8 + lin % 8; }
    else { const int64_t r = lin - full * gn; mt = full + r / gn; nb = r % gn; }
    m0 = mt * bm;
    n0 = (int)nb * bn;
}

// ---- fp32 GEMMs: one operand tile (128 x 16, as [k][m]) = 512 float4, two per thread -------------------------------------------------
// KC: the operand is contiguous along the contraction index (float4 along k, transposed into the tile), else along the tile's long
// index.  Loads are unconditional (out-of-range pieces read a clamped in-range address and are zeroed by `ok` when the tile is
// stored): a load under a branch makes hipcc wait for each one separately.
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

// ---- f16x3 GEMMs (fp32-grade fp16 arithmetic: hi/lo split, 3 MFMAs per product) --------------------------------------------------------
// LDS image of an operand tile: 16-byte units (u = k/8, row) at u*128 + (row ^ 4u); an MFMA fragment (8 consecutive k of one row) is one
// conflict-free ds_read_b128
__device__ __forceinline__ int unit(int u, int row) { return u * 128 + (row ^ (4 * u)); }

// LDS slot of tile row l for an operand staged by a transposing store (tile_store<false> of the f16x3 kernels): the 4 x 4 index
// transpose inside every 16-row block (an involution), which makes that store conflict-free; the accumulator rows / columns come out in
// slot order and are mapped back by epilogue<PA, PB>.
__device__ __forceinline__ int slot16(int x) { return (x & ~15) | ((x & 3) << 2) | ((x >> 2) & 3); }

// The power of two an operand is multiplied by before the fp16 hi/lo split (s) and its inverse: 2^static_exp, or -- when amax points
// at a device word holding the bit pattern of max|operand| (diner_train_amax) -- the one that maps that maximum into [2^13, 2^14)
__device__ __forceinline__ void scale_of(const unsigned int *amax, int static_exp, float &s, float &inv)
{
    int e = static_exp;
    if (amax) {
        const unsigned int b = *amax;
        const int ex = (int)((b >> 23) & 0xffu) - 127;
        e = (b == 0u) ? 0 : 13 - ex;
    }
    e = e < -100 ? -100 : e > 100 ? 100 : e;
    s = __uint_as_float((unsigned int)(127 + e) << 23);
    inv = __uint_as_float((unsigned int)(127 - e) << 23);
}

// One streamed operand tile = 128 (long index l) x 32 (k) fp32 = 1024 float4, four per thread.
// KC (contiguous along k): float4 along k.  else: a 4(k) x 4(l) micro-tile per thread, float4 along l.
template <bool KC>
__device__ __forceinline__ unsigned tile_load(f32x4 (&v)[4], const float *__restrict__ base, int64_t s_long, int64_t s_k, int64_t l0,
                                              int64_t l_end, int64_t k0, int64_t k_end, int tid)
{
    unsigned ok = 0;  // unconditional loads from clamped addresses + a validity bit per piece (see the fp32 tile_load)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (KC) {
            const int idx = tid + 256 * i;
            const int64_t l = l0 + (idx >> 3), k = k0 + (idx & 7) * 4;
            ok |= (unsigned)(l < l_end && k < k_end) << i;
            v[i] = *(const f32x4 *)(base + (l < l_end ? l : l_end - 1) * s_long + (k < k_end ? k : k_end - 4));
        } else {
            // thread = (k-quad kq4 of 8, l-quad lq4 of 32); a 16-lane group = 4 k-quads x 4 consecutive l-quads (see the units' tile_store)
            const int kq4 = (tid & 3) | ((tid >> 4) & 4), lq4 = ((tid >> 2) & 15) | ((tid >> 3) & 16);
            const int64_t k = k0 + kq4 * 4 + i, l = l0 + lq4 * 4;
            ok |= (unsigned)(k < k_end && l < l_end) << i;
            v[i] = *(const f32x4 *)(base + (k < k_end ? k : k_end - 1) * s_k + (l < l_end ? l : l_end - 4));
        }
    }
    return ok;
}

// (x * sc, floored) -> fp16 hi / lo pairs: hi = cvt_pk(t), lo = fma_mix(hi * -1 + t) rounded once to fp16 = (f16)(t - (float)hi) (the
// difference is exact in fp32).  2.5 VALU slots per value (4.5 with the relu) where the C++ form costs hipcc about 8: scalar converts
// both ways, v_pack; in the dW kernel that split, not the MFMAs, was the longest phase of a k-step.
// RELU keeps NaN like torch.relu: v_cmp_ngt + v_cndmask, the 4 compares ahead of the 4 selects (gfx950: 2 wait states between a VALU
// write of an SGPR and its VALU read).
template <bool RELU>
__device__ __forceinline__ void split4_pk(float x0, float x1, float x2, float x3, float sc, unsigned &h01, unsigned &h23, unsigned &l01, unsigned &l23)
{
    float t0, t1, t2, t3;
    if constexpr (RELU) {
        unsigned long long m0, m1, m2, m3;
        asm volatile("v_mul_f32 %4, %12, %16\n\tv_mul_f32 %5, %13, %16\n\tv_mul_f32 %6, %14, %16\n\tv_mul_f32 %7, %15, %16\n\t"
                     "v_cmp_ngt_f32_e64 %8, 0, %4\n\tv_cmp_ngt_f32_e64 %9, 0, %5\n\tv_cmp_ngt_f32_e64 %10, 0, %6\n\tv_cmp_ngt_f32_e64 %11, 0, %7\n\t"
                     "v_cndmask_b32_e64 %4, 0, %4, %8\n\tv_cndmask_b32_e64 %5, 0, %5, %9\n\tv_cndmask_b32_e64 %6, 0, %6, %10\n\tv_cndmask_b32_e64 %7, 0, %7, %11\n\t"
                     "v_cvt_pk_f16_f32 %0, %4, %5\n\tv_cvt_pk_f16_f32 %1, %6, %7\n\t"
                     "v_fma_mixlo_f16 %2, %0, -1.0, %4 op_sel_hi:[1,0,0]\n\tv_fma_mixlo_f16 %3, %1, -1.0, %6 op_sel_hi:[1,0,0]\n\t"
                     "v_fma_mixhi_f16 %2, %0, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\tv_fma_mixhi_f16 %3, %1, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                     : "=&v"(h01), "=&v"(h23), "=&v"(l01), "=&v"(l23), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
                     : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(sc));
    } else {
        asm volatile("v_mul_f32 %4, %8, %12\n\tv_mul_f32 %5, %9, %12\n\tv_mul_f32 %6, %10, %12\n\tv_mul_f32 %7, %11, %12\n\t"
                     "v_cvt_pk_f16_f32 %0, %4, %5\n\tv_cvt_pk_f16_f32 %1, %6, %7\n\t"
                     "v_fma_mixlo_f16 %2, %0, -1.0, %4 op_sel_hi:[1,0,0]\n\tv_fma_mixlo_f16 %3, %1, -1.0, %6 op_sel_hi:[1,0,0]\n\t"
                     "v_fma_mixhi_f16 %2, %0, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\tv_fma_mixhi_f16 %3, %1, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                     : "=&v"(h01), "=&v"(h23), "=&v"(l01), "=&v"(l23), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                     : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(sc));
    }
}

// four consecutive k of tile row l (x sc, relu'd if relu: wave-uniform; NaN stays NaN) -> the hi and lo images
__device__ __forceinline__ void put4(h8 *Thi, h8 *Tlo, int l, int kq, float x0, float x1, float x2, float x3, bool relu, float sc)
{
    u32x2 hi, lo;
    unsigned a, b, c, d;
    if (relu) split4_pk<true>(x0, x1, x2, x3, sc, a, b, c, d);
    else split4_pk<false>(x0, x1, x2, x3, sc, a, b, c, d);
    hi.x = a; hi.y = b; lo.x = c; lo.y = d;
    const int o = unit(kq >> 3, l) * 8 + (kq & 4);
    *(u32x2 *)((_Float16 *)Thi + o) = hi;
    *(u32x2 *)((_Float16 *)Tlo + o) = lo;
}

// ---- the epilogue of the 128 x 128 GEMM kernels (4 waves as 2 x 2, each 2 x 2 MFMA tiles of 32 x 32) ---------------------------------
// C[m][n] = (old C +) deriv(acc * unscale + bias[n], S[m][n]), stored or added atomically.  g: the kernel's GemmArgs (bias, S, C, M, N,
// ldc, lds_, accumulate, atomic); bz: the workgroup's split-K index (the bias is added where it is 0); deriv(v, s): the derivative of the
// activation that produced S, applied as the kernel applies it (s = 1 where there is no S).
// C layout of the 32x32 MFMA accumulators: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)
// PA / PB: the A / B operand tile was staged in slot order (rows / columns of the tile permuted by slot16)
template <bool PA, bool PB, class Args, class Deriv>
__device__ __forceinline__ void epilogue(const Args &g, const f32x16 (&acc)[2][2], int64_t m0, int n0, int wm, int wn, int lane, int64_t bz,
                                         float unscale, Deriv deriv)
{
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const int nc = wn + tb * 32 + (lane & 31), n = n0 + (PB ? slot16(nc) : nc);
        if (n >= g.N) continue;
        const float bias = (g.bias && bz == 0) ? g.bias[n] : 0.0f;
#pragma unroll
        for (int ta = 0; ta < 2; ++ta) {
            // all 16 reads of the tile (old C, S) are issued before the first dependent store: one memory round trip per tile
            // instead of one per element
            const int mbl = wm + ta * 32 + 4 * (lane >> 5);
            auto row_of = [&](int i) -> int64_t { const int r = mbl + (i & 3) + 8 * (i >> 2); return m0 + (PA ? slot16(r) : r); };
            float old[16], msk[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { old[i] = 0.0f; msk[i] = 1.0f; }
            if (g.accumulate && !g.atomic) {  // uniform branches, unconditional loads from clamped rows
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t m = row_of(i);
                    old[i] = g.C[(m < g.M ? m : g.M - 1) * g.ldc + n];
                }
            }
            if (g.S) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int64_t m = row_of(i);
                    msk[i] = g.S[(m < g.M ? m : g.M - 1) * g.lds_ + n];
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t m = row_of(i);
                if (m >= g.M) continue;
                float v = acc[ta][tb][i] * unscale + bias;
                v = deriv(v, msk[i]);
                float *c = g.C + m * g.ldc + n;
                if (g.atomic) atomicAdd(c, v);
                else *c = old[i] + v;
            }
        }
    }
}

}  // namespace train_blocks
}  // namespace diner
