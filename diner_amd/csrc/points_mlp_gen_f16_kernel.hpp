// Device code of the shape-general f16x3 point/MLP kernels (points_mlp_gen_f16.hip has the description): the packed weight layout, the
// LDS A image, the split-fp16 MFMA GEMM, the tap records, the building blocks every kernel of the family is made of (tap_of,
// store_input_plane, resnet_block, finish; the view geometry, the input columns and the tile order are common.hpp's), the kernel
// template and its launcher.  Each kernel shows its inputs, its per-point records, the view loop (input stage, lin_in, gather,
// resnet_block) and the finish; the gathers stay in the kernels.  One lookup mode = one instantiation of
// the template, each in a translation unit of its own (points_mlp_gen_f16.hip and points_mlp_gen_f16_{ix,bc,lz,lz_bc}.hip).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace diner {
namespace genf16 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE_P = 64;                     // points per workgroup
constexpr int NWAVES = 8;                      // waves per workgroup
constexpr int KMAX = 512;                      // columns of the LDS A image
constexpr int A_H8 = KMAX / 8 * 2 * TILE_P;    // 16-byte slots of the A image (8192 = 128 KiB)
constexpr float ACT_SCALE = 0.0625f;           // the hidden state, its inputs and the biases are carried * 2^-4

struct Layout {
    int H, NT;             // d_hidden, 32-feature tiles
    int din, nkb_in;       // d_in (7 + 8F), its k-blocks of 16
    int dlat, nkb_lat;     // d_latent, its k-blocks of 16 (d_latent % 16 == 8: the last block is half zeros)
    int nb, cl, nlz, nvb;  // n_blocks, combine_layer, lin_z layers = min(cl, nb), blocks evaluated per view = nlz
    int F;                 // num_freqs
    float beta;            // Softplus beta, 0 = ReLU
    int64_t w_in, w_z, w_h;                     // halfs of one layer of each kind
    int64_t off_in, off_z, off_fc0, off_fc1, halfs;   // in halfs
    int64_t off_bias, off_wout, total;          // in floats
    __host__ __device__ int bias_lin_in() const { return 0; }
    __host__ __device__ int bias_lin_z(int b) const { return (1 + b) * H; }
    __host__ __device__ int bias_fc0(int b) const { return (1 + nlz + b) * H; }
    __host__ __device__ int bias_fc1(int b) const { return (1 + nlz + nb + b) * H; }
    __host__ __device__ int bias_lin_out() const { return (1 + nlz + 2 * nb) * H; }
};

inline Layout layout_of(const DinerMlpShape &m)
{
    Layout L;
    L.H = m.d_hidden; L.NT = m.d_hidden / 32;
    L.din = m.d_in; L.nkb_in = (m.d_in + 15) / 16;
    L.dlat = m.d_latent; L.nkb_lat = (m.d_latent + 15) / 16;
    L.nb = m.n_blocks; L.cl = m.combine_layer; L.nlz = m.combine_layer < m.n_blocks ? m.combine_layer : m.n_blocks; L.nvb = L.nlz;
    L.F = m.num_freqs; L.beta = m.beta;
    L.w_in = (int64_t)L.NT * L.nkb_in * 1024;
    L.w_z = (int64_t)L.NT * L.nkb_lat * 1024;
    L.w_h = (int64_t)L.NT * (L.H / 16) * 1024;
    L.off_in = 0;
    L.off_z = L.off_in + L.w_in;
    L.off_fc0 = L.off_z + L.nlz * L.w_z;
    L.off_fc1 = L.off_fc0 + L.nb * L.w_h;
    L.halfs = L.off_fc1 + L.nb * L.w_h;
    L.off_bias = L.halfs / 2;
    L.off_wout = L.off_bias + (int64_t)(1 + L.nlz + 2 * L.nb) * L.H + 32;
    L.total = L.off_wout + 4 * (int64_t)L.H;
    return L;
}

__device__ __forceinline__ void split(float s, _Float16 &hi, _Float16 &lo)
{
    hi = (_Float16)s;
    lo = (_Float16)(s - (float)hi);
}

// 16-byte slot of (plane = k / 8, part, point) in the A image
__device__ __forceinline__ int a_slot(int plane, int part, int point) { return (plane * 2 + part) * TILE_P + point; }

// acc[tm][tn] += (W^T tile) x (A^T block) over k-blocks kb0 .. kb0 + nkb of the layer (A image plane 0 = the layer's column 16 kb0).
// Wl: packed layer of nkb_layer k-blocks per feature tile; this wave's tiles ct0 .. ct0 + CT - 1 (clamped to NT - 1), point blocks
// rb0 .. rb0 + RB - 1.
template <int RB, int CT>
__device__ __forceinline__ void gemm(f32x16 (&acc)[RB][CT], const h8 *A8, const h8 *__restrict__ Wl, int nkb_layer, int kb0, int nkb,
                                     int rb0, int ct0, int NT, int lane)
{
    const h8 *ap = A8 + a_slot(lane >> 5, 0, rb0 * 32 + (lane & 31));
    const h8 *bp[CT];
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) {
        const int t = ct0 + tn < NT ? ct0 + tn : NT - 1;
        bp[tn] = Wl + ((int64_t)t * nkb_layer + kb0) * 128 + lane;
    }
    h8 w_cur[CT][2], w_nxt[CT][2];
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) { w_cur[tn][0] = bp[tn][0]; w_cur[tn][1] = bp[tn][64]; }
#pragma unroll 2
    for (int kb = 0; kb < nkb; ++kb) {
        const int kn = kb + 1 < nkb ? kb + 1 : kb;  // last iteration re-loads (harmless, keeps the loop branch-free)
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) { w_nxt[tn][0] = bp[tn][kn * 128]; w_nxt[tn][1] = bp[tn][kn * 128 + 64]; }
        h8 a[RB][2];
#pragma unroll
        for (int tm = 0; tm < RB; ++tm) {
            a[tm][0] = ap[kb * 4 * TILE_P + 32 * tm];
            a[tm][1] = ap[kb * 4 * TILE_P + TILE_P + 32 * tm];
        }
#pragma unroll
        for (int tn = 0; tn < CT; ++tn)
#pragma unroll
            for (int tm = 0; tm < RB; ++tm) {   // a_hi w_hi + a_hi w_lo + a_lo w_hi, back to back on one accumulator
                acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_cur[tn][0], a[tm][0], acc[tm][tn], 0, 0, 0);
                acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_cur[tn][1], a[tm][0], acc[tm][tn], 0, 0, 0);
                acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w_cur[tn][0], a[tm][1], acc[tm][tn], 0, 0, 0);
            }
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) { w_cur[tn][0] = w_nxt[tn][0]; w_cur[tn][1] = w_nxt[tn][1]; }
    }
}

// accumulator register i of lane half h is feature 32 tile + 8 (i >> 2) + 4 h + (i & 3) of point lane & 31 (the 32x32 C/D layout,
// transposed product)
template <int RB, int CT>
__device__ __forceinline__ void acc_bias(f32x16 (&acc)[RB][CT], const float *__restrict__ bias, bool add, int ct0, int NT, int lane)
{
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) {
        const int t = ct0 + tn < NT ? ct0 + tn : NT - 1;
        const f32x4 *bq = (const f32x4 *)(bias + t * 32 + 4 * (lane >> 5));
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 b = bq[2 * g];
#pragma unroll
            for (int tm = 0; tm < RB; ++tm)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[tm][tn][4 * g + j] = add ? acc[tm][tn][4 * g + j] + b[j] : b[j];
        }
    }
}

// the activation of a value carried * 2^-4: ReLU keeps NaN, like torch.relu; Softplus(beta) as torch evaluates it on the unscaled
// value (x * beta > 20: linear), scaled back
__device__ __forceinline__ float act(float v, float beta)
{
    if (beta > 0.0f) {
        const float xb = v * (1.0f / ACT_SCALE) * beta;
        return xb > 20.0f ? v : log1pf(expf(xb)) / beta * ACT_SCALE;
    }
    return v < 0.0f ? 0.0f : v;
}

__device__ __forceinline__ unsigned pack2(_Float16 a, _Float16 b)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 v = {a, b};
    return __builtin_bit_cast(unsigned, v);
}

// act(acc) -> LDS A image, split hi / lo: this wave's features become k = 32 tile + .. of the next layer (resnetfc.py:62-63,158).
// Register runs g = 2 gp and 2 gp + 1 of the two lane halves are exchanged (v_permlane32_swap) so that lanes 0-31 hold the 8
// features of plane 4 tile + 2 gp and lanes 32-63 those of plane 4 tile + 2 gp + 1.
template <int RB, int CT>
__device__ __forceinline__ void store_act(const f32x16 (&acc)[RB][CT], u32x4 *A, float beta, int rb0, int ct0, int NT, int lane)
{
    const int h = lane >> 5;
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) {
        if (ct0 + tn >= NT) continue;
#pragma unroll
        for (int tm = 0; tm < RB; ++tm) {
            const int point = (rb0 + tm) * 32 + (lane & 31);
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                unsigned p[2][2][2];   // [run 2 gp + e][part][dword]
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    _Float16 hi[4], lo[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) split(act(acc[tm][tn][8 * gp + 4 * e + j], beta), hi[j], lo[j]);
                    p[e][0][0] = pack2(hi[0], hi[1]); p[e][0][1] = pack2(hi[2], hi[3]);
                    p[e][1][0] = pack2(lo[0], lo[1]); p[e][1][1] = pack2(lo[2], lo[3]);
                }
#pragma unroll
                for (int part = 0; part < 2; ++part) {
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        const auto r = __builtin_amdgcn_permlane32_swap(p[0][part][d], p[1][part][d], false, false);
                        p[0][part][d] = r[0]; p[1][part][d] = r[1];
                    }
                    const u32x4 v = {p[0][part][0], p[0][part][1], p[1][part][0], p[1][part][1]};
                    A[a_slot((ct0 + tn) * 4 + 2 * gp + h, part, point)] = v;
                }
            }
        }
    }
}

struct Tap {        // footprint of one (point, view) in the latent map
    int o00, o01, o10, o11;  // float4 offsets of the 4 texels (clamped, always readable)
    float nw, ne, sw, se;    // weights * 2^-4; a tap outside the map has its weight forced to 0
};

struct TapBc {      // bicubic footprint of one (point, view) in the latent map (common.hpp BicubicFoot), 64 bytes
    int xo[4], yo[4];        // float4 offsets of the 4 columns (x * c4) and the 4 rows (y * w * c4); texel (i, j) = xo[i] + yo[j]
    float cx[4], cy[4];      // weights per axis, cy * 2^-4; zeros padding: 0 for a column / row outside the map
};

// ---- building blocks of the kernels: points_mlp_gen_f16_kernel below and the forms of it that units of their own define ----
// the Tap of a 4-tap footprint in a map lw texels wide, c4 float4 per texel; the weights * 2^-4
__device__ __forceinline__ Tap tap_of(const LatentFoot &f, int lw, int c4)
{
    Tap t;
    t.o00 = (f.y0 * lw + f.x0) * c4; t.o01 = (f.y0 * lw + f.x1) * c4;
    t.o10 = (f.y1 * lw + f.x0) * c4; t.o11 = (f.y1 * lw + f.x1) * c4;
    t.nw = f.nw * ACT_SCALE; t.ne = f.ne * ACT_SCALE; t.sw = f.sw * ACT_SCALE; t.se = f.se * ACT_SCALE;
    return t;
}

// the 8 values of one point in one plane -> the plane's hi and lo 16-byte slots
__device__ __forceinline__ void split8(const float (&v)[8], u32x4 &vh, u32x4 &vl)
{
    unsigned ph[4], plo[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        _Float16 hi[2], lo[2];
        split(v[2 * jj], hi[0], lo[0]); split(v[2 * jj + 1], hi[1], lo[1]);
        ph[jj] = pack2(hi[0], hi[1]); plo[jj] = pack2(lo[0], lo[1]);
    }
    vh = u32x4{ph[0], ph[1], ph[2], ph[3]}; vl = u32x4{plo[0], plo[1], plo[2], plo[3]};
}

// plane pl of a point's MLP inputs (columns 8 pl .. 8 pl + 7 of the layout pixelnerf.py:128, * 2^-4, split hi / lo) -> A
__device__ __forceinline__ void store_input_plane(u32x4 *A, int pl, int row, float px, float py, float pz, float dcx, float dcy, float dcz,
                                                  float delta, int F, float freq_factor)
{
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = input_element(pl * 8 + j, px, py, pz, dcx, dcy, dcz, delta, F, freq_factor) * ACT_SCALE;
    u32x4 vh, vl;
    split8(v, vh, vl);
    A[a_slot(pl, 0, row)] = vh;
    A[a_slot(pl, 1, row)] = vl;
}

// ResNet block b on the hidden state x (resnetfc.py:62-69): x = x + fc_1(act(fc_0(act(x)))).  The A image must be free on entry and
// is free on return (four barriers).
template <int RB, int CT>
__device__ __forceinline__ void resnet_block(f32x16 (&x)[RB][CT], u32x4 *A, const float *__restrict__ Wp, const Layout &L, int b, int rb0,
                                             int ct0, int lane)
{
    const h8 *A8 = (const h8 *)A, *Wh = (const h8 *)Wp;
    const float *bias = Wp + L.off_bias;
    const int NT = L.NT, H = L.H;
    f32x16 net[RB][CT];
    store_act(x, A, L.beta, rb0, ct0, NT, lane);                                                    // :62 fc_0(act(x))
    __syncthreads();
    acc_bias(net, bias + L.bias_fc0(b), false, ct0, NT, lane);
    gemm(net, A8, Wh + (L.off_fc0 + b * L.w_h) / 8, H / 16, 0, H / 16, rb0, ct0, NT, lane);
    __syncthreads();
    store_act(net, A, L.beta, rb0, ct0, NT, lane);                                                  // :63 fc_1(act(net))
    __syncthreads();
    acc_bias(x, bias + L.bias_fc1(b), true, ct0, NT, lane);                                         // :69 x + dx
    gemm(x, A8, Wh + (L.off_fc1 + b * L.w_h) / 8, H / 16, 0, H / 16, rb0, ct0, NT, lane);
    __syncthreads();
}

// what follows the view loop: combine() = the mean of the per-view states xsum over NV views (resnetfc.py:146-149), the blocks after
// combine_layer, lin_out (:158) and the head (pixelnerf.py:139-143: sigmoid rgb, ReLU sigma) -> rgbsigma [SB,P,4], points of the tail
// tile past P masked
template <int RB, int CT>
__device__ __forceinline__ void finish(f32x16 (&xsum)[RB][CT], u32x4 *A, const float *__restrict__ Wp, const Layout &L, int NV, int rb0,
                                       int ct0, int tid, int sb, int64_t tile, int64_t P, float *__restrict__ rgbsigma)
{
    const int lane = tid & 63, wave = tid >> 6;
    const float *bias = Wp + L.off_bias;
    const int NT = L.NT, H = L.H;
    {   // combine(): mean over views (combine_layer >= n_blocks: NV = 1 and this divides by 1, i.e. is exact)
        const float nv = (float)NV;
#pragma unroll
        for (int tm = 0; tm < RB; ++tm)
#pragma unroll
            for (int tn = 0; tn < CT; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) xsum[tm][tn][i] = xsum[tm][tn][i] / nv;
    }
    for (int b = L.nvb; b < L.nb; ++b) resnet_block(xsum, A, Wp, L, b, rb0, ct0, lane);
    // ---- lin_out(act(x)) (:158) in fp32 on the VALU: every lane's partial dot products over its own features -> LDS (the A image is
    // free: the barrier above), [slot = 2 (tile group) + h][point][4]; a tile group past NT contributes zeros ----------------------
    float *red = (float *)A;
    const float *wout = Wp + L.off_wout;
    const int h = lane >> 5, grp = RB == 2 ? wave : (wave >> 1);
#pragma unroll
    for (int tm = 0; tm < RB; ++tm) {
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) {
            if (ct0 + tn >= NT) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float a[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = act(xsum[tm][tn][4 * g + j], L.beta);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f32x4 wq = *(const f32x4 *)(wout + c * H + (ct0 + tn) * 32 + 8 * g + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[c] = __builtin_fmaf(a[j], wq[j], o[c]);
                }
            }
        }
        const f32x4 ov = {o[0], o[1], o[2], o[3]};
        ((f32x4 *)red)[(grp * 2 + h) * TILE_P + (rb0 + tm) * 32 + (lane & 31)] = ov;
    }
    __syncthreads();
    if (tid < TILE_P * 4) {
        const int r = tid >> 2, c = tid & 3;
        const int ngrp = RB == 2 ? NWAVES : NWAVES / 2;   // <1,1>: the point block of r was written by the waves of its parity only
        float sum = 0.0f;
        for (int g = 0; g < 2 * ngrp; ++g) sum += red[(g * TILE_P + r) * 4 + c];
        const int64_t pp = tile * TILE_P + r;
        if (pp < P) {
            const float val = (sum + bias[L.bias_lin_out() + c]) * (1.0f / ACT_SCALE);
            rgbsigma[((int64_t)sb * P + pp) * 4 + c] = c < 3 ? 1.0f / (1.0f + expf(-val)) : (val < 0.0f ? 0.0f : val);
        }
    }
}

// ---- lookup modes -------------------------------------------------------------------------------------------------------------------
// The kernel's first template parameter, as in points_mlp_gen_kernel.hpp.  ix: the footprint of any 4-tap lookup (ix_interp / ix_padding,
// DINER_INDEX_*; common.hpp latent_footprint) instead of bilinear / border; bc: the 16-tap bicubic lookup (common.hpp bicubic_footprint)
// with the padding ix_padding; lz: the lin_z-map form, which gathers d_hidden channels of the fp32 maps M_b = W_b F of linz_maps_gen.hip
// through the same tap records and adds them, as they are, to the fp32 accumulators: no operand is split, and the maps are more exact
// than the split GEMM they replace.
template <bool IX, bool BC, bool LZ>
struct ModeOf {
    static constexpr bool ix = IX, bc = BC, lz = LZ;
    typedef std::conditional_t<BC, TapBc, Tap> tap;                     // a point's tap record in LDS
    static constexpr int TAP_SLOTS = sizeof(tap) / sizeof(u32x4);       // its 16-byte slots
};
struct Default : ModeOf<false, false, false> { static constexpr const char *name = "points_mlp_gen_f16_kernel<Default>"; };
struct Ix : ModeOf<true, false, false> { static constexpr const char *name = "points_mlp_gen_f16_kernel<Ix>"; };
struct Bc : ModeOf<true, true, false> { static constexpr const char *name = "points_mlp_gen_f16_kernel<Bc>"; };
struct Lz : ModeOf<true, false, true> { static constexpr const char *name = "points_mlp_gen_f16_kernel<Lz>"; };
struct LzBc : ModeOf<true, true, true> { static constexpr const char *name = "points_mlp_gen_f16_kernel<LzBc>"; };

constexpr int BC_ROW_UNROLL = 2;   // rows of the 4 x 4 bicubic footprint whose loads are in flight together in the gather

// Every mode takes the same arguments: Default reads neither ix_interp nor ix_padding, Bc / LzBc no ix_interp, only Lz / LzBc lzmaps.
template <class Mode, int RB, int CT>
__global__ __launch_bounds__(NWAVES * 64) void points_mlp_gen_f16_kernel(DinerScene s, Layout L, const float *__restrict__ Wp,
                                                                         const float *__restrict__ rays, const float *__restrict__ zsamp,
                                                                         int64_t NR, int K, float *__restrict__ rgbsigma, int ix_interp,
                                                                         int ix_padding, const float *__restrict__ lzmaps)
{
    typedef typename Mode::tap TapRec;
    __shared__ u32x4 lds[A_H8 + TILE_P * Mode::TAP_SLOTS];  // A image + one Tap (bicubic: one TapBc) per point
    u32x4 *A = lds;
    const h8 *A8 = (const h8 *)lds;
    TapRec *taps = (TapRec *)(lds + A_H8);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT, H = L.H;
    const int sb = blockIdx.y;
    const int64_t P = NR * (int64_t)K;
    const int64_t tile = xcd_tile(gridDim.x, blockIdx.x);
    const h8 *Wh = (const h8 *)Wp;
    const float *bias = Wp + L.off_bias;

    // ---- this thread's point: sample p of the scene, at o + z d on its ray ----------
    const int row = tid & 63;
    int64_t p = tile * TILE_P + row;
    if (p > P - 1) p = P - 1;  // tail tile: duplicate the last point, masked at the store
    const int64_t ray = p / K;
    const float *rp = rays + ((int64_t)sb * NR + ray) * 8;
    const float zz = zsamp[(int64_t)sb * P + p];
    const float dwx = rp[3], dwy = rp[4], dwz = rp[5];
    const float wx = rp[0] + zz * dwx, wy = rp[1] + zz * dwy, wz = rp[2] + zz * dwz;  // nerf_renderer.py:304

    f32x16 x[RB][CT], xsum[RB][CT];
    acc_zero(xsum);

    const float sxl = pad_scale(s.w, s.feature_padding), syl = pad_scale(s.h, s.feature_padding);
    const int F = L.F, e_pe3 = 3 + 6 * F, e_dir = e_pe3 + 3, e_pe1 = e_dir + 1;
    // float4 per texel the taps address.  lz: of a lin_z map, the latent itself is never read; else of the latent
    const int c4 = Mode::lz ? H / 4 : L.dlat / 4;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> planes 0 .. 2 nkb_in of A (a wave writes whole planes); footprint -> taps ----------
        {
            float px, py, pz, u, w;
            if constexpr (Mode::lz) {   // view_geometry + store_input_plane, written out: through input_element Lz<2,2> spills 123 VGPRs, not 122
                const View vw = load_view(s, sb, v);
                project(vw, s.image_w, s.image_h, wx, wy, wz, px, py, pz, u, w);   // pixelnerf.py:91-93,105-108
                float dcx, dcy, dcz;
                rotate(vw, dwx, dwy, dwz, dcx, dcy, dcz);                            // :99-101
                const float4 *tex = (const float4 *)s.maps + ((int64_t)sb * s.NV + v) * s.H * s.W * 2;
                const int ddx = safe_idx(__builtin_rintf(clipf(unnorm(u, (float)s.W / 2.0f), (float)(s.W - 1))), s.W);
                const int ddy = safe_idx(__builtin_rintf(clipf(unnorm(w, (float)s.H / 2.0f), (float)(s.H - 1))), s.H);
                const float delta = tex[((int64_t)ddy * s.W + ddx) * 2].w - pz;     // :114-115
                const float half_pi = 1.5707963267948966f;
                for (int pl = wave; pl < 2 * L.nkb_in; pl += NWAVES) {              // input layout :128
                    unsigned ph[4], plo[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        _Float16 hi[2], lo[2];
#pragma unroll
                        for (int j2 = 0; j2 < 2; ++j2) {
                            const int e = pl * 8 + jj * 2 + j2;
                            float val;
                            if (e < 3) val = e == 0 ? px : e == 1 ? py : pz;
                            else if (e < e_pe3) { const int j = (e - 3) / 3, i = (e - 3) % 3;    // positional_encoding.py:45-49
                                val = sinf(__builtin_fmaf(i == 0 ? px : i == 1 ? py : pz, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
                            else if (e < e_dir) val = e == e_pe3 ? dcx : e == e_pe3 + 1 ? dcy : dcz;
                            else if (e == e_dir) val = delta;
                            else if (e < e_pe1 + 2 * F) { const int j = e - e_pe1;
                                val = sinf(__builtin_fmaf(delta, ldexpf(s.freq_factor, j >> 1), (j & 1) ? half_pi : 0.0f)); }
                            else val = 0.0f;
                            split(val * ACT_SCALE, hi[j2], lo[j2]);
                        }
                        ph[jj] = pack2(hi[0], hi[1]); plo[jj] = pack2(lo[0], lo[1]);
                    }
                    const u32x4 vh = {ph[0], ph[1], ph[2], ph[3]}, vl = {plo[0], plo[1], plo[2], plo[3]};
                    A[a_slot(pl, 0, row)] = vh;
                    A[a_slot(pl, 1, row)] = vl;
                }
            } else {
                float dcx, dcy, dcz, delta;
                view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);   // pixelnerf.py:91-115
                for (int pl = wave; pl < 2 * L.nkb_in; pl += NWAVES)                                          // input layout :128
                    store_input_plane(A, pl, row, px, py, pz, dcx, dcy, dcz, delta, F, s.freq_factor);
            }
            if constexpr (Mode::bc) {
                if (wave == 0) {  // the 4 x 4 bicubic footprint in the latent map (image_encoder.py:97-127; common.hpp); the scale rides on cy
                    const BicubicFoot f = bicubic_footprint(u, w, sxl, syl, s.w, s.h, ix_padding);
                    TapBc t;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        t.xo[i] = f.x[i] * c4; t.yo[i] = f.y[i] * s.w * c4;
                        t.cx[i] = f.cx[i]; t.cy[i] = f.cy[i] * ACT_SCALE;
                    }
                    taps[row] = t;
                }
            } else {
                if (wave == 0)   // footprint of the lookup mode in the latent map (image_encoder.py:97-127; common.hpp)
                    taps[row] = tap_of(latent_footprint<Mode::ix>(u, w, sxl, syl, s.w, s.h, ix_interp, ix_padding), s.w, c4);
            }
        }
        __syncthreads();
        acc_bias(x, bias + L.bias_lin_in(), false, ct0, NT, lane);
        gemm(x, A8, Wh + L.off_in / 8, L.nkb_in, 0, L.nkb_in, rb0, ct0, NT, lane);                  // resnetfc.py:139
        __syncthreads();

        const f32x4 *lat = Mode::lz ? nullptr : (const f32x4 *)s.latent + ((int64_t)sb * s.NV + v) * s.h * s.w * c4;
        for (int b = 0; b < L.nvb; ++b) {
            acc_bias(x, bias + L.bias_lin_z(b), true, ct0, NT, lane);                               // :152-153 x = x + lin_z(z)
            if constexpr (Mode::lz) {
                // ---- (W_b z)[:, 0 : H] / 16 = the lookup of the 64 points in map M_b (the scale rides on the tap weights) -> LDS as fp32
                // [point][c4 quads], quad ^ (point & msk) so that the 16-byte reads of neighbouring points fall into different banks;
                // then every lane adds the 4 runs of 4 features per tile that its accumulators hold.  No operand image lives in the
                // 128 KiB meanwhile; while H <= 256 the staging area lies behind the planes store_act writes next, and no barrier is
                // needed between the adds and that store.
                const int msk = (c4 & 15) ? 7 : 15;
                const bool apart = 2 * H * TILE_P <= A_H8 * 4;
                f32x4 *S4 = (f32x4 *)lds + (apart ? H * TILE_P / 4 : 0);
                const f32x4 *mp = (const f32x4 *)lzmaps + (((int64_t)b * s.SB + sb) * s.NV + v) * s.h * s.w * c4;
                for (int idx = lane; idx < (TILE_P / NWAVES) * c4; idx += 64) {   // a wave gathers 8 points, c4 quads each
                    const int rr = idx / c4, q = idx - rr * c4, r = wave * (TILE_P / NWAVES) + rr;
                    f32x4 val;
                    if constexpr (Mode::bc) {
                        const TapBc *tp = taps + r;   // rows then columns, contracted FMAs: the gather of the bicubic kernel
                        const f32x4 *lq = mp + q;
                        const int x0 = tp->xo[0], x1 = tp->xo[1], x2 = tp->xo[2], x3 = tp->xo[3];
                        const float w0 = tp->cx[0], w1 = tp->cx[1], w2 = tp->cx[2], w3 = tp->cx[3];
#pragma unroll BC_ROW_UNROLL
                        for (int j = 0; j < 4; ++j) {
                            const f32x4 *lr = lq + tp->yo[j];
                            const float wy = tp->cy[j];
                            const f32x4 a = lr[x0], bb = lr[x1], c = lr[x2], d = lr[x3];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float rowv = __builtin_fmaf(d[i], w3, __builtin_fmaf(c[i], w2, __builtin_fmaf(bb[i], w1, a[i] * w0)));
                                val[i] = j == 0 ? rowv * wy : __builtin_fmaf(rowv, wy, val[i]);
                            }
                        }
                    } else {
                        const Tap t = taps[r];
                        const f32x4 a = mp[t.o00 + q], bb = mp[t.o01 + q], c = mp[t.o10 + q], d = mp[t.o11 + q];
#pragma unroll
                        for (int i = 0; i < 4; ++i) val[i] = tap_sum(a[i], bb[i], c[i], d[i], t);
                    }
                    S4[r * c4 + (q ^ (r & msk))] = val;
                }
                __syncthreads();
                const int h = lane >> 5;
#pragma unroll
                for (int tn = 0; tn < CT; ++tn) {
                    const int t = ct0 + tn < NT ? ct0 + tn : NT - 1;
#pragma unroll
                    for (int tm = 0; tm < RB; ++tm) {
                        const int point = (rb0 + tm) * 32 + (lane & 31);
                        const f32x4 *sp = S4 + point * c4;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 mv = sp[(8 * t + 2 * g + h) ^ (point & msk)];
#pragma unroll
                            for (int j = 0; j < 4; ++j) x[tm][tn][4 * g + j] += mv[j];
                        }
                    }
                }
                if (!apart) __syncthreads();
            } else {
                for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
                    // ---- z[:, k0 : k0 + kc] / 16 = the latent of the 64 points -> A: a wave gathers 8 points, a lane 8 columns of one ----
                    const int kc = L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX;
                    const int npl = (kc + 15) / 16 * 2;   // planes the GEMM reads (the last one zero when kc % 16 == 8)
                    const int r = wave * (TILE_P / NWAVES) + (lane & 7);
                    if constexpr (Mode::bc) {
                        // 16 texels per channel quad: sum_j cy[j] * (sum_i cx[i] * texel_ij) in fp32, rows then columns, contracted FMAs; the
                        // hi / lo split takes the SUM (the outer weights are negative and sum |w| > 1: splitting taps would cancel halves).
                        // The row loop is unrolled by BC_ROW_UNROLL only, as in points_mlp_gen.hip.
                        const TapBc *tp = taps + r;
                        const int x0 = tp->xo[0], x1 = tp->xo[1], x2 = tp->xo[2], x3 = tp->xo[3];
                        const float w0 = tp->cx[0], w1 = tp->cx[1], w2 = tp->cx[2], w3 = tp->cx[3];
                        for (int pl = lane >> 3; pl < npl; pl += 8) {
                            u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
                            if (pl * 8 < kc) {
                                unsigned ph[4], plo[4];
#pragma unroll
                                for (int half = 0; half < 2; ++half) {
                                    const f32x4 *lq = lat + (k0 / 4 + pl * 2 + half);
                                    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll BC_ROW_UNROLL
                                    for (int j = 0; j < 4; ++j) {
                                        const f32x4 *lr = lq + tp->yo[j];
                                        const float wy = tp->cy[j];
                                        const f32x4 a = lr[x0], bb = lr[x1], c = lr[x2], d = lr[x3];
#pragma unroll
                                        for (int i = 0; i < 4; ++i) {
                                            const float rowv = __builtin_fmaf(d[i], w3, __builtin_fmaf(c[i], w2, __builtin_fmaf(bb[i], w1, a[i] * w0)));
                                            acc[i] = j == 0 ? rowv * wy : __builtin_fmaf(rowv, wy, acc[i]);
                                        }
                                    }
                                    _Float16 hi[4], lo[4];
#pragma unroll
                                    for (int i = 0; i < 4; ++i) split(acc[i], hi[i], lo[i]);
                                    ph[2 * half] = pack2(hi[0], hi[1]); ph[2 * half + 1] = pack2(hi[2], hi[3]);
                                    plo[2 * half] = pack2(lo[0], lo[1]); plo[2 * half + 1] = pack2(lo[2], lo[3]);
                                }
                                vh = u32x4{ph[0], ph[1], ph[2], ph[3]}; vl = u32x4{plo[0], plo[1], plo[2], plo[3]};
                            }
                            A[a_slot(pl, 0, r)] = vh;
                            A[a_slot(pl, 1, r)] = vl;
                        }
                    } else {
                        const Tap t = taps[r];
                        for (int pl = lane >> 3; pl < npl; pl += 8) {
                            u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
                            if (pl * 8 < kc) {
                                unsigned ph[4], plo[4];
#pragma unroll
                                for (int half = 0; half < 2; ++half) {
                                    const int qq = k0 / 4 + pl * 2 + half;
                                    const f32x4 a = lat[t.o00 + qq], bb = lat[t.o01 + qq], c = lat[t.o10 + qq], d = lat[t.o11 + qq];
                                    _Float16 hi[4], lo[4];
#pragma unroll
                                    for (int i = 0; i < 4; ++i) split(tap_sum(a[i], bb[i], c[i], d[i], t), hi[i], lo[i]);
                                    ph[2 * half] = pack2(hi[0], hi[1]); ph[2 * half + 1] = pack2(hi[2], hi[3]);
                                    plo[2 * half] = pack2(lo[0], lo[1]); plo[2 * half + 1] = pack2(lo[2], lo[3]);
                                }
                                vh = u32x4{ph[0], ph[1], ph[2], ph[3]}; vl = u32x4{plo[0], plo[1], plo[2], plo[3]};
                            }
                            A[a_slot(pl, 0, r)] = vh;
                            A[a_slot(pl, 1, r)] = vl;
                        }
                    }
                    __syncthreads();
                    gemm(x, A8, Wh + (L.off_z + b * L.w_z) / 8, L.nkb_lat, k0 / 16, npl / 2, rb0, ct0, NT, lane);
                    __syncthreads();
                }
            }
            resnet_block(x, A, Wp, L, b, rb0, ct0, lane);
        }
        acc_add(xsum, x);                                                                           // :146-149
    }
    finish(xsum, A, Wp, L, s.NV, rb0, ct0, tid, sb, tile, P, rgbsigma);
}
// ---- launch ---------------------------------------------------------------------------------------------------------------------------
struct Launch {   // what a validated call passes to a mode's launcher (points_mlp_gen_f16.hip validate())
    const DinerScene *s;
    Layout L;
    int ix_interp, ix_padding;   // DINER_INDEX_*; bicubic: ix_padding only
    const float *mlp_packed, *rays, *z;
    int64_t NR;
    int K;
    float *rgbsigma;
    const float *lzmaps;         // Lz / LzBc, else null
    hipStream_t st;
};

// the instantiation a d_hidden runs on: <1,1> for up to 128 features, <2,1> up to 256, <2,2> up to 512
template <class Mode>
int launch_mode(const Launch &a)
{
    const dim3 grid((unsigned)((a.NR * (int64_t)a.K + TILE_P - 1) / TILE_P), (unsigned)a.s->SB), block(NWAVES * 64);
    void (*const kernel)(DinerScene, Layout, const float *, const float *, const float *, int64_t, int, float *, int, int, const float *) =
        a.L.H <= 128   ? points_mlp_gen_f16_kernel<Mode, 1, 1>
        : a.L.H <= 256 ? points_mlp_gen_f16_kernel<Mode, 2, 1>
                       : points_mlp_gen_f16_kernel<Mode, 2, 2>;
    hipLaunchKernelGGL(kernel, grid, block, 0, a.st, *a.s, a.L, a.mlp_packed, a.rays, a.z, a.NR, a.K, a.rgbsigma, a.ix_interp, a.ix_padding,
                       a.lzmaps);
    return check_launch(Mode::name);
}

// one explicit instantiation each, in the translation unit named after the mode: its kernels get a code object of their own, and adding
// a mode cannot change the register allocation of the others
extern template int launch_mode<Default>(const Launch &);   // points_mlp_gen_f16.hip
extern template int launch_mode<Ix>(const Launch &);        // points_mlp_gen_f16_ix.hip
extern template int launch_mode<Bc>(const Launch &);        // points_mlp_gen_f16_bc.hip
extern template int launch_mode<Lz>(const Launch &);        // points_mlp_gen_f16_lz.hip
extern template int launch_mode<LzBc>(const Launch &);      // points_mlp_gen_f16_lz_bc.hip

}  // namespace genf16
}  // namespace diner
