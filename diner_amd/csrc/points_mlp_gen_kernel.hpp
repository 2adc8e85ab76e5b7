// Device code of the shape-general fp32 point/MLP kernels (points_mlp_gen.hip has the description): the packed weight layout, the LDS A
// image, the MFMA GEMM, the tap records, the building blocks every kernel of the family is made of (tap_of, resnet_block, finish; the
// view geometry, the input columns and the tile order are common.hpp's), the kernel template and its launcher.  Each kernel shows its
// inputs, its per-point records, the view loop (input stage, lin_in, gather, resnet_block) and the finish; the gathers stay in the
// kernels.  One lookup mode = one instantiation of the template,
// each in a translation unit of its own (points_mlp_gen.hip and points_mlp_gen_{ix,bc,lz,lz_bc}.hip); linz_maps_gen.hip takes the
// layout and gemm() only.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace diner {
namespace gen {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE_P = 64;                     // points per workgroup
constexpr int NWAVES = 8;                      // waves per workgroup
constexpr int KMAX = 512;                      // columns of the LDS A image
constexpr int A_F4 = KMAX / 8 * 2 * TILE_P;    // float4 entries of the A image (8192 = 128 KiB)

// ---- packed weight image ---------------------------------------------------------------------------------------------------------
// layers in order lin_in | lin_z[0..nlz) | fc_0[0..nb) | fc_1[0..nb) | lin_out, each [col_tile][jb][lane][4]: lane = h*32+c holds
// W[n = 32*col_tile + c][k = 8*jb + 2*ji + h], ji = 0..3 (zero outside the layer); then the biases: lin_in | lin_z[b] | fc_0[b] |
// fc_1[b] (d_hidden floats each) | lin_out padded to 32.
struct Layout {
    int H, NT;             // d_hidden, 32-column tiles
    int din, njb_in;       // d_in (7 + 8F), its k-blocks of 8
    int dlat, njb_lat;     // d_latent, its k-blocks
    int nb, cl, nlz, nvb;  // n_blocks, combine_layer, lin_z layers = min(cl, nb), blocks evaluated per view = nlz
    int F;                 // num_freqs
    float beta;            // Softplus beta, 0 = ReLU
    int64_t w_in, w_z, w_h, w_out;              // floats of one layer of each kind
    int64_t off_in, off_z, off_fc0, off_fc1, off_out, off_bias, total;
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
    L.din = m.d_in; L.njb_in = (m.d_in + 7) / 8;
    L.dlat = m.d_latent; L.njb_lat = m.d_latent / 8;
    L.nb = m.n_blocks; L.cl = m.combine_layer; L.nlz = m.combine_layer < m.n_blocks ? m.combine_layer : m.n_blocks; L.nvb = L.nlz;
    L.F = m.num_freqs; L.beta = m.beta;
    L.w_in = (int64_t)L.NT * L.njb_in * 256;
    L.w_z = (int64_t)L.NT * L.njb_lat * 256;
    L.w_h = (int64_t)L.NT * (L.H / 8) * 256;
    L.w_out = (int64_t)(L.H / 8) * 256;
    L.off_in = 0;
    L.off_z = L.off_in + L.w_in;
    L.off_fc0 = L.off_z + L.nlz * L.w_z;
    L.off_fc1 = L.off_fc0 + L.nb * L.w_h;
    L.off_out = L.off_fc1 + L.nb * L.w_h;
    L.off_bias = L.off_out + L.w_out;
    L.total = L.off_bias + (int64_t)(1 + L.nlz + 2 * L.nb) * L.H + 32;
    return L;
}

// ---- LDS A image (points_mlp.hip) -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int a_off(int row, int k) { return ((((k >> 3) * 2 + (k & 1)) * TILE_P + row) << 2) + ((k >> 1) & 3); }

// acc[tm][tn] += A[rows of row block rb0 + tm] x W^T over k-blocks jb0 .. jb0 + njb of the layer (A image column 0 = k-block jb0).
// Wl: packed layer of njb_layer k-blocks per column tile; this wave's tiles ct0 .. ct0 + CT - 1 (clamped to NT - 1).
template <int RB, int CT>
__device__ __forceinline__ void gemm(f32x16 (&acc)[RB][CT], const f32x4 *A4, const f32x4 *__restrict__ Wl, int njb_layer, int jb0,
                                     int njb, int rb0, int ct0, int NT, int lane)
{
    const f32x4 *ap = A4 + (lane >> 5) * TILE_P + rb0 * 32 + (lane & 31);
    const f32x4 *bp[CT];
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) {
        const int t = ct0 + tn < NT ? ct0 + tn : NT - 1;
        bp[tn] = Wl + ((int64_t)t * njb_layer + jb0) * 64 + lane;
    }
    f32x4 b_cur[CT], b_nxt[CT];
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) b_cur[tn] = bp[tn][0];
#pragma unroll 2
    for (int jb = 0; jb < njb; ++jb) {
        const int jn = jb + 1 < njb ? jb + 1 : jb;  // last iteration re-loads (harmless, keeps the loop branch-free)
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) b_nxt[tn] = bp[tn][jn * 64];
        f32x4 a[RB];
#pragma unroll
        for (int tm = 0; tm < RB; ++tm) a[tm] = ap[jb * 2 * TILE_P + 32 * tm];
#pragma unroll
        for (int ji = 0; ji < 4; ++ji)
#pragma unroll
            for (int tn = 0; tn < CT; ++tn)
#pragma unroll
                for (int tm = 0; tm < RB; ++tm)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][ji], b_cur[tn][ji], acc[tm][tn], 0, 0, 0);
#pragma unroll
        for (int tn = 0; tn < CT; ++tn) b_cur[tn] = b_nxt[tn];
    }
}

template <int RB, int CT>
__device__ __forceinline__ void acc_bias(f32x16 (&acc)[RB][CT], const float *__restrict__ bias, bool add, int ct0, int NT, int lane)
{
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) {
        const int t = ct0 + tn < NT ? ct0 + tn : NT - 1;
        const float b = bias[t * 32 + (lane & 31)];
#pragma unroll
        for (int tm = 0; tm < RB; ++tm)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[tm][tn][i] = add ? acc[tm][tn][i] + b : b;
    }
}

// Softplus(beta) as torch evaluates it (x * beta > 20: linear); a NaN stays NaN
__device__ __forceinline__ float softplus(float v, float beta)
{
    const float xb = v * beta;
    return xb > 20.0f ? v : log1pf(expf(xb)) / beta;
}

// activation(acc) -> LDS A image: this wave's columns become k = 32 * tile + c of the next layer (resnetfc.py:62-63,158)
template <int RB, int CT>
__device__ __forceinline__ void store_act(const f32x16 (&acc)[RB][CT], float *A, float beta, int rb0, int ct0, int NT, int lane)
{
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int tn = 0; tn < CT; ++tn) {
        if (ct0 + tn >= NT) continue;
        const int k = (ct0 + tn) * 32 + c;
        float *col = A + ((((k >> 3) * 2 + (k & 1)) * TILE_P) << 2) + ((k >> 1) & 3);
#pragma unroll
        for (int tm = 0; tm < RB; ++tm) {
            const int r0 = (rb0 + tm) * 32 + 4 * h;
            if (beta > 0.0f) {
#pragma unroll
                for (int i = 0; i < 16; ++i) col[(r0 + 8 * (i >> 2) + (i & 3)) << 2] = softplus(acc[tm][tn][i], beta);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {   // C/D layout of the 32x32 MFMA; keeps NaN, like torch.relu
                    const float v = acc[tm][tn][i];
                    col[(r0 + 8 * (i >> 2) + (i & 3)) << 2] = v < 0.0f ? 0.0f : v;
                }
            }
        }
    }
}

struct Tap {        // bilinear footprint of one (point, view) in the latent map
    int o00, o01, o10, o11;  // float4 offsets of the 4 texels (clamped, always readable)
    float nw, ne, sw, se;    // weights; a tap outside the map has its weight forced to 0
};

struct TapBc {      // bicubic footprint of one (point, view) in the latent map (common.hpp BicubicFoot), 64 bytes
    int xo[4], yo[4];        // float4 offsets of the 4 columns (x * c4) and the 4 rows (y * w * c4); texel (i, j) = xo[i] + yo[j]
    float cx[4], cy[4];      // weights per axis; zeros padding: 0 for a column / row outside the map
};

// ---- building blocks of the kernels: points_mlp_gen_kernel below and the forms of it that units of their own define ----
// the Tap of a 4-tap footprint in a map lw texels wide, c4 float4 per texel
__device__ __forceinline__ Tap tap_of(const LatentFoot &f, int lw, int c4)
{
    Tap t;
    t.o00 = (f.y0 * lw + f.x0) * c4; t.o01 = (f.y0 * lw + f.x1) * c4;
    t.o10 = (f.y1 * lw + f.x0) * c4; t.o11 = (f.y1 * lw + f.x1) * c4;
    t.nw = f.nw; t.ne = f.ne; t.sw = f.sw; t.se = f.se;
    return t;
}

// ResNet block b on the hidden state x (resnetfc.py:62-69): x = x + fc_1(act(fc_0(act(x)))).  The A
// image must be free on entry and is free on return (four barriers).
template <int RB, int CT>
__device__ __forceinline__ void resnet_block(f32x16 (&x)[RB][CT], float *A, const float *__restrict__ Wp, const Layout &L, int b,
                                             int rb0, int ct0, int lane)
{
    const f32x4 *A4 = (const f32x4 *)A;
    const float *bias = Wp + L.off_bias;
    const int NT = L.NT, H = L.H;
    f32x16 net[RB][CT];
    store_act(x, A, L.beta, rb0, ct0, NT, lane);                                                    // :62 fc_0(act(x))
    __syncthreads();
    acc_bias(net, bias + L.bias_fc0(b), false, ct0, NT, lane);
    gemm(net, A4, (const f32x4 *)(Wp + L.off_fc0 + b * L.w_h), H / 8, 0, H / 8, rb0, ct0, NT, lane);
    __syncthreads();
    store_act(net, A, L.beta, rb0, ct0, NT, lane);                                                  // :63 fc_1(act(net))
    __syncthreads();
    acc_bias(x, bias + L.bias_fc1(b), true, ct0, NT, lane);                                         // :69 x + dx
    gemm(x, A4, (const f32x4 *)(Wp + L.off_fc1 + b * L.w_h), H / 8, 0, H / 8, rb0, ct0, NT, lane);
    __syncthreads();
}

// what follows the view loop: combine() = the mean of the per-view states xsum over NV views (resnetfc.py:146-149), the blocks after
// combine_layer, lin_out (:158) and the head (pixelnerf.py:139-143: sigmoid rgb, ReLU sigma) -> rgbsigma [SB,P,4], rows of the tail
// tile past P masked
template <int RB, int CT>
__device__ __forceinline__ void finish(f32x16 (&xsum)[RB][CT], float *A, const float *__restrict__ Wp, const Layout &L,
                                       int NV, int rb0, int ct0, int lane, int wave, int sb, int64_t tile,
                                       int64_t P, float *__restrict__ rgbsigma)
{
    const f32x4 *A4 = (const f32x4 *)A;
    const float *bias = Wp + L.off_bias;
    const int H = L.H;
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
    store_act(xsum, A, L.beta, rb0, ct0, L.NT, lane);                                               // :158 lin_out(act(x))
    __syncthreads();
    if (wave < 2) {  // lin_out: one 32-column tile (4 real outputs), wave w = rows 32w..32w+31
        f32x16 o;
        const float bo = bias[L.bias_lin_out() + (lane & 31)];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = bo;
        const f32x4 *ap = A4 + (lane >> 5) * TILE_P + wave * 32 + (lane & 31);
        const f32x4 *bp = (const f32x4 *)(Wp + L.off_out) + lane;
#pragma unroll 4
        for (int jb = 0; jb < H / 8; ++jb) {
            const f32x4 a = ap[jb * 2 * TILE_P], bq = bp[jb * 64];
#pragma unroll
            for (int ji = 0; ji < 4; ++ji) o = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ji], bq[ji], o, 0, 0, 0);
        }
        const int c = lane & 31, h = lane >> 5;
        if (c < 4) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = wave * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                const int64_t pp = tile * TILE_P + r;
                if (pp < P) {
                    const float val = o[i];
                    rgbsigma[((int64_t)sb * P + pp) * 4 + c] = c < 3 ? 1.0f / (1.0f + expf(-val)) : (val < 0.0f ? 0.0f : val);
                }
            }
        }
    }
}

// ---- lookup modes -------------------------------------------------------------------------------------------------------------------
// The kernel's first template parameter.  ix: the footprint of any 4-tap lookup (ix_interp / ix_padding, DINER_INDEX_*; common.hpp
// latent_footprint) instead of the written-out bilinear / border one; bc: the 16-tap bicubic lookup (common.hpp bicubic_footprint)
// with the padding ix_padding; lz: the lin_z-map form.  lin_z[b] is linear and the lookup a weighted sum of texels, so
// lin_z[b](lookup(F)) = sum_i w_i (W_b F_i) + bias_b: instead of gathering d_latent channels and multiplying per point, view and block
// the lz kernels gather d_hidden channels of the map M_b = W_b F (linz_maps_gen.hip; no bias in it, so it is exactly linear in the taps
// and every lookup mode, bicubic's negative weights and zeros padding's missing taps included, reads the same maps) and add them to x.
template <bool IX, bool BC, bool LZ>
struct ModeOf {
    static constexpr bool ix = IX, bc = BC, lz = LZ;
    typedef std::conditional_t<BC, TapBc, Tap> tap;                     // a row's tap record in LDS
    static constexpr int TAP_F4 = sizeof(tap) / sizeof(f32x4);          // its float4 entries
};
struct Default : ModeOf<false, false, false> { static constexpr const char *name = "points_mlp_gen_kernel<Default>"; };
struct Ix : ModeOf<true, false, false> { static constexpr const char *name = "points_mlp_gen_kernel<Ix>"; };
struct Bc : ModeOf<true, true, false> { static constexpr const char *name = "points_mlp_gen_kernel<Bc>"; };
struct Lz : ModeOf<true, false, true> { static constexpr const char *name = "points_mlp_gen_kernel<Lz>"; };
struct LzBc : ModeOf<true, true, true> { static constexpr const char *name = "points_mlp_gen_kernel<LzBc>"; };

constexpr int BC_ROW_UNROLL = 2;   // rows of the 4 x 4 bicubic footprint whose loads are in flight together in the gather

// Every mode takes the same arguments: Default reads neither ix_interp nor ix_padding, Bc / LzBc no ix_interp, only Lz / LzBc lzmaps.
template <class Mode, int RB, int CT>
__global__ __launch_bounds__(NWAVES * 64) void points_mlp_gen_kernel(DinerScene s, Layout L, const float *__restrict__ Wp,
                                                                     const float *__restrict__ rays, const float *__restrict__ zsamp,
                                                                     int64_t NR, int K, float *__restrict__ rgbsigma, int ix_interp,
                                                                     int ix_padding, const float *__restrict__ lzmaps)
{
    typedef typename Mode::tap TapRec;
    __shared__ f32x4 lds[A_F4 + TILE_P * Mode::TAP_F4];  // A image + one Tap (bicubic: one TapBc) per row
    f32x4 *A4 = lds;
    float *A = (float *)lds;
    TapRec *taps = (TapRec *)(lds + A_F4);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb0 = RB == 2 ? 0 : (wave & 1), ct0 = RB == 2 ? wave * CT : (wave >> 1) * CT;
    const int NT = L.NT, H = L.H;
    const int sb = blockIdx.y;
    const int64_t P = NR * (int64_t)K;
    const int64_t tile = xcd_tile(gridDim.x, blockIdx.x);
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
    const int F = L.F, din_pad = 8 * L.njb_in;
    // float4 per texel the taps address.  lz: of a lin_z map, the latent itself is never read; else of the latent
    const int c4 = Mode::lz ? H / 4 : L.dlat / 4;

    for (int v = 0; v < s.NV; ++v) {
        // ---- geometry + positional encodings -> A[:, 0:din_pad]; bilinear footprint -> taps.  (The column loop is written in each
        // kernel: inside a helper of its own the <2,2> kernels spill 4 to 7 VGPRs more.) ----------
        {
            float px, py, pz, u, w, dcx, dcy, dcz, delta;
            view_geometry(s, sb, v, wx, wy, wz, dwx, dwy, dwz, px, py, pz, u, w, dcx, dcy, dcz, delta);   // pixelnerf.py:91-115
            for (int e = wave; e < din_pad; e += NWAVES)                                                  // input layout :128
                A[a_off(row, e)] = input_element(e, px, py, pz, dcx, dcy, dcz, delta, F, s.freq_factor);
            if constexpr (Mode::bc) {
                if (wave == 0) {  // the 4 x 4 bicubic footprint in the latent map (image_encoder.py:97-127; common.hpp)
                    const BicubicFoot f = bicubic_footprint(u, w, sxl, syl, s.w, s.h, ix_padding);
                    TapBc t;
#pragma unroll
                    for (int i = 0; i < 4; ++i) { t.xo[i] = f.x[i] * c4; t.yo[i] = f.y[i] * s.w * c4; t.cx[i] = f.cx[i]; t.cy[i] = f.cy[i]; }
                    taps[row] = t;
                }
            } else if constexpr (Mode::ix) {
                if (wave == 0)   // footprint of any lookup mode in the latent map (image_encoder.py:97-127; common.hpp)
                    taps[row] = tap_of(latent_footprint<true>(u, w, sxl, syl, s.w, s.h, ix_interp, ix_padding), s.w, c4);
            } else if (wave == 0) {  // bilinear / border footprint in the latent map (image_encoder.py:97-127; = latent_footprint<false>,
                                     // written out: through the helper the compiler schedules this kernel differently)
                const float ix = clipf(unnorm(u * sxl, (float)s.w / 2.0f), (float)(s.w - 1));
                const float iy = clipf(unnorm(w * syl, (float)s.h / 2.0f), (float)(s.h - 1));
                const float x0f = floorf(ix), y0f = floorf(iy);
                const float fx = ix - x0f, ex = 1.0f - fx, fy = iy - y0f, ey = 1.0f - fy;
                const int x0 = safe_idx(x0f, s.w), y0 = safe_idx(y0f, s.h);
                const bool x1ok = x0 + 1 <= s.w - 1, y1ok = y0 + 1 <= s.h - 1;
                const int x1 = x1ok ? x0 + 1 : x0, y1 = y1ok ? y0 + 1 : y0;
                Tap t;
                t.o00 = (y0 * s.w + x0) * c4; t.o01 = (y0 * s.w + x1) * c4;
                t.o10 = (y1 * s.w + x0) * c4; t.o11 = (y1 * s.w + x1) * c4;
                t.nw = ey * ex; t.ne = x1ok ? ey * fx : 0.0f;
                t.sw = y1ok ? fy * ex : 0.0f; t.se = (x1ok && y1ok) ? fy * fx : 0.0f;
                taps[row] = t;
            }
        }
        __syncthreads();
        acc_bias(x, bias + L.bias_lin_in(), false, ct0, NT, lane);
        gemm(x, A4, (const f32x4 *)(Wp + L.off_in), L.njb_in, 0, L.njb_in, rb0, ct0, NT, lane);   // resnetfc.py:139
        __syncthreads();

        const f32x4 *lat = Mode::lz ? nullptr : (const f32x4 *)s.latent + ((int64_t)sb * s.NV + v) * s.h * s.w * c4;
        for (int b = 0; b < L.nvb; ++b) {
            acc_bias(x, bias + L.bias_lin_z(b), true, ct0, NT, lane);                               // :152-153 x = x + lin_z(z)
            if constexpr (Mode::lz) {
                // ---- (W_b z)[:, 0 : H] = the lookup of the 64 points in map M_b -> LDS as fp32 [row][LD], column ^ 32 for the rows of lane
                // half 1 (the two halves of a wave read rows 4 apart: 64 banks, no conflict); then every lane adds the elements of its
                // accumulators (the C/D layout of the 32x32 MFMA, store_act's index map read backwards).  While H <= 256 the staging area
                // lies behind the columns store_act writes next, and no barrier is needed between the adds and that store.
                const int LD = (H + 63) & ~63;
                const bool apart = (H + LD) * TILE_P <= A_F4 * 4;
                float *S = A + (apart ? H * TILE_P : 0);
                const f32x4 *mp = (const f32x4 *)lzmaps + (((int64_t)b * s.SB + sb) * s.NV + v) * s.h * s.w * c4;
                for (int idx = lane; idx < (TILE_P / NWAVES) * c4; idx += 64) {   // a wave gathers 8 rows, c4 quads each
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
                    *(f32x4 *)(S + r * LD + ((4 * q) ^ (((r >> 2) & 1) << 5))) = val;
                }
                __syncthreads();
                const int c = lane & 31, h = lane >> 5;
#pragma unroll
                for (int tn = 0; tn < CT; ++tn) {
                    const int t = ct0 + tn < NT ? ct0 + tn : NT - 1;
                    const float *col = S + ((t * 32 + c) ^ (h << 5));
#pragma unroll
                    for (int tm = 0; tm < RB; ++tm) {
                        const int r0 = (rb0 + tm) * 32 + 4 * h;
#pragma unroll
                        for (int i = 0; i < 16; ++i) x[tm][tn][i] += col[(r0 + 8 * (i >> 2) + (i & 3)) * LD];
                    }
                }
                if (!apart) __syncthreads();
            } else {
                for (int k0 = 0; k0 < L.dlat; k0 += KMAX) {
                    // ---- z[:, k0 : k0 + kc] = bilinear latent of the 64 points -> A (each wave gathers 8 rows) ---------
                    const int kc4 = (L.dlat - k0 < KMAX ? L.dlat - k0 : KMAX) / 4;
                    if constexpr (Mode::bc) {
                        // 16 texels per channel quad: sum_j cy[j] * (sum_i cx[i] * texel_ij), rows then columns, contracted FMAs.  The row
                        // loop is unrolled by BC_ROW_UNROLL only (4 x that many 16-byte loads in flight per lane): fully unrolled, the 16
                        // loads of a quad compete with the kernel's accumulators for registers.
                        for (int rr = 0; rr < TILE_P / NWAVES; ++rr) {
                            const int r = wave * (TILE_P / NWAVES) + rr;
                            const TapBc *tp = taps + r;
                            const int x0 = tp->xo[0], x1 = tp->xo[1], x2 = tp->xo[2], x3 = tp->xo[3];
                            const float w0 = tp->cx[0], w1 = tp->cx[1], w2 = tp->cx[2], w3 = tp->cx[3];
                            for (int q = lane; q < kc4; q += 64) {
                                const f32x4 *lq = lat + (k0 / 4 + q);
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
#pragma unroll
                                for (int i = 0; i < 4; ++i) A[a_off(r, 4 * q + i)] = acc[i];
                            }
                        }
                    } else {
                        for (int rr = 0; rr < TILE_P / NWAVES; ++rr) {
                            const int r = wave * (TILE_P / NWAVES) + rr;
                            const Tap t = taps[r];
                            for (int q = lane; q < kc4; q += 64) {
                                const int qq = k0 / 4 + q;
                                const f32x4 a = lat[t.o00 + qq], bb = lat[t.o01 + qq], c = lat[t.o10 + qq], d = lat[t.o11 + qq];
#pragma unroll
                                for (int i = 0; i < 4; ++i) A[a_off(r, 4 * q + i)] = tap_sum(a[i], bb[i], c[i], d[i], t);
                            }
                        }
                    }
                    __syncthreads();
                    gemm(x, A4, (const f32x4 *)(Wp + L.off_z + b * L.w_z), L.njb_lat, k0 / 8, kc4 / 2, rb0, ct0, NT, lane);
                    __syncthreads();
                }
            }
            if constexpr (Mode::bc && !Mode::lz) {   // resnet_block(), written out: through the helper Bc<2,1> spills 36 SGPRs, not 33
                f32x16 net[RB][CT];
                store_act(x, A, L.beta, rb0, ct0, NT, lane);
                __syncthreads();
                acc_bias(net, bias + L.bias_fc0(b), false, ct0, NT, lane);
                gemm(net, A4, (const f32x4 *)(Wp + L.off_fc0 + b * L.w_h), H / 8, 0, H / 8, rb0, ct0, NT, lane);
                __syncthreads();
                store_act(net, A, L.beta, rb0, ct0, NT, lane);
                __syncthreads();
                acc_bias(x, bias + L.bias_fc1(b), true, ct0, NT, lane);
                gemm(x, A4, (const f32x4 *)(Wp + L.off_fc1 + b * L.w_h), H / 8, 0, H / 8, rb0, ct0, NT, lane);
                __syncthreads();
            } else {
                resnet_block(x, A, Wp, L, b, rb0, ct0, lane);
            }
        }
        acc_add(xsum, x);                                                                           // :146-149
    }
    finish(xsum, A, Wp, L, s.NV, rb0, ct0, lane, wave, sb, tile, P, rgbsigma);
}
// ---- launch ---------------------------------------------------------------------------------------------------------------------------
struct Launch {   // what a validated call passes to a mode's launcher (points_mlp_gen.hip validate())
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

// the instantiation a d_hidden runs on: <1,1> for up to 128 columns, <2,1> up to 256, <2,2> up to 512
template <class Mode>
int launch_mode(const Launch &a)
{
    const dim3 grid((unsigned)((a.NR * (int64_t)a.K + TILE_P - 1) / TILE_P), (unsigned)a.s->SB), block(NWAVES * 64);
    void (*const kernel)(DinerScene, Layout, const float *, const float *, const float *, int64_t, int, float *, int, int, const float *) =
        a.L.H <= 128 ? points_mlp_gen_kernel<Mode, 1, 1> : a.L.H <= 256 ? points_mlp_gen_kernel<Mode, 2, 1> : points_mlp_gen_kernel<Mode, 2, 2>;
    hipLaunchKernelGGL(kernel, grid, block, 0, a.st, *a.s, a.L, a.mlp_packed, a.rays, a.z, a.NR, a.K, a.rgbsigma, a.ix_interp, a.ix_padding,
                       a.lzmaps);
    return check_launch(Mode::name);
}

// one explicit instantiation each, in the translation unit named after the mode: its kernels get a code object of their own, and adding
// a mode cannot change the register allocation of the others
extern template int launch_mode<Default>(const Launch &);   // points_mlp_gen.hip
extern template int launch_mode<Ix>(const Launch &);        // points_mlp_gen_ix.hip
extern template int launch_mode<Bc>(const Launch &);        // points_mlp_gen_bc.hip
extern template int launch_mode<Lz>(const Launch &);        // points_mlp_gen_lz.hip
extern template int launch_mode<LzBc>(const Launch &);      // points_mlp_gen_lz_bc.hip

}  // namespace gen
}  // namespace diner
