// The tail of SpatialEncoder.forward (reference src/models/image_encoder.py:262-272) in one kernel: the ResNet's feature levels, each
// upsampled to the first level's size (F.interpolate, mode="bilinear", align_corners=True) and joined along the channels -- written once,
// directly in the [N,h,w,C] layout the gathers of the render and training kernels read (what diner_pack_latent makes of the NCHW
// latent), and its exact adjoint in gather form (no atomics: fixed-order sums, run-to-run deterministic).
// Both directions take every tap and weight from assemble_tap() below, so they agree on them bit for bit.
// The same pair for upsample_interp = "bicubic" (mode="bicubic", align_corners=True: 16 taps per value) follows it, with entry points of
// its own; there both directions take every tap and coefficient from assemble_tap_bc().
#include "common.hpp"

namespace diner {

namespace {

constexpr int MAXL = DINER_LATENT_MAX_LEVELS;
constexpr int TP = 32;   // pixels (forward) / coarse texels (backward) per tile
constexpr int TC = 64;   // channels per LDS pass: 256-byte pieces of an NHWC texel

struct AssembleArgs {          // by value in the kernel arguments: every field is read with a compile-time index
    const float *data[MAXL];   // NCHW [N, C_l, h_l, w_l]
    int C[MAXL], h[MAXL], w[MAXL], off[MAXL];   // off: first output channel of the level
    float sh[MAXL], sw[MAXL];  // ATen's area_pixel_compute_scale(align_corners=True): (in - 1) / (out - 1) in fp32, 0 when out == 1
    int n;
};

struct Tap {
    int i0, i1;
    float l0, l1;
};

// ATen's align_corners=True source index of output index `dst` (upsample_bilinear2d: src = scale * dst, i0 = (int)src,
// i1 = i0 + (i0 < in - 1), lambda1 = src - i0, lambda0 = 1 - lambda1).  in == out: scale == 1, lambda1 == 0 exactly.
__device__ __forceinline__ Tap assemble_tap(float scale, int dst, int in)
{
    const float src = scale * (float)dst;
    Tap t;
    t.i0 = min((int)src, in - 1);   // (the clamp never acts for a size below 2^22: it only keeps every index inside the level)
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// Fine indices that can land on coarse index I: src = s * dst lies in (I - 1, I + 1), inverted with a margin of one on either side;
// assemble_tap() decides membership.  Same size: the index itself (a plain copy).  s == 0 (in == 1 or out == 1): every fine index.
__device__ __forceinline__ void fine_range(int I, float s, int in, int out, int &lo, int &hi)
{
    if (in == out) { lo = hi = I; return; }
    if (s == 0.f) { lo = 0; hi = out - 1; return; }
    const double a = floor((double)(I - 1) / (double)s) - 1.0, b = ceil((double)(I + 1) / (double)s) + 1.0;
    lo = (int)fmax(a, 0.0);
    hi = (int)fmin(b, (double)(out - 1));
}

// Output-stationary: one workgroup = 32 consecutive output pixels of one image x all C channels, 64 channels per LDS pass.
// Read side: lanes 0..31 of a wave are neighbouring output pixels of one channel plane (they share coarse texels: L1/L2);
// write side: a wave stores 256 contiguous bytes of one NHWC texel.  A group of 8 consecutive output channels lies in one level
// (every C_l is a multiple of 8), so the level of a load is uniform across the workgroup.
__global__ __launch_bounds__(256) void assemble_latent_kernel(AssembleArgs a, int h, int w, int C, float *__restrict__ out)
{
    __shared__ float tile[TP][TC + 1];
    const int64_t img = blockIdx.y, hw = (int64_t)h * w, p0 = (int64_t)blockIdx.x * TP;
    const int px = threadIdx.x & 31, c0 = threadIdx.x >> 5;
    const int64_t p = p0 + px;
    const bool live = p < hw;
    const int y = live ? (int)(p / w) : 0, x = live ? (int)(p - (int64_t)y * w) : 0;
    for (int cb = 0; cb < C; cb += TC) {
        for (int j = 0; j < TC / 8; ++j) {
            const int grp = cb + 8 * j;
            float v = 0.f;
            if (live && grp < C) {
                const float *data = a.data[0];
                int Cl = a.C[0], hl = a.h[0], wl = a.w[0], off = 0;
                float sh = a.sh[0], sw = a.sw[0];
#pragma unroll
                for (int k = 1; k < MAXL; ++k)
                    if (k < a.n && grp >= a.off[k]) {
                        data = a.data[k]; Cl = a.C[k]; hl = a.h[k]; wl = a.w[k]; off = a.off[k]; sh = a.sh[k]; sw = a.sw[k];
                    }
                const Tap ty = assemble_tap(sh, y, hl), tx = assemble_tap(sw, x, wl);
                const float *src = data + (img * Cl + (grp + c0 - off)) * ((int64_t)hl * wl);
                const int64_t r0 = (int64_t)ty.i0 * wl, r1 = (int64_t)ty.i1 * wl;
                const float t00 = src[r0 + tx.i0], t01 = src[r0 + tx.i1], t10 = src[r1 + tx.i0], t11 = src[r1 + tx.i1];
                v = ty.l0 * (tx.l0 * t00 + tx.l1 * t01) + ty.l1 * (tx.l0 * t10 + tx.l1 * t11);
            }
            tile[px][8 * j + c0] = v;
        }
        __syncthreads();
        float *dst = out + (img * hw + p0) * C + cb;
        for (int i = threadIdx.x; i < TP * TC; i += 256) {
            const int q = i / TC, k = i - q * TC;
            if (p0 + q < hw && cb + k < C) dst[(int64_t)q * C + k] = tile[q][k];
        }
        __syncthreads();
    }
}

// The adjoint of one level, in gather form: one workgroup = 32 consecutive coarse texels of one image x 64 channels of the level.
// Lanes run along the channels (a wave reads 256 contiguous bytes of a fine NHWC texel); a thread walks the fine rows and columns
// whose i0 or i1 is its texel, rows outside, columns inside, in ascending order: the sum has one fixed order.  The tile is transposed
// through LDS so that the NCHW writes are 128 contiguous bytes per plane.  Every element of the level's gradient is written.
__global__ __launch_bounds__(256) void assemble_latent_bwd_kernel(const float *__restrict__ d_out, int h, int w, int C, int off, int Cl,
                                                                  int hl, int wl, float sh, float sw, float *__restrict__ grad)
{
    __shared__ float tile[TC][TP + 1];
    const int64_t img = blockIdx.z, hwl = (int64_t)hl * wl, t0 = (int64_t)blockIdx.x * TP;
    const int cb = blockIdx.y * TC, cx = threadIdx.x & 63, t4 = threadIdx.x >> 6;
    const float *g = d_out + img * h * w * C + off + cb + cx;
    for (int i = 0; i < TP / 4; ++i) {
        const int tt = t4 + 4 * i;
        const int64_t t = t0 + tt;
        float acc = 0.f;
        if (t < hwl && cb + cx < Cl) {
            const int Y = (int)(t / wl), X = (int)(t - (int64_t)Y * wl);
            int ylo, yhi, xlo, xhi;
            fine_range(Y, sh, hl, h, ylo, yhi);
            fine_range(X, sw, wl, w, xlo, xhi);
            for (int y = ylo; y <= yhi; ++y) {
                const Tap ty = assemble_tap(sh, y, hl);
                if (ty.i0 != Y && ty.i1 != Y) continue;
                const float wy = (ty.i0 == Y ? ty.l0 : 0.f) + (ty.i1 == Y ? ty.l1 : 0.f);
                const float *row = g + (int64_t)y * w * C;
                for (int x = xlo; x <= xhi; ++x) {
                    const Tap tx = assemble_tap(sw, x, wl);
                    if (tx.i0 != X && tx.i1 != X) continue;
                    const float wx = (tx.i0 == X ? tx.l0 : 0.f) + (tx.i1 == X ? tx.l1 : 0.f);
                    acc = acc + (wy * wx) * row[(int64_t)x * C];
                }
            }
        }
        tile[cx][tt] = acc;
    }
    __syncthreads();
    const int px = threadIdx.x & 31, cr = threadIdx.x >> 5;
    for (int c = cr; c < TC; c += 8)
        if (cb + c < Cl && t0 + px < hwl) grad[(img * Cl + cb + c) * hwl + t0 + px] = tile[c][px];
}

// ---- upsample_interp = "bicubic": F.interpolate(mode="bicubic", align_corners=True), ATen's upsample_bicubic2d ----------------------
struct Tap4 {
    int i[4];     // i - 1 .. i + 2, each clamped to [0, in - 1]
    float w[4];   // the cubic convolution coefficients of t = src - i, A = -0.75
};

// ATen's align_corners=True taps and coefficients of output index `dst` (upsample_bicubic2d: src = scale * dst, i = (int)src,
// t = src - i, get_cubic_upsample_coefficients).  The coefficients are ATen's cubics
//   w0 = ((A (t+1) - 5A)(t+1) + 8A)(t+1) - 4A,  w1 = ((A+2) t - (A+3)) t t + 1,  w2 = w1(1 - t),  w3 = w0(1 - t),  A = -0.75
// evaluated in their factored forms, w0 = A t (1-t)^2 and w1 = (1-t) (1 + t - (A+2) t^2): the same polynomials, but every coefficient comes
// out to a few ulp of ITSELF.  ATen's Horner forms pass through intermediates of magnitude 3..6 and leave an absolute error of up to
// 12 * 2^-24 on coefficients as small as 0.02, which a coarse texel with a handful of fine pixels on it (a level larger than the output)
// shows in its gradient.  in == out: scale == 1, t == 0 and the coefficients are (-0, 1, 0, -0) exactly.
__device__ __forceinline__ Tap4 assemble_tap_bc(float scale, int dst, int in)
{
    constexpr float A = -0.75f;
    const float src = scale * (float)dst;
    const int i = min((int)src, in - 1);
    const float t = src - (float)i, u = 1.0f - t;
    Tap4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.i[k] = min(max(i - 1 + k, 0), in - 1);
    r.w[0] = (A * t) * (u * u);
    r.w[1] = u * ((1.0f + t) - ((A + 2.0f) * t) * t);
    r.w[2] = t * ((1.0f + u) - ((A + 2.0f) * u) * u);
    r.w[3] = (A * u) * (t * t);
    return r;
}

// The adjoint's weight of coarse index I in the taps of one fine index: the sum (k ascending) of the coefficients whose clamped tap is I
// -- at a border several taps of one fine index land on the same texel.  False when no tap does.
__device__ __forceinline__ bool tap_weight_bc(const Tap4 &t, int I, float &wsum)
{
    bool any = false;
    wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (t.i[k] == I) { wsum = wsum + t.w[k]; any = true; }
    return any;
}

// Fine indices that can have a tap on coarse index I: i = (int)src in [I - 2, I + 1] before clamping, so src = s * dst lies in
// (I - 3, I + 3), inverted with a margin of one on either side; assemble_tap_bc() decides membership.  Same size: the index itself (its
// neighbours' taps on I carry the coefficient 0).  s == 0 (in == 1 or out == 1): every fine index.
__device__ __forceinline__ void fine_range_bc(int I, float s, int in, int out, int &lo, int &hi)
{
    if (in == out) { lo = hi = I; return; }
    if (s == 0.f) { lo = 0; hi = out - 1; return; }
    const double a = floor((double)(I - 3) / (double)s) - 1.0, b = ceil((double)(I + 3) / (double)s) + 1.0;
    lo = (int)fmax(a, 0.0);
    hi = (int)fmin(b, (double)(out - 1));
}

// assemble_latent_kernel's shape (32 consecutive output pixels x all C channels per workgroup, 64 channels per LDS pass, lanes along
// neighbouring pixels on the read side, 256 contiguous bytes of an NHWC texel per wave on the write side) with 16 taps per value.
// The taps and coefficients of a pixel depend on its level only: they are computed when the level of the channel group changes (the level
// is uniform across the workgroup and ascends with the group), not per channel.  A level of the output's size is copied (bit-identical
// whatever it holds: no 0 * inf).
__global__ __launch_bounds__(256) void assemble_latent_bc_kernel(AssembleArgs a, int h, int w, int C, float *__restrict__ out)
{
    __shared__ float tile[TP][TC + 1];
    const int64_t img = blockIdx.y, hw = (int64_t)h * w, p0 = (int64_t)blockIdx.x * TP;
    const int px = threadIdx.x & 31, c0 = threadIdx.x >> 5;
    const int64_t p = p0 + px;
    const bool live = p < hw;
    const int y = live ? (int)(p / w) : 0, x = live ? (int)(p - (int64_t)y * w) : 0;
    int cur = -1, Cl = 0, hl = 0, wl = 0, off = 0;
    const float *data = nullptr;
    Tap4 ty = {}, tx = {};
    for (int cb = 0; cb < C; cb += TC) {
        for (int j = 0; j < TC / 8; ++j) {
            const int grp = cb + 8 * j;
            float v = 0.f;
            if (live && grp < C) {
                int lvl = 0;
#pragma unroll
                for (int k = 1; k < MAXL; ++k)
                    if (k < a.n && grp >= a.off[k]) lvl = k;
                if (lvl != cur) {
                    cur = lvl;
                    data = a.data[0]; Cl = a.C[0]; hl = a.h[0]; wl = a.w[0]; off = 0;
                    float sh = a.sh[0], sw = a.sw[0];
#pragma unroll
                    for (int k = 1; k < MAXL; ++k)
                        if (k == lvl) {
                            data = a.data[k]; Cl = a.C[k]; hl = a.h[k]; wl = a.w[k]; off = a.off[k]; sh = a.sh[k]; sw = a.sw[k];
                        }
                    ty = assemble_tap_bc(sh, y, hl);
                    tx = assemble_tap_bc(sw, x, wl);
                }
                const float *src = data + (img * Cl + (grp + c0 - off)) * ((int64_t)hl * wl);
                if (hl == h && wl == w) {
                    v = src[(int64_t)y * wl + x];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float *row = src + (int64_t)ty.i[i] * wl;
                        const float r = tx.w[0] * row[tx.i[0]] + tx.w[1] * row[tx.i[1]] + tx.w[2] * row[tx.i[2]] + tx.w[3] * row[tx.i[3]];
                        v = i ? v + ty.w[i] * r : ty.w[i] * r;
                    }
                }
            }
            tile[px][8 * j + c0] = v;
        }
        __syncthreads();
        float *dst = out + (img * hw + p0) * C + cb;
        for (int i = threadIdx.x; i < TP * TC; i += 256) {
            const int q = i / TC, k = i - q * TC;
            if (p0 + q < hw && cb + k < C) dst[(int64_t)q * C + k] = tile[q][k];
        }
        __syncthreads();
    }
}

// The adjoint of one level, in gather form, in assemble_latent_bwd_kernel's shape: one workgroup = 32 consecutive coarse texels of one
// image x 64 channels of the level, lanes along the channels, the tile transposed through LDS for the NCHW store.  A thread walks the
// fine rows and columns that have at least one clamped tap on its texel, rows outside, columns inside, in ascending order: the sum has one
// fixed order (no atomics).  Every element of the level's gradient is written.
__global__ __launch_bounds__(256) void assemble_latent_bc_bwd_kernel(const float *__restrict__ d_out, int h, int w, int C, int off, int Cl,
                                                                     int hl, int wl, float sh, float sw, float *__restrict__ grad)
{
    __shared__ float tile[TC][TP + 1];
    const int64_t img = blockIdx.z, hwl = (int64_t)hl * wl, t0 = (int64_t)blockIdx.x * TP;
    const int cb = blockIdx.y * TC, cx = threadIdx.x & 63, t4 = threadIdx.x >> 6;
    const float *g = d_out + img * h * w * C + off + cb + cx;
    for (int i = 0; i < TP / 4; ++i) {
        const int tt = t4 + 4 * i;
        const int64_t t = t0 + tt;
        float acc = 0.f;
        if (t < hwl && cb + cx < Cl) {
            const int Y = (int)(t / wl), X = (int)(t - (int64_t)Y * wl);
            int ylo, yhi, xlo, xhi;
            fine_range_bc(Y, sh, hl, h, ylo, yhi);
            fine_range_bc(X, sw, wl, w, xlo, xhi);
            // the candidate columns trimmed to the first and last with a tap on X, once instead of in every row (uniform across the wave)
            float wy, wx;
            while (xlo <= xhi && !tap_weight_bc(assemble_tap_bc(sw, xlo, wl), X, wx)) ++xlo;
            while (xhi >= xlo && !tap_weight_bc(assemble_tap_bc(sw, xhi, wl), X, wx)) --xhi;
            for (int y = ylo; y <= yhi; ++y) {
                if (!tap_weight_bc(assemble_tap_bc(sh, y, hl), Y, wy)) continue;
                const float *row = g + (int64_t)y * w * C;
                for (int x = xlo; x <= xhi; ++x) {
                    if (!tap_weight_bc(assemble_tap_bc(sw, x, wl), X, wx)) continue;
                    acc = acc + (wy * wx) * row[(int64_t)x * C];
                }
            }
        }
        tile[cx][tt] = acc;
    }
    __syncthreads();
    const int px = threadIdx.x & 31, cr = threadIdx.x >> 5;
    for (int c = cr; c < TC; c += 8)
        if (cb + c < Cl && t0 + px < hwl) grad[(img * Cl + cb + c) * hwl + t0 + px] = tile[c][px];
}

int invalid(const char *who, const char *what)
{
    set_error("%s: %s", who, what);
    return DINER_E_INVALID;
}

// argument checks of both directions (before any launch); fills the kernel arguments
int check_levels(const char *who, const DinerLatentLevels *lv, int32_t n_levels, int64_t N, int32_t h, int32_t w, const void *other,
                 AssembleArgs &a, int &C)
{
    if (!lv || !other) return invalid(who, "NULL pointer");
    if (n_levels < 1 || n_levels > MAXL) {
        set_error("%s: n_levels=%d outside 1..%d", who, n_levels, MAXL);
        return DINER_E_INVALID;
    }
    if (N <= 0 || h <= 0 || w <= 0) return invalid(who, "non-positive size (N, h, w)");
    C = 0;
    for (int l = 0; l < n_levels; ++l) {
        const DinerLatentLevel &L = lv->level[l];
        if (!L.data) return invalid(who, "NULL pointer (a level's data)");
        if (L.C <= 0 || L.h <= 0 || L.w <= 0) {
            set_error("%s: non-positive size in level %d (C=%d, h=%d, w=%d)", who, l, L.C, L.h, L.w);
            return DINER_E_INVALID;
        }
        if ((int64_t)L.h * L.w > (int64_t)TP * 0x7fffffff) {
            set_error("%s: level %d of %d x %d texels is beyond one launch's grid", who, l, L.h, L.w);
            return DINER_E_UNSUPPORTED;
        }
        if (L.C % 8 || L.C > 1024) {
            set_error("%s: level %d has C=%d channels, unsupported (a multiple of 8 up to 1024)", who, l, L.C);
            return DINER_E_UNSUPPORTED;
        }
        a.data[l] = L.data; a.C[l] = L.C; a.h[l] = L.h; a.w[l] = L.w; a.off[l] = C;
        a.sh[l] = h > 1 ? (float)(L.h - 1) / (float)(h - 1) : 0.f;
        a.sw[l] = w > 1 ? (float)(L.w - 1) / (float)(w - 1) : 0.f;
        C += L.C;
    }
    for (int l = n_levels; l < MAXL; ++l) {
        a.data[l] = nullptr; a.C[l] = a.h[l] = a.w[l] = 0; a.off[l] = 0; a.sh[l] = a.sw[l] = 0.f;
    }
    a.n = n_levels;
    if (C > 1024) {
        set_error("%s: C=%d output channels unsupported (a multiple of 8 up to 1024)", who, C);
        return DINER_E_UNSUPPORTED;
    }
    if ((int64_t)h * w > (int64_t)TP * 0x7fffffff) {
        set_error("%s: an output of %d x %d pixels is beyond one launch's grid", who, h, w);
        return DINER_E_UNSUPPORTED;
    }
    if (N > 65535) {
        set_error("%s: N=%lld images unsupported (at most 65535)", who, (long long)N);
        return DINER_E_UNSUPPORTED;
    }
    return DINER_OK;
}

}  // namespace

}  // namespace diner

using namespace diner;

int diner_assemble_latent(const DinerLatentLevels *levels, int32_t n_levels, int64_t N, int32_t h, int32_t w, float *out_nhwc, void *stream)
{
    AssembleArgs a;
    int C = 0;
    if (const int rc = check_levels("assemble_latent", levels, n_levels, N, h, w, out_nhwc, a, C)) return rc;
    const int64_t tiles = ((int64_t)h * w + TP - 1) / TP;
    hipLaunchKernelGGL(assemble_latent_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a, h, w, C, out_nhwc);
    return check_launch("assemble_latent_kernel");
}

int diner_assemble_latent_backward(const float *d_out_nhwc, int32_t n_levels, int64_t N, int32_t h, int32_t w,
                                   const DinerLatentLevels *levels_grad, void *stream)
{
    AssembleArgs a;
    int C = 0;
    if (const int rc = check_levels("assemble_latent_backward", levels_grad, n_levels, N, h, w, d_out_nhwc, a, C)) return rc;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t tiles = ((int64_t)a.h[l] * a.w[l] + TP - 1) / TP;
        hipLaunchKernelGGL(assemble_latent_bwd_kernel, dim3((unsigned)tiles, (unsigned)((a.C[l] + TC - 1) / TC), (unsigned)N), dim3(256), 0,
                           (hipStream_t)stream, d_out_nhwc, h, w, C, a.off[l], a.C[l], a.h[l], a.w[l], a.sh[l], a.sw[l],
                           const_cast<float *>(a.data[l]));
        if (const int rc = check_launch("assemble_latent_bwd_kernel")) return rc;
    }
    return DINER_OK;
}

int diner_assemble_latent_bicubic(const DinerLatentLevels *levels, int32_t n_levels, int64_t N, int32_t h, int32_t w, float *out_nhwc,
                                  void *stream)
{
    AssembleArgs a;
    int C = 0;
    if (const int rc = check_levels("assemble_latent_bicubic", levels, n_levels, N, h, w, out_nhwc, a, C)) return rc;
    const int64_t tiles = ((int64_t)h * w + TP - 1) / TP;
    hipLaunchKernelGGL(assemble_latent_bc_kernel, dim3((unsigned)tiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a, h, w, C, out_nhwc);
    return check_launch("assemble_latent_bc_kernel");
}

int diner_assemble_latent_bicubic_backward(const float *d_out_nhwc, int32_t n_levels, int64_t N, int32_t h, int32_t w,
                                           const DinerLatentLevels *levels_grad, void *stream)
{
    AssembleArgs a;
    int C = 0;
    if (const int rc = check_levels("assemble_latent_bicubic_backward", levels_grad, n_levels, N, h, w, d_out_nhwc, a, C)) return rc;
    for (int l = 0; l < n_levels; ++l) {
        const int64_t tiles = ((int64_t)a.h[l] * a.w[l] + TP - 1) / TP;
        hipLaunchKernelGGL(assemble_latent_bc_bwd_kernel, dim3((unsigned)tiles, (unsigned)((a.C[l] + TC - 1) / TC), (unsigned)N), dim3(256), 0,
                           (hipStream_t)stream, d_out_nhwc, h, w, C, a.off[l], a.C[l], a.h[l], a.w[l], a.sh[l], a.sw[l],
                           const_cast<float *>(a.data[l]));
        if (const int rc = check_launch("assemble_latent_bc_bwd_kernel")) return rc;
    }
    return DINER_OK;
}
