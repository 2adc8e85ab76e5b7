// The tail of SpatialEncoder.forward (reference src/models/image_encoder.py:262-272) in one kernel: the ResNet's feature levels, each
// upsampled to the first level's size (F.interpolate, mode="bilinear", align_corners=True) and joined along the channels -- written once,
// directly in the [N,h,w,C] layout the gathers of the render and training kernels read (what diner_pack_latent makes of the NCHW
// latent), and its exact adjoint in gather form (no atomics: fixed-order sums, run-to-run deterministic).
// Both directions take every tap and weight from assemble_tap() below, so they agree on them bit for bit.
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
