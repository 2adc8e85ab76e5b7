// The datasets' image resizes on the device, fused with the byte decode (image_pixel.hpp):
//   decode + resize, float   reference src/data/multiface.py:341-350: read_img + gammaCorrect + the white fill at full size, then
//                            torchvision's resize(rgb, (h, w)) = F.interpolate(mode="bilinear", align_corners=False, antialias=True)
//                            (or the plain 4-tap bilinear of older torchvision), the alpha by InterpolationMode.NEAREST
//   fixed-point resize       src/data/dtu.py:79-83: PIL's Image.resize on the uint8 image, its 8-bit bicubic with 22 fractional bits
//   nearest planes           multiface.py:352-354: read_depth and the std at (h, w), the texel F.interpolate(mode="nearest") selects
// The filters are separable and tabulated on the host in double (diner_resize_table): per output index the first source index, the number
// of taps and the normalised weights, rounded once to fp32 (float resamplers) or to fixed point (PIL's).  The kernels only multiply and
// add, in the order of the taps, so two runs give the same bits; no atomics; every output element is written; what a table says is
// clamped before it addresses anything.  Element offsets are 64-bit.
#include <math.h>

#include "image_pixel.hpp"

namespace diner {

namespace {

constexpr int RS_CHUNK = 2048;          // source pixels of a row staged in LDS at a time (24 KiB)
constexpr int RS_PRECISION_BITS = 22;   // PIL's PRECISION_BITS = 32 - 8 - 2

// ---- the tables (host, double) --------------------------------------------------------------------------------------------------------
// PIL's bicubic_filter, a = -0.5
double pil_bicubic(double x)
{
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// the window of output index i: its first source index and its number of taps; w (optional, room for the taps) gets the normalised weights
int axis_window(int in, int out, int mode, int i, int &xmin, double *w)
{
    const double scale = (double)in / (double)out;
    if (mode == DINER_RESIZE_BILINEAR) {   // align_corners=False, 2 taps (1 at the last source index)
        double src = scale * (i + 0.5) - 0.5;
        if (src < 0.0) src = 0.0;
        int i0 = (int)src;
        if (i0 > in - 1) i0 = in - 1;
        const int n = i0 < in - 1 ? 2 : 1;
        const double l = src - i0;
        xmin = i0;
        if (w) {
            w[0] = n == 2 ? 1.0 - l : 1.0;
            if (n == 2) w[1] = l;
        }
        return n;
    }
    const bool pil = mode == DINER_RESIZE_BICUBIC_U8;
    const double fs = scale >= 1.0 ? scale : 1.0, support = pil ? 2.0 * fs : fs, center = scale * (i + 0.5);
    const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    if (w && n > 0) {
        double sum = 0.0;
        for (int j = 0; j < n; ++j) {
            if (pil) w[j] = pil_bicubic((j + xmin - center + 0.5) / fs);
            else {
                const double t = 1.0 - fabs((j + xmin - center + 0.5) * inv);
                w[j] = t > 0.0 ? t : 0.0;
            }
            sum += w[j];
        }
        if (sum != 0.0)
            for (int j = 0; j < n; ++j) w[j] /= sum;
    }
    return n;
}

int check_axis(const char *who, int32_t in, int32_t out, int32_t mode)
{
    if (in <= 0 || out <= 0) return invalid(who, "non-positive size (in, out)");
    if (mode != DINER_RESIZE_BILINEAR_AA && mode != DINER_RESIZE_BILINEAR && mode != DINER_RESIZE_BICUBIC_U8)
        return invalid(who, "unknown mode (DINER_RESIZE_*)");
    return DINER_OK;
}

// ---- device helpers -------------------------------------------------------------------------------------------------------------------
// ATen's nearest_idx: min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out, the product in fp32
__device__ __forceinline__ int nearest_src(int dst, int in, float scale)
{
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? (s < 0 ? 0 : s) : in - 1;
}

// a table's window of output index o, clamped into the source: first in [0, in - 1], first + n <= in, n in [0, taps]
__device__ __forceinline__ void window(const int32_t *__restrict__ bounds, int o, int in, int taps, int &first, int &n)
{
    first = bounds[2 * o];
    n = bounds[2 * o + 1];
    first = first < 0 ? 0 : (first > in - 1 ? in - 1 : first);
    const int room = in - first < taps ? in - first : taps;
    n = n < 0 ? 0 : (n > room ? room : n);
}

// Pass 1 of decode + resize: one workgroup = one source row (blockIdx.x = n H + y) and IW_THREADS output columns of it (blockIdx.y).
// The span of source pixels the columns read is decoded ONCE into LDS (every source pixel feeds about two outputs at a downscale, and
// a decode costs divisions and a root per channel), RS_CHUNK pixels at a time, V pixels per thread and load (V = 4: W % 4 == 0 and aligned
// bases, the 16 / 12 / 4-byte loads of load_pixels4); then thread = output column sums its taps in their order, three channels.
// tmp [N,3,H,w]
template <int V>
__global__ __launch_bounds__(IW_THREADS) void decode_resize_rows_kernel(PixelSource src, ImageFmt fmt, int H, int W, int w,
                                                                        const int32_t *__restrict__ bounds,
                                                                        const float *__restrict__ weights, int taps,
                                                                        float *__restrict__ tmp)
{
    __shared__ float row[3][RS_CHUNK];
    __shared__ int span[2][IW_THREADS / DINER_WAVE];
    const int64_t r = blockIdx.x;
    const int ox = blockIdx.y * IW_THREADS + threadIdx.x;
    const bool live = ox < w;
    int first = 0, n = 0;
    if (live) window(bounds, ox, W, taps, first, n);
    // the columns' span [lo, hi) of the row: block-uniform, so every thread takes the same trips through the barriers below
    int lo = n > 0 ? first : W, hi = n > 0 ? first + n : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        span[0][threadIdx.x >> 6] = lo;
        span[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IW_THREADS / DINER_WAVE; ++i) {
        lo = min(lo, span[0][i]);
        hi = max(hi, span[1][i]);
    }
    const int64_t p0 = r * W;   // the row's first pixel
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int c0 = lo & ~3; c0 < hi; c0 += RS_CHUNK) {
        const int len = min(RS_CHUNK, hi - c0);
        if constexpr (V == 4) {
            for (int g = threadIdx.x; g < (len + 3) / 4; g += IW_THREADS) {   // W % 4 == 0: a group of 4 never leaves the row
                uint32_t b[4][4];
                load_pixels4(src, (p0 + c0) / 4 + g, b);
                float v[3][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float rgb[3], a;
                    decode_pixel(b[i], fmt, rgb, a);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][i] = rgb[c];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(&row[c][4 * g]) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            }
        } else {
            for (int i = threadIdx.x; i < len; i += IW_THREADS) {
                uint32_t b[4];
                float rgb[3], a;
                load_pixel(src, p0 + c0 + i, b);
                decode_pixel(b, fmt, rgb, a);
#pragma unroll
                for (int c = 0; c < 3; ++c) row[c][i] = rgb[c];
            }
        }
        __syncthreads();
        const int j0 = max(first, c0), j1 = min(first + n, c0 + len);
        for (int j = j0; j < j1; ++j) {
            const float wj = weights[(int64_t)ox * taps + (j - first)];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wj, row[c][j - c0], acc[c]);
        }
        __syncthreads();
    }
    if (!live) return;
    const int64_t img = r / H, y = r - img * H;
#pragma unroll
    for (int c = 0; c < 3; ++c) tmp[((img * 3 + c) * H + y) * w + ox] = acc[c];
}

// Pass 2: one thread per output pixel (consecutive threads = consecutive columns) sums its taps down tmp's column, three channels; the
// alpha is the nearest resample of alpha / 255.  rgb_out [N,3,h,w], alpha_out [N,1,h,w] (optional)
__global__ __launch_bounds__(IW_THREADS) void resize_cols_kernel(const float *__restrict__ tmp, PixelSource src, int64_t N, int H, int W, int h,
                                                                 int w, const int32_t *__restrict__ bounds,
                                                                 const float *__restrict__ weights, int taps, float sy, float sx,
                                                                 float *__restrict__ rgb_out, float *__restrict__ alpha_out)
{
    const int64_t i = (int64_t)blockIdx.x * IW_THREADS + threadIdx.x;
    if (i >= N * h * w) return;
    const int64_t img = i / ((int64_t)h * w);
    const int p = (int)(i - img * h * w), oy = p / w, ox = p - oy * w;
    int first, n;
    window(bounds, oy, H, taps, first, n);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *col = tmp + ((img * 3 + c) * H + first) * w + ox;
        float acc = 0.0f;
        for (int k = 0; k < n; ++k) acc = __builtin_fmaf(weights[(int64_t)oy * taps + k], col[(int64_t)k * w], acc);
        rgb_out[((img * 3 + c) * h + oy) * w + ox] = acc;
    }
    if (alpha_out) {
        const int64_t q = (img * H + nearest_src(oy, H, sy)) * W + nearest_src(ox, W, sx);
        const uint32_t a = src.alpha ? src.alpha[q] : src.pixels[q * 4 + 3];
        alpha_out[i] = (float)a / 255.0f;
    }
}

// One axis of PIL's 8-bit resize: in [outer, len_in, inner] -> out [outer, len_out, inner], one thread per output byte:
// clip((2^21 + sum byte k) >> 22, 0, 255), integer arithmetic (ImagingResampleHorizontal_8bpc / Vertical_8bpc)
__global__ __launch_bounds__(IW_THREADS) void resize_u8_axis_kernel(const uint8_t *__restrict__ in, int64_t total, int len_in, int len_out,
                                                                    int64_t inner, const int32_t *__restrict__ bounds,
                                                                    const int32_t *__restrict__ k, int taps, uint8_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * IW_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t t = i / inner, e = i - t * inner, q = t / len_out;
    const int o = (int)(t - q * len_out);
    int first, n;
    window(bounds, o, len_in, taps, first, n);
    const uint8_t *p = in + (q * len_in + first) * inner + e;
    uint32_t acc = 1u << (RS_PRECISION_BITS - 1);   // unsigned: wraps like the two's complement sum, whatever a table holds
    for (int j = 0; j < n; ++j) acc += (uint32_t)p[(int64_t)j * inner] * (uint32_t)k[(int64_t)o * taps + j];
    const int v = (int32_t)acc >> RS_PRECISION_BITS;
    out[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One thread per output texel: decode_depth_texel_mf of the texel that the nearest resample selects
__global__ __launch_bounds__(IW_THREADS) void decode_depth_mf_nearest_kernel(const unsigned short *__restrict__ depth,
                                                                             const unsigned short *__restrict__ conf, int64_t N, int H, int W,
                                                                             int h, int w, float sy, float sx, float mul0, float std_a,
                                                                             float std_b, float const_std, float *__restrict__ depth_out,
                                                                             float *__restrict__ std_out, float *__restrict__ mask_out)
{
    const int64_t i = (int64_t)blockIdx.x * IW_THREADS + threadIdx.x;
    if (i >= N * h * w) return;
    const int64_t img = i / ((int64_t)h * w);
    const int p = (int)(i - img * h * w), oy = p / w, ox = p - oy * w;
    float d, s;
    decode_depth_texel_mf(depth, conf, (img * H + nearest_src(oy, H, sy)) * W + nearest_src(ox, W, sx), mul0, std_a, std_b, const_std, d, s);
    depth_out[i] = d;
    std_out[i] = s;
    if (mask_out) mask_out[i] = d > 0.0f ? 1.0f : 0.0f;
}

// sizes every entry shares: N images of H x W to h x w (before any launch)
int check_resize_sizes(const char *who, int64_t N, int32_t H, int32_t W, int32_t h, int32_t w)
{
    if (N <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return invalid(who, "non-positive size (N, H, W, h, w)");
    if ((int64_t)H * W > 0x7fffffff || (int64_t)h * w > 0x7fffffff || (int64_t)H * w > 0x7fffffff || N > 65535 || N * H > 0x7fffffff) {
        set_error("%s: N=%lld images of %d x %d to %d x %d unsupported (planes below 2^31 elements, N <= 65535, N H < 2^31)", who,
                  (long long)N, H, W, h, w);
        return DINER_E_UNSUPPORTED;
    }
    return DINER_OK;
}

int64_t blocks_of(int64_t n) { return (n + IW_THREADS - 1) / IW_THREADS; }

int check_grid(const char *who, int64_t blocks)
{
    if (blocks > 0x7fffffff) {
        set_error("%s: %lld workgroups are beyond one launch's grid", who, (long long)blocks);
        return DINER_E_UNSUPPORTED;
    }
    return DINER_OK;
}

}  // namespace

}  // namespace diner

using namespace diner;

int diner_resize_taps(int32_t in, int32_t out, int32_t mode)
{
    if (const int rc = check_axis("resize_taps", in, out, mode)) return rc;
    int taps = 1;
    for (int i = 0; i < out; ++i) {
        int xmin;
        const int n = axis_window(in, out, mode, i, xmin, nullptr);
        taps = n > taps ? n : taps;
    }
    return taps;
}

int diner_resize_table(int32_t in, int32_t out, int32_t mode, int32_t taps, int32_t *bounds, void *weights)
{
    const char *who = "resize_table";
    if (const int rc = check_axis(who, in, out, mode)) return rc;
    if (!bounds || !weights) return invalid(who, "NULL pointer");
    const int need = diner_resize_taps(in, out, mode);
    if (taps < need) return invalid(who, "taps below diner_resize_taps(in, out, mode)");
    double *w = new double[need];
    for (int i = 0; i < out; ++i) {
        int xmin;
        int n = axis_window(in, out, mode, i, xmin, w);
        n = n < 0 ? 0 : n;
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = n;
        for (int j = 0; j < taps; ++j) {
            const double v = j < n ? w[j] : 0.0;
            if (mode == DINER_RESIZE_BICUBIC_U8)   // PIL's normalize_coeffs_8bpc
                static_cast<int32_t *>(weights)[(int64_t)i * taps + j] =
                    v < 0 ? (int32_t)(-0.5 + v * (1 << RS_PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << RS_PRECISION_BITS));
            else
                static_cast<float *>(weights)[(int64_t)i * taps + j] = (float)v;
        }
    }
    delete[] w;
    return DINER_OK;
}

int diner_decode_image_u8_resized(const uint8_t *pixels, const uint8_t *alpha, int64_t N, int32_t H, int32_t W, int32_t C, int32_t bg_rule,
                                  float bg, int32_t gamma, int32_t symmetric_range, int32_t h, int32_t w, const int32_t *bounds_x,
                                  const float *weights_x, int32_t taps_x, const int32_t *bounds_y, const float *weights_y, int32_t taps_y,
                                  float *tmp, float *rgb_out, float *alpha_out, void *stream)
{
    const char *who = "decode_image_u8_resized";
    if (const int rc = check_source(who, pixels, alpha, C, bg_rule)) return rc;
    if (!rgb_out || !tmp || !bounds_x || !weights_x || !bounds_y || !weights_y) return invalid(who, "NULL pointer");
    if (alpha_out && C != 4 && !alpha) return invalid(who, "alpha_out without any alpha (neither C == 4 nor a plane)");
    if (taps_x <= 0 || taps_y <= 0) return invalid(who, "non-positive number of taps");
    if (const int rc = check_resize_sizes(who, N, H, W, h, w)) return rc;
    const int64_t cols = blocks_of(w), blocks2 = blocks_of(N * h * w);
    if (cols > 65535) {
        set_error("%s: w=%d is beyond one launch's grid", who, w);
        return DINER_E_UNSUPPORTED;
    }
    if (const int rc = check_grid(who, blocks2)) return rc;
    const PixelSource src = {pixels, alpha, C};
    const ImageFmt fmt = {bg_rule, bg, gamma != 0, symmetric_range != 0};
    const bool vec = W % 4 == 0 && ((uintptr_t)pixels & (C == 4 ? 15 : 3)) == 0 && ((uintptr_t)alpha & 3) == 0;
    const dim3 grid1((unsigned)(N * H), (unsigned)cols);
    if (vec)
        hipLaunchKernelGGL(decode_resize_rows_kernel<4>, grid1, dim3(IW_THREADS), 0, (hipStream_t)stream, src, fmt, H, W, w, bounds_x,
                           weights_x, taps_x, tmp);
    else
        hipLaunchKernelGGL(decode_resize_rows_kernel<1>, grid1, dim3(IW_THREADS), 0, (hipStream_t)stream, src, fmt, H, W, w, bounds_x,
                           weights_x, taps_x, tmp);
    if (const int rc = check_launch("decode_resize_rows_kernel")) return rc;
    hipLaunchKernelGGL(resize_cols_kernel, dim3((unsigned)blocks2), dim3(IW_THREADS), 0, (hipStream_t)stream, tmp, src, N, H, W, h, w,
                       bounds_y, weights_y, taps_y, (float)H / (float)h, (float)W / (float)w, rgb_out, alpha_out);
    return check_launch("resize_cols_kernel");
}

int diner_resize_u8(const uint8_t *pixels, int64_t N, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, const int32_t *bounds_x,
                    const int32_t *weights_x, int32_t taps_x, const int32_t *bounds_y, const int32_t *weights_y, int32_t taps_y,
                    uint8_t *tmp, uint8_t *out, void *stream)
{
    const char *who = "resize_u8";
    if (!pixels || !out) return invalid(who, "NULL pointer");
    if (C != 1 && C != 3) return invalid(who, "C must be 1 or 3 (PIL premultiplies RGBA: not served)");
    if (const int rc = check_resize_sizes(who, N, H, W, h, w)) return rc;
    const bool horiz = w != W, vert = h != H;   // a pass whose size does not change is skipped, as PIL skips it
    if (horiz && (!bounds_x || !weights_x || taps_x <= 0)) return invalid(who, "NULL pointer or non-positive taps (the horizontal table)");
    if (vert && (!bounds_y || !weights_y || taps_y <= 0)) return invalid(who, "NULL pointer or non-positive taps (the vertical table)");
    if (horiz && vert && !tmp) return invalid(who, "NULL pointer (tmp with both passes)");
    const int64_t n1 = N * H * w * C, n2 = N * h * w * C;
    if (const int rc = check_grid(who, blocks_of(n1 > n2 ? n1 : n2))) return rc;
    if (!horiz && !vert) {
        if (hipMemcpyAsync(out, pixels, (size_t)n2, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
            set_error("%s: the copy failed", who);
            return DINER_E_LAUNCH;
        }
        return DINER_OK;
    }
    const uint8_t *mid = pixels;
    if (horiz) {
        uint8_t *dst = vert ? tmp : out;
        hipLaunchKernelGGL(resize_u8_axis_kernel, dim3((unsigned)blocks_of(n1)), dim3(IW_THREADS), 0, (hipStream_t)stream, pixels, n1, W, w,
                           (int64_t)C, bounds_x, weights_x, taps_x, dst);
        if (const int rc = check_launch("resize_u8_axis_kernel")) return rc;
        mid = dst;
    }
    if (vert) {
        hipLaunchKernelGGL(resize_u8_axis_kernel, dim3((unsigned)blocks_of(n2)), dim3(IW_THREADS), 0, (hipStream_t)stream, mid, n2, H, h,
                           (int64_t)w * C, bounds_y, weights_y, taps_y, out);
        return check_launch("resize_u8_axis_kernel");
    }
    return DINER_OK;
}

int diner_decode_depth_u16_mf_nearest(const uint16_t *depth, const uint16_t *conf, int64_t N, int32_t H, int32_t W, int32_t h, int32_t w,
                                      float mul0, float std_a, float std_b, float const_std, float *depth_out, float *std_out,
                                      float *mask_out, void *stream)
{
    const char *who = "decode_depth_u16_mf_nearest";
    if (!depth || !depth_out || !std_out) return invalid(who, "NULL pointer");
    if (const int rc = check_resize_sizes(who, N, H, W, h, w)) return rc;
    const int64_t blocks = blocks_of(N * h * w);
    if (const int rc = check_grid(who, blocks)) return rc;
    hipLaunchKernelGGL(decode_depth_mf_nearest_kernel, dim3((unsigned)blocks), dim3(IW_THREADS), 0, (hipStream_t)stream, depth, conf, N, H, W,
                       h, w, (float)H / (float)h, (float)W / (float)w, mul0, std_a, std_b, const_std, depth_out, std_out, mask_out);
    return check_launch("decode_depth_mf_nearest_kernel");
}
