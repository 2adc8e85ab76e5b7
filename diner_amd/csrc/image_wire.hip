// The datasets' image bytes and Multiface's depth planes, decoded on the device (PNG decoding stays on the host):
//   decode_image      reference src/data/facescape.py:59-66 (read_rgba), src/data/dtu.py:83-88 (read_rgb),
//                     src/data/multiface.py:65-95 (read_img, read_alpha, gammaCorrect) and :322-323 (the white fill)
//   decode_depth_mf   src/data/multiface.py:103-109 (read_depth) and :305-311 (the std: a constant or clip(a conf + b, min=0), 0 at depth 0)
//   encoder_input_u8  conv1's input straight from the bytes: encoder_input_kernel.hpp's kernel with a loader that decodes a pixel
// One device function, decode_pixel (image_pixel.hpp, shared with image_resize.hip), holds the readers' arithmetic: one rounding per
// reference operation (-ffp-contract=off), a true division by 255, a correctly rounded root.  No atomics, no LDS; every output element is
// written; element offsets are 64-bit.
#include "image_pixel.hpp"

namespace diner {

namespace {

// One thread = V consecutive pixels (V = 4: W % 4 == 0, so the four share a row and the planes' float4 stores are aligned).
// rgb_out [N,3,H,W], alpha_out [N,1,H,W] (optional)
template <int V>
__global__ __launch_bounds__(IW_THREADS) void decode_image_kernel(PixelSource src, ImageFmt fmt, int64_t groups, int64_t HW,
                                                                  float *__restrict__ rgb_out, float *__restrict__ alpha_out)
{
    const int64_t q = (int64_t)blockIdx.x * IW_THREADS + threadIdx.x;
    if (q >= groups) return;
    uint32_t b[V][4];
    if constexpr (V == 4) load_pixels4(src, q, b);
    else load_pixel(src, q, b[0]);
    float v[3][V], a[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float rgb[3];
        decode_pixel(b[i], fmt, rgb, a[i]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][i] = rgb[c];
    }
    const int64_t p = q * V, n = p / HW, r = p - n * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) store_pixels<V>(rgb_out + (n * 3 + c) * HW + r, v[c]);
    if (alpha_out) store_pixels<V>(alpha_out + p, a);
}

// the bytes as the loader of encoder_input_kernel: the pixel decoded where the fp32 loader reads it
struct ByteImages {
    PixelSource src;
    ImageFmt fmt;
    __device__ __forceinline__ void load(int n, int H, int W, int y, int x, float (&rgb)[3]) const
    {
        uint32_t b[4];
        float a;
        load_pixel(src, ((int64_t)n * H + y) * W + x, b);
        decode_pixel(b, fmt, rgb, a);
    }
};

// One thread per OUTPUT pixel, out(y, x) = in(y stride, x stride) as decode_depth_kernel (encode_glue.hip).  depth = u16 * mul0
// (multiface.py:107); std = max(std_a * (conf * mul0) + std_b, 0) (:309-310, a multiplication and an addition) or const_std without a
// confidence plane (:307); std = 0 where depth == 0 (:311)
__global__ __launch_bounds__(IW_THREADS) void decode_depth_mf_kernel(const unsigned short *__restrict__ depth,
                                                                     const unsigned short *__restrict__ conf, int64_t N, int Hin, int Win,
                                                                     int stride, float mul0, float std_a, float std_b, float const_std,
                                                                     float *__restrict__ depth_out, float *__restrict__ std_out,
                                                                     float *__restrict__ mask_out)
{
    const int Ho = Hin / stride, Wo = Win / stride;
    const int64_t i = (int64_t)blockIdx.x * IW_THREADS + threadIdx.x;
    if (i >= N * Ho * Wo) return;
    const int64_t n = i / ((int64_t)Ho * Wo);
    const int p = (int)(i - n * Ho * Wo), y = p / Wo, x = p - y * Wo;
    const int64_t src = (n * Hin + (int64_t)y * stride) * Win + (int64_t)x * stride;
    float d, s;
    decode_depth_texel_mf(depth, conf, src, mul0, std_a, std_b, const_std, d, s);
    depth_out[i] = d;
    std_out[i] = s;
    if (mask_out) mask_out[i] = d > 0.0f ? 1.0f : 0.0f;
}

}  // namespace

}  // namespace diner

using namespace diner;

int diner_decode_image_u8(const uint8_t *pixels, const uint8_t *alpha, int64_t N, int32_t H, int32_t W, int32_t C, int32_t bg_rule, float bg,
                          int32_t gamma, int32_t symmetric_range, float *rgb_out, float *alpha_out, void *stream)
{
    const char *who = "decode_image_u8";
    if (const int rc = check_source(who, pixels, alpha, C, bg_rule)) return rc;
    if (!rgb_out) return invalid(who, "NULL pointer");
    if (alpha_out && C != 4 && !alpha) return invalid(who, "alpha_out without any alpha (neither C == 4 nor a plane)");
    if (N <= 0 || H <= 0 || W <= 0) return invalid(who, "non-positive size (N, H, W)");
    const int64_t HW = (int64_t)H * W;
    if (HW > 0x7fffffff || N > 65535) {
        set_error("%s: N=%lld images of %d x %d pixels unsupported (H W < 2^31, N <= 65535)", who, (long long)N, H, W);
        return DINER_E_UNSUPPORTED;
    }
    const bool vec = W % 4 == 0 && ((uintptr_t)pixels & (C == 4 ? 15 : 3)) == 0 && ((uintptr_t)alpha & 3) == 0 &&
                     ((uintptr_t)rgb_out & 15) == 0 && ((uintptr_t)alpha_out & 15) == 0;
    const int64_t groups = N * HW / (vec ? 4 : 1), blocks = (groups + IW_THREADS - 1) / IW_THREADS;
    if (blocks > 0x7fffffff) {
        set_error("%s: N=%lld images of %d x %d pixels are beyond one launch's grid", who, (long long)N, H, W);
        return DINER_E_UNSUPPORTED;
    }
    const PixelSource src = {pixels, alpha, C};
    const ImageFmt fmt = {bg_rule, bg, gamma != 0, symmetric_range != 0};
    if (vec)
        hipLaunchKernelGGL(decode_image_kernel<4>, dim3((unsigned)blocks), dim3(IW_THREADS), 0, (hipStream_t)stream, src, fmt, groups, HW,
                           rgb_out, alpha_out);
    else
        hipLaunchKernelGGL(decode_image_kernel<1>, dim3((unsigned)blocks), dim3(IW_THREADS), 0, (hipStream_t)stream, src, fmt, groups, HW,
                           rgb_out, alpha_out);
    return check_launch("decode_image_kernel");
}

int diner_decode_depth_u16_mf(const uint16_t *depth, const uint16_t *conf, int64_t N, int32_t H, int32_t W, int32_t stride, float mul0,
                              float std_a, float std_b, float const_std, float *depth_out, float *std_out, float *mask_out, void *stream)
{
    const char *who = "decode_depth_u16_mf";
    if (!depth || !depth_out || !std_out) return invalid(who, "NULL pointer");
    if (N < 0 || H <= 0 || W <= 0 || stride <= 0 || H % stride || W % stride) return invalid(who, "bad size (stride must divide H and W)");
    if ((int64_t)H * W > 0x7fffffff || N > 65535) {
        set_error("%s: N=%lld planes of %d x %d unsupported (H W < 2^31, N <= 65535)", who, (long long)N, H, W);
        return DINER_E_UNSUPPORTED;
    }
    const int64_t n = N * (H / stride) * (int64_t)(W / stride), blocks = (n + IW_THREADS - 1) / IW_THREADS;
    if (blocks > 0x7fffffff) {
        set_error("%s: N=%lld planes of %d x %d are beyond one launch's grid", who, (long long)N, H, W);
        return DINER_E_UNSUPPORTED;
    }
    if (n == 0) return DINER_OK;
    hipLaunchKernelGGL(decode_depth_mf_kernel, dim3((unsigned)blocks), dim3(IW_THREADS), 0, (hipStream_t)stream, depth, conf, N, H, W, stride,
                       mul0, std_a, std_b, const_std, depth_out, std_out, mask_out);
    return check_launch("decode_depth_mf_kernel");
}

int diner_encoder_input_u8(const uint8_t *pixels, const uint8_t *alpha, int32_t C, int32_t bg_rule, float bg, int32_t gamma,
                           int32_t symmetric_range, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, const float *xs,
                           const float *ys, float mean0, float mean1, float mean2, float std0, float std1, float std2, float *out,
                           void *stream)
{
    const char *who = "encoder_input_u8";
    const Norm3 nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    int Cpe = 0;
    if (const int rc = check_sizes(who, N, H, W, pad, pe_freqs, nm.std, Cpe)) return rc;
    if (const int rc = check_source(who, pixels, alpha, C, bg_rule)) return rc;
    const ByteImages images = {{pixels, alpha, C}, {bg_rule, bg, gamma != 0, symmetric_range != 0}};
    return launch_encoder_input(who, images, N, H, W, pad, Cpe, xs, ys, nm, out, stream);
}
