// The loader of the datasets' image bytes, shared by the units that read them: image_wire.hip (decode, the encoder's head from bytes)
// and image_resize.hip (decode fused with the resize).  One device function, decode_pixel, holds the readers' arithmetic: one rounding
// per reference operation (-ffp-contract=off), a true division by 255, a correctly rounded root; decode_depth_texel_mf holds Multiface's
// depth / std rule of one texel.
#pragma once
#include "encoder_input_kernel.hpp"

namespace diner {

namespace {

constexpr int IW_THREADS = 256;

// where the bytes are: pixels [N,H,W,C] interleaved, C in {3, 4}; alpha (optional) [N,H,W], which wins over a fourth channel
struct PixelSource {
    const uint8_t *__restrict__ pixels;
    const uint8_t *__restrict__ alpha;
    int C;
};

struct ImageFmt {
    int bg_rule;    // DINER_BG_*
    float bg;
    int gamma, symmetric;
};

// MultiFaceDataset.gammaCorrect (multiface.py:81-95) of channel c, then read_img's clip(0, 1) (:68)
__device__ __forceinline__ float gamma_correct(float v, int c)
{
    const float scale = c == 0 ? 1.4f : (c == 1 ? 1.1f : 1.6f);                      // color_scale as torch.tensor(..): float32
    const float black = (float)(3.0 / 255.0), offset = (float)(15.0 / 255.0);
    const float gain = (float)((1.0 / (1 - 3.0 / 255.0)) * 0.95);                    // a python double that meets a float32 tensor
    float t = (v * scale) / 1.1f;                                                    // :93
    t = fminf(fmaxf(t - black, 0.0f), 2.0f);                                         // :95 torch.clamp(img - black, 0, 2)
    t = gain * t;
    t = sqrtf(t);                                                                    // ** (1 / gamma), gamma = 2: correctly rounded
    t = fminf(fmaxf(t - offset, 0.0f), 2.0f);
    return fminf(fmaxf(t, 0.0f), 1.0f);                                              // :68
}

// THE place that decodes a pixel: its bytes (b[3] = 255 when the source has no alpha) -> the three colour values and alpha, in the
// readers' order: / 255, gamma, the symmetric range, and last the background fill with `bg` as given (facescape.py:60-65,
// multiface.py:66-71,322-323)
__device__ __forceinline__ void decode_pixel(const uint32_t (&b)[4], const ImageFmt &fmt, float (&rgb)[3], float &a)
{
    a = (float)b[3] / 255.0f;
    const bool hole = fmt.bg_rule == DINER_BG_BELOW_HALF ? a < 0.5f : (fmt.bg_rule == DINER_BG_BELOW_ONE ? a < 1.0f : false);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = (float)b[c] / 255.0f;
        if (fmt.gamma) v = gamma_correct(v, c);
        if (fmt.symmetric) {
            v = v * 2.0f;
            v = v - 1.0f;
        }
        rgb[c] = hole ? fmt.bg : v;
    }
}

// the bytes of pixel p (an index into [N,H,W]), any alignment
__device__ __forceinline__ void load_pixel(const PixelSource &s, int64_t p, uint32_t (&b)[4])
{
    const uint8_t *q = s.pixels + p * s.C;
    b[0] = q[0]; b[1] = q[1]; b[2] = q[2];
    b[3] = s.alpha ? s.alpha[p] : (s.C == 4 ? q[3] : 255u);
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }

// the bytes of the 4 pixels 4 q .. 4 q + 3: 16 bytes in one load (C = 4: pixels 16-byte aligned) or 12 bytes in three 4-byte loads
// (C = 3: 4-byte aligned), the alpha plane's 4 bytes in one (4-byte aligned)
__device__ __forceinline__ void load_pixels4(const PixelSource &s, int64_t q, uint32_t (&b)[4][4])
{
    if (s.C == 4) {
        const uint4 w = reinterpret_cast<const uint4 *>(s.pixels)[q];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) b[i][c] = byte_of(ws[i], c);
    } else {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(s.pixels) + q * 3;
        const uint32_t ws[3] = {src[0], src[1], src[2]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) b[i][c] = byte_of(ws[(3 * i + c) / 4], (3 * i + c) % 4);
            b[i][3] = 255u;
        }
    }
    if (s.alpha) {
        const uint32_t w = reinterpret_cast<const uint32_t *>(s.alpha)[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i][3] = byte_of(w, i);
    }
}

// Multiface's depth and std of one texel: depth = u16 * mul0 (multiface.py:107); std = max(std_a * (conf * mul0) + std_b, 0) (:309-310, a
// multiplication and an addition) or const_std without a confidence plane (:307); std = 0 where depth == 0 (:311)
__device__ __forceinline__ void decode_depth_texel_mf(const unsigned short *__restrict__ depth, const unsigned short *__restrict__ conf,
                                                      int64_t src, float mul0, float std_a, float std_b, float const_std, float &d, float &s)
{
    d = (float)depth[src] * mul0;
    s = const_std;
    if (conf) {
        s = std_a * ((float)conf[src] * mul0) + std_b;
        s = s < 0.0f ? 0.0f : s;
    }
    s = d == 0.0f ? 0.0f : s;
}

// the checks of a byte source and its format (before any launch)
int check_source(const char *who, const uint8_t *pixels, const uint8_t *alpha, int32_t C, int32_t bg_rule)
{
    if (!pixels) return invalid(who, "NULL pointer");
    if (C != 3 && C != 4) return invalid(who, "C must be 3 (RGB) or 4 (RGBA)");
    if (bg_rule != DINER_BG_NONE && bg_rule != DINER_BG_BELOW_HALF && bg_rule != DINER_BG_BELOW_ONE)
        return invalid(who, "unknown bg_rule (DINER_BG_*)");
    if (bg_rule != DINER_BG_NONE && C != 4 && !alpha) return invalid(who, "a background rule without any alpha (neither C == 4 nor a plane)");
    return DINER_OK;
}

}  // namespace

}  // namespace diner
