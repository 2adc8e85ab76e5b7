// The forward kernel of the encoder's head (encoder_input.hip explains what it computes), as a template over where a pixel's three
// colour values come from: `Loader::load(n, H, W, y, x, rgb)` returns the pixel (y, x) of image n before Normalize.  Two translation
// units instantiate it: encoder_input.hip with the fp32 images [N,3,H,W] (diner_encoder_input), image_wire.hip with the datasets' bytes
// decoded on the fly (diner_encoder_input_u8).  The normalise, the replicate pad, the padding's positional encoding, the argument checks
// and the launch exist here only.
#pragma once
#include "common.hpp"

namespace diner {

namespace {

constexpr int EI_THREADS = 256;
constexpr int EI_MAX_FREQS = 30;      // f_k = fp32(pi) * 2^k from an int shift
constexpr int EI_MAX_PAD = 4095;      // the backward holds 2 (pad + 1) column sums in LDS (32 KiB)

struct Norm3 {
    float mean[3], std[3];
};

// the fp32 images [N,3,H,W]
struct FloatImages {
    const float *__restrict__ images;
    __device__ __forceinline__ void load(int n, int H, int W, int y, int x, float (&rgb)[3]) const
    {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = images[(((int64_t)n * 3 + c) * H + y) * W + x];
    }
};

template <int V>
__device__ __forceinline__ void store_pixels(float *__restrict__ dst, const float (&v)[V])
{
    if constexpr (V == 4) *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[0] = v[0];
}

// One thread = V consecutive pixels of one padded row (V = 4: one 16-byte store per channel plane; V = 1: any width or alignment).
// blockIdx.y = n: the thread writes image n's three channels, and the encoding's channels k = n, n + gridDim.y, ... to every image,
// so each encoding value is computed by exactly one thread and the stores are spread over the whole grid.
template <int V, class Loader>
__global__ __launch_bounds__(EI_THREADS) void encoder_input_kernel(Loader images, int N, int H, int W, int pad, int Cpe,
                                                                   const float *__restrict__ xs, const float *__restrict__ ys, Norm3 nm,
                                                                   float *__restrict__ out)
{
    const int Hp = H + 2 * pad, Wp = W + 2 * pad, Wq = Wp / V, Ct = 3 + Cpe;
    const int64_t q = (int64_t)blockIdx.x * EI_THREADS + threadIdx.x;
    if (q >= (int64_t)Hp * Wq) return;
    const int y = (int)(q / Wq), x0 = (int)(q - (int64_t)y * Wq) * V;
    const int64_t plane = (int64_t)Hp * Wp, pix = (int64_t)y * Wp + x0;
    const int n = blockIdx.y;

    // channels 0..2: replicate pad of the normalised image (a true fp32 divide, as Normalize's)
    const int ys_ = min(max(y - pad, 0), H - 1);
    float v[3][V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float rgb[3];
        images.load(n, H, W, ys_, min(max(x0 + i - pad, 0), W - 1), rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][i] = (rgb[c] - nm.mean[c]) / nm.std[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_pixels<V>(out + ((int64_t)n * Ct + c) * plane + pix, v[c]);
    if (Cpe == 0) return;

    // channels 3..: [x, y, e_0, ...], e[2 j + i] = sin(phi_j + v_i f_(j / 2)); 0 on the image's own pixels, which compute no sine
    const bool row_in = y >= pad && y < Hp - pad;
    bool in[V], all_in = true;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        in[i] = row_in && x0 + i >= pad && x0 + i < Wp - pad;
        all_in = all_in && in[i];
    }
    float vx[V], vy = 0.f;
    if (!all_in) {
        vy = ys[y];
#pragma unroll
        for (int i = 0; i < V; ++i) vx[i] = xs[x0 + i];
    }
    const float pi = 3.14159265358979323846f, half_pi = 1.5707963267948966f;
    for (int k = n; k < Cpe; k += gridDim.y) {
        float e[V];
#pragma unroll
        for (int i = 0; i < V; ++i) e[i] = 0.f;
        if (!all_in) {
            if (k < 2) {
#pragma unroll
                for (int i = 0; i < V; ++i) e[i] = in[i] ? 0.f : (k == 0 ? vx[i] : vy);
            } else {
                const int j = (k - 2) >> 1;
                const float f = pi * (float)(1 << (j >> 1)), phi = (j & 1) ? half_pi : 0.0f;
                if ((k - 2) & 1) {   // the y component: one value for the row
                    const float s = pe_sin(__builtin_fmaf(vy, f, phi));
#pragma unroll
                    for (int i = 0; i < V; ++i) e[i] = in[i] ? 0.f : s;
                } else {
#pragma unroll
                    for (int i = 0; i < V; ++i) e[i] = in[i] ? 0.f : pe_sin(__builtin_fmaf(vx[i], f, phi));
                }
            }
        }
        float *dst = out + (int64_t)(3 + k) * plane + pix;
        for (int m = 0; m < N; ++m, dst += (int64_t)Ct * plane) store_pixels<V>(dst, e);
    }
}

int invalid(const char *who, const char *what)
{
    set_error("%s: %s", who, what);
    return DINER_E_INVALID;
}

// argument checks shared by both directions and both sources (before any launch); Cpe: channels of the encoding
int check_sizes(const char *who, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, const float *std3, int &Cpe)
{
    if (N <= 0 || H <= 0 || W <= 0) return invalid(who, "non-positive size (N, H, W)");
    if (pad < 0) return invalid(who, "negative pad");
    if (pe_freqs < -1) return invalid(who, "pe_freqs below -1 (-1: no encoding channels)");
    if ((int64_t)H + 2 * (int64_t)pad < 2 || (int64_t)W + 2 * (int64_t)pad < 2)
        return invalid(who, "a padded size below 2 (H + 2 pad and W + 2 pad must be at least 2)");
    for (int c = 0; c < 3; ++c)
        if (!(std3[c] != 0.0f)) return invalid(who, "std of 0 or NaN");
    if (pe_freqs > EI_MAX_FREQS || (int64_t)H + 2 * (int64_t)pad > 0x3fffffff || (int64_t)W + 2 * (int64_t)pad > 0x3fffffff) {
        set_error("%s: pe_freqs=%d, pad=%d, H=%d, W=%d unsupported (pe_freqs up to %d, padded sizes below 2^30)", who, pe_freqs, pad, H, W,
                  EI_MAX_FREQS);
        return DINER_E_UNSUPPORTED;
    }
    Cpe = (pe_freqs >= 0 && pad > 0) ? 2 * (1 + 2 * pe_freqs) : 0;
    return DINER_OK;
}

// the forward's launch: `images` has been checked by the caller, the sizes by check_sizes
template <class Loader>
int launch_encoder_input(const char *who, Loader images, int64_t N, int32_t H, int32_t W, int32_t pad, int Cpe, const float *xs,
                         const float *ys, const Norm3 &nm, float *out, void *stream)
{
    if (!out) return invalid(who, "NULL pointer");
    if (Cpe > 0 && (!xs || !ys)) return invalid(who, "NULL pointer (xs / ys with the encoding on)");
    if (N > 65535) {
        set_error("%s: N=%lld images unsupported (at most 65535)", who, (long long)N);
        return DINER_E_UNSUPPORTED;
    }
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const bool vec = Wp % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const int64_t blocks = ((int64_t)Hp * (Wp / (vec ? 4 : 1)) + EI_THREADS - 1) / EI_THREADS;
    if (blocks > 0x7fffffff) {
        set_error("%s: a padded image of %d x %d pixels is beyond one launch's grid", who, Hp, Wp);
        return DINER_E_UNSUPPORTED;
    }
    const dim3 grid((unsigned)blocks, (unsigned)N);
    if (vec)
        hipLaunchKernelGGL((encoder_input_kernel<4, Loader>), grid, dim3(EI_THREADS), 0, (hipStream_t)stream, images, (int)N, H, W, pad, Cpe,
                           xs, ys, nm, out);
    else
        hipLaunchKernelGGL((encoder_input_kernel<1, Loader>), grid, dim3(EI_THREADS), 0, (hipStream_t)stream, images, (int)N, H, W, pad, Cpe,
                           xs, ys, nm, out);
    return check_launch("encoder_input_kernel");
}

}  // namespace

}  // namespace diner
