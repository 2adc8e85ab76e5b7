// The head of the encoder (reference src/models/pixelnerf.py:44 + src/models/image_encoder.py:222-232) in one kernel: conv1's input
// [N, 3 + Cpe, H + 2 pad, W + 2 pad] = the images normalised ((x - mean) / std), replicate-padded by `pad`, and -- when the encoder has
// a positional encoding of its padding (padding_pe >= 0 and pad > 0) -- the Cpe = 2 (1 + 2F) channels of
// PositionalEncoding(F, freq_factor = pi, d_in = 2) of the pixel's (x, y) in [-1, 1]^2, zero over the image's own pixels.  The reference
// builds it from a dozen ATen launches (normalise, pad, linspace x 2, meshgrid, stack, the encoding's repeat / addcmul / sin / cat, the
// interior's zero fill, expand, cat) that move the tensor about three times; here it is written once.  The encoding does not depend on
// the image: every value is computed once per pixel and stored to all N images.
// And the adjoint to the images: the replicate pad's gather (an edge pixel sums the padding that was copied from it), in a fixed order.
#include "common.hpp"

namespace diner {

namespace {

constexpr int EI_THREADS = 256;
constexpr int EI_MAX_FREQS = 30;      // f_k = fp32(pi) * 2^k from an int shift
constexpr int EI_MAX_PAD = 4095;      // the backward holds 2 (pad + 1) column sums in LDS (32 KiB)

struct Norm3 {
    float mean[3], std[3];
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
template <int V>
__global__ __launch_bounds__(EI_THREADS) void encoder_input_kernel(const float *__restrict__ images, int N, int H, int W, int pad,
                                                                   int Cpe, const float *__restrict__ xs, const float *__restrict__ ys,
                                                                   Norm3 nm, float *__restrict__ out)
{
    const int Hp = H + 2 * pad, Wp = W + 2 * pad, Wq = Wp / V, Ct = 3 + Cpe;
    const int64_t q = (int64_t)blockIdx.x * EI_THREADS + threadIdx.x;
    if (q >= (int64_t)Hp * Wq) return;
    const int y = (int)(q / Wq), x0 = (int)(q - (int64_t)y * Wq) * V;
    const int64_t plane = (int64_t)Hp * Wp, pix = (int64_t)y * Wp + x0;
    const int n = blockIdx.y;

    // channels 0..2: replicate pad of the normalised image (a true fp32 divide, as Normalize's)
    const int ys_ = min(max(y - pad, 0), H - 1);
    int sx[V];
#pragma unroll
    for (int i = 0; i < V; ++i) sx[i] = min(max(x0 + i - pad, 0), W - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *src = images + (((int64_t)n * 3 + c) * H + ys_) * W;
        float v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = (src[sx[i]] - nm.mean[c]) / nm.std[c];
        float *dst = out + ((int64_t)n * Ct + c) * plane + pix;
        store_pixels<V>(dst, v);
    }
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
        float v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = 0.f;
        if (!all_in) {
            if (k < 2) {
#pragma unroll
                for (int i = 0; i < V; ++i) v[i] = in[i] ? 0.f : (k == 0 ? vx[i] : vy);
            } else {
                const int j = (k - 2) >> 1;
                const float f = pi * (float)(1 << (j >> 1)), phi = (j & 1) ? half_pi : 0.0f;
                if ((k - 2) & 1) {   // the y component: one value for the row
                    const float s = pe_sin(__builtin_fmaf(vy, f, phi));
#pragma unroll
                    for (int i = 0; i < V; ++i) v[i] = in[i] ? 0.f : s;
                } else {
#pragma unroll
                    for (int i = 0; i < V; ++i) v[i] = in[i] ? 0.f : pe_sin(__builtin_fmaf(vx[i], f, phi));
                }
            }
        }
        float *dst = out + (int64_t)(3 + k) * plane + pix;
        for (int m = 0; m < N; ++m, dst += (int64_t)Ct * plane) store_pixels<V>(dst, v);
    }
}

// first and last padded column (row alike) that the replicate pad copies from image column x
__device__ __forceinline__ void pad_sources(int x, int W, int pad, int &lo, int &hi)
{
    lo = x == 0 ? 0 : x + pad;
    hi = x == W - 1 ? W - 1 + 2 * pad : x + pad;
}

// LDS slot of the column sum of padded column xp, for the columns that belong to image column 0 or W - 1
__device__ __forceinline__ int edge_slot(int xp, int W, int pad) { return xp <= pad ? xp : xp - (W - 1 + pad) + pad + 1; }

// The adjoint of channels 0..2, in gather form: one workgroup = one row y of one channel plane of d_images.  Pass 1: a thread per
// padded column sums the padded rows copied from y (1, or pad + 1 at the first / last row), top to bottom; a column of the image's
// inside is finished with that and written, the others (the left and right padding with the image's first / last column) go to LDS.
// Pass 2: one thread each sums the slots of image column 0 and of column W - 1, left to right.  No thread sums more than
// 2 pad + 1 values per pass, the order is fixed: two runs agree bit for bit.
__global__ __launch_bounds__(EI_THREADS) void encoder_input_bwd_kernel(const float *__restrict__ d_out, int H, int W, int pad, int Ct,
                                                                       Norm3 nm, float *__restrict__ d_images)
{
    extern __shared__ float edge[];   // 2 (pad + 1) column sums
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int64_t row = blockIdx.x;                     // (n * 3 + c) * H + y
    const int y = (int)(row % H), c = (int)((row / H) % 3);
    const int64_t n = row / ((int64_t)3 * H);
    const float sd = nm.std[c];
    int ylo, yhi;
    pad_sources(y, H, pad, ylo, yhi);
    const float *g = d_out + ((n * Ct + c) * Hp) * (int64_t)Wp;
    float *dst = d_images + row * W;
    for (int xp = threadIdx.x; xp < Wp; xp += EI_THREADS) {
        float acc = g[(int64_t)ylo * Wp + xp];
        for (int yp = ylo + 1; yp <= yhi; ++yp) acc = acc + g[(int64_t)yp * Wp + xp];
        const int x = xp - pad;
        if (x > 0 && x < W - 1) dst[x] = acc / sd;
        else edge[edge_slot(xp, W, pad)] = acc;
    }
    __syncthreads();
    const int wave = threadIdx.x / DINER_WAVE, lane = threadIdx.x % DINER_WAVE;
    if (lane == 0 && (wave == 0 || (wave == 1 && W > 1))) {
        const int x = wave == 0 ? 0 : W - 1;
        int lo, hi;
        pad_sources(x, W, pad, lo, hi);
        float acc = edge[edge_slot(lo, W, pad)];
        for (int xp = lo + 1; xp <= hi; ++xp) acc = acc + edge[edge_slot(xp, W, pad)];
        dst[x] = acc / sd;
    }
}

int invalid(const char *who, const char *what)
{
    set_error("%s: %s", who, what);
    return DINER_E_INVALID;
}

// argument checks shared by both directions (before any launch); Cpe: channels of the encoding
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

}  // namespace

}  // namespace diner

using namespace diner;

int diner_encoder_input(const float *images, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, const float *xs,
                        const float *ys, float mean0, float mean1, float mean2, float std0, float std1, float std2, float *out,
                        void *stream)
{
    const char *who = "encoder_input";
    const Norm3 nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    int Cpe = 0;
    if (const int rc = check_sizes(who, N, H, W, pad, pe_freqs, nm.std, Cpe)) return rc;
    if (!images || !out) return invalid(who, "NULL pointer");
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
        hipLaunchKernelGGL(encoder_input_kernel<4>, grid, dim3(EI_THREADS), 0, (hipStream_t)stream, images, (int)N, H, W, pad, Cpe,
                           xs, ys, nm, out);
    else
        hipLaunchKernelGGL(encoder_input_kernel<1>, grid, dim3(EI_THREADS), 0, (hipStream_t)stream, images, (int)N, H, W, pad, Cpe,
                           xs, ys, nm, out);
    return check_launch("encoder_input_kernel");
}

int diner_encoder_input_backward(const float *d_out, int64_t N, int32_t H, int32_t W, int32_t pad, int32_t pe_freqs, float std0, float std1,
                                 float std2, float *d_images, void *stream)
{
    const char *who = "encoder_input_backward";
    const Norm3 nm = {{0.f, 0.f, 0.f}, {std0, std1, std2}};
    int Cpe = 0;
    if (const int rc = check_sizes(who, N, H, W, pad, pe_freqs, nm.std, Cpe)) return rc;
    if (!d_out || !d_images) return invalid(who, "NULL pointer");
    if (pad > EI_MAX_PAD) {
        set_error("%s: pad=%d unsupported (up to %d: the edge column sums are held in LDS)", who, pad, EI_MAX_PAD);
        return DINER_E_UNSUPPORTED;
    }
    const int64_t rows = N * 3 * (int64_t)H;
    if (rows > 0x7fffffff) {
        set_error("%s: N * 3 * H = %lld rows are beyond one launch's grid", who, (long long)rows);
        return DINER_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(encoder_input_bwd_kernel, dim3((unsigned)rows), dim3(EI_THREADS), (size_t)(2 * (pad + 1)) * sizeof(float),
                       (hipStream_t)stream, d_out, H, W, pad, 3 + Cpe, nm, d_images);
    return check_launch("encoder_input_bwd_kernel");
}
