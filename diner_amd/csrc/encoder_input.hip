// The head of the encoder (reference src/models/pixelnerf.py:44 + src/models/image_encoder.py:222-232) in one kernel: conv1's input
// [N, 3 + Cpe, H + 2 pad, W + 2 pad] = the images normalised ((x - mean) / std), replicate-padded by `pad`, and -- when the encoder has
// a positional encoding of its padding (padding_pe >= 0 and pad > 0) -- the Cpe = 2 (1 + 2F) channels of
// PositionalEncoding(F, freq_factor = pi, d_in = 2) of the pixel's (x, y) in [-1, 1]^2, zero over the image's own pixels.  The reference
// builds it from a dozen ATen launches (normalise, pad, linspace x 2, meshgrid, stack, the encoding's repeat / addcmul / sin / cat, the
// interior's zero fill, expand, cat) that move the tensor about three times; here it is written once.  The encoding does not depend on
// the image: every value is computed once per pixel and stored to all N images.
// And the adjoint to the images: the replicate pad's gather (an edge pixel sums the padding that was copied from it), in a fixed order.
#include "encoder_input_kernel.hpp"   // the forward kernel (shared with image_wire.hip, which feeds it bytes), the checks, the launch

namespace diner {

namespace {

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
    if (!images) return invalid(who, "NULL pointer");
    return launch_encoder_input(who, FloatImages{images}, N, H, W, pad, Cpe, xs, ys, nm, out, stream);
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
