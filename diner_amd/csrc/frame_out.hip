// What the reference's evaluation path does with a rendered frame, on the device:
//   depth_range   src/util/torch_helpers.py:64-65   np.min / np.max per image (a NaN anywhere makes both NaN)
//   depth_cmap    src/util/torch_helpers.py:43-76   torch_cmap: normalise in double, matplotlib's Colormap._get_rgba_and_mask index rule,
//                                                   rows of the [nc + 3, 3] float64 table
//   frames_u8     src/models/diner.py:129-133 (torchvision save_image's quantisation) and :209 + src/util/torch_helpers.py:91
//                 (cat(dim=-2) and save_torch_video's quantisation): NCHW float -> HWC bytes, colour above depth when stacked
//   image_scores  src/evaluation/eval_suite.py:63-68   l1, l2, psnr and skimage's structural_similarity of a byte image pair
// The sums of the scores are integers (the inputs are bytes) and are formed exactly; each window's SSIM value is formed in fp64 from its
// five integer sums.  Partials are stored per workgroup and added in block order by a second kernel: no atomics, two runs agree bit for
// bit.  Nothing here synchronises with the host.
#include "common.hpp"

namespace diner {

namespace {

constexpr int FO_THREADS = 256;

int invalid(const char *who, const char *what)
{
    set_error("%s: %s", who, what);
    return DINER_E_INVALID;
}

int unsupported(const char *who, const char *what)
{
    set_error("%s: %s", who, what);
    return DINER_E_UNSUPPORTED;
}

// N images of H x W pixels: sizes every function here accepts (npix: pixels of one image)
int check_image_sizes(const char *who, int64_t N, int32_t H, int32_t W, int64_t &npix)
{
    if (N <= 0 || H <= 0 || W <= 0) return invalid(who, "non-positive size (N, H, W)");
    npix = (int64_t)H * W;
    if (npix > 0x7fffffff) return unsupported(who, "H * W of 2^31 or more");
    if (N > 65535) return unsupported(who, "more than 65535 images");
    return DINER_OK;
}

// ---- depth range ------------------------------------------------------------------------------------------------------------------
// pass 1: one (lo, hi) pair per (image, block); a NaN in the block's share makes both NaN.  pass 2: one thread per image walks its
// partials in block order.  min / max of floats are exact, so the result does not depend on the split.
constexpr int DR_MAX_BLOCKS = 64, DR_PER_BLOCK = FO_THREADS * 16;

int depth_range_blocks(int64_t npix)
{
    const int64_t n = (npix + DR_PER_BLOCK - 1) / DR_PER_BLOCK;
    return n < 1 ? 1 : (n > DR_MAX_BLOCKS ? DR_MAX_BLOCKS : (int)n);
}

template <int V>
__global__ __launch_bounds__(FO_THREADS) void depth_range_partial_kernel(const float *__restrict__ depth, int64_t npix, int nblk,
                                                                         float *__restrict__ part)
{
    __shared__ float lo_s[FO_THREADS], hi_s[FO_THREADS];
    __shared__ int nan_s[FO_THREADS];
    const int n = blockIdx.y, tid = threadIdx.x;
    const float *d = depth + (int64_t)n * npix;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    int nan = 0;
    for (int64_t i = ((int64_t)blockIdx.x * FO_THREADS + tid) * V; i < npix; i += (int64_t)nblk * FO_THREADS * V) {
        float v[V];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(d + i);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = d[i];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            nan |= v[k] != v[k];
            lo = fminf(lo, v[k]);     // fminf / fmaxf skip a NaN: it is carried by the flag
            hi = fmaxf(hi, v[k]);
        }
    }
    lo_s[tid] = lo; hi_s[tid] = hi; nan_s[tid] = nan;
    __syncthreads();
    for (int s = FO_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            lo_s[tid] = fminf(lo_s[tid], lo_s[tid + s]);
            hi_s[tid] = fmaxf(hi_s[tid], hi_s[tid + s]);
            nan_s[tid] |= nan_s[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float qnan = __builtin_nanf("");
        float *p = part + ((int64_t)n * nblk + blockIdx.x) * 2;
        p[0] = nan_s[0] ? qnan : lo_s[0];
        p[1] = nan_s[0] ? qnan : hi_s[0];
    }
}

__global__ __launch_bounds__(64) void depth_range_final_kernel(const float *__restrict__ part, int64_t N, int nblk, double *__restrict__ range)
{
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    bool nan = false;
    for (int b = 0; b < nblk; ++b) {   // block order
        const float l = part[(n * nblk + b) * 2], h = part[(n * nblk + b) * 2 + 1];
        nan = nan || l != l;
        lo = fminf(lo, l);
        hi = fmaxf(hi, h);
    }
    const double qnan = __builtin_nan("");
    range[n * 2] = nan ? qnan : (double)lo;
    range[n * 2 + 1] = nan ? qnan : (double)hi;
}

// ---- colour map -------------------------------------------------------------------------------------------------------------------
// The row of the [nc + 3, 3] table that matplotlib's Colormap._get_rgba_and_mask picks for x = (d - vmin) / (vmax - vmin), all in double:
// xa = x nc; xa == nc counts as nc - 1; under (row nc) below 0, over (row nc + 1) from nc on, bad (row nc + 2) for a NaN -- which is
// what a flat image gives (0 / 0) --, else xa truncated.
__device__ __forceinline__ int cmap_index(float d, double vmin, double vmax, int nc)
{
    const double t = ((double)d - vmin) / (vmax - vmin);
    double xa = t * (double)nc;
    if (xa == (double)nc) xa = (double)(nc - 1);
    if (xa < 0.0) return nc;
    if (xa >= (double)nc) return nc + 1;
    if (xa != xa) return nc + 2;
    return (int)xa;
}

// the limits of image n: a given scalar, or the image's own range
__device__ __forceinline__ void cmap_limits(const double *__restrict__ range, int64_t n, double vmin, double vmax, int has_vmin, int has_vmax,
                                            double &lo, double &hi)
{
    lo = has_vmin ? vmin : range[n * 2];
    hi = has_vmax ? vmax : range[n * 2 + 1];
}

// one thread = V consecutive pixels of one image (V = 2: a 16-byte store per channel plane)
template <int V>
__global__ __launch_bounds__(FO_THREADS) void depth_cmap_kernel(const float *__restrict__ depth, int64_t npix, int64_t total,
                                                                const double *__restrict__ range, double vmin, double vmax, int has_vmin,
                                                                int has_vmax, const double *__restrict__ table, int nc,
                                                                double *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * FO_THREADS + threadIdx.x;
    if (q >= total) return;
    const int64_t per = npix / V, n = q / per, p = (q - n * per) * V;
    double lo, hi;
    cmap_limits(range, n, vmin, vmax, has_vmin, has_vmax, lo, hi);
    int idx[V];
#pragma unroll
    for (int k = 0; k < V; ++k) idx[k] = cmap_index(depth[n * npix + p + k], lo, hi, nc);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double *dst = out + (n * 3 + c) * npix + p;
        if constexpr (V == 2) *reinterpret_cast<double2 *>(dst) = make_double2(table[idx[0] * 3 + c], table[idx[1] * 3 + c]);
        else dst[0] = table[idx[0] * 3 + c];
    }
}

// ---- frames to bytes --------------------------------------------------------------------------------------------------------------
// R = DINER_ROUND_SAVE_IMAGE: (uint8) clamp(x 255 + 0.5, 0, 255), the multiply and the add two fp32 roundings (torchvision's
// mul(255).add_(0.5).clamp_(0, 255).to(uint8));  R = DINER_ROUND_VIDEO: (uint8) ((double) x 255) (save_torch_video on frames that the
// float64 colour map promoted).  Where the cast is undefined in numpy / torch: saturate, NaN gives 0.
template <int R>
__device__ __forceinline__ uint32_t quantise(float x)
{
    if constexpr (R == DINER_ROUND_SAVE_IMAGE) {
        float v = x * 255.0f;
        v = v + 0.5f;
        return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)(int)v);
    } else {
        const double v = (double)x * 255.0;
        return !(v > 0.0) ? 0u : (v >= 255.0 ? 255u : (uint32_t)(int)v);
    }
}

template <int V>
__device__ __forceinline__ void load_pixels(const float *__restrict__ src, float (&v)[V])
{
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = src[0];
    }
}

// b: V pixels x 3 channels, pixel-major, to the HWC row at dst (V = 4: 12 contiguous bytes per lane as three dwords)
template <int V>
__device__ __forceinline__ void store_hwc(uint8_t *__restrict__ dst, const uint32_t (&b)[V * 3])
{
    if constexpr (V == 4) {
        uint3 w;
        w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        *reinterpret_cast<uint3 *>(dst) = w;
    } else {
        dst[0] = (uint8_t)b[0]; dst[1] = (uint8_t)b[1]; dst[2] = (uint8_t)b[2];
    }
}

// One thread = V consecutive pixels of one row of image n: its colour (three planes of rgb) to rgb_out + n rgb_stride and, with a
// depth, the byte row of the colour map to dep_out + n dep_stride.  The stacked frame is the same kernel with dep_out = rgb_out + 3 H W
// and both strides 6 H W.
template <int V, int R>
__global__ __launch_bounds__(FO_THREADS) void frames_u8_kernel(const float *__restrict__ rgb, const float *__restrict__ depth, int64_t npix,
                                                               int64_t total, const double *__restrict__ range, double vmin, double vmax,
                                                               int has_vmin, int has_vmax, const uint8_t *__restrict__ table, int nc,
                                                               uint8_t *__restrict__ rgb_out, int64_t rgb_stride,
                                                               uint8_t *__restrict__ dep_out, int64_t dep_stride)
{
    const int64_t q = (int64_t)blockIdx.x * FO_THREADS + threadIdx.x;
    if (q >= total) return;
    const int64_t per = npix / V, n = q / per, p = (q - n * per) * V;   // W % V == 0: the V pixels share a row
    uint32_t b[V * 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[V];
        load_pixels<V>(rgb + (n * 3 + c) * npix + p, v);
#pragma unroll
        for (int k = 0; k < V; ++k) b[k * 3 + c] = quantise<R>(v[k]);
    }
    store_hwc<V>(rgb_out + n * rgb_stride + p * 3, b);
    if (depth == nullptr) return;
    double lo, hi;
    cmap_limits(range, n, vmin, vmax, has_vmin, has_vmax, lo, hi);
    float d[V];
    load_pixels<V>(depth + n * npix + p, d);
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int idx = cmap_index(d[k], lo, hi, nc);
#pragma unroll
        for (int c = 0; c < 3; ++c) b[k * 3 + c] = table[idx * 3 + c];
    }
    store_hwc<V>(dep_out + n * dep_stride + p * 3, b);
}

// ---- image scores -----------------------------------------------------------------------------------------------------------------
// A workgroup owns SC_TH x SC_TW windows (7 x 7, top-left corners) of one image pair, all three channels: the tile's pixels plus the
// 6-pixel halo are staged in LDS as bytes; per channel the five sums Sx, Sy, Sxx, Syy, Sxy run along rows first (hs: 7-pixel row sums,
// int32: at most 7 255^2), then down columns (a thread slides over 4 windows: at most 49 255^2).  From the exact sums, in fp64:
//   mx = Sx / (49 255), vx = (49 Sxx - Sx^2) / (49 48 255^2)  [the sample variance of x / 255: cov_norm = 49 / 48], vxy alike,
//   S = (2 mx my + C1) (2 vxy + C2) / ((mx^2 + my^2 + C1) (vx + vy + C2)),  C1 = 0.01^2, C2 = 0.03^2  (data_range = 1).
// The tile also owns the |d| and d^2 sums of its own pixels (the last tile of a row / column takes the 6 trailing ones): integers
// carried in doubles, exact below 2^53 (255^2 3 (2^31 - 1) < 2^49).
constexpr int SC_TW = 64, SC_TH = 16, SC_ROWS = SC_TH + 6, SC_COLS = SC_TW + 6, SC_PITCH = SC_COLS * 3 + 2, SC_STRIP = 4, SC_SUMS = 5;
static_assert(SC_TW * (SC_TH / SC_STRIP) == FO_THREADS, "one thread per window column and strip");

__global__ __launch_bounds__(FO_THREADS) void image_scores_partial_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int H,
                                                                          int W, int ntx, int nty, double *__restrict__ part)
{
    __shared__ uint8_t px[2][SC_ROWS][SC_PITCH];
    __shared__ int hs[SC_SUMS][SC_ROWS][SC_TW];
    __shared__ double red[SC_SUMS][FO_THREADS];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * SC_TH, x0 = tx * SC_TW;
    const int rows = min(SC_ROWS, H - y0), cols = min(SC_COLS, W - x0);                  // staged pixels
    const int own_rows = ty == nty - 1 ? rows : SC_TH, own_cols = tx == ntx - 1 ? cols : SC_TW;
    const int win_rows = min(SC_TH, H - 6 - y0), win_cols = min(SC_TW, W - 6 - x0);      // >= 1 both
    const uint8_t *ia = a + (int64_t)n * H * W * 3, *ib = b + (int64_t)n * H * W * 3;

    uint32_t sad = 0, ssd = 0;                                                           // at most 19 bytes per thread
    const int rowbytes = cols * 3;
    for (int i = tid; i < rows * rowbytes; i += FO_THREADS) {
        const int r = i / rowbytes, j = i - r * rowbytes;
        const int64_t g = ((int64_t)(y0 + r) * W + x0) * 3 + j;
        const int va = ia[g], vb = ib[g];
        px[0][r][j] = (uint8_t)va;
        px[1][r][j] = (uint8_t)vb;
        if (r < own_rows && j < own_cols * 3) {
            const int d = va - vb;
            sad += (uint32_t)(d < 0 ? -d : d);
            ssd += (uint32_t)(d * d);
        }
    }
    __syncthreads();

    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, MU = 49.0 * 255.0, VAR = 49.0 * 48.0 * 255.0 * 255.0;
    const int wx = tid % SC_TW, wy0 = (tid / SC_TW) * SC_STRIP, wy1 = min(wy0 + SC_STRIP, win_rows);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < rows * SC_TW; i += FO_THREADS) {       // along rows
            const int r = i / SC_TW, w = i - r * SC_TW;
            if (w >= win_cols) continue;
            int s[SC_SUMS] = {0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int x = px[0][r][(w + k) * 3 + c], y = px[1][r][(w + k) * 3 + c];
                s[0] += x; s[1] += y; s[2] += x * x; s[3] += y * y; s[4] += x * y;
            }
#pragma unroll
            for (int q = 0; q < SC_SUMS; ++q) hs[q][r][w] = s[q];
        }
        __syncthreads();
        if (wx < win_cols && wy0 < win_rows) {                       // down columns
            int s[SC_SUMS] = {0, 0, 0, 0, 0};
            for (int k = 0; k < 7; ++k)
#pragma unroll
                for (int q = 0; q < SC_SUMS; ++q) s[q] += hs[q][wy0 + k][wx];
            for (int wy = wy0;;) {
                const double mx = (double)s[0] / MU, my = (double)s[1] / MU;
                const int64_t nx = 49ll * s[2] - (int64_t)s[0] * s[0], ny = 49ll * s[3] - (int64_t)s[1] * s[1];
                const int64_t nxy = 49ll * s[4] - (int64_t)s[0] * s[1];
                const double vx = (double)nx / VAR, vy = (double)ny / VAR, vxy = (double)nxy / VAR;
                const double a1 = 2.0 * mx * my + C1, a2 = 2.0 * vxy + C2;
                const double b1 = mx * mx + my * my + C1, b2 = vx + vy + C2;
                acc[c] += (a1 * a2) / (b1 * b2);
                if (++wy >= wy1) break;
#pragma unroll
                for (int q = 0; q < SC_SUMS; ++q) s[q] += hs[q][wy + 6][wx] - hs[q][wy - 1][wx];
            }
        }
        __syncthreads();                                             // hs is rewritten for the next channel
    }
    red[0][tid] = acc[0]; red[1][tid] = acc[1]; red[2][tid] = acc[2];
    red[3][tid] = (double)sad; red[4][tid] = (double)ssd;
    __syncthreads();
    for (int s = FO_THREADS / 2; s > 0; s >>= 1) {   // fixed tree
        if (tid < s)
#pragma unroll
            for (int q = 0; q < SC_SUMS; ++q) red[q][tid] += red[q][tid + s];
        __syncthreads();
    }
    if (tid < SC_SUMS) part[((int64_t)n * gridDim.x + blockIdx.x) * SC_SUMS + tid] = red[tid][0];
}

// scores [4, N]: ssim, psnr, l2, l1 of image n from its partials, added in block order.  The workgroup copies SC_FINAL_CHUNK partial sets
// at a time into LDS (coalesced), then one thread per sum adds them from there, first block first: the order is that of a plain loop,
// without a global-memory latency per term.
constexpr int SC_FINAL_CHUNK = 256;

__global__ __launch_bounds__(FO_THREADS) void image_scores_final_kernel(const double *__restrict__ part, int nblk, int64_t N, int H, int W,
                                                                        double *__restrict__ scores)
{
    __shared__ double buf[SC_FINAL_CHUNK * SC_SUMS];
    __shared__ double s[SC_SUMS];
    const int64_t n = blockIdx.x;
    const int q = threadIdx.x;
    const double *p = part + n * nblk * SC_SUMS;
    double acc = 0.0;
    for (int base = 0; base < nblk; base += SC_FINAL_CHUNK) {
        const int cnt = min(SC_FINAL_CHUNK, nblk - base);
        for (int i = q; i < cnt * SC_SUMS; i += FO_THREADS) buf[i] = p[(int64_t)base * SC_SUMS + i];
        __syncthreads();
        if (q < SC_SUMS)
            for (int i = 0; i < cnt; ++i) acc += buf[i * SC_SUMS + q];
        __syncthreads();
    }
    if (q < SC_SUMS) s[q] = acc;
    __syncthreads();
    if (q != 0) return;
    const double nwin = (double)(H - 6) * (double)(W - 6), nval = 3.0 * (double)H * (double)W;
    const double l1 = s[3] / (255.0 * nval), l2 = s[4] / (65025.0 * nval);
    scores[n] = (s[0] / nwin + s[1] / nwin + s[2] / nwin) / 3.0;
    scores[N + n] = 10.0 * log10(1.0 / l2);
    scores[2 * N + n] = l2;
    scores[3 * N + n] = l1;
}

int check_cmap(const char *who, const double *range, double vmin, double vmax, int32_t has_vmin, int32_t has_vmax, const void *table,
               int32_t ncolors)
{
    if (!table) return invalid(who, "NULL colour table");
    if (ncolors < 1 || ncolors > (1 << 20)) return invalid(who, "ncolors outside 1..2^20");
    if (!(has_vmin && has_vmax) && !range) return invalid(who, "NULL range with vmin or vmax absent");
    if ((uintptr_t)range % 8) return invalid(who, "range not 8-byte aligned");
    return DINER_OK;
}

int check_grid(const char *who, int64_t blocks)
{
    if (blocks > 0x7fffffff) return unsupported(who, "beyond one launch's grid");
    return DINER_OK;
}

struct ScoreGrid {
    int ntx, nty;
};

int check_scores(const char *who, int64_t N, int32_t H, int32_t W, ScoreGrid &G)
{
    if (N <= 0 || H <= 0 || W <= 0) return invalid(who, "non-positive size (N, H, W)");
    if (H < 7 || W < 7) return invalid(who, "an image side below 7 (the 7 x 7 window does not fit)");
    if ((int64_t)H * W > 0x7fffffff) return unsupported(who, "H * W of 2^31 or more");
    if (N > 65535) return unsupported(who, "more than 65535 image pairs");
    G.ntx = (W - 6 + SC_TW - 1) / SC_TW;
    G.nty = (H - 6 + SC_TH - 1) / SC_TH;
    return DINER_OK;
}

}  // namespace

}  // namespace diner

using namespace diner;

int64_t diner_depth_range_workspace_floats(int64_t N, int32_t H, int32_t W)
{
    if (N <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffff) return -1;
    return N * depth_range_blocks((int64_t)H * W) * 2;
}

int diner_depth_range(const float *depth, int64_t N, int32_t H, int32_t W, double *range_out, float *workspace, void *stream)
{
    const char *who = "depth_range";
    int64_t npix = 0;
    if (const int rc = check_image_sizes(who, N, H, W, npix)) return rc;
    if (!depth || !range_out || !workspace) return invalid(who, "NULL pointer");
    if ((uintptr_t)range_out % 8) return invalid(who, "range_out not 8-byte aligned");
    const int nblk = depth_range_blocks(npix);
    const dim3 grid((unsigned)nblk, (unsigned)N);
    if (npix % 4 == 0 && (uintptr_t)depth % 16 == 0)
        hipLaunchKernelGGL(depth_range_partial_kernel<4>, grid, dim3(FO_THREADS), 0, (hipStream_t)stream, depth, npix, nblk, workspace);
    else
        hipLaunchKernelGGL(depth_range_partial_kernel<1>, grid, dim3(FO_THREADS), 0, (hipStream_t)stream, depth, npix, nblk, workspace);
    if (const int rc = check_launch("depth_range_partial_kernel")) return rc;
    hipLaunchKernelGGL(depth_range_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float *)workspace, N,
                       nblk, range_out);
    return check_launch("depth_range_final_kernel");
}

int diner_depth_cmap(const float *depth, int64_t N, int32_t H, int32_t W, const double *range, double vmin, double vmax, int32_t has_vmin,
                     int32_t has_vmax, const double *table, int32_t ncolors, double *out, void *stream)
{
    const char *who = "depth_cmap";
    int64_t npix = 0;
    if (const int rc = check_image_sizes(who, N, H, W, npix)) return rc;
    if (!depth || !out) return invalid(who, "NULL pointer");
    if (const int rc = check_cmap(who, range, vmin, vmax, has_vmin, has_vmax, table, ncolors)) return rc;
    if ((uintptr_t)table % 8 || (uintptr_t)out % 8) return invalid(who, "table or out not 8-byte aligned");
    const bool vec = npix % 2 == 0 && (uintptr_t)out % 16 == 0;
    const int64_t total = N * (npix / (vec ? 2 : 1)), blocks = (total + FO_THREADS - 1) / FO_THREADS;
    if (const int rc = check_grid(who, blocks)) return rc;
    if (vec)
        hipLaunchKernelGGL(depth_cmap_kernel<2>, dim3((unsigned)blocks), dim3(FO_THREADS), 0, (hipStream_t)stream, depth, npix, total, range,
                           vmin, vmax, has_vmin != 0, has_vmax != 0, table, ncolors, out);
    else
        hipLaunchKernelGGL(depth_cmap_kernel<1>, dim3((unsigned)blocks), dim3(FO_THREADS), 0, (hipStream_t)stream, depth, npix, total, range,
                           vmin, vmax, has_vmin != 0, has_vmax != 0, table, ncolors, out);
    return check_launch("depth_cmap_kernel");
}

int diner_frames_u8(const float *rgb, const float *depth, int64_t N, int32_t H, int32_t W, int32_t rounding, int32_t stacked,
                    const double *range, double vmin, double vmax, int32_t has_vmin, int32_t has_vmax, const uint8_t *table_u8,
                    int32_t ncolors, uint8_t *rgb_out, uint8_t *depth_out, void *stream)
{
    const char *who = "frames_u8";
    int64_t npix = 0;
    if (const int rc = check_image_sizes(who, N, H, W, npix)) return rc;
    if (rounding != DINER_ROUND_SAVE_IMAGE && rounding != DINER_ROUND_VIDEO) return invalid(who, "unknown rounding");
    if (!rgb || !rgb_out) return invalid(who, "NULL pointer");
    if (stacked && !depth) return invalid(who, "stacked frames need a depth");
    if (depth) {
        if (!stacked && !depth_out) return invalid(who, "NULL depth_out");
        if (const int rc = check_cmap(who, range, vmin, vmax, has_vmin, has_vmax, table_u8, ncolors)) return rc;
    }
    uint8_t *dep = stacked ? rgb_out + npix * 3 : depth_out;
    const int64_t rgb_stride = (stacked ? 2 : 1) * npix * 3, dep_stride = rgb_stride;
    const bool vec = W % 4 == 0 && (uintptr_t)rgb % 16 == 0 && (uintptr_t)depth % 16 == 0 && (uintptr_t)rgb_out % 4 == 0 &&
                     (uintptr_t)dep % 4 == 0;
    const int64_t total = N * (npix / (vec ? 4 : 1)), blocks = (total + FO_THREADS - 1) / FO_THREADS;
    if (const int rc = check_grid(who, blocks)) return rc;
#define DINER_FRAMES_LAUNCH(V, R)                                                                                                          \
    hipLaunchKernelGGL((frames_u8_kernel<V, R>), dim3((unsigned)blocks), dim3(FO_THREADS), 0, (hipStream_t)stream, rgb, depth, npix, total, \
                       range, vmin, vmax, has_vmin != 0, has_vmax != 0, table_u8, ncolors, rgb_out, rgb_stride, dep, dep_stride)
    if (vec && rounding == DINER_ROUND_SAVE_IMAGE) DINER_FRAMES_LAUNCH(4, DINER_ROUND_SAVE_IMAGE);
    else if (vec) DINER_FRAMES_LAUNCH(4, DINER_ROUND_VIDEO);
    else if (rounding == DINER_ROUND_SAVE_IMAGE) DINER_FRAMES_LAUNCH(1, DINER_ROUND_SAVE_IMAGE);
    else DINER_FRAMES_LAUNCH(1, DINER_ROUND_VIDEO);
#undef DINER_FRAMES_LAUNCH
    return check_launch("frames_u8_kernel");
}

int64_t diner_image_scores_workspace_floats(int64_t N, int32_t H, int32_t W)
{
    ScoreGrid G;
    if (check_scores("image_scores", N, H, W, G)) return -1;
    return N * G.ntx * G.nty * SC_SUMS * 2;   // doubles
}

int diner_image_scores(const uint8_t *pred, const uint8_t *gt, int64_t N, int32_t H, int32_t W, double *scores_out, float *workspace,
                       void *stream)
{
    const char *who = "image_scores";
    ScoreGrid G;
    if (const int rc = check_scores(who, N, H, W, G)) return rc;
    if (!pred || !gt || !scores_out || !workspace) return invalid(who, "NULL pointer");
    if ((uintptr_t)workspace % 8 || (uintptr_t)scores_out % 8) return invalid(who, "workspace or scores_out not 8-byte aligned");
    const int64_t nblk = (int64_t)G.ntx * G.nty;
    if (const int rc = check_grid(who, nblk)) return rc;
    double *part = (double *)workspace;
    hipLaunchKernelGGL(image_scores_partial_kernel, dim3((unsigned)nblk, (unsigned)N), dim3(FO_THREADS), 0, (hipStream_t)stream, pred, gt, H, W,
                       G.ntx, G.nty, part);
    if (const int rc = check_launch("image_scores_partial_kernel")) return rc;
    hipLaunchKernelGGL(image_scores_final_kernel, dim3((unsigned)N), dim3(FO_THREADS), 0, (hipStream_t)stream, (const double *)part, (int)nblk, N, H, W,
                       scores_out);
    return check_launch("image_scores_final_kernel");
}
