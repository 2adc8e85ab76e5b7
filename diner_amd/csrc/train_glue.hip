// The two stretches of a training step on either side of renderer.forward (reference DINER.calc_losses, src/models/diner.py:217-290):
//   gen_rays_at   :224-227 + :257-258   gen_rays at the SB x B selected pixels only (rays.view(SB, H*W, -1)[batch_idx_helper, pix_idcs])
//   photo_loss    :265-267 + :280-282   the ground-truth gather, MSELoss and AntibiasLoss (src/losses/antibiasloss.py) with its view / permute
// Both backwards sum with the store-and-sum scheme of encode_glue.hip: fp64 partials per workgroup, a second pass adds them in block
// order, no atomics -- two runs agree bit for bit.  An index outside [0, H*W) is clamped into it: nothing is read or written out of bounds.
#include "common.hpp"

namespace diner {

namespace {

__device__ __forceinline__ int load_pixel(const void *__restrict__ idx, int is64, int64_t i, int npix)
{
    const int64_t p = is64 ? ((const int64_t *)idx)[i] : (int64_t)((const int32_t *)idx)[i];
    return p < 0 ? 0 : (p > (int64_t)npix - 1 ? npix - 1 : (int)p);
}

// ---- gen_rays_at ------------------------------------------------------------------------------------------------------------------
// rays [SB,B,8]: ray j of camera b is gen_rays' ray at pixel idx[b,j] = x + y W (common.hpp gen_ray: the arithmetic of gen_rays_kernel)
__global__ void gen_rays_at_kernel(const float *__restrict__ extr, const float *__restrict__ intr, const float *__restrict__ z_near,
                                   const float *__restrict__ z_far, const void *__restrict__ idx, int is64, int SB, int B, int H, int W,
                                   float *__restrict__ rays)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)SB * B) return;
    const int b = (int)(i / B);
    const int p = load_pixel(idx, is64, i, H * W), y = p / W, x = p - y * W;
    gen_ray(extr + b * 16, intr + b * 9, x, y, z_near[b], z_far[b], rays + i * 8);
}

// ---- backward: the GR_SUMS = 18 per-camera sums of gen_rays_bwd_partial_kernel (encode_glue.hip; the derivation is there), taken over
// the B selected rays instead of the H W pixels.  A pixel selected twice is two terms.  Pass 1 writes one fp64 partial per
// (camera, block), pass 2 adds them in block order and forms the gradients exactly as gen_rays_bwd_final_kernel does.
constexpr int GA_SUMS = 18, GA_THREADS = 256, GA_MAX_BLOCKS = 64;

// blocks per camera of pass 1: a function of B only (the summation order must not depend on anything else)
int gen_rays_at_bwd_blocks(int B)
{
    const int n = (B + GA_THREADS - 1) / GA_THREADS;
    return n < 1 ? 1 : (n > GA_MAX_BLOCKS ? GA_MAX_BLOCKS : n);
}

__global__ __launch_bounds__(GA_THREADS) void gen_rays_at_bwd_partial_kernel(const float *__restrict__ extr, const float *__restrict__ intr,
                                                                             const float *__restrict__ d_rays, const void *__restrict__ idx,
                                                                             int is64, int B, int H, int W, int nblk,
                                                                             double *__restrict__ part)
{
    __shared__ double red[GA_SUMS][GA_THREADS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float *E = extr + b * 16, *Kk = intr + b * 9;
    double R[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) R[k][r] = (double)E[k * 4 + r];
    const double fx = Kk[0], fy = Kk[4], cx = Kk[2], cy = Kk[5];
    double acc[GA_SUMS];
#pragma unroll
    for (int q = 0; q < GA_SUMS; ++q) acc[q] = 0.0;
    for (int j = blockIdx.x * GA_THREADS + tid; j < B; j += nblk * GA_THREADS) {
        const int64_t i = (int64_t)b * B + j;
        const int p = load_pixel(idx, is64, i, H * W), y = p / W, x = p - y * W;
        const double px = ((double)x + 0.5 - cx) / fx, py = ((double)y + 0.5 - cy) / fy;
        const double n = sqrt(px * px + py * py + 1.0);
        const double dh[3] = {px / n, py / n, 1.0 / n};
        const float *g = d_rays + i * 8;
        const double gd[3] = {(double)g[3], (double)g[4], (double)g[5]};
        double gh[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int r = 0; r < 3; ++r) acc[k * 3 + r] += gd[r] * dh[k];
            gh[k] = R[k][0] * gd[0] + R[k][1] * gd[1] + R[k][2] * gd[2];
        }
        const double dot = dh[0] * gh[0] + dh[1] * gh[1] + dh[2] * gh[2];
        const double gpx = (gh[0] - dh[0] * dot) / n, gpy = (gh[1] - dh[1] * dot) / n;
        acc[9] += gpx;
        acc[10] += gpx * px;
        acc[11] += gpy;
        acc[12] += gpy * py;
        acc[13] += (double)g[0];
        acc[14] += (double)g[1];
        acc[15] += (double)g[2];
        acc[16] += (double)g[6];
        acc[17] += (double)g[7];
    }
#pragma unroll
    for (int q = 0; q < GA_SUMS; ++q) red[q][tid] = acc[q];
    __syncthreads();
    for (int s = GA_THREADS / 2; s > 0; s >>= 1) {   // fixed tree
        if (tid < s)
#pragma unroll
            for (int q = 0; q < GA_SUMS; ++q) red[q][tid] += red[q][tid + s];
        __syncthreads();
    }
    if (tid < GA_SUMS) part[((int64_t)b * nblk + blockIdx.x) * GA_SUMS + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void gen_rays_at_bwd_final_kernel(const float *__restrict__ extr, const float *__restrict__ intr, int nblk,
                                                                   const double *__restrict__ part, float *__restrict__ d_extr,
                                                                   float *__restrict__ d_intr, float *__restrict__ d_near,
                                                                   float *__restrict__ d_far)
{
    __shared__ double s[GA_SUMS];
    const int b = blockIdx.x, q = threadIdx.x;
    if (q < GA_SUMS) {
        double a = 0.0;
        for (int i = 0; i < nblk; ++i) a += part[((int64_t)b * nblk + i) * GA_SUMS + q];   // block order
        s[q] = a;
    }
    __syncthreads();
    if (q != 0) return;
    const float *E = extr + b * 16, *Kk = intr + b * 9;
    float *dE = d_extr + b * 16, *dK = d_intr + b * 9;
    const double Go[3] = {s[13], s[14], s[15]};
    for (int k = 0; k < 3; ++k) {
        const double tk = (double)E[k * 4 + 3];
        double dt = 0.0;
        for (int r = 0; r < 3; ++r) {
            dE[k * 4 + r] = (float)(s[k * 3 + r] - Go[r] * tk);
            dt -= (double)E[k * 4 + r] * Go[r];
        }
        dE[k * 4 + 3] = (float)dt;
    }
    for (int j = 12; j < 16; ++j) dE[j] = 0.0f;                 // E[3,:] is not read
    const double fx = Kk[0], fy = Kk[4];
    for (int j = 0; j < 9; ++j) dK[j] = 0.0f;                   // only fx, fy, cx, cy are read
    dK[0] = (float)(-s[10] / fx);
    dK[4] = (float)(-s[12] / fy);
    dK[2] = (float)(-s[9] / fx);
    dK[5] = (float)(-s[11] / fy);
    d_near[b] = (float)s[16];
    d_far[b] = (float)s[17];
}

// ---- photo_loss -------------------------------------------------------------------------------------------------------------------
// The B rays of a scene form a grid of `height` rows x `width` columns, row-major: the s x s patch (pooling cells of p x p pixels,
// nc = s / p of them per side, trailing rows and columns outside every cell), or 1 x B without a patch (nc = 0).  A workgroup owns the
// tile (band, chunk): the rows of one cell row (band >= nc: the trailing rows) x tw columns = whole cells (the trailing columns follow
// the last cell, in its chunk or in one of their own).  It gathers the ground truth of its pixels from the NCHW target, writes gt_colors, sums the squared error and,
// from a copy of the tile in LDS, pools prediction and ground truth of every cell SEPARATELY in the same row-major order, then
// subtracts: equal cells give an exact 0.  Sums are fp64; one partial pair per workgroup.
constexpr int PL_THREADS = 256, PL_TILE = 2048, PL_TILE_RAYS = 1024, PL_MAX_POOL = 32;

struct PhotoGrid {
    int width, height, p, nc, band_rows, tw, nchunk, nband;
};

PhotoGrid photo_grid(int B, int patch, int pool)
{
    PhotoGrid g;
    if (patch > 0) {
        const int cells = PL_TILE / (pool * pool);     // >= 2 for pool <= PL_MAX_POOL
        g.width = g.height = patch; g.p = pool; g.nc = patch / pool; g.band_rows = pool;
        g.tw = cells * pool;
    } else {
        g.width = B; g.height = 1; g.p = 1; g.nc = 0; g.band_rows = 1;
        g.tw = PL_TILE_RAYS;
    }
    g.nchunk = (g.width + g.tw - 1) / g.tw;
    g.nband = (g.height + g.band_rows - 1) / g.band_rows;
    return g;
}

__global__ __launch_bounds__(PL_THREADS) void photo_loss_partial_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                                        const void *__restrict__ idx, int is64, int B, int H, int W,
                                                                        PhotoGrid G, float *__restrict__ gt, float *__restrict__ sign,
                                                                        double *__restrict__ part)
{
    __shared__ float stage[6][PL_TILE];           // prediction (0..2) and ground truth (3..5) of the tile's pixels
    __shared__ double red[2][PL_THREADS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int band = blockIdx.x / G.nchunk, chunk = blockIdx.x - band * G.nchunk;
    const int r0 = band * G.band_rows, c0 = chunk * G.tw;
    const int rows = min(G.height, r0 + G.band_rows) - r0, tcols = min(G.width, c0 + G.tw) - c0;
    const int npx = rows * tcols, npix = H * W;
    const bool pool = band < G.nc;                // (uniform) a band of cells: rows == p and npx <= PL_TILE
    const float *tb = target + (int64_t)b * 3 * npix;
    double sq = 0.0, ab = 0.0;
    for (int t = tid; t < npx; t += PL_THREADS) {
        const int r = t / tcols, c = t - r * tcols;
        const int64_t q = (int64_t)b * B + (int64_t)(r0 + r) * G.width + (c0 + c);
        const int pix = load_pixel(idx, is64, q, npix);
        float v[6];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            v[ch] = pred[q * 3 + ch];
            v[3 + ch] = tb[(int64_t)ch * npix + pix];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            gt[q * 3 + ch] = v[3 + ch];
            const double d = (double)v[ch] - (double)v[3 + ch];
            sq += d * d;
        }
        if (pool)
#pragma unroll
            for (int k = 0; k < 6; ++k) stage[k][t] = v[k];
    }
    if (pool) {
        __syncthreads();
        const int p = G.p, cell0 = c0 / p, ncell = min(G.nc, (c0 + tcols) / p) - cell0;   // whole cells of this tile
        const double inv = 1.0 / ((double)p * p);
        for (int i = tid; i < ncell * 3; i += PL_THREADS) {
            const int cl = i / 3, ch = i - cl * 3;
            double sp = 0.0, sg = 0.0;
            for (int yy = 0; yy < p; ++yy)
                for (int xx = 0; xx < p; ++xx) {
                    const int t = yy * tcols + cl * p + xx;
                    sp += (double)stage[ch][t];
                    sg += (double)stage[3 + ch][t];
                }
            const double diff = sp * inv - sg * inv;
            ab += fabs(diff);
            sign[(((int64_t)b * 3 + ch) * G.nc + band) * G.nc + cell0 + cl] = diff > 0.0 ? 1.0f : (diff < 0.0 ? -1.0f : 0.0f);
        }
    }
    red[0][tid] = sq;
    red[1][tid] = ab;
    __syncthreads();
    for (int s = PL_THREADS / 2; s > 0; s >>= 1) {   // fixed tree
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid < 2) part[((int64_t)b * gridDim.x + blockIdx.x) * 2 + tid] = red[tid][0];
}

// losses[0] = sum of squared errors / n_mse, losses[1] = sum of |pooled difference| / n_ab (0 without cells); block order
__global__ __launch_bounds__(64) void photo_loss_final_kernel(const double *__restrict__ part, int64_t nparts, double n_mse, double n_ab,
                                                              float *__restrict__ losses)
{
    const int q = threadIdx.x;
    if (q >= 2) return;
    double a = 0.0;
    for (int64_t i = 0; i < nparts; ++i) a += part[i * 2 + q];
    losses[q] = q == 0 ? (float)(a / n_mse) : (n_ab > 0.0 ? (float)(a / n_ab) : 0.0f);
}

// d_pred = g_mse 2 (pred - gt) / n_mse + g_ab sign(cell) / (p^2 n_ab), formed in fp64 and rounded once; a pixel outside every cell
// (and every pixel without a patch) gets the first term only.  g_mse / g_ab: device scalars, NULL = 0.
__global__ void photo_loss_bwd_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ sign,
                                      const float *__restrict__ g_mse, const float *__restrict__ g_ab, int64_t total, int B, PhotoGrid G,
                                      double n_mse, double n_ab, float *__restrict__ d_pred)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const double gm = g_mse ? (double)g_mse[0] * 2.0 / n_mse : 0.0;
    const double ga = (g_ab && G.nc > 0) ? (double)g_ab[0] / ((double)G.p * G.p * n_ab) : 0.0;
    const int b = (int)(q / B), j = (int)(q - (int64_t)b * B);
    int cy = 0, cx = 0;
    bool in_cell = false;
    if (G.nc > 0) {
        const int r = j / G.width, c = j - r * G.width;
        cy = r / G.p; cx = c / G.p;
        in_cell = cy < G.nc && cx < G.nc;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double d = gm * ((double)pred[q * 3 + ch] - (double)gt[q * 3 + ch]);
        if (in_cell) d += ga * (double)sign[(((int64_t)b * 3 + ch) * G.nc + cy) * G.nc + cx];
        d_pred[q * 3 + ch] = (float)d;
    }
}

int invalid(const char *who, const char *what)
{
    set_error("%s: %s", who, what);
    return DINER_E_INVALID;
}

int check_rays(const char *who, int32_t SB, int32_t B, int32_t H, int32_t W)
{
    if (SB < 0 || B < 0 || H <= 0 || W <= 0) return invalid(who, "bad size (SB, B >= 0; H, W > 0)");
    if ((int64_t)H * W > 0x7fffffff) return invalid(who, "H * W beyond 2^31 - 1");
    if (SB > 65535 || (int64_t)SB * B > 0x7fffffff) {
        set_error("%s: SB=%d, B=%d unsupported (at most 65535 scenes and 2^31 - 1 rays in all)", who, SB, B);
        return DINER_E_UNSUPPORTED;
    }
    return DINER_OK;
}

// patch = 0: no patch (pool is not read); else B == patch^2, pool a power of two in [1, PL_MAX_POOL] and <= patch
int check_patch(const char *who, int32_t B, int32_t patch, int32_t pool)
{
    if (patch < 0) return invalid(who, "negative patch");
    if (patch == 0) return DINER_OK;
    if ((int64_t)patch * patch != B) return invalid(who, "B is not patch * patch");
    if (pool < 1 || (pool & (pool - 1))) return invalid(who, "pool is not a power of two");
    if (patch < pool) return invalid(who, "patch smaller than the pooling cell");
    if (pool > PL_MAX_POOL) {
        set_error("%s: pool=%d unsupported (cells of up to %d x %d pixels: a cell row is pooled from LDS)", who, pool, PL_MAX_POOL, PL_MAX_POOL);
        return DINER_E_UNSUPPORTED;
    }
    return DINER_OK;
}

}  // namespace

}  // namespace diner

using namespace diner;

int diner_gen_rays_at(const float *extrinsics, const float *intrinsics, const float *z_near, const float *z_far, const void *pix_idcs,
                      int32_t idx_is_int64, int32_t SB, int32_t B, int32_t H, int32_t W, float *rays_out, void *stream)
{
    const char *who = "gen_rays_at";
    if (const int rc = check_rays(who, SB, B, H, W)) return rc;
    const int64_t total = (int64_t)SB * B;
    if (total == 0) return DINER_OK;
    if (!extrinsics || !intrinsics || !z_near || !z_far || !pix_idcs || !rays_out) return invalid(who, "NULL pointer");
    hipLaunchKernelGGL(gen_rays_at_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, extrinsics, intrinsics,
                       z_near, z_far, pix_idcs, idx_is_int64 != 0, SB, B, H, W, rays_out);
    return check_launch("gen_rays_at_kernel");
}

int64_t diner_gen_rays_at_backward_workspace_floats(int32_t SB, int32_t B)
{
    if (SB < 0 || B < 0) return -1;
    return (int64_t)SB * gen_rays_at_bwd_blocks(B) * GA_SUMS * 2;   // doubles
}

int diner_gen_rays_at_backward(const float *extrinsics, const float *intrinsics, const float *d_rays, const void *pix_idcs,
                               int32_t idx_is_int64, int32_t SB, int32_t B, int32_t H, int32_t W, float *d_extrinsics, float *d_intrinsics,
                               float *d_near, float *d_far, float *workspace, void *stream)
{
    const char *who = "gen_rays_at_backward";
    if (const int rc = check_rays(who, SB, B, H, W)) return rc;
    if (SB == 0) return DINER_OK;
    if (!extrinsics || !intrinsics || !d_extrinsics || !d_intrinsics || !d_near || !d_far || !workspace || (B > 0 && (!d_rays || !pix_idcs)))
        return invalid(who, "NULL pointer");
    if ((uintptr_t)workspace % 8) return invalid(who, "workspace not 8-byte aligned");
    const int nblk = gen_rays_at_bwd_blocks(B);
    double *part = (double *)workspace;
    hipLaunchKernelGGL(gen_rays_at_bwd_partial_kernel, dim3((unsigned)nblk, (unsigned)SB), dim3(GA_THREADS), 0, (hipStream_t)stream, extrinsics,
                       intrinsics, d_rays, pix_idcs, idx_is_int64 != 0, B, H, W, nblk, part);
    if (const int rc = check_launch("gen_rays_at_bwd_partial_kernel")) return rc;
    hipLaunchKernelGGL(gen_rays_at_bwd_final_kernel, dim3((unsigned)SB), dim3(64), 0, (hipStream_t)stream, extrinsics, intrinsics, nblk,
                       (const double *)part, d_extrinsics, d_intrinsics, d_near, d_far);
    return check_launch("gen_rays_at_bwd_final_kernel");
}

int64_t diner_photo_loss_workspace_floats(int32_t SB, int32_t B, int32_t patch, int32_t pool)
{
    if (SB <= 0 || B <= 0 || check_patch("photo_loss", B, patch, pool)) return -1;
    const PhotoGrid G = photo_grid(B, patch, pool);
    return (int64_t)SB * G.nband * G.nchunk * 2 * 2;   // doubles
}

int diner_photo_loss(const float *pred, const float *target_rgb, const void *pix_idcs, int32_t idx_is_int64, int32_t SB, int32_t B, int32_t H,
                     int32_t W, int32_t patch, int32_t pool, float *gt_colors_out, float *losses_out, float *cell_sign_out, float *workspace,
                     void *stream)
{
    const char *who = "photo_loss";
    if (const int rc = check_rays(who, SB, B, H, W)) return rc;
    if (SB == 0 || B == 0) return invalid(who, "no rays (the mean of nothing)");
    if (const int rc = check_patch(who, B, patch, pool)) return rc;
    if (!pred || !target_rgb || !pix_idcs || !gt_colors_out || !losses_out || !workspace || (patch > 0 && !cell_sign_out))
        return invalid(who, "NULL pointer");
    if ((uintptr_t)workspace % 8) return invalid(who, "workspace not 8-byte aligned");
    const PhotoGrid G = photo_grid(B, patch, pool);
    const int nblk = G.nband * G.nchunk;
    double *part = (double *)workspace;
    hipLaunchKernelGGL(photo_loss_partial_kernel, dim3((unsigned)nblk, (unsigned)SB), dim3(PL_THREADS), 0, (hipStream_t)stream, pred, target_rgb,
                       pix_idcs, idx_is_int64 != 0, B, H, W, G, gt_colors_out, cell_sign_out, part);
    if (const int rc = check_launch("photo_loss_partial_kernel")) return rc;
    hipLaunchKernelGGL(photo_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)part, (int64_t)SB * nblk,
                       (double)SB * B * 3.0, (double)SB * 3.0 * G.nc * G.nc, losses_out);
    return check_launch("photo_loss_final_kernel");
}

int diner_photo_loss_backward(const float *pred, const float *gt_colors, const float *cell_sign, const float *g_mse, const float *g_ab,
                              int32_t SB, int32_t B, int32_t patch, int32_t pool, float *d_pred_out, void *stream)
{
    const char *who = "photo_loss_backward";
    if (SB <= 0 || B <= 0) return invalid(who, "no rays");
    if (const int rc = check_patch(who, B, patch, pool)) return rc;
    if (!pred || !gt_colors || !d_pred_out || (patch > 0 && !cell_sign)) return invalid(who, "NULL pointer");
    const PhotoGrid G = photo_grid(B, patch, pool);
    const int64_t total = (int64_t)SB * B;
    hipLaunchKernelGGL(photo_loss_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, gt_colors, cell_sign,
                       g_mse, g_ab, total, B, G, (double)SB * B * 3.0, (double)SB * 3.0 * G.nc * G.nc, d_pred_out);
    return check_launch("photo_loss_bwd_kernel");
}
