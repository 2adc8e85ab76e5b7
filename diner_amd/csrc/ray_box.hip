// Rendering inside a scene's axis-aligned bounding box: which pixels' rays meet the box, over which depth interval, and the way from
// the compact hit rays back to a frame.  The device form of FacescapeDataSet.get_near_far / get_mask_at_box (reference
// src/data/facescape.py:128-185) on the project's own rays (common.hpp gen_ray: pixel centres, unit directions):
//   ray_box_select   per pixel: the six face planes of the box b_min = bounds[0] + lo, b_max = bounds[1] + hi, direction components
//                    below 1e-5 in magnitude replaced by 1e-5, t = (b - o) / d per face, the face counts when its point t d + o lies
//                    within eps = 1e-6 of the box in the two other axes (:155-170); t0 / t1 = the smallest / largest such t, SIGNED;
//                    near = max(t0, z_near), far = min(t1, z_far); a hit has two or more such faces and far > near.
//   gen_rays_box     the compact rays [SB,B,8]: gen_ray at the hit pixels with the box's near / far
//   frame_from_hits  one thread per pixel gathers its colour and depth through `slot`, or writes the background
// Two deliberate differences from get_near_far (it takes the unsigned distances |p - o| and min / max of the two): a box behind the
// camera is a miss here (there its mirror image in front is hit), and a camera inside the box gets near = z_near (there the nearer face,
// which may be the one behind the camera).  A ray through an edge or a corner meets more than two faces within eps: a hit here, a miss
// for the reference's "exactly two" count.
// The compaction is ordered: each workgroup ranks its hits (ballot + popcount) and stores its count, one workgroup per scene scans the
// counts, a third pass adds the offsets.  No atomics: idx is ascending and two runs give the same bytes.
#include "common.hpp"

namespace diner {

namespace {

constexpr int RB_THREADS = 256, RB_WAVES = RB_THREADS / DINER_WAVE;

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

struct Box {
    float lo[3], hi[3];
};

__device__ __forceinline__ Box load_box(const float *__restrict__ bounds, int sb, float off_lo, float off_hi)
{
    Box b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = bounds[sb * 6 + a] + off_lo;       // bounds + boffset[:, None] (:155)
        b.hi[a] = bounds[sb * 6 + 3 + a] + off_hi;
    }
    return b;
}

// r = origin(3), direction(3) of gen_ray.  The only place that intersects a ray with a box: the select and the ray kernels both call
// it, so a compact ray's near / far are the select's bit for bit.  A miss returns the camera's interval.
__device__ __forceinline__ bool box_near_far(const float *r, const Box &b, float zn, float zf, float &near, float &far)
{
    const float eps = 1e-6f;
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = fabsf(r[3 + a]) < 1e-5f ? 1e-5f : r[3 + a];    // :158
    float t0 = __builtin_inff(), t1 = -__builtin_inff();
    int faces = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int a = f % 3, u = (a + 1) % 3, v = (a + 2) % 3;
        const float t = ((f < 3 ? b.lo[a] : b.hi[a]) - r[a]) / d[a];                  // :156, :159
        const float pu = t * d[u] + r[u], pv = t * d[v] + r[v];                       // :161 (the face's own axis is on it by construction)
        const bool on = pu >= b.lo[u] - eps && pu <= b.hi[u] + eps && pv >= b.lo[v] - eps && pv <= b.hi[v] + eps;   // NaN: off
        if (on) {
            t0 = fminf(t0, t);
            t1 = fmaxf(t1, t);
            ++faces;
        }
    }
    const float n = fmaxf(t0, zn), fa = fminf(t1, zf);
    const bool hit = faces >= 2 && fa > n;
    near = hit ? n : zn;
    far = hit ? fa : zf;
    return hit;
}

// pass 1: slot = the rank of a hit pixel among its workgroup's hits (-1: a miss), blk = the workgroup's number of hits
__global__ __launch_bounds__(RB_THREADS) void ray_box_mark_kernel(const float *__restrict__ extr, const float *__restrict__ intr,
                                                                  const float *__restrict__ z_near, const float *__restrict__ z_far,
                                                                  const float *__restrict__ bounds, float off_lo, float off_hi, int npix,
                                                                  int W, int nblk, float *__restrict__ near_far, int *__restrict__ slot,
                                                                  int *__restrict__ blk)
{
    __shared__ int wave_n[RB_WAVES];
    const int sb = blockIdx.y, tid = threadIdx.x, lane = tid & (DINER_WAVE - 1), wv = tid / DINER_WAVE;
    const int64_t pix = (int64_t)blockIdx.x * RB_THREADS + tid;
    bool hit = false;
    if (pix < npix) {
        const int y = (int)pix / W, x = (int)pix - y * W;
        const float zn = z_near[sb], zf = z_far[sb];
        float r[8], near, far;
        gen_ray(extr + sb * 16, intr + sb * 9, x, y, zn, zf, r);
        hit = box_near_far(r, load_box(bounds, sb, off_lo, off_hi), zn, zf, near, far);
        if (near_far != nullptr) *reinterpret_cast<float2 *>(near_far + ((int64_t)sb * npix + pix) * 2) = make_float2(near, far);
    }
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) wave_n[wv] = __popcll(votes);
    __syncthreads();
    int before = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < RB_WAVES; ++w) {
        before += w < wv ? wave_n[w] : 0;
        total += wave_n[w];
    }
    if (pix < npix) slot[(int64_t)sb * npix + pix] = hit ? before : -1;
    if (tid == 0) blk[(int64_t)sb * nblk + blockIdx.x] = total;
}

// pass 2: one workgroup per scene turns its workgroup counts into exclusive offsets, in place, RB_THREADS at a time with a carry
__global__ __launch_bounds__(RB_THREADS) void ray_box_scan_kernel(int *__restrict__ blk, int nblk, int *__restrict__ count)
{
    __shared__ int wave_n[RB_WAVES];
    const int tid = threadIdx.x, lane = tid & (DINER_WAVE - 1), wv = tid / DINER_WAVE;
    int *c = blk + (int64_t)blockIdx.x * nblk;
    int carry = 0;
    for (int base = 0; base < nblk; base += RB_THREADS) {
        const int i = base + tid, v = i < nblk ? c[i] : 0;
        const int incl = wave_scan_add_i(v, lane);
        if (lane == DINER_WAVE - 1) wave_n[wv] = incl;
        __syncthreads();
        int off = carry, chunk = 0;
#pragma unroll
        for (int w = 0; w < RB_WAVES; ++w) {
            off += w < wv ? wave_n[w] : 0;
            chunk += wave_n[w];
        }
        if (i < nblk) c[i] = off + incl - v;
        carry += chunk;
        __syncthreads();                 // wave_n is rewritten by the next chunk
    }
    if (tid == 0) count[blockIdx.x] = carry;
}

// pass 3: slot = the rank among the scene's hits; idx[rank] = the pixel; the entries of idx from count on are -1
__global__ __launch_bounds__(RB_THREADS) void ray_box_compact_kernel(const int *__restrict__ blk, const int *__restrict__ count, int npix,
                                                                     int nblk, int *__restrict__ slot, int *__restrict__ idx)
{
    const int sb = blockIdx.y;
    const int64_t pix = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (pix >= npix) return;
    const int64_t row = (int64_t)sb * npix;
    int s = slot[row + pix];
    if (s >= 0) {
        s += blk[(int64_t)sb * nblk + blockIdx.x];
        if (s < npix) {                  // always: a rank is below the number of pixels
            slot[row + pix] = s;
            idx[row + s] = (int)pix;
        }
    }
    if (pix >= count[sb]) idx[row + pix] = -1;
}

// rays [SB,B,8]: entry j of scene sb is the ray of its hit min(j, count - 1); a scene without hits repeats pixel 0 with the camera's
// interval
__global__ __launch_bounds__(RB_THREADS) void gen_rays_box_kernel(const float *__restrict__ extr, const float *__restrict__ intr,
                                                                  const float *__restrict__ z_near, const float *__restrict__ z_far,
                                                                  const float *__restrict__ bounds, float off_lo, float off_hi,
                                                                  const int *__restrict__ idx, const int *__restrict__ count, int64_t total,
                                                                  int B, int npix, int W, float *__restrict__ rays)
{
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (i >= total) return;
    const int sb = (int)(i / B), j = (int)(i - (int64_t)sb * B);
    int cnt = count[sb];
    cnt = cnt < 0 ? 0 : (cnt > npix ? npix : cnt);
    int p = cnt > 0 ? idx[(int64_t)sb * npix + (j < cnt ? j : cnt - 1)] : 0;
    p = p < 0 ? 0 : (p > npix - 1 ? npix - 1 : p);
    const int y = p / W, x = p - y * W;
    const float zn = z_near[sb], zf = z_far[sb];
    float r[8], near = zn, far = zf;
    gen_ray(extr + sb * 16, intr + sb * 9, x, y, zn, zf, r);
    if (cnt > 0) box_near_far(r, load_box(bounds, sb, off_lo, off_hi), zn, zf, near, far);
    float4 *dst = reinterpret_cast<float4 *>(rays + i * 8);
    dst[0] = make_float4(r[0], r[1], r[2], r[3]);
    dst[1] = make_float4(r[4], r[5], near, far);
}

// rgb_out [SB,H W,3], depth_out [SB,H W], mask_out [SB,H W] bytes (optional) from the compact results rgb_c [SB,B,3], depth_c [SB,B]
__global__ __launch_bounds__(RB_THREADS) void frame_from_hits_kernel(const float *__restrict__ rgb_c, const float *__restrict__ depth_c,
                                                                     const int *__restrict__ slot, int64_t total, int npix, int B, float bg,
                                                                     float *__restrict__ rgb_out, float *__restrict__ depth_out,
                                                                     uint8_t *__restrict__ mask_out)
{
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t sb = i / npix;
    const int s = slot[i];
    const bool hit = s >= 0 && s < B;
    float c0 = bg, c1 = bg, c2 = bg, d = 0.0f;
    if (hit) {
        const float *c = rgb_c + (sb * B + s) * 3;
        c0 = c[0]; c1 = c[1]; c2 = c[2];
        d = depth_c[sb * B + s];
    }
    rgb_out[i * 3] = c0; rgb_out[i * 3 + 1] = c1; rgb_out[i * 3 + 2] = c2;
    depth_out[i] = d;
    if (mask_out != nullptr) mask_out[i] = hit ? 1 : 0;
}

// the sizes every function here takes: < 0 an error, 0 nothing to do (rc = DINER_OK with npix = 0)
int check_sizes(const char *who, int32_t SB, int32_t H, int32_t W, int64_t &npix)
{
    npix = 0;
    if (SB < 0 || H < 0 || W < 0) return invalid(who, "negative size (SB, H, W)");
    if ((int64_t)H * W > 0x7fffffff) return unsupported(who, "H * W of 2^31 or more");
    if (SB > 65535) return unsupported(who, "more than 65535 scenes");
    npix = SB == 0 ? 0 : (int64_t)H * W;
    return DINER_OK;
}

int check_cam(const char *who, const DinerTargetCam *cam, const float *bounds)
{
    if (!cam) return invalid(who, "NULL camera");
    if (!cam->extrinsics || !cam->intrinsics || !cam->z_near || !cam->z_far) return invalid(who, "NULL pointer in the camera");
    if (!bounds) return invalid(who, "NULL bounds");
    return DINER_OK;
}

int blocks_of(int64_t npix) { return (int)((npix + RB_THREADS - 1) / RB_THREADS); }

}  // namespace

}  // namespace diner

using namespace diner;

int64_t diner_ray_box_select_workspace_floats(int32_t SB, int32_t H, int32_t W)
{
    if (SB < 0 || H < 0 || W < 0 || (int64_t)H * W > 0x7fffffff || SB > 65535) return -1;
    return (int64_t)SB * blocks_of((int64_t)H * W);
}

int diner_ray_box_select(const DinerTargetCam *cam, int32_t SB, const float *bounds, float box_lo, float box_hi, float *near_far,
                         int32_t *idx, int32_t *slot, int32_t *count, float *workspace, void *stream)
{
    const char *who = "ray_box_select";
    if (!cam) return invalid(who, "NULL camera");
    int64_t npix = 0;
    if (const int rc = check_sizes(who, SB, cam->H, cam->W, npix)) return rc;
    if (npix == 0) return DINER_OK;
    if (const int rc = check_cam(who, cam, bounds)) return rc;
    if (!idx || !slot || !count || !workspace) return invalid(who, "NULL pointer");
    if ((uintptr_t)workspace % 4 || (uintptr_t)idx % 4 || (uintptr_t)slot % 4 || (uintptr_t)count % 4)
        return invalid(who, "workspace, idx, slot or count not 4-byte aligned");
    if ((uintptr_t)near_far % 8) return invalid(who, "near_far not 8-byte aligned");
    const int nblk = blocks_of(npix);
    int *blk = reinterpret_cast<int *>(workspace);
    const dim3 grid((unsigned)nblk, (unsigned)SB);
    hipLaunchKernelGGL(ray_box_mark_kernel, grid, dim3(RB_THREADS), 0, (hipStream_t)stream, cam->extrinsics, cam->intrinsics, cam->z_near,
                       cam->z_far, bounds, box_lo, box_hi, (int)npix, cam->W, nblk, near_far, slot, blk);
    if (const int rc = check_launch("ray_box_mark_kernel")) return rc;
    hipLaunchKernelGGL(ray_box_scan_kernel, dim3((unsigned)SB), dim3(RB_THREADS), 0, (hipStream_t)stream, blk, nblk, count);
    if (const int rc = check_launch("ray_box_scan_kernel")) return rc;
    hipLaunchKernelGGL(ray_box_compact_kernel, grid, dim3(RB_THREADS), 0, (hipStream_t)stream, (const int *)blk, (const int *)count, (int)npix,
                       nblk, slot, idx);
    return check_launch("ray_box_compact_kernel");
}

int diner_gen_rays_box(const DinerTargetCam *cam, int32_t SB, const float *bounds, float box_lo, float box_hi, const int32_t *idx,
                       const int32_t *count, const int32_t *count_host, int32_t B, float *rays, void *stream)
{
    const char *who = "gen_rays_box";
    if (!cam) return invalid(who, "NULL camera");
    int64_t npix = 0;
    if (const int rc = check_sizes(who, SB, cam->H, cam->W, npix)) return rc;
    if (B < 0) return invalid(who, "negative B");
    if (count_host)
        for (int sb = 0; sb < SB; ++sb)
            if (count_host[sb] > B) return invalid(who, "B below a scene's number of hits");
    if (npix == 0 || B == 0) return DINER_OK;
    if (const int rc = check_cam(who, cam, bounds)) return rc;
    if (!idx || !count || !rays) return invalid(who, "NULL pointer");
    if ((uintptr_t)rays % 16) return invalid(who, "rays not 16-byte aligned");
    const int64_t total = (int64_t)SB * B, blocks = (total + RB_THREADS - 1) / RB_THREADS;
    if (blocks > 0x7fffffff) return unsupported(who, "beyond one launch's grid");
    hipLaunchKernelGGL(gen_rays_box_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), 0, (hipStream_t)stream, cam->extrinsics, cam->intrinsics,
                       cam->z_near, cam->z_far, bounds, box_lo, box_hi, idx, count, total, B, (int)npix, cam->W, rays);
    return check_launch("gen_rays_box_kernel");
}

int diner_frame_from_hits(const float *rgb_c, const float *depth_c, const int32_t *slot, int32_t SB, int32_t B, int32_t H, int32_t W,
                          int32_t white_bkgd, float *rgb_out, float *depth_out, uint8_t *mask_out, void *stream)
{
    const char *who = "frame_from_hits";
    int64_t npix = 0;
    if (const int rc = check_sizes(who, SB, H, W, npix)) return rc;
    if (B < 0) return invalid(who, "negative B");
    if (npix == 0) return DINER_OK;
    if (!slot || !rgb_out || !depth_out) return invalid(who, "NULL pointer");
    if (B > 0 && (!rgb_c || !depth_c)) return invalid(who, "NULL compact colour or depth with B > 0");
    const int64_t total = (int64_t)SB * npix, blocks = (total + RB_THREADS - 1) / RB_THREADS;
    if (blocks > 0x7fffffff) return unsupported(who, "beyond one launch's grid");
    hipLaunchKernelGGL(frame_from_hits_kernel, dim3((unsigned)blocks), dim3(RB_THREADS), 0, (hipStream_t)stream, rgb_c, depth_c, slot, total,
                       (int)npix, B, white_bkgd ? 1.0f : 0.0f, rgb_out, depth_out, mask_out);
    return check_launch("frame_from_hits_kernel");
}
