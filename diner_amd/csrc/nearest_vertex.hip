// Nearest mesh vertex of every point, and the deformation the fork's NOVEL / NOVEL_PE renderers build on it (reference
// src/models/novel/nerf_novel_renderer.py:40-50: knn_points(points, target_vertices, K=1), points + offsets[nearest]).
//
// Arithmetic contract (include/diner_hip.h): d2 = ((px - vx)^2 + (py - vy)^2) + (pz - vz)^2, every operation rounded once to fp32 (the
// library is built with -ffp-contract=off and nothing here is an fma); the winner is the vertex of smallest (d2, original index) among
// those with d2 < +inf; a point without one (NaN / inf distances only) gets index 0 and d2 = +inf.  Every comparison is written so that
// a NaN d2 loses it.  No array index comes from a point's coordinates; the Morton keys, which come from vertex coordinates, are clamped
// with fmaxf / fminf before the conversion to int.
//
//   nv_brute_kernel    the device truth and the route for small V: the scene's vertices pass through LDS in SoA tiles, every lane reads
//                      the same vertex (a broadcast read) and holds P points in registers; vertices in ascending order with a strict
//                      `<`, so the lowest index wins a tie.
//   nv_keys_kernel     one workgroup per scene: the bounding box of the finite vertex coordinates, then a 30-bit Morton key per vertex
//                      (10 bits per axis; an axis of zero extent contributes 0).  The stable sort of the keys is the caller's.
//   nv_cluster_kernel  one wave per cluster of 64 consecutive sorted vertices: the permuted copy (x, y, z, original index) -- the ragged
//                      end padded with NaN vertices, which can never win -- and the cluster's AABB.
//   nv_pruned_kernel   one point per lane.  lb = (ex^2 + ey^2) + ez^2 with e = max(lo - p, p - hi, 0) per axis is the fp32 lower bound of
//                      a cluster: subtraction, squaring of non-negatives and addition are monotone in fp32, so lb <= d2 of every member,
//                      and a cluster with lb > best can hold neither a nearer vertex nor a tie.  Pass A finds each lane's cluster of
//                      smallest lb (the seed); the wave scans the distinct seeds of its lanes; pass B walks the clusters once more and
//                      the wave scans one when any lane has lb <= best and it was no seed.  A scan is wave-uniform: all lanes read the
//                      same 64 vertices and update with the lexicographic (d2, index) comparison, so a cluster scanned for a
//                      neighbour's sake cannot change a lane's result -- the kernel returns the brute-force kernel's bits for every input.
//                      The AABBs of a scene sit in LDS, NV_TILE_C clusters at a time.
// The epilogue is shared: idx / d2, or out = p + offsets[idx] for one or two offset sets (and the point itself), with the point read from
// `points` or formed from a ray as o + z d (multiply, then add: :412).  No atomics; every output element is written.
#include "common.hpp"

namespace diner {

namespace {

constexpr int NV_THREADS = 256;
constexpr int NV_TILE_V = 1024;     // vertices per LDS tile of the brute-force kernel (12 KiB)
constexpr int NV_TILE_C = 1024;     // cluster AABBs per LDS tile of the pruned kernel (24 KiB)
constexpr int NV_CLUSTER = 64;
constexpr int64_t NV_MAX_V = (int64_t)1 << 24;

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

// where a kernel's points come from and where its results go (device pointers; the optional ones may be NULL)
struct NvIo {
    const float *points;      // [SB,N,3], or NULL: rays + z
    const float *rays;        // [SB,B,8]
    const float *z;           // [SB,B,K]
    int K;
    int64_t N;                // points per scene (B K in the ray form)
    int V;
    const float *off1, *off2; // [SB,V,3] (off2 optional); off1 NULL: the search form
    int32_t *idx;             // [SB,N]
    float *d2;                // [SB,N]
    float *out1, *out2, *pts; // [SB,N,3]
};

__device__ __forceinline__ void load_point(const NvIo &io, int sb, int64_t n, float &px, float &py, float &pz)
{
    if (io.points != nullptr) {
        const float *p = io.points + ((int64_t)sb * io.N + n) * 3;
        px = p[0]; py = p[1]; pz = p[2];
    } else {
        const int64_t b = n / io.K;
        const float *r = io.rays + ((int64_t)sb * (io.N / io.K) + b) * 8;
        const float zz = io.z[(int64_t)sb * io.N + n];
        px = r[0] + zz * r[3]; py = r[1] + zz * r[4]; pz = r[2] + zz * r[5];     // no contraction: -ffp-contract=off
    }
}

__device__ __forceinline__ void store_result(const NvIo &io, int sb, int64_t n, float px, float py, float pz, int bi, float bd)
{
    const int64_t row = (int64_t)sb * io.N + n;
    if (io.off1 == nullptr) {
        io.idx[row] = bi;
        io.d2[row] = bd;
        return;
    }
    bi = bi < 0 ? 0 : (bi > io.V - 1 ? io.V - 1 : bi);     // a vertex index by construction; clamped all the same (a foreign workspace)
    const int64_t v = ((int64_t)sb * io.V + bi) * 3;
    io.out1[row * 3] = px + io.off1[v]; io.out1[row * 3 + 1] = py + io.off1[v + 1]; io.out1[row * 3 + 2] = pz + io.off1[v + 2];
    if (io.off2 != nullptr) {
        io.out2[row * 3] = px + io.off2[v]; io.out2[row * 3 + 1] = py + io.off2[v + 1]; io.out2[row * 3 + 2] = pz + io.off2[v + 2];
    }
    if (io.pts != nullptr) {
        io.pts[row * 3] = px; io.pts[row * 3 + 1] = py; io.pts[row * 3 + 2] = pz;
    }
}

// ---- brute force ---------------------------------------------------------------------------------------------------------------------------
// vertices [SB,V,3]; grid (ceil(N / (NV_THREADS P)), SB); point j of a thread is block base + j NV_THREADS + tid (coalesced)
template <int P>
__global__ __launch_bounds__(NV_THREADS) void nv_brute_kernel(NvIo io, const float *__restrict__ vertices)
{
    __shared__ float sx[NV_TILE_V], sy[NV_TILE_V], sz[NV_TILE_V];
    const int sb = blockIdx.y, tid = threadIdx.x, V = io.V;
    const int64_t base = (int64_t)blockIdx.x * (NV_THREADS * P);
    float px[P], py[P], pz[P], bd[P];
    int bi[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t n = base + j * NV_THREADS + tid;
        px[j] = py[j] = pz[j] = 0.0f;
        if (n < io.N) load_point(io, sb, n, px[j], py[j], pz[j]);
        bd[j] = __builtin_inff();
        bi[j] = 0;
    }
    const float *vs = vertices + (int64_t)sb * V * 3;
    for (int v0 = 0; v0 < V; v0 += NV_TILE_V) {
        const int nt = V - v0 < NV_TILE_V ? V - v0 : NV_TILE_V;
        __syncthreads();                                   // the previous tile has been read
        for (int i = tid; i < nt; i += NV_THREADS) {
            const float *v = vs + (int64_t)(v0 + i) * 3;
            sx[i] = v[0]; sy[i] = v[1]; sz[i] = v[2];
        }
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            const float vx = sx[i], vy = sy[i], vz = sz[i];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const float dx = px[j] - vx, dy = py[j] - vy, dz = pz[j] - vz;
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < bd[j]) {                           // strict, ascending index: the lowest index wins a tie; NaN: false
                    bd[j] = d;
                    bi[j] = v0 + i;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int64_t n = base + j * NV_THREADS + tid;
        if (n < io.N) store_result(io, sb, n, px[j], py[j], pz[j], bi[j], bd[j]);
    }
}

// ---- cluster build -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t spread10(uint32_t x)      // bit i of the low 10 -> bit 3 i
{
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// keys [SB,V] int32 in [0, 2^30); one workgroup per scene
__global__ __launch_bounds__(NV_THREADS) void nv_keys_kernel(const float *__restrict__ vertices, int V, int32_t *__restrict__ keys)
{
    __shared__ float red[6][NV_THREADS];
    const int sb = blockIdx.x, tid = threadIdx.x;
    const float *vs = vertices + (int64_t)sb * V * 3;
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int i = tid; i < V; i += NV_THREADS)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = vs[(int64_t)i * 3 + a];
            if (fabsf(x) < inf) {                          // finite coordinates only (NaN: false)
                lo[a] = x < lo[a] ? x : lo[a];
                hi[a] = x > hi[a] ? x : hi[a];
            }
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        red[a][tid] = lo[a];
        red[3 + a][tid] = hi[a];
    }
    __syncthreads();
    for (int s = NV_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                red[a][tid] = fminf(red[a][tid], red[a][tid + s]);
                red[3 + a][tid] = fmaxf(red[3 + a][tid], red[3 + a][tid + s]);
            }
        __syncthreads();
    }
    float scale[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = red[a][0];
        const float ext = red[3 + a][0] - lo[a];
        scale[a] = (ext > 0.0f && ext < inf) ? 1024.0f / ext : 0.0f;      // zero extent (or no finite coordinate): key bits 0
    }
    for (int i = tid; i < V; i += NV_THREADS) {
        uint32_t key = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float q = (vs[(int64_t)i * 3 + a] - lo[a]) * scale[a];
            const int qi = (int)fminf(fmaxf(q, 0.0f), 1023.0f);          // fmaxf(NaN, 0) = 0: clamped before the conversion
            key |= spread10((uint32_t)qi) << (2 - a);
        }
        keys[(int64_t)sb * V + i] = (int32_t)key;
    }
}

// order [SB,V] int32: the vertices in sorted order.  sorted [SB,nclus 64] float4 (x, y, z, original index), aabb [SB,nclus,6] (lo, hi).
// grid (nclus, SB), one wave per cluster
__global__ __launch_bounds__(NV_CLUSTER) void nv_cluster_kernel(const float *__restrict__ vertices, const int32_t *__restrict__ order, int V,
                                                                int nclus, float4 *__restrict__ sorted, float *__restrict__ aabb)
{
    const int c = blockIdx.x, sb = blockIdx.y, lane = threadIdx.x;
    const int s = c * NV_CLUSTER + lane;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    float x = nan, y = nan, z = nan;
    int oi = 0;
    if (s < V) {
        oi = order[(int64_t)sb * V + s];
        oi = oi < 0 ? 0 : (oi > V - 1 ? V - 1 : oi);       // whatever the caller's order holds, a vertex index
        const float *v = vertices + ((int64_t)sb * V + oi) * 3;
        x = v[0]; y = v[1]; z = v[2];
    }
    sorted[((int64_t)sb * nclus + c) * NV_CLUSTER + lane] = make_float4(x, y, z, __int_as_float(oi));
    float lo[3] = {x == x ? x : inf, y == y ? y : inf, z == z ? z : inf};          // a NaN coordinate (the padding too) bounds nothing
    float hi[3] = {x == x ? x : -inf, y == y ? y : -inf, z == z ? z : -inf};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
    if (lane < 6) {
        const float val = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lane == 3 ? hi[0] : lane == 4 ? hi[1] : hi[2];
        aabb[((int64_t)sb * nclus + c) * 6 + lane] = val;
    }
}

// ---- pruned query --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float axis_excess(float lo, float hi, float p)
{
    float e = 0.0f;
    const float a = lo - p, b = p - hi;
    e = a > e ? a : e;                                     // max(lo - p, p - hi, 0); a NaN p leaves 0: the cluster is scanned
    e = b > e ? b : e;
    return e;
}

// all lanes of the wave scan cluster c (wave-uniform): the same 64 vertices for every lane
__device__ __forceinline__ void scan_cluster(const float4 *__restrict__ sv, int c, float px, float py, float pz, float &bd, int &bi)
{
    const float4 *v = sv + (int64_t)c * NV_CLUSTER;
#pragma unroll 8
    for (int j = 0; j < NV_CLUSTER; ++j) {
        const float4 q = v[j];
        const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        const int oi = __float_as_int(q.w);
        if (d < bd || (d == bd && oi < bi)) {              // lexicographic (d2, original index); NaN: false twice
            bd = d;
            bi = oi;
        }
    }
}

__device__ __forceinline__ void load_aabb_tile(float (*sa)[NV_TILE_C], const float *__restrict__ aabb, int c0, int nt, int tid)
{
    for (int i = tid; i < nt * 6; i += NV_THREADS) sa[i % 6][i / 6] = aabb[(int64_t)c0 * 6 + i];
}

// grid (ceil(N / NV_THREADS), SB)
__global__ __launch_bounds__(NV_THREADS) void nv_pruned_kernel(NvIo io, const float4 *__restrict__ sorted, const float *__restrict__ aabb,
                                                               int nclus)
{
    __shared__ float sa[6][NV_TILE_C];
    const int sb = blockIdx.y, tid = threadIdx.x;
    const int64_t n = (int64_t)blockIdx.x * NV_THREADS + tid;
    const bool valid = n < io.N;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (valid) load_point(io, sb, n, px, py, pz);
    const float4 *sv = sorted + (int64_t)sb * nclus * NV_CLUSTER;
    const float *ab = aabb + (int64_t)sb * nclus * 6;
    const bool single = nclus <= NV_TILE_C;               // one tile: loaded once for both passes

    // pass A: the cluster of smallest lower bound (the first of equals)
    float lbmin = __builtin_inff();
    int seed = 0;
    for (int c0 = 0; c0 < nclus; c0 += NV_TILE_C) {
        const int nt = nclus - c0 < NV_TILE_C ? nclus - c0 : NV_TILE_C;
        __syncthreads();
        load_aabb_tile(sa, ab, c0, nt, tid);
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            const float ex = axis_excess(sa[0][i], sa[3][i], px), ey = axis_excess(sa[1][i], sa[4][i], py),
                        ez = axis_excess(sa[2][i], sa[5][i], pz);
            const float lb = (ex * ex + ey * ey) + ez * ez;
            if (lb < lbmin) {
                lbmin = lb;
                seed = c0 + i;
            }
        }
    }
    if (!valid) seed = -1;                                 // equals no cluster

    // the distinct seeds of the wave's lanes, each scanned once by all of them
    float bd = __builtin_inff();
    int bi = 0;
    unsigned long long pending = __ballot(valid);
    while (pending != 0ull) {
        const int leader = __ffsll((long long)pending) - 1;
        int c = __builtin_amdgcn_readfirstlane(__shfl(seed, leader, 64));
        c = c < 0 ? 0 : (c > nclus - 1 ? nclus - 1 : c);
        scan_cluster(sv, c, px, py, pz, bd, bi);
        pending &= ~(__ballot(seed == c) | (1ull << leader));     // (the leader's bit: the loop ends whatever seed holds)
    }

    // pass B: every other cluster that some lane cannot exclude
    for (int c0 = 0; c0 < nclus; c0 += NV_TILE_C) {
        const int nt = nclus - c0 < NV_TILE_C ? nclus - c0 : NV_TILE_C;
        if (!single) {
            __syncthreads();
            load_aabb_tile(sa, ab, c0, nt, tid);
            __syncthreads();
        }
        for (int i = 0; i < nt; ++i) {
            const float ex = axis_excess(sa[0][i], sa[3][i], px), ey = axis_excess(sa[1][i], sa[4][i], py),
                        ez = axis_excess(sa[2][i], sa[5][i], pz);
            const float lb = (ex * ex + ey * ey) + ez * ez;
            const int c = c0 + i;
            const bool was_seed = __ballot(seed == c) != 0ull;
            const bool wanted = __ballot(valid && lb <= bd) != 0ull;       // <=: a tie with a lower index may sit in the cluster
            if (!was_seed && wanted) scan_cluster(sv, c, px, py, pz, bd, bi);
        }
    }
    if (valid) store_result(io, sb, n, px, py, pz, bi, bd);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
int nclusters(int64_t V) { return (int)((V + NV_CLUSTER - 1) / NV_CLUSTER); }

// the sizes every function here takes; N == 0 (or SB == 0) is nothing to do and is the caller's to test after this
int check_sizes(const char *who, int32_t SB, int64_t N, int32_t V)
{
    if (V <= 0) return invalid(who, "non-positive V");
    if (SB < 0 || N < 0) return invalid(who, "negative size (SB, N)");
    if (V > NV_MAX_V) return unsupported(who, "more than 2^24 vertices");
    if (N > 0x7fffffffll) return unsupported(who, "2^31 or more points per scene");
    if (SB > 65535) return unsupported(who, "more than 65535 scenes");
    return DINER_OK;
}

// workspace == NULL: brute force.  The launch of either search kernel with the epilogue io describes.
int launch_search(const char *who, NvIo io, int32_t SB, const float *vertices, const float *workspace, void *stream)
{
    if (workspace != nullptr) {
        if ((uintptr_t)workspace % 16) return invalid(who, "workspace not 16-byte aligned");
        const int nclus = nclusters(io.V);
        const float4 *sorted = reinterpret_cast<const float4 *>(workspace);
        const float *aabb = workspace + (int64_t)SB * nclus * NV_CLUSTER * 4;
        const dim3 grid((unsigned)((io.N + NV_THREADS - 1) / NV_THREADS), (unsigned)SB);
        hipLaunchKernelGGL(nv_pruned_kernel, grid, dim3(NV_THREADS), 0, (hipStream_t)stream, io, sorted, aabb, nclus);
        return check_launch("nv_pruned_kernel");
    }
    // 4 points per thread once that still fills the device with workgroups
    const int64_t blocks4 = (io.N + NV_THREADS * 4 - 1) / (NV_THREADS * 4);
    if (blocks4 * SB >= 2 * (int64_t)device_cus()) {
        hipLaunchKernelGGL(nv_brute_kernel<4>, dim3((unsigned)blocks4, (unsigned)SB), dim3(NV_THREADS), 0, (hipStream_t)stream, io, vertices);
    } else {
        const dim3 grid((unsigned)((io.N + NV_THREADS - 1) / NV_THREADS), (unsigned)SB);
        hipLaunchKernelGGL(nv_brute_kernel<1>, grid, dim3(NV_THREADS), 0, (hipStream_t)stream, io, vertices);
    }
    return check_launch("nv_brute_kernel");
}

}  // namespace

}  // namespace diner

using namespace diner;

int64_t diner_nearest_vertex_workspace_floats(int32_t SB, int32_t V)
{
    if (SB < 0 || SB > 65535 || V <= 0 || V > NV_MAX_V) return -1;
    return (int64_t)SB * nclusters(V) * (NV_CLUSTER * 4 + 6);
}

int diner_nearest_vertex_keys(const float *vertices, int32_t SB, int32_t V, int32_t *keys, void *stream)
{
    const char *who = "nearest_vertex_keys";
    if (const int rc = check_sizes(who, SB, 0, V)) return rc;
    if (SB == 0) return DINER_OK;
    if (!vertices || !keys) return invalid(who, "NULL pointer");
    hipLaunchKernelGGL(nv_keys_kernel, dim3((unsigned)SB), dim3(NV_THREADS), 0, (hipStream_t)stream, vertices, V, keys);
    return check_launch("nv_keys_kernel");
}

int diner_nearest_vertex_build(const float *vertices, const int32_t *order, int32_t SB, int32_t V, float *workspace, void *stream)
{
    const char *who = "nearest_vertex_build";
    if (const int rc = check_sizes(who, SB, 0, V)) return rc;
    if (SB == 0) return DINER_OK;
    if (!vertices || !order || !workspace) return invalid(who, "NULL pointer");
    if ((uintptr_t)workspace % 16) return invalid(who, "workspace not 16-byte aligned");
    const int nclus = nclusters(V);
    float4 *sorted = reinterpret_cast<float4 *>(workspace);
    float *aabb = workspace + (int64_t)SB * nclus * NV_CLUSTER * 4;
    hipLaunchKernelGGL(nv_cluster_kernel, dim3((unsigned)nclus, (unsigned)SB), dim3(NV_CLUSTER), 0, (hipStream_t)stream, vertices, order, V,
                       nclus, sorted, aabb);
    return check_launch("nv_cluster_kernel");
}

int diner_nearest_vertex(const float *points, const float *vertices, const float *workspace, int32_t SB, int64_t N, int32_t V, int32_t *idx,
                         float *d2, void *stream)
{
    const char *who = "nearest_vertex";
    if (const int rc = check_sizes(who, SB, N, V)) return rc;
    if (N == 0 || SB == 0) return DINER_OK;
    if (!points || !vertices || !idx || !d2) return invalid(who, "NULL pointer");
    NvIo io = {};
    io.points = points; io.N = N; io.V = V; io.K = 1; io.idx = idx; io.d2 = d2;
    return launch_search(who, io, SB, vertices, workspace, stream);
}

int diner_deform_points(const float *points, const float *vertices, const float *workspace, const float *offsets, const float *offsets2,
                        int32_t SB, int64_t N, int32_t V, float *out, float *out2, void *stream)
{
    const char *who = "deform_points";
    if (const int rc = check_sizes(who, SB, N, V)) return rc;
    if (N == 0 || SB == 0) return DINER_OK;
    if (!points || !vertices || !offsets || !out) return invalid(who, "NULL pointer");
    if ((offsets2 == nullptr) != (out2 == nullptr)) return invalid(who, "offsets2 and out2 go together");
    NvIo io = {};
    io.points = points; io.N = N; io.V = V; io.K = 1; io.off1 = offsets; io.off2 = offsets2; io.out1 = out; io.out2 = out2;
    return launch_search(who, io, SB, vertices, workspace, stream);
}

int diner_deform_ray_points(const float *rays, const float *z, const float *vertices, const float *workspace, const float *offsets,
                            const float *offsets2, int32_t SB, int64_t B, int32_t K, int32_t V, float *out, float *out2, float *points_out,
                            void *stream)
{
    const char *who = "deform_ray_points";
    if (B < 0 || K < 0) return invalid(who, "negative size (B, K)");
    if (B > 0x7fffffffll) return unsupported(who, "2^31 or more rays per scene");
    if (const int rc = check_sizes(who, SB, B * K, V)) return rc;
    if (B * K == 0 || SB == 0) return DINER_OK;
    if (!rays || !z || !vertices || !offsets || !out) return invalid(who, "NULL pointer");
    if ((offsets2 == nullptr) != (out2 == nullptr)) return invalid(who, "offsets2 and out2 go together");
    NvIo io = {};
    io.rays = rays; io.z = z; io.K = K; io.N = B * K; io.V = V; io.off1 = offsets; io.off2 = offsets2; io.out1 = out; io.out2 = out2;
    io.pts = points_out;
    return launch_search(who, io, SB, vertices, workspace, stream);
}
