// extern "C" entry points of libdiner_hip.so (declared in include/diner_hip.h): argument
// validation, error strings, stream plumbing.  No kernel code here.
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

#include "common.hpp"

namespace diner {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return DINER_E_LAUNCH;
    }
    return DINER_OK;
}

// ---- per-device launch state (common.hpp) ---------------------------------------------------------------------------------------
constexpr int MAX_DEVICES = 64;
static std::atomic<int> g_cus[MAX_DEVICES];                       // 0 = not asked yet
static std::atomic<int> g_lds_set[MAX_DEVICES][LDS_SLOT_COUNT];   // bytes the kernel of a slot has been raised to on a device

static int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    return dev;
}

int device_cus()
{
    const int dev = current_device();
    if (dev < 0 || dev >= MAX_DEVICES) {      // beyond the table: ask every time
        int n = 0;
        return (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    int n = g_cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
        g_cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int ensure_dynamic_lds(const void *kernel, int bytes, int slot)
{
    const int dev = current_device();
    const bool cached = dev >= 0 && dev < MAX_DEVICES && slot >= 0 && slot < LDS_SLOT_COUNT;
    if (cached && g_lds_set[dev][slot].load(std::memory_order_acquire) == bytes) return DINER_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return check_launch("hipFuncSetAttribute(dynamic LDS)");
    if (cached) g_lds_set[dev][slot].store(bytes, std::memory_order_release);
    return DINER_OK;
}

int launch_composite(const float *, const float *, const float *, int64_t, int, int, float *, float *, float *, unsigned int *, hipStream_t);
int launch_pack_maps(const float *, const float *, const float *, int64_t, int, int, float *, hipStream_t);
int launch_pack_latent(const float *, int64_t, int, int, int, float *, hipStream_t);
int launch_pack_mlp(const DinerMlpRaw &, float *, hipStream_t);
int64_t mlp_packed_floats();
int launch_train_gemm(const float *, const float *, const float *, const float *, float *, int64_t, int, int, int64_t, int64_t, int64_t,
                      int64_t, int64_t, int64_t, int, int, int, int, int64_t, int, const unsigned int *, const unsigned int *, int, int,
                      hipStream_t);
int launch_train_amax(const float *, int64_t, unsigned int *, hipStream_t);
int launch_train_colsum_amax(const float *, int64_t, int, int64_t, float *, unsigned int *, hipStream_t);
int launch_train_split_panel(const float *, int, int64_t, int, int, void *, void *, hipStream_t);
int launch_train_pack_core(const float *, int64_t, int, int, void *, hipStream_t);
int launch_train_gemm_core(const float *, int64_t, const void *, const float *, const float *, int64_t, const float *, int64_t, float *, int64_t,
                           int64_t, int, const unsigned int *, int, int, float *, unsigned int *, hipStream_t);
int launch_train_gemm_panel(const float *, int64_t, const void *, const void *, const float *, const float *, int64_t, const float *,
                            int64_t, float *, int64_t, int64_t, int, int, const unsigned int *, int, int, hipStream_t);
int launch_train_colsum(const float *, int64_t, int, int64_t, float *, hipStream_t);
int launch_train_point_inputs(const DinerScene &, const DinerLatentIndex &, const float *, int, const float *, const float *, int64_t, int, int, float *, float *,
                              float *, hipStream_t);
int launch_train_bilinear_scatter(const float *, const float *, int64_t, int, int, int, int, int, float *, hipStream_t);
int launch_train_view_mean(const float *, int64_t, int, float *, int, hipStream_t);
int launch_train_nhwc_to_nchw(const float *, int64_t, int, int, int, float *, hipStream_t);
int launch_train_head(const float *, const float *, const float *, int64_t, float *, int, hipStream_t);
int launch_train_composite_bwd(const float *, const float *, const float *, const float *, const float *, const float *, int64_t, int,
                               int, float *, hipStream_t);
int launch_train_composite_bwd_far(const float *, const float *, const float *, const float *, const float *, const float *, int64_t, int,
                                   int, float *, float *, hipStream_t);
int64_t train_camera_workspace_floats(int64_t, int, int);
int launch_train_point_inputs_bwd(const DinerScene &, const DinerLatentIndex &, const float *, const float *, const float *, int64_t, int, int,
                                  const float *, const float *, const float *, float *, float *, float *, float *, float *, float *, float *,
                                  hipStream_t);
int launch_gen_rays(const float *, const float *, const float *, const float *, int, int, int, float *, hipStream_t);
int launch_depth2normal(const float *, const float *, int, int, int, float *, hipStream_t);
int64_t gen_rays_bwd_workspace_floats(int, int, int);
int launch_gen_rays_bwd(const float *, const float *, const float *, int, int, int, float *, float *, float *, float *, float *, hipStream_t);
int launch_pack_maps_from_depth(const float *, const float *, const float *, int, int, int, float *, hipStream_t);
int launch_decode_depth(const unsigned short *, const unsigned short *, const unsigned short *, int64_t, int, int, int, float, float, float,
                        float, float, float *, float *, float *, hipStream_t);
int launch_linz_maps(const float *, int64_t, const float *, float *, hipStream_t);
int launch_linz_maps_ring(const float *, int64_t, int, int, const float *, float *, hipStream_t);
int launch_sampler(const DinerScene &, const float *, const DinerTargetCam *, float *, int64_t, const DinerSamplerCfg &, const float *,
                   const float *, const float *, const float *, uint64_t, float *, float *, float *, hipStream_t);
int launch_sampler_points(const DinerScene &, const float *, const float *, const float *, int64_t, const DinerSamplerCfg &, const float *,
                          const float *, uint64_t, float *, float *, float *, hipStream_t);
int launch_sample_coarse(const float *, int64_t, int, const float *, uint64_t, float *, hipStream_t);
int launch_fill_up(const float *, const float *, int64_t, int, const float *, uint64_t, float *, hipStream_t);
int launch_points_mlp(const DinerScene &, const DinerLatentIndex &, const float *, const float *, const float *, int64_t, int, float *, hipStream_t);
int64_t mlp_f16_packed_floats();
int launch_pack_mlp_f16(const DinerMlpRaw &, float *, hipStream_t);
int launch_points_mlp_f16(const DinerScene &, const DinerLatentIndex &, const float *, const float *, const float *, int64_t, int, float *, float *, hipStream_t);
int64_t points_mlp_f16_scratch_floats(int64_t SB, int NV);
namespace gen {
int check_shape(const DinerMlpShape &);
int64_t packed_floats(const DinerMlpShape &);
int launch_pack_mlp(const DinerMlpShape &, const DinerMlpGenRaw &, float *, hipStream_t);
int launch_points_mlp(const DinerScene &, const DinerLatentIndex &, const DinerMlpShape &, const float *, const float *, const float *, int64_t, int, float *, hipStream_t,
                      int bicubic_pad = -1);
int launch_points_mlp_lz(const DinerScene &, const DinerLatentIndex &, const DinerMlpShape &, const float *, const float *, const float *, int64_t, int, float *,
                         hipStream_t, int bicubic_pad, const float *lzmaps);
int64_t linz_maps_floats(const DinerMlpShape &, int64_t texels);
int launch_linz_maps(const DinerMlpShape &, const float *, int64_t, const float *, float *, hipStream_t);
int launch_points_mlp_novel(const DinerScene &, const DinerLatentIndex &, const DinerNovelGen &, const DinerMlpShape &, const float *, const float *,
                            const float *, const float *, int64_t, float *, hipStream_t);
int launch_points_mlp_novel_pe(const DinerScene &, const DinerLatentIndex &, const DinerNovelGen &, const DinerNovelPe &, const DinerMlpShape &,
                               const float *, const float *, const float *, const float *, const float *, int64_t, float *, hipStream_t);
int launch_novel_pe_map(const float *, int64_t, int, const float *, float *, hipStream_t);
}
namespace genf16 {
int64_t packed_floats(const DinerMlpShape &);
int launch_pack_mlp(const DinerMlpShape &, const DinerMlpGenRaw &, float *, hipStream_t);
int launch_points_mlp(const DinerScene &, const DinerLatentIndex &, const DinerMlpShape &, const float *, const float *, const float *, int64_t, int, float *, hipStream_t,
                      int bicubic_pad = -1);
int launch_points_mlp_lz(const DinerScene &, const DinerLatentIndex &, const DinerMlpShape &, const float *, const float *, const float *, int64_t, int, float *,
                         hipStream_t, int bicubic_pad, const float *lzmaps);
int launch_points_mlp_novel(const DinerScene &, const DinerLatentIndex &, const DinerNovelGen &, const DinerMlpShape &, const float *, const float *,
                            const float *, const float *, int64_t, float *, hipStream_t);
int launch_points_mlp_novel_pe(const DinerScene &, const DinerLatentIndex &, const DinerNovelGen &, const DinerNovelPe &, const DinerMlpShape &,
                               const float *, const float *, const float *, const float *, const float *, int64_t, float *, hipStream_t);
}

int launch_train_point_inputs_gen_bc(const DinerScene &, int, const float *, const float *, const float *, int64_t, int, int, float *, int64_t,
                                     float *, float *, hipStream_t);
int launch_train_point_inputs_bwd_gen_bc(const DinerScene &, int, const float *, const float *, const float *, int64_t, int, int, const float *,
                                         int64_t, const float *, const float *, float *, float *, float *, float *, float *, float *, float *,
                                         hipStream_t);
int launch_train_bicubic_scatter(const float *, const float *, int64_t, int, int, int, int, int, float *, hipStream_t);
int launch_train_point_inputs_novel(const DinerScene &, const DinerLatentIndex &, const float *, const DinerNovelGen &, const float *, const float *,
                                    const float *, int64_t, int, float *, int64_t, float *, float *, float *, hipStream_t);
int launch_train_novel_gen_scatter(const float *, const float *, int64_t, int, int, float *, hipStream_t);
int launch_train_gemm_act(const float *, const float *, const float *, const float *, float *, int64_t, int, int, int64_t, int64_t, int64_t,
                          int64_t, int64_t, int64_t, int, int, int, float, int, int, int64_t, hipStream_t);
int launch_train_point_inputs_gen(const DinerScene &, const DinerLatentIndex &, const float *, const float *, const float *, int64_t, int, int,
                                  float *, int64_t, float *, float *, hipStream_t);
int launch_train_point_inputs_bwd_gen(const DinerScene &, const DinerLatentIndex &, const float *, const float *, const float *, int64_t, int,
                                      int, const float *, int64_t, const float *, const float *, float *, float *, float *, float *, float *,
                                      float *, float *, hipStream_t);

static int bad(const char *msg)
{
    set_error("%s", msg);
    return DINER_E_INVALID;
}

static int check_scene(const DinerScene *s, bool need_latent)
{
    if (!s) return bad("scene is NULL");
    if (s->SB < 0 || s->NV <= 0 || s->H <= 0 || s->W <= 0) return bad("scene: bad SB/NV/H/W");
    if (!s->poses || !s->focal || !s->c || !s->maps) return bad("scene: NULL camera or map pointer");
    if (!(s->image_w > 0.f) || !(s->image_h > 0.f)) return bad("scene: bad image_shape");
    if (need_latent) {
        if (!s->latent) return bad("scene: latent is NULL");
        if (s->h <= 0 || s->w <= 0) return bad("scene: bad latent size");
    }
    return DINER_OK;
}

static const DinerLatentIndex k_default_index = {DINER_INDEX_BILINEAR, DINER_INDEX_PAD_BORDER};

// NULL = bilinear / border (the entry points without _ix)
static int check_index(const DinerLatentIndex *ix, const char *who)
{
    if (!ix) return DINER_OK;
    if (ix->interp != DINER_INDEX_BILINEAR && ix->interp != DINER_INDEX_NEAREST) {
        set_error("%s: latent index interp=%d unknown (DINER_INDEX_BILINEAR 0 or DINER_INDEX_NEAREST 1)", who, ix->interp);
        return DINER_E_INVALID;
    }
    if (ix->padding != DINER_INDEX_PAD_BORDER && ix->padding != DINER_INDEX_PAD_ZEROS && ix->padding != DINER_INDEX_PAD_REFLECTION) {
        set_error("%s: latent index padding=%d unknown (DINER_INDEX_PAD_BORDER 0, _ZEROS 1 or _REFLECTION 2)", who, ix->padding);
        return DINER_E_INVALID;
    }
    return DINER_OK;
}

// the padding argument of the bicubic (_bc) entry points
static int check_bicubic_padding(int32_t padding, const char *who)
{
    if (padding != DINER_INDEX_PAD_BORDER && padding != DINER_INDEX_PAD_ZEROS && padding != DINER_INDEX_PAD_REFLECTION) {
        set_error("%s: bicubic padding=%d unknown (DINER_INDEX_PAD_BORDER 0, _ZEROS 1 or _REFLECTION 2)", who, padding);
        return DINER_E_INVALID;
    }
    return DINER_OK;
}

static int check_cfg(const DinerSamplerCfg *c)
{
    if (!c) return bad("sampler cfg is NULL");
    if (c->n_candidates < 1) return bad("n_candidates must be >= 1");
    if (c->n_samples < 1 || c->n_samples > 8192) return bad("n_samples must be in [1, 8192]");
    if (c->n_gaussian < 0 || c->n_gaussian > c->n_samples) return bad("need 0 <= n_gaussian <= n_samples");  // nerf_renderer.py:89
    return DINER_OK;
}

}  // namespace diner

using namespace diner;

extern "C" {

const char *diner_last_error(void) { return g_err; }
int diner_version(void) { return DINER_ABI_VERSION; }

int diner_gen_rays(const float *extrinsics, const float *intrinsics, const float *z_near, const float *z_far, int32_t B,
                   int32_t H, int32_t W, float *rays_out, void *stream)
{
    if (B < 0 || H <= 0 || W <= 0) return bad("gen_rays: bad size");
    if (B > 0 && (!extrinsics || !intrinsics || !z_near || !z_far || !rays_out)) return bad("gen_rays: NULL pointer");
    return launch_gen_rays(extrinsics, intrinsics, z_near, z_far, B, H, W, rays_out, (hipStream_t)stream);
}

int64_t diner_gen_rays_backward_workspace_floats(int32_t B, int32_t H, int32_t W)
{
    if (B < 0 || H <= 0 || W <= 0) return -1;
    return gen_rays_bwd_workspace_floats(B, H, W);
}

int diner_gen_rays_backward(const float *extrinsics, const float *intrinsics, const float *d_rays, int32_t B, int32_t H, int32_t W,
                            float *d_extrinsics, float *d_intrinsics, float *d_near, float *d_far, float *workspace, void *stream)
{
    if (B < 0 || H <= 0 || W <= 0) return bad("gen_rays_backward: bad size");
    if (B == 0) return DINER_OK;
    if (!extrinsics || !intrinsics || !d_rays || !d_extrinsics || !d_intrinsics || !d_near || !d_far || !workspace)
        return bad("gen_rays_backward: NULL pointer");
    if ((uintptr_t)workspace % 8) return bad("gen_rays_backward: workspace not 8-byte aligned");
    return launch_gen_rays_bwd(extrinsics, intrinsics, d_rays, B, H, W, d_extrinsics, d_intrinsics, d_near, d_far, workspace,
                               (hipStream_t)stream);
}

int diner_depth2normal(const float *dmap, const float *intrinsics, int32_t N, int32_t H, int32_t W, float *normals_out,
                       void *stream)
{
    if (N < 0 || H <= 0 || W <= 0) return bad("depth2normal: bad size");
    if (N > 0 && (!dmap || !intrinsics || !normals_out)) return bad("depth2normal: NULL pointer");
    return launch_depth2normal(dmap, intrinsics, N, H, W, normals_out, (hipStream_t)stream);
}

int diner_pack_maps(const float *depths, const float *depths_std, const float *normals, int64_t N, int32_t H,
                    int32_t W, float *maps_out, void *stream)
{
    if (!depths || !depths_std || !normals || !maps_out) return bad("pack_maps: NULL pointer");
    if (N < 0 || H <= 0 || W <= 0) return bad("pack_maps: bad size");
    return launch_pack_maps(depths, depths_std, normals, N, H, W, maps_out, (hipStream_t)stream);
}

int diner_pack_maps_from_depth(const float *depths, const float *depths_std, const float *intrinsics, int64_t N, int32_t H,
                               int32_t W, float *maps_out, void *stream)
{
    if (!depths || !depths_std || !intrinsics || !maps_out) return bad("pack_maps_from_depth: NULL pointer");
    if (N < 0 || N > 0x7fffffff || H <= 0 || W <= 0) return bad("pack_maps_from_depth: bad size");
    return launch_pack_maps_from_depth(depths, depths_std, intrinsics, (int)N, H, W, maps_out, (hipStream_t)stream);
}

int diner_decode_depth_u16(const uint16_t *depth, const uint16_t *conf, const uint16_t *mesh, int64_t N, int32_t H, int32_t W, int32_t stride,
                           float mul0, float div, float mul1, float std_a, float std_b, float *depth_out, float *std_out, float *mask_out,
                           void *stream)
{
    if (!depth || !conf || !depth_out || !std_out) return bad("decode_depth_u16: NULL pointer");
    if (N < 0 || H <= 0 || W <= 0 || stride <= 0 || H % stride || W % stride) return bad("decode_depth_u16: bad size (stride must divide H and W)");
    if (!(div != 0.0f)) return bad("decode_depth_u16: div must be non-zero");
    return launch_decode_depth(depth, conf, mesh, N, H, W, stride, mul0, div, mul1, std_a, std_b, depth_out, std_out, mask_out,
                               (hipStream_t)stream);
}

int diner_pack_latent(const float *latent_nchw, int64_t N, int32_t C, int32_t h, int32_t w, float *latent_out,
                      void *stream)
{
    if (!latent_nchw || !latent_out) return bad("pack_latent: NULL pointer");
    if (N < 0 || h <= 0 || w <= 0) return bad("pack_latent: bad size");
    return launch_pack_latent(latent_nchw, N, C, h, w, latent_out, (hipStream_t)stream);
}

int64_t diner_mlp_packed_floats(void) { return mlp_packed_floats() + mlp_f16_packed_floats(); }

int diner_pack_mlp(const DinerMlpRaw *raw, float *packed_out, void *stream)
{
    if (!raw || !packed_out) return bad("pack_mlp: NULL pointer");
    const float *const *p = (const float *const *)raw;
    for (size_t i = 0; i < sizeof(DinerMlpRaw) / sizeof(float *); ++i)
        if (!p[i]) return bad("pack_mlp: NULL weight pointer");
    const int rc = launch_pack_mlp(*raw, packed_out, (hipStream_t)stream);
    if (rc) return rc;
    return launch_pack_mlp_f16(*raw, packed_out + mlp_packed_floats(), (hipStream_t)stream);
}

int diner_pack_linz_maps(const float *latent_packed, int64_t N, int32_t h, int32_t w, const float *mlp_packed, float *out,
                         void *stream)
{
    if (!latent_packed || !mlp_packed || !out) return bad("pack_linz_maps: NULL pointer");
    if (N < 0 || h <= 0 || w <= 0) return bad("pack_linz_maps: bad size");
    return launch_linz_maps(latent_packed, N * h * w, mlp_packed, out, (hipStream_t)stream);
}

int diner_sample_coarse(const float *rays, int64_t N, int32_t NC, const float *u_coarse, uint64_t seed, float *z_out,
                        void *stream)
{
    if (N < 0 || NC < 1) return bad("sample_coarse: bad N / NC");
    if (N > 0 && (!rays || !z_out)) return bad("sample_coarse: NULL pointer");
    return launch_sample_coarse(rays, N, NC, u_coarse, seed, z_out, (hipStream_t)stream);
}

int diner_fill_up_uniform_samples(const float *rays, const float *z_in, int64_t N, int32_t K, const float *u_fill,
                                  uint64_t seed, float *z_out, void *stream)
{
    if (N < 0 || K < 1 || K > 8192) return bad("fill_up: bad N / K");
    if (N > 0 && (!rays || !z_in || !z_out)) return bad("fill_up: NULL pointer");
    return launch_fill_up(rays, z_in, N, K, u_fill, seed, z_out, (hipStream_t)stream);
}

int diner_sample_depthguided(const DinerScene *scene, const float *rays, int64_t NR, const DinerSamplerCfg *cfg,
                             const float *u_coarse, const float *n_gauss, const float *u_fill, const float *z_cand,
                             uint64_t seed, float *z_out, float *z_dg_out, float *lik_out, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, false)) || (rc = check_cfg(cfg))) return rc;
    if (NR < 0) return bad("NR < 0");
    if (NR > 0 && scene->SB > 0 && (!rays || !z_out)) return bad("sample_depthguided: NULL rays / z_out");
    return launch_sampler(*scene, rays, nullptr, nullptr, NR, *cfg, u_coarse, n_gauss, u_fill, z_cand, seed, z_out, z_dg_out, lik_out,
                          (hipStream_t)stream);
}

int diner_sample_depthguided_points(const DinerScene *scene, const float *rays, const float *z_cand, const float *xyz_cand,
                                    int64_t NR, const DinerSamplerCfg *cfg, const float *n_gauss, const float *u_fill,
                                    uint64_t seed, float *z_out, float *z_dg_out, float *lik_out, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, false)) || (rc = check_cfg(cfg))) return rc;   // (check_cfg: K < G)
    if (NR < 0) return bad("NR < 0");
    if (cfg->n_candidates > 4096) {
        set_error("sample_depthguided_points: n_candidates=%d > 4096 unsupported", cfg->n_candidates);
        return DINER_E_UNSUPPORTED;
    }
    if (NR > 0 && scene->SB > 0) {
        if (!rays || !z_out) return bad("sample_depthguided_points: NULL rays / z_out");
        if (!z_cand || !xyz_cand) return bad("sample_depthguided_points: NULL z_cand / xyz_cand");
    }
    return launch_sampler_points(*scene, rays, z_cand, xyz_cand, NR, *cfg, n_gauss, u_fill, seed, z_out, z_dg_out, lik_out,
                                 (hipStream_t)stream);
}

int64_t diner_linz_maps_floats(int64_t N, int32_t h, int32_t w, const DinerLatentIndex *index)
{
    if (check_index(index, "linz_maps_floats")) return DINER_E_INVALID;
    if (N < 0 || h <= 0 || w <= 0) return bad("linz_maps_floats: bad size");
    const int r = (index && index->padding == DINER_INDEX_PAD_ZEROS) ? 1 : 0;
    return 3 * N * (int64_t)(h + 2 * r) * (w + 2 * r) * DINER_D_LATENT;
}

int diner_pack_linz_maps_ix(const float *latent_packed, int64_t N, int32_t h, int32_t w, const float *mlp_packed,
                            const DinerLatentIndex *index, float *out, void *stream)
{
    int rc;
    if ((rc = check_index(index, "pack_linz_maps_ix"))) return rc;
    if (!index || index->padding != DINER_INDEX_PAD_ZEROS) return diner_pack_linz_maps(latent_packed, N, h, w, mlp_packed, out, stream);
    if (!latent_packed || !mlp_packed || !out) return bad("pack_linz_maps_ix: NULL pointer");
    if (N < 0 || h <= 0 || w <= 0) return bad("pack_linz_maps_ix: bad size");
    return launch_linz_maps_ring(latent_packed, N, h, w, mlp_packed, out, (hipStream_t)stream);
}

int64_t diner_render_points_scratch_floats(int64_t SB, int32_t NV, int32_t precision)
{
    return precision == DINER_PRECISION_F16X3 ? points_mlp_f16_scratch_floats(SB, NV) : 0;
}

int diner_render_points(const DinerScene *scene, const float *mlp_packed, const float *rays, const float *z,
                        int64_t NR, int32_t K, int32_t precision, float *scratch, float *rgbsigma_out, void *stream)
{
    return diner_render_points_ix(scene, nullptr, mlp_packed, rays, z, NR, K, precision, scratch, rgbsigma_out, stream);
}

int diner_render_points_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *mlp_packed, const float *rays,
                           const float *z, int64_t NR, int32_t K, int32_t precision, float *scratch, float *rgbsigma_out, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, true)) || (rc = check_index(index, "render_points"))) return rc;
    const DinerLatentIndex &ix = index ? *index : k_default_index;
    if (NR < 0 || K < 1) return bad("render_points: bad NR / K");
    if (!mlp_packed) return bad("render_points: mlp_packed is NULL");
    if (NR > 0 && scene->SB > 0 && (!rays || !z || !rgbsigma_out)) return bad("render_points: NULL rays / z / out");
    if (precision == DINER_PRECISION_F16X3 && scene->linz_maps && ix.padding == DINER_INDEX_PAD_ZEROS && scene->SB > 0) {
        // zeros padding reads the RINGED lin_z maps ((h+2) x (w+2) texels per view, diner_pack_linz_maps_ix); DinerScene cannot say which
        // layout linz_maps holds, so refuse a buffer whose allocation ends before the ringed size (the plain maps of diner_pack_linz_maps)
        // instead of reading past it.  (A caller who sub-allocates can still hand plain maps in a larger block: wrong values, no fault.)
        const size_t need = (size_t)3 * scene->SB * scene->NV * (size_t)(scene->h + 2) * (size_t)(scene->w + 2) * DINER_D_LATENT * sizeof(float);
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)scene->linz_maps) == hipSuccess) {
            if ((const char *)scene->linz_maps + need > (const char *)base + size) {
                set_error("render_points(f16x3, zeros padding): linz_maps must be the ringed maps of diner_pack_linz_maps_ix "
                          "(%zu bytes), its allocation ends %zu bytes earlier", need,
                          (size_t)((const char *)scene->linz_maps + need - ((const char *)base + size)));
                return DINER_E_INVALID;
            }
        } else {
            (void)hipGetLastError();   // not a runtime allocation (e.g. virtual memory): nothing to check against
        }
    }
    if (precision == DINER_PRECISION_FP32) return launch_points_mlp(*scene, ix, mlp_packed, rays, z, NR, K, rgbsigma_out, (hipStream_t)stream);
    if (precision == DINER_PRECISION_F16X3)
        return launch_points_mlp_f16(*scene, ix, mlp_packed + mlp_packed_floats(), rays, z, NR, K, scratch, rgbsigma_out,
                                     (hipStream_t)stream);
    return bad("render_points: unknown precision");
}

int diner_composite(const float *rays, const float *z, const float *rgbsigma, int64_t N, int32_t K,
                    int32_t white_bkgd, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream)
{
    if (N < 0 || K < 1) return bad("composite: bad N / K");
    if (N > 0 && (!rays || !z || !rgbsigma || !rgb_out || !depth_out)) return bad("composite: NULL pointer");
    return launch_composite(rays, z, rgbsigma, N, K, white_bkgd, rgb_out, depth_out, weights_out, status, (hipStream_t)stream);
}

/* ---- training path building blocks (train.hip) ------------------------------------------------ */
int diner_train_gemm(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M, int32_t N, int32_t K,
                     int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc, int64_t lds, int32_t relu_a, int32_t relu_b,
                     int32_t accumulate, int32_t atomic, int64_t k_chunk, int32_t precision, const void *amax_a, const void *amax_b,
                     int32_t exp_a, int32_t exp_b, void *stream)
{
    if (!A || !B || !C) return bad("train_gemm: NULL pointer");
    if (precision != DINER_PRECISION_FP32 && precision != DINER_PRECISION_F16X3) return bad("train_gemm: unknown precision");
    if (M < 0 || N <= 0 || K <= 0 || (N & 3) || (k_chunk & 31)) return bad("train_gemm: bad size (N % 4, k_chunk % 32 must be 0)");
    if (exp_a < -60 || exp_a > 60 || exp_b < -60 || exp_b > 60) return bad("train_gemm: scale exponent out of range");
    // the tile loads read float4 pieces along an operand's contiguous index (a piece is valid when its first element is): what
    // diner_train_gemm_act refuses is refused here
    if (sak != 1 && sam != 1) return bad("train_gemm: A must be contiguous along m or k");
    if (sbn != 1 && sbk != 1) return bad("train_gemm: B must be contiguous along k or n");
    if ((sak == 1 ? (K & 3) || (sam & 3) : (M & 3) || (sak & 3)) || (sbn == 1 ? (sbk & 3) : (K & 3) || (sbn & 3)))
        return bad("train_gemm: the contiguous extent and the other stride of each operand must be multiples of 4");
    return launch_train_gemm(A, B, bias, S, C, M, N, K, sam, sak, sbk, sbn, ldc, lds, relu_a, relu_b, accumulate, atomic, k_chunk,
                             precision, (const unsigned int *)amax_a, (const unsigned int *)amax_b, exp_a, exp_b, (hipStream_t)stream);
}

int diner_train_amax(const float *x, int64_t n, void *amax_out, void *stream)
{
    if (!x || !amax_out || n < 0) return bad("train_amax: bad argument");
    return launch_train_amax(x, n, (unsigned int *)amax_out, (hipStream_t)stream);
}

int diner_train_colsum_amax(const float *dY, int64_t M, int32_t N, int64_t ld, float *db, void *amax_out, void *stream)
{
    if (!dY || M < 0 || N <= 0 || (N & 3) || 256 % (N / 4) || (ld & 3)) return bad("train_colsum_amax: bad argument (N % 4 == 0 and (N/4) | 256)");
    if (!db && !amax_out) return bad("train_colsum_amax: nothing to compute");
    return launch_train_colsum_amax(dY, M, N, ld, db, (unsigned int *)amax_out, (hipStream_t)stream);
}

int diner_train_split_panel(const float *W, int32_t K, int64_t ld, int32_t transpose, int32_t exp, void *hi, void *lo, void *stream)
{
    if (!W || !hi || !lo || K <= 0 || ld <= 0) return bad("train_split_panel: bad argument");
    if (exp < -60 || exp > 60) return bad("train_split_panel: scale exponent out of range");
    return launch_train_split_panel(W, K, ld, transpose, exp, hi, lo, (hipStream_t)stream);
}

int diner_train_gemm_panel(const float *A, int64_t sam, const void *Bhi, const void *Blo, const float *bias, const float *S, int64_t lds,
                           const float *addend, int64_t ldadd, float *C, int64_t ldc, int64_t M, int32_t K, int32_t relu_a,
                           const void *amax_a, int32_t exp_a, int32_t exp_b, void *stream)
{
    if (!A || !Bhi || !Blo || !C) return bad("train_gemm_panel: NULL pointer");
    if (M < 0 || K < 4 || (K & 3) || (sam & 3) || (ldc < DINER_D_HIDDEN)) return bad("train_gemm_panel: bad size (K % 4, sam % 4 must be 0)");
    if (((uintptr_t)A & 15) || ((uintptr_t)Bhi & 15) || ((uintptr_t)Blo & 15)) return bad("train_gemm_panel: operands must be 16-byte aligned");
    if (exp_a < -60 || exp_a > 60 || exp_b < -60 || exp_b > 60) return bad("train_gemm_panel: scale exponent out of range");
    return launch_train_gemm_panel(A, sam, Bhi, Blo, bias, S, lds, addend, ldadd, C, ldc, M, K, relu_a, (const unsigned int *)amax_a, exp_a,
                                   exp_b, (hipStream_t)stream);
}

int diner_train_pack_core(const float *W, int64_t ld, int32_t transpose, int32_t exp, void *out, void *stream)
{
    if (!W || !out) return bad("train_pack_core: NULL pointer");
    if (ld < DINER_D_HIDDEN || exp < -60 || exp > 60) return bad("train_pack_core: bad leading dimension / exponent");
    return launch_train_pack_core(W, ld, transpose, exp, out, (hipStream_t)stream);
}

int diner_train_gemm_core(const float *A, int64_t sam, const void *Wcore, const float *bias, const float *S, int64_t lds, const float *addend,
                          int64_t ldadd, float *C, int64_t ldc, int64_t M, int32_t relu_a, const void *amax_a, int32_t exp_a, int32_t exp_b,
                          float *colsum, void *amax_out, void *stream)
{
    if (!A || !Wcore || !C) return bad("train_gemm_core: NULL pointer");
    if (M < 0 || sam < DINER_D_HIDDEN || (sam & 3) || ldc < DINER_D_HIDDEN || (ldc & 3) || (S && (lds & 3)) || (addend && (ldadd & 3)))
        return bad("train_gemm_core: bad size (K = N = 512; leading dimensions % 4 must be 0)");
    if (((uintptr_t)A & 15) || ((uintptr_t)Wcore & 15) || ((uintptr_t)C & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)S & 15) || ((uintptr_t)addend & 15))
        return bad("train_gemm_core: operands must be 16-byte aligned");
    if (exp_a < -60 || exp_a > 60 || exp_b < -60 || exp_b > 60) return bad("train_gemm_core: scale exponent out of range");
    return launch_train_gemm_core(A, sam, Wcore, bias, S, lds, addend, ldadd, C, ldc, M, relu_a, (const unsigned int *)amax_a, exp_a, exp_b, colsum,
                                  (unsigned int *)amax_out, (hipStream_t)stream);
}

int diner_train_colsum(const float *dY, int64_t M, int32_t N, int64_t ld, float *db, void *stream)
{
    if (!dY || !db || M < 0 || N <= 0) return bad("train_colsum: bad argument");
    return launch_train_colsum(dY, M, N, ld, db, (hipStream_t)stream);
}

int diner_train_point_inputs(const DinerScene *scene, const float *latent, int32_t latent_is_nhwc, const float *rays, const float *z,
                             int64_t NR, int32_t K, int32_t sb, float *in56, float *zlat, float *taps, void *stream)
{
    return diner_train_point_inputs_ix(scene, nullptr, latent, latent_is_nhwc, rays, z, NR, K, sb, in56, zlat, taps, stream);
}

int diner_train_point_inputs_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *latent, int32_t latent_is_nhwc,
                                const float *rays, const float *z, int64_t NR, int32_t K, int32_t sb, float *in56, float *zlat,
                                float *taps, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, false)) || (rc = check_index(index, "train_point_inputs"))) return rc;
    if (!latent || !rays || !z || !in56 || !zlat || !taps) return bad("train_point_inputs: NULL pointer");
    if (scene->C != DINER_D_LATENT || scene->h <= 0 || scene->w <= 0 || sb < 0 || sb >= scene->SB) return bad("train_point_inputs: bad scene");
    return launch_train_point_inputs(*scene, index ? *index : k_default_index, latent, latent_is_nhwc, rays, z, NR, K, sb, in56, zlat, taps, (hipStream_t)stream);
}

int diner_train_bilinear_scatter(const float *dz, const float *taps, int64_t P, int32_t C, int32_t h, int32_t w, int32_t NV, int32_t sb,
                                 float *dlatent_nhwc, void *stream)
{
    if (!dz || !taps || !dlatent_nhwc) return bad("train_bilinear_scatter: NULL pointer");
    return launch_train_bilinear_scatter(dz, taps, P, C, h, w, NV, sb, dlatent_nhwc, (hipStream_t)stream);
}

int diner_train_nhwc_to_nchw(const float *nhwc, int64_t N, int32_t C, int32_t h, int32_t w, float *nchw_out, void *stream)
{
    if (!nhwc || !nchw_out || N < 0 || C <= 0 || h <= 0 || w <= 0) return bad("train_nhwc_to_nchw: bad argument");
    return launch_train_nhwc_to_nchw(nhwc, N, C, h, w, nchw_out, (hipStream_t)stream);
}

int diner_train_view_mean(const float *x, int64_t PC, int32_t NV, float *out, int32_t backward, void *stream)
{
    if (!x || !out || NV < 1) return bad("train_view_mean: bad argument");
    return launch_train_view_mean(x, PC, NV, out, backward, (hipStream_t)stream);
}

int diner_train_head(const float *out, const float *rgbsigma, const float *d_rgbsigma, int64_t n4, float *result, int32_t backward,
                     void *stream)
{
    if (!out || !result || (backward && (!rgbsigma || !d_rgbsigma))) return bad("train_head: NULL pointer");
    return launch_train_head(out, rgbsigma, d_rgbsigma, n4, result, backward, (hipStream_t)stream);
}

int diner_composite_backward(const float *rays, const float *z, const float *rgbsigma, const float *d_rgb, const float *d_depth,
                             const float *d_weights, int64_t N, int32_t K, int32_t white_bkgd, float *d_rgbsigma, void *stream)
{
    if (N < 0 || K < 1) return bad("composite_backward: bad N / K");
    if (N > 0 && (!rays || !z || !rgbsigma || !d_rgb || !d_rgbsigma)) return bad("composite_backward: NULL pointer");
    return launch_train_composite_bwd(rays, z, rgbsigma, d_rgb, d_depth, d_weights, N, K, white_bkgd, d_rgbsigma, (hipStream_t)stream);
}

int diner_composite_backward_far(const float *rays, const float *z, const float *rgbsigma, const float *d_rgb, const float *d_depth,
                                 const float *d_weights, int64_t N, int32_t K, int32_t white_bkgd, float *d_rgbsigma, float *d_far,
                                 void *stream)
{
    if (N < 0 || K < 1) return bad("composite_backward_far: bad N / K");
    if (N > 0 && (!rays || !z || !rgbsigma || !d_rgb || !d_rgbsigma || !d_far)) return bad("composite_backward_far: NULL pointer");
    return launch_train_composite_bwd_far(rays, z, rgbsigma, d_rgb, d_depth, d_weights, N, K, white_bkgd, d_rgbsigma, d_far,
                                          (hipStream_t)stream);
}

int64_t diner_train_camera_workspace_floats(int64_t NR, int32_t K, int32_t NV)
{
    if (NR < 0 || K < 1 || NV < 1) return -1;
    return train_camera_workspace_floats(NR, K, NV);
}

int diner_train_point_inputs_backward(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc, const float *rays,
                                      const float *z, int64_t NR, int32_t K, int32_t sb, const float *d_in56, const float *d_zlat,
                                      const float *d_far, float *workspace, float *d_rays, float *d_poses, float *d_focal, float *d_c,
                                      float *d_image_shape, float *d_depths, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, false)) || (rc = check_index(index, "train_point_inputs_backward"))) return rc;
    if (!latent_nhwc || !rays || !z || !d_in56 || !d_zlat || !workspace) return bad("train_point_inputs_backward: NULL pointer");
    if (scene->C != DINER_D_LATENT || scene->h <= 0 || scene->w <= 0) {
        set_error("train_point_inputs_backward: bad scene (latent C %d, h %d, w %d)", scene->C, scene->h, scene->w);
        return DINER_E_INVALID;
    }
    if (sb < 0 || sb >= scene->SB) {
        set_error("train_point_inputs_backward: sb %d outside [0, %d)", sb, scene->SB);
        return DINER_E_INVALID;
    }
    if (NR < 0 || K < 1) return bad("train_point_inputs_backward: bad NR / K");
    return launch_train_point_inputs_bwd(*scene, index ? *index : k_default_index, latent_nhwc, rays, z, NR, K, sb, d_in56, d_zlat, d_far,
                                         workspace, d_rays, d_poses, d_focal, d_c, d_image_shape, d_depths, (hipStream_t)stream);
}

/* ---- shape-general training path (train_gen.hip) ---------------------------------------------------------------------------- */
static bool act_known(int32_t a) { return a == DINER_ACT_NONE || a == DINER_ACT_RELU || a == DINER_ACT_SOFTPLUS; }

int diner_train_gemm_act(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M, int32_t N, int32_t K,
                         int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc, int64_t lds, int32_t act_a, int32_t act_b,
                         int32_t act_s, float beta, int32_t accumulate, int32_t atomic, int64_t k_chunk, void *stream)
{
    if (!A || !B || !C) return bad("train_gemm_act: NULL pointer");
    if (!act_known(act_a) || !act_known(act_b) || !act_known(act_s)) {
        set_error("train_gemm_act: unknown activation code (act_a %d, act_b %d, act_s %d; DINER_ACT_NONE 0, _RELU 1, _SOFTPLUS 2)", act_a,
                  act_b, act_s);
        return DINER_E_INVALID;
    }
    if ((act_a == DINER_ACT_SOFTPLUS || act_b == DINER_ACT_SOFTPLUS || act_s == DINER_ACT_SOFTPLUS) && !(beta > 0.0f && beta < __builtin_inff()))
        return bad("train_gemm_act: Softplus needs a finite beta > 0");
    if (M < 0 || N <= 0 || K <= 0 || (N & 3) || k_chunk < 0 || (k_chunk & 31)) return bad("train_gemm_act: bad size (N % 4, k_chunk % 32 must be 0)");
    if (sak != 1 && sam != 1) return bad("train_gemm_act: A must be contiguous along m or k");
    if (sbn != 1 && sbk != 1) return bad("train_gemm_act: B must be contiguous along k or n");
    if ((sak == 1 ? (K & 3) || (sam & 3) : (M & 3) || (sak & 3)) || (sbn == 1 ? (sbk & 3) : (K & 3) || (sbn & 3)))
        return bad("train_gemm_act: the contiguous extent and the other stride of each operand must be multiples of 4");
    return launch_train_gemm_act(A, B, bias, S, C, M, N, K, sam, sak, sbk, sbn, ldc, lds, act_a, act_b, act_s, beta, accumulate, atomic, k_chunk,
                                 (hipStream_t)stream);
}

// scene, lookup mode, F, C and ld_in of the two point-input entry points
static int check_train_gen_inputs(const DinerScene *scene, const DinerLatentIndex *index, int64_t NR, int32_t K, int32_t sb, int64_t ld_in,
                                  const char *who)
{
    int rc;
    if ((rc = check_scene(scene, false)) || (rc = check_index(index, who))) return rc;
    if (scene->num_freqs < 1 || scene->num_freqs > 63) {
        set_error("%s: num_freqs %d outside 1..63", who, scene->num_freqs);
        return DINER_E_UNSUPPORTED;
    }
    if (scene->C < 8 || scene->C > 1024 || scene->C % 8) {
        set_error("%s: latent width C %d unsupported (a multiple of 8 in [8, 1024])", who, scene->C);
        return DINER_E_UNSUPPORTED;
    }
    if (ld_in < 7 + 8 * (int64_t)scene->num_freqs || (ld_in & 3)) {
        set_error("%s: ld_in %lld must be >= 7 + 8 * num_freqs = %d and a multiple of 4", who, (long long)ld_in, 7 + 8 * scene->num_freqs);
        return DINER_E_INVALID;
    }
    if (scene->h <= 0 || scene->w <= 0) {
        set_error("%s: bad latent size (h %d, w %d)", who, scene->h, scene->w);
        return DINER_E_INVALID;
    }
    if (sb < 0 || sb >= scene->SB) {
        set_error("%s: sb %d outside [0, %d)", who, sb, scene->SB);
        return DINER_E_INVALID;
    }
    if (NR < 0 || K < 1) {
        set_error("%s: bad NR / K", who);
        return DINER_E_INVALID;
    }
    return DINER_OK;
}

int diner_train_point_inputs_gen(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc, const float *rays,
                                 const float *z, int64_t NR, int32_t K, int32_t sb, float *in_out, int64_t ld_in, float *zlat, float *taps,
                                 void *stream)
{
    int rc;
    if ((rc = check_train_gen_inputs(scene, index, NR, K, sb, ld_in, "train_point_inputs_gen"))) return rc;
    if (!latent_nhwc || !rays || !z || !in_out || !zlat || !taps) return bad("train_point_inputs_gen: NULL pointer");
    return launch_train_point_inputs_gen(*scene, index ? *index : k_default_index, latent_nhwc, rays, z, NR, K, sb, in_out, ld_in, zlat, taps,
                                         (hipStream_t)stream);
}

int diner_train_point_inputs_backward_gen(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc, const float *rays,
                                          const float *z, int64_t NR, int32_t K, int32_t sb, const float *d_in, int64_t ld_in,
                                          const float *d_zlat, const float *d_far, float *workspace, float *d_rays, float *d_poses,
                                          float *d_focal, float *d_c, float *d_image_shape, float *d_depths, void *stream)
{
    int rc;
    if ((rc = check_train_gen_inputs(scene, index, NR, K, sb, ld_in, "train_point_inputs_backward_gen"))) return rc;
    if (!latent_nhwc || !rays || !z || !d_in || !d_zlat || !workspace) return bad("train_point_inputs_backward_gen: NULL pointer");
    return launch_train_point_inputs_bwd_gen(*scene, index ? *index : k_default_index, latent_nhwc, rays, z, NR, K, sb, d_in, ld_in, d_zlat,
                                             d_far, workspace, d_rays, d_poses, d_focal, d_c, d_image_shape, d_depths, (hipStream_t)stream);
}

int64_t diner_render_workspace_floats(int64_t SB, int64_t NR, int32_t K, int32_t NV, int32_t precision)
{
    return SB * NR * (int64_t)K * 5 + diner_render_points_scratch_floats(SB, NV, precision);
}

int diner_render(const DinerScene *scene, const float *mlp_packed, const float *rays, int64_t NR,
                 const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, const float *u_coarse, const float *n_gauss,
                 const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                 float *weights_out, uint32_t *status, void *stream)
{
    return diner_render_ix(scene, nullptr, mlp_packed, rays, NR, cfg, white_bkgd, precision, u_coarse, n_gauss, u_fill, seed, workspace,
                           rgb_out, depth_out, weights_out, status, stream);
}

int diner_render_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *mlp_packed, const float *rays, int64_t NR,
                    const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, const float *u_coarse, const float *n_gauss,
                    const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                    float *weights_out, uint32_t *status, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, true)) || (rc = check_cfg(cfg)) || (rc = check_index(index, "render"))) return rc;
    if (NR < 0) return bad("NR < 0");
    if (NR == 0 || scene->SB == 0) return DINER_OK;
    if (!workspace) return bad("render: workspace is NULL");
    const int64_t N = (int64_t)scene->SB * NR;
    float *z = workspace, *rgbsigma = workspace + N * cfg->n_samples, *scratch = workspace + N * cfg->n_samples * 5;
    if ((rc = diner_sample_depthguided(scene, rays, NR, cfg, u_coarse, n_gauss, u_fill, nullptr, seed, z, nullptr,
                                       nullptr, stream)))
        return rc;
    if ((rc = diner_render_points_ix(scene, index, mlp_packed, rays, z, NR, cfg->n_samples, precision, scratch, rgbsigma, stream))) return rc;
    return diner_composite(rays, z, rgbsigma, N, cfg->n_samples, white_bkgd, rgb_out, depth_out, weights_out, status, stream);
}

int64_t diner_render_image_workspace_floats(int64_t SB, int32_t H, int32_t W, int32_t K, int32_t NV, int32_t precision)
{
    const int64_t NR = (int64_t)H * W;
    return SB * NR * 8 + diner_render_workspace_floats(SB, NR, K, NV, precision);
}

int diner_render_image(const DinerScene *scene, const float *mlp_packed, const DinerTargetCam *cam, const DinerSamplerCfg *cfg,
                       int32_t white_bkgd, int32_t precision, uint64_t seed, float *workspace, float *rays_out, float *rgb_out,
                       float *depth_out, float *weights_out, uint32_t *status, void *stream)
{
    return diner_render_image_ix(scene, nullptr, mlp_packed, cam, cfg, white_bkgd, precision, seed, workspace, rays_out, rgb_out, depth_out,
                                 weights_out, status, stream);
}

int diner_render_image_ix(const DinerScene *scene, const DinerLatentIndex *index, const float *mlp_packed, const DinerTargetCam *cam,
                          const DinerSamplerCfg *cfg, int32_t white_bkgd, int32_t precision, uint64_t seed, float *workspace,
                          float *rays_out, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream)
{
    int rc;
    if ((rc = check_scene(scene, true)) || (rc = check_cfg(cfg)) || (rc = check_index(index, "render_image"))) return rc;
    if (!cam || !cam->extrinsics || !cam->intrinsics || !cam->z_near || !cam->z_far) return bad("render_image: NULL camera");
    if (cam->H <= 0 || cam->W <= 0) return bad("render_image: bad image size");
    if (scene->SB == 0) return DINER_OK;
    if (!workspace) return bad("render_image: workspace is NULL");
    const int64_t NR = (int64_t)cam->H * cam->W, N = (int64_t)scene->SB * NR;
    float *rays = rays_out ? rays_out : workspace;                 // generated by the sampler, read by the two later stages
    float *z = workspace + N * 8, *rgbsigma = z + N * cfg->n_samples, *scratch = z + N * cfg->n_samples * 5;
    if ((rc = launch_sampler(*scene, nullptr, cam, rays, NR, *cfg, nullptr, nullptr, nullptr, nullptr, seed, z, nullptr, nullptr,
                             (hipStream_t)stream)))
        return rc;
    if ((rc = diner_render_points_ix(scene, index, mlp_packed, rays, z, NR, cfg->n_samples, precision, scratch, rgbsigma, stream))) return rc;
    return diner_composite(rays, z, rgbsigma, N, cfg->n_samples, white_bkgd, rgb_out, depth_out, weights_out, status, stream);
}

/* ---- shape-general inference path (points_mlp_gen.hip; the *_f16 entry points: points_mlp_gen_f16.hip) -------------------- */
static int check_gen_raw(const DinerMlpShape *shape, const DinerMlpGenRaw *raw, const char *who)
{
    const auto fail = [&](const char *what) { set_error("%s: %s", who, what); return (int)DINER_E_INVALID; };
    const int nlz = shape->combine_layer < shape->n_blocks ? shape->combine_layer : shape->n_blocks;
    if (!raw->lin_in_w || !raw->lin_in_b || !raw->lin_out_w || !raw->lin_out_b) return fail("NULL weight pointer");
    if ((nlz && (!raw->lin_z_w || !raw->lin_z_b)) || !raw->fc0_w || !raw->fc0_b || !raw->fc1_w || !raw->fc1_b) return fail("NULL layer array");
    for (int b = 0; b < nlz; ++b)
        if (!raw->lin_z_w[b] || !raw->lin_z_b[b]) return fail("NULL lin_z pointer");
    for (int b = 0; b < shape->n_blocks; ++b)
        if (!raw->fc0_w[b] || !raw->fc0_b[b] || !raw->fc1_w[b] || !raw->fc1_b[b]) return fail("NULL block pointer");
    return DINER_OK;
}

int64_t diner_mlp_gen_packed_floats(const DinerMlpShape *shape)
{
    if (!shape) return bad("mlp_gen_packed_floats: shape is NULL");
    const int rc = gen::check_shape(*shape);
    return rc ? rc : gen::packed_floats(*shape);
}

int diner_pack_mlp_gen(const DinerMlpShape *shape, const DinerMlpGenRaw *raw, float *packed_out, void *stream)
{
    if (!shape || !raw || !packed_out) return bad("pack_mlp_gen: NULL pointer");
    int rc;
    if ((rc = gen::check_shape(*shape)) || (rc = check_gen_raw(shape, raw, "pack_mlp_gen"))) return rc;
    return gen::launch_pack_mlp(*shape, *raw, packed_out, (hipStream_t)stream);
}

int64_t diner_mlp_gen_f16_packed_floats(const DinerMlpShape *shape)
{
    if (!shape) return bad("mlp_gen_f16_packed_floats: shape is NULL");
    const int rc = gen::check_shape(*shape);
    return rc ? rc : genf16::packed_floats(*shape);
}

int diner_pack_mlp_gen_f16(const DinerMlpShape *shape, const DinerMlpGenRaw *raw, float *packed_out, void *stream)
{
    if (!shape || !raw || !packed_out) return bad("pack_mlp_gen_f16: NULL pointer");
    if ((uintptr_t)packed_out % 16) return bad("pack_mlp_gen_f16: packed_out not 16-byte aligned");
    int rc;
    if ((rc = gen::check_shape(*shape)) || (rc = check_gen_raw(shape, raw, "pack_mlp_gen_f16"))) return rc;
    return genf16::launch_pack_mlp(*shape, *raw, packed_out, (hipStream_t)stream);
}

/* the three stages of a shape-general render, on the fp32 (f16 = false) or the f16x3 (f16 = true) point kernel */
/* bicubic_pad >= 0: the bicubic lookup with that padding (the _bc entry points; index is then NULL) */
static int render_points_gen(bool f16, const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,
                             const float *mlp_packed, const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out,
                             void *stream, int bicubic_pad = -1, const float *lz = nullptr)
{
    int rc;
    if (!shape) return bad("render_points_gen: shape is NULL");
    if ((rc = check_index(index, "render_points_gen"))) return rc;
    if ((rc = gen::check_shape(*shape))) return rc;
    if ((rc = check_scene(scene, shape->combine_layer > 0))) return rc;
    if (NR < 0 || K < 1) return bad("render_points_gen: bad NR / K");
    if (!mlp_packed) return bad("render_points_gen: mlp_packed is NULL");
    if (f16 && (uintptr_t)mlp_packed % 16) return bad("render_points_gen_f16: mlp_packed not 16-byte aligned");
    if (NR > 0 && scene->SB > 0 && (!rays || !z || !rgbsigma_out)) return bad("render_points_gen: NULL rays / z / out");
    if (lz)   /* the lin_z-map forms (the _lz entry points, nlz > 0) */
        return (f16 ? genf16::launch_points_mlp_lz : gen::launch_points_mlp_lz)(*scene, index ? *index : k_default_index, *shape, mlp_packed,
                                                                                 rays, z, NR, K, rgbsigma_out, (hipStream_t)stream,
                                                                                 bicubic_pad, lz);
    return (f16 ? genf16::launch_points_mlp : gen::launch_points_mlp)(*scene, index ? *index : k_default_index, *shape, mlp_packed, rays, z,
                                                                       NR, K, rgbsigma_out, (hipStream_t)stream, bicubic_pad);
}

static int render_gen(bool f16, const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                      const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,
                      const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                      float *weights_out, uint32_t *status, void *stream, int bicubic_pad = -1, const float *lz = nullptr)
{
    int rc;
    if (!shape) return bad("render_gen: shape is NULL");
    if ((rc = check_index(index, "render_gen"))) return rc;
    if ((rc = gen::check_shape(*shape)) || (rc = check_scene(scene, shape->combine_layer > 0)) || (rc = check_cfg(cfg))) return rc;
    if (NR < 0) return bad("NR < 0");
    if (NR == 0 || scene->SB == 0) return DINER_OK;
    if (!workspace) return bad("render_gen: workspace is NULL");
    const int64_t N = (int64_t)scene->SB * NR;
    float *z = workspace, *rgbsigma = workspace + N * cfg->n_samples;
    if ((rc = diner_sample_depthguided(scene, rays, NR, cfg, u_coarse, n_gauss, u_fill, nullptr, seed, z, nullptr, nullptr, stream))) return rc;
    if ((rc = render_points_gen(f16, scene, index, shape, mlp_packed, rays, z, NR, cfg->n_samples, rgbsigma, stream, bicubic_pad, lz))) return rc;
    return diner_composite(rays, z, rgbsigma, N, cfg->n_samples, white_bkgd, rgb_out, depth_out, weights_out, status, stream);
}

static int render_image_gen(bool f16, const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,
                            const float *mlp_packed, const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd,
                            uint64_t seed, float *workspace, float *rays_out, float *rgb_out, float *depth_out, float *weights_out,
                            uint32_t *status, void *stream, int bicubic_pad = -1, const float *lz = nullptr)
{
    int rc;
    if (!shape) return bad("render_image_gen: shape is NULL");
    if ((rc = check_index(index, "render_image_gen"))) return rc;
    if ((rc = gen::check_shape(*shape)) || (rc = check_scene(scene, shape->combine_layer > 0)) || (rc = check_cfg(cfg))) return rc;
    if (!cam || !cam->extrinsics || !cam->intrinsics || !cam->z_near || !cam->z_far) return bad("render_image_gen: NULL camera");
    if (cam->H <= 0 || cam->W <= 0) return bad("render_image_gen: bad image size");
    if (scene->SB == 0) return DINER_OK;
    if (!workspace) return bad("render_image_gen: workspace is NULL");
    const int64_t NR = (int64_t)cam->H * cam->W, N = (int64_t)scene->SB * NR;
    float *rays = rays_out ? rays_out : workspace;
    float *z = workspace + N * 8, *rgbsigma = z + N * cfg->n_samples;
    if ((rc = launch_sampler(*scene, nullptr, cam, rays, NR, *cfg, nullptr, nullptr, nullptr, nullptr, seed, z, nullptr, nullptr,
                             (hipStream_t)stream)))
        return rc;
    if ((rc = render_points_gen(f16, scene, index, shape, mlp_packed, rays, z, NR, cfg->n_samples, rgbsigma, stream, bicubic_pad, lz))) return rc;
    return diner_composite(rays, z, rgbsigma, N, cfg->n_samples, white_bkgd, rgb_out, depth_out, weights_out, status, stream);
}

#define DEFINE_GEN_ENTRY_POINTS(SUFFIX, F16)                                                                                                  \
    int diner_render_points_gen##SUFFIX(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const float *rays,     \
                                        const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream)                            \
    {                                                                                                                                        \
        return render_points_gen(F16, scene, nullptr, shape, mlp_packed, rays, z, NR, K, rgbsigma_out, stream);                              \
    }                                                                                                                                        \
    int diner_render_points_gen##SUFFIX##_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,             \
                                             const float *mlp_packed, const float *rays, const float *z, int64_t NR, int32_t K,              \
                                             float *rgbsigma_out, void *stream)                                                              \
    {                                                                                                                                        \
        return render_points_gen(F16, scene, index, shape, mlp_packed, rays, z, NR, K, rgbsigma_out, stream);                                \
    }                                                                                                                                        \
    int diner_render_gen##SUFFIX(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, const float *rays,            \
                                 int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse, const float *n_gauss,    \
                                 const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,                     \
                                 float *weights_out, uint32_t *status, void *stream)                                                         \
    {                                                                                                                                        \
        return render_gen(F16, scene, nullptr, shape, mlp_packed, rays, NR, cfg, white_bkgd, u_coarse, n_gauss, u_fill, seed, workspace,     \
                          rgb_out, depth_out, weights_out, status, stream);                                                                  \
    }                                                                                                                                        \
    int diner_render_gen##SUFFIX##_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,                    \
                                      const float *mlp_packed, const float *rays, int64_t NR, const DinerSamplerCfg *cfg,                    \
                                      int32_t white_bkgd, const float *u_coarse, const float *n_gauss, const float *u_fill, uint64_t seed,   \
                                      float *workspace, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status,              \
                                      void *stream)                                                                                          \
    {                                                                                                                                        \
        return render_gen(F16, scene, index, shape, mlp_packed, rays, NR, cfg, white_bkgd, u_coarse, n_gauss, u_fill, seed, workspace,       \
                          rgb_out, depth_out, weights_out, status, stream);                                                                  \
    }                                                                                                                                        \
    int diner_render_image_gen##SUFFIX(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed,                         \
                                       const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed,             \
                                       float *workspace, float *rays_out, float *rgb_out, float *depth_out, float *weights_out,              \
                                       uint32_t *status, void *stream)                                                                       \
    {                                                                                                                                        \
        return render_image_gen(F16, scene, nullptr, shape, mlp_packed, cam, cfg, white_bkgd, seed, workspace, rays_out, rgb_out,            \
                                depth_out, weights_out, status, stream);                                                                     \
    }                                                                                                                                        \
    int diner_render_image_gen##SUFFIX##_ix(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape,              \
                                            const float *mlp_packed, const DinerTargetCam *cam, const DinerSamplerCfg *cfg,                  \
                                            int32_t white_bkgd, uint64_t seed, float *workspace, float *rays_out, float *rgb_out,            \
                                            float *depth_out, float *weights_out, uint32_t *status, void *stream)                            \
    {                                                                                                                                        \
        return render_image_gen(F16, scene, index, shape, mlp_packed, cam, cfg, white_bkgd, seed, workspace, rays_out, rgb_out, depth_out,   \
                                weights_out, status, stream);                                                                                \
    }

DEFINE_GEN_ENTRY_POINTS(, false)
DEFINE_GEN_ENTRY_POINTS(_f16, true)
#undef DEFINE_GEN_ENTRY_POINTS

/* ---- the bicubic latent lookup (points_mlp_gen_bc.hip, points_mlp_gen_f16_bc.hip, train_gen_bc.hip) ------------------------------ */
#define DEFINE_GEN_BC_ENTRY_POINTS(SUFFIX, F16)                                                                                               \
    int diner_render_points_gen##SUFFIX##_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,  \
                                             const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream)    \
    {                                                                                                                                        \
        if (check_bicubic_padding(padding, "render_points_gen" #SUFFIX "_bc")) return DINER_E_INVALID;                                       \
        return render_points_gen(F16, scene, nullptr, shape, mlp_packed, rays, z, NR, K, rgbsigma_out, stream, padding);                     \
    }                                                                                                                                        \
    int diner_render_gen##SUFFIX##_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,         \
                                      const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,  \
                                      const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out,            \
                                      float *depth_out, float *weights_out, uint32_t *status, void *stream)                                  \
    {                                                                                                                                        \
        if (check_bicubic_padding(padding, "render_gen" #SUFFIX "_bc")) return DINER_E_INVALID;                                              \
        return render_gen(F16, scene, nullptr, shape, mlp_packed, rays, NR, cfg, white_bkgd, u_coarse, n_gauss, u_fill, seed, workspace,     \
                          rgb_out, depth_out, weights_out, status, stream, padding);                                                         \
    }                                                                                                                                        \
    int diner_render_image_gen##SUFFIX##_bc(const DinerScene *scene, int32_t padding, const DinerMlpShape *shape, const float *mlp_packed,   \
                                            const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed,        \
                                            float *workspace, float *rays_out, float *rgb_out, float *depth_out, float *weights_out,         \
                                            uint32_t *status, void *stream)                                                                  \
    {                                                                                                                                        \
        if (check_bicubic_padding(padding, "render_image_gen" #SUFFIX "_bc")) return DINER_E_INVALID;                                        \
        return render_image_gen(F16, scene, nullptr, shape, mlp_packed, cam, cfg, white_bkgd, seed, workspace, rays_out, rgb_out, depth_out, \
                                weights_out, status, stream, padding);                                                                       \
    }

DEFINE_GEN_BC_ENTRY_POINTS(, false)
DEFINE_GEN_BC_ENTRY_POINTS(_f16, true)
#undef DEFINE_GEN_BC_ENTRY_POINTS

/* ---- lin_z hoisted into per-texel maps (linz_maps_gen.hip, points_mlp_gen_lz.hip, points_mlp_gen_f16_lz.hip and their _bc twins) -- */
int64_t diner_linz_maps_gen_floats(const DinerScene *scene, const DinerMlpShape *shape)
{
    if (!scene || !shape) return bad("linz_maps_gen_floats: NULL pointer");
    const int rc = gen::check_shape(*shape);
    if (rc) return rc;
    if (scene->SB < 0 || scene->NV <= 0 || scene->h <= 0 || scene->w <= 0) return bad("linz_maps_gen_floats: bad SB / NV / h / w");
    return gen::linz_maps_floats(*shape, (int64_t)scene->SB * scene->NV * scene->h * scene->w);
}

int diner_pack_linz_maps_gen(const DinerScene *scene, const DinerMlpShape *shape, const float *mlp_packed, float *maps_out, void *stream)
{
    if (!scene || !shape || !mlp_packed || !maps_out) return bad("pack_linz_maps_gen: NULL pointer");
    const int rc = gen::check_shape(*shape);
    if (rc) return rc;
    if (scene->SB < 0 || scene->NV <= 0 || scene->h <= 0 || scene->w <= 0) return bad("pack_linz_maps_gen: bad SB / NV / h / w");
    if (!scene->latent) return bad("pack_linz_maps_gen: scene latent is NULL");
    if (scene->C != shape->d_latent) {
        set_error("pack_linz_maps_gen: latent channels C=%d != d_latent=%d", scene->C, shape->d_latent);
        return DINER_E_INVALID;
    }
    return gen::launch_linz_maps(*shape, scene->latent, (int64_t)scene->SB * scene->NV * scene->h * scene->w, mlp_packed, maps_out,
                                 (hipStream_t)stream);
}

/* precision, bicubic_padding and the maps of the _lz entry points -> f16, the maps to hand on (NULL when nlz = 0: the parent's route) */
static int check_lz(const DinerMlpShape *shape, int32_t precision, int32_t bicubic_padding, const float *maps, const char *who, bool &f16,
                    const float *&lz)
{
    if (precision != DINER_PRECISION_FP32 && precision != DINER_PRECISION_F16X3) {
        set_error("%s: precision=%d unknown (DINER_PRECISION_FP32 0 or DINER_PRECISION_F16X3 1)", who, precision);
        return DINER_E_INVALID;
    }
    if (bicubic_padding != -1 && check_bicubic_padding(bicubic_padding, who)) return DINER_E_INVALID;
    if (!shape) { set_error("%s: shape is NULL", who); return DINER_E_INVALID; }
    const int rc = gen::check_shape(*shape);
    if (rc) return rc;
    const bool has_lz = shape->combine_layer > 0;   /* nlz = min(combine_layer, n_blocks) > 0 */
    if (has_lz && !maps) { set_error("%s: linz_maps_gen is NULL (the shape has lin_z layers: diner_pack_linz_maps_gen)", who); return DINER_E_INVALID; }
    f16 = precision == DINER_PRECISION_F16X3;
    lz = has_lz ? maps : nullptr;
    return DINER_OK;
}

int diner_render_points_gen_lz(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                               const float *rays, const float *z, int64_t NR, int32_t K, float *rgbsigma_out, void *stream,
                               int32_t precision, int32_t bicubic_padding, const float *linz_maps_gen)
{
    bool f16;
    const float *lz;
    int rc;
    if ((rc = check_lz(shape, precision, bicubic_padding, linz_maps_gen, "render_points_gen_lz", f16, lz))) return rc;
    return render_points_gen(f16, scene, bicubic_padding >= 0 ? nullptr : index, shape, mlp_packed, rays, z, NR, K, rgbsigma_out, stream,
                             bicubic_padding, lz);
}

int diner_render_gen_lz(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                        const float *rays, int64_t NR, const DinerSamplerCfg *cfg, int32_t white_bkgd, const float *u_coarse,
                        const float *n_gauss, const float *u_fill, uint64_t seed, float *workspace, float *rgb_out, float *depth_out,
                        float *weights_out, uint32_t *status, void *stream, int32_t precision, int32_t bicubic_padding,
                        const float *linz_maps_gen)
{
    bool f16;
    const float *lz;
    int rc;
    if ((rc = check_lz(shape, precision, bicubic_padding, linz_maps_gen, "render_gen_lz", f16, lz))) return rc;
    return render_gen(f16, scene, bicubic_padding >= 0 ? nullptr : index, shape, mlp_packed, rays, NR, cfg, white_bkgd, u_coarse, n_gauss,
                      u_fill, seed, workspace, rgb_out, depth_out, weights_out, status, stream, bicubic_padding, lz);
}

int diner_render_image_gen_lz(const DinerScene *scene, const DinerLatentIndex *index, const DinerMlpShape *shape, const float *mlp_packed,
                              const DinerTargetCam *cam, const DinerSamplerCfg *cfg, int32_t white_bkgd, uint64_t seed, float *workspace,
                              float *rays_out, float *rgb_out, float *depth_out, float *weights_out, uint32_t *status, void *stream,
                              int32_t precision, int32_t bicubic_padding, const float *linz_maps_gen)
{
    bool f16;
    const float *lz;
    int rc;
    if ((rc = check_lz(shape, precision, bicubic_padding, linz_maps_gen, "render_image_gen_lz", f16, lz))) return rc;
    return render_image_gen(f16, scene, bicubic_padding >= 0 ? nullptr : index, shape, mlp_packed, cam, cfg, white_bkgd, seed, workspace,
                            rays_out, rgb_out, depth_out, weights_out, status, stream, bicubic_padding, lz);
}

int diner_train_point_inputs_gen_bc(const DinerScene *scene, int32_t padding, const float *latent_nhwc, const float *rays, const float *z,
                                    int64_t NR, int32_t K, int32_t sb, float *in_out, int64_t ld_in, float *zlat, float *taps, void *stream)
{
    int rc;
    if ((rc = check_bicubic_padding(padding, "train_point_inputs_gen_bc"))) return rc;
    if ((rc = check_train_gen_inputs(scene, nullptr, NR, K, sb, ld_in, "train_point_inputs_gen_bc"))) return rc;
    if (!latent_nhwc || !rays || !z || !in_out || !zlat || !taps) return bad("train_point_inputs_gen_bc: NULL pointer");
    return launch_train_point_inputs_gen_bc(*scene, padding, latent_nhwc, rays, z, NR, K, sb, in_out, ld_in, zlat, taps, (hipStream_t)stream);
}

int diner_train_point_inputs_backward_gen_bc(const DinerScene *scene, int32_t padding, const float *latent_nhwc, const float *rays,
                                             const float *z, int64_t NR, int32_t K, int32_t sb, const float *d_in, int64_t ld_in,
                                             const float *d_zlat, const float *d_far, float *workspace, float *d_rays, float *d_poses,
                                             float *d_focal, float *d_c, float *d_image_shape, float *d_depths, void *stream)
{
    int rc;
    if ((rc = check_bicubic_padding(padding, "train_point_inputs_backward_gen_bc"))) return rc;
    if ((rc = check_train_gen_inputs(scene, nullptr, NR, K, sb, ld_in, "train_point_inputs_backward_gen_bc"))) return rc;
    if (!latent_nhwc || !rays || !z || !d_in || !d_zlat || !workspace) return bad("train_point_inputs_backward_gen_bc: NULL pointer");
    return launch_train_point_inputs_bwd_gen_bc(*scene, padding, latent_nhwc, rays, z, NR, K, sb, d_in, ld_in, d_zlat, d_far, workspace, d_rays,
                                                d_poses, d_focal, d_c, d_image_shape, d_depths, (hipStream_t)stream);
}

int diner_train_bicubic_scatter(const float *dz, const float *taps, int64_t P, int32_t C, int32_t h, int32_t w, int32_t NV, int32_t sb,
                                float *dlatent_nhwc, void *stream)
{
    if (!dz || !taps || !dlatent_nhwc) return bad("train_bicubic_scatter: NULL pointer");
    if (P < 0 || C <= 0 || h <= 0 || w <= 0 || NV < 1 || sb < 0) return bad("train_bicubic_scatter: bad size");
    return launch_train_bicubic_scatter(dz, taps, P, C, h, w, NV, sb, dlatent_nhwc, (hipStream_t)stream);
}

/* ---- the NOVEL point model on the shape-general kernels (points_mlp_gen_nv.hip, points_mlp_gen_f16_nv.hip) ------------------------- */
int diner_render_points_novel(const DinerScene *scene, const DinerLatentIndex *index, const DinerNovelGen *gen, const DinerMlpShape *shape,
                              const float *mlp_packed, const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P,
                              int32_t precision, float *rgbsigma_out, void *stream)
{
    const char *who = "render_points_novel";
    int rc;
    if (!shape) return bad("render_points_novel: shape is NULL");
    if (!gen) return bad("render_points_novel: gen is NULL");
    if (precision != DINER_PRECISION_FP32 && precision != DINER_PRECISION_F16X3) {
        set_error("%s: precision=%d unknown (DINER_PRECISION_FP32 0 or DINER_PRECISION_F16X3 1)", who, precision);
        return DINER_E_INVALID;
    }
    const bool f16 = precision == DINER_PRECISION_F16X3;
    if ((rc = check_index(index, who))) return rc;   /* the 4-tap modes only: DinerLatentIndex does not carry bicubic */
    if ((rc = gen::check_shape(*shape))) return rc;
    const bool has_lz = shape->combine_layer > 0;    /* else neither latent is read */
    if ((rc = check_scene(scene, has_lz))) return rc;
    if (shape->combine_layer >= shape->n_blocks && scene->NV != 1) {
        set_error("%s: combine_layer=%d >= n_blocks=%d never averages over views, which the reference supports for NV = 1 only "
                  "(src/models/novel/novel_pixelnerf.py:234 reshapes (SB, NV, B, 4) to (SB, B, 4)); NV=%d", who, shape->combine_layer,
                  shape->n_blocks, scene->NV);
        return DINER_E_UNSUPPORTED;
    }
    if (scene->C != shape->d_latent) { set_error("%s: latent channels C=%d != d_latent=%d", who, scene->C, shape->d_latent); return DINER_E_INVALID; }
    if (gen->C != shape->d_latent) { set_error("%s: general latent channels C=%d != d_latent=%d", who, gen->C, shape->d_latent); return DINER_E_INVALID; }
    if (scene->num_freqs != shape->num_freqs) {
        set_error("%s: scene num_freqs=%d != shape num_freqs=%d", who, scene->num_freqs, shape->num_freqs);
        return DINER_E_INVALID;
    }
    if (gen->h < 1 || gen->w < 1) { set_error("%s: general latent size h=%d, w=%d (both >= 1)", who, gen->h, gen->w); return DINER_E_INVALID; }
    if ((int64_t)gen->h * gen->w * (gen->C / 4) > 0x7fffffffLL || (int64_t)scene->h * scene->w * (scene->C / 4) > 0x7fffffffLL)
        return bad("render_points_novel: a latent map of 2^31 or more float4 (the tap offsets are 32-bit)");
    if (has_lz && !gen->latent) return bad("render_points_novel: general latent is NULL");
    if (!gen->poses || !gen->focal || !gen->c) return bad("render_points_novel: NULL general camera pointer");
    if (!(gen->image_w > 0.f) || !(gen->image_h > 0.f)) return bad("render_points_novel: bad general image shape");
    if (P < 0) return bad("render_points_novel: bad P");
    if ((P + 63) / 64 > 0x7fffffffLL) { set_error("%s: too many points (%lld)", who, (long long)P); return DINER_E_INVALID; }
    if (!mlp_packed) return bad("render_points_novel: mlp_packed is NULL");
    if (f16 && (uintptr_t)mlp_packed % 16) return bad("render_points_novel: mlp_packed not 16-byte aligned (f16x3)");
    if (has_lz && ((uintptr_t)gen->latent % 16 || (uintptr_t)scene->latent % 16)) return bad("render_points_novel: latent not 16-byte aligned");
    if (P == 0 || scene->SB == 0) return DINER_OK;
    if (!xyz_in || !xyz_gen || !viewdirs || !rgbsigma_out) return bad("render_points_novel: NULL points / viewdirs / out");
    return (f16 ? genf16::launch_points_mlp_novel : gen::launch_points_mlp_novel)(*scene, index ? *index : k_default_index, *gen, *shape,
                                                                                 mlp_packed, xyz_in, xyz_gen, viewdirs, P, rgbsigma_out,
                                                                                 (hipStream_t)stream);
}

/* ---- the NOVEL_PE point model (points_mlp_gen_nvpe.hip, points_mlp_gen_f16_nvpe.hip; the deformation map: novel_pe_map.hip) --------- */
static int check_novel_pe_map_scene(const DinerScene *scene, const char *who)
{
    if (!scene) { set_error("%s: scene is NULL", who); return DINER_E_INVALID; }
    if (scene->SB < 0 || scene->NV <= 0 || scene->h <= 0 || scene->w <= 0) { set_error("%s: bad SB / NV / h / w", who); return DINER_E_INVALID; }
    if (scene->C < 8 || scene->C % 8) { set_error("%s: latent channels C=%d (a multiple of 8, >= 8)", who, scene->C); return DINER_E_INVALID; }
    if (scene->C + 8 > 1024) {
        set_error("%s: latent channels C=%d unsupported (the fusion MLP's padded d_latent = C + 8 must not exceed 1024)", who, scene->C);
        return DINER_E_UNSUPPORTED;
    }
    return DINER_OK;
}

int64_t diner_novel_pe_map_floats(const DinerScene *scene)
{
    const int rc = check_novel_pe_map_scene(scene, "novel_pe_map_floats");
    if (rc) return rc;
    return (int64_t)scene->SB * scene->NV * scene->h * scene->w * scene->C;
}

int diner_pack_novel_pe_map(const DinerScene *scene, const float *w_latent_part, float *map_out, void *stream)
{
    const int rc = check_novel_pe_map_scene(scene, "pack_novel_pe_map");
    if (rc) return rc;
    if (!w_latent_part || !map_out) return bad("pack_novel_pe_map: NULL pointer");
    if (!scene->latent) return bad("pack_novel_pe_map: scene latent is NULL");
    if ((uintptr_t)scene->latent % 16) return bad("pack_novel_pe_map: latent not 16-byte aligned");
    return gen::launch_novel_pe_map(scene->latent, (int64_t)scene->SB * scene->NV * scene->h * scene->w, scene->C, w_latent_part, map_out,
                                    (hipStream_t)stream);
}

int diner_render_points_novel_pe(const DinerScene *scene, const DinerLatentIndex *index, const DinerNovelGen *gen, const DinerNovelPe *pe,
                                 const DinerMlpShape *shape, const float *mlp_packed, const float *xyz_in, const float *xyz_gen,
                                 const float *xyz_tgt, const float *viewdirs, int64_t P, int32_t precision, float *rgbsigma_out,
                                 void *stream)
{
    const char *who = "render_points_novel_pe";
    int rc;
    if (!shape) return bad("render_points_novel_pe: shape is NULL");
    if (!gen) return bad("render_points_novel_pe: gen is NULL");
    if (!pe) return bad("render_points_novel_pe: pe is NULL");
    if (precision != DINER_PRECISION_FP32 && precision != DINER_PRECISION_F16X3) {
        set_error("%s: precision=%d unknown (DINER_PRECISION_FP32 0 or DINER_PRECISION_F16X3 1)", who, precision);
        return DINER_E_INVALID;
    }
    const bool f16 = precision == DINER_PRECISION_F16X3;
    if ((rc = check_index(index, who))) return rc;   /* the 4-tap modes only: DinerLatentIndex does not carry bicubic */
    if ((rc = gen::check_shape(*shape))) return rc;  /* d_latent = C + 8 <= 1024 */
    const bool has_lz = shape->combine_layer > 0;    /* else no latent, map or pos-encoding is read */
    if ((rc = check_scene(scene, false))) return rc;
    if (shape->combine_layer >= shape->n_blocks && scene->NV != 1) {
        set_error("%s: combine_layer=%d >= n_blocks=%d never averages over views, which the reference supports for NV = 1 only "
                  "(src/models/novel_pe/pe_novel_pixelnerf.py:284 reshapes (SB, NV, B, 4) to (SB, B, 4)); NV=%d", who, shape->combine_layer,
                  shape->n_blocks, scene->NV);
        return DINER_E_UNSUPPORTED;
    }
    if (scene->C != shape->d_latent - 8) {
        set_error("%s: latent channels C=%d != d_latent - 8 = %d (the MLP's latent input is C + 6 columns, padded to C + 8)", who, scene->C,
                  shape->d_latent - 8);
        return DINER_E_INVALID;
    }
    if (gen->C != shape->d_latent - 8) {
        set_error("%s: general latent channels C=%d != d_latent - 8 = %d", who, gen->C, shape->d_latent - 8);
        return DINER_E_INVALID;
    }
    if (scene->num_freqs != shape->num_freqs) {
        set_error("%s: scene num_freqs=%d != shape num_freqs=%d", who, scene->num_freqs, shape->num_freqs);
        return DINER_E_INVALID;
    }
    if (scene->h < 1 || scene->w < 1) { set_error("%s: deformation map size h=%d, w=%d (both >= 1)", who, scene->h, scene->w); return DINER_E_INVALID; }
    if (gen->h < 1 || gen->w < 1) { set_error("%s: general latent size h=%d, w=%d (both >= 1)", who, gen->h, gen->w); return DINER_E_INVALID; }
    if (pe->src_h < 1 || pe->src_w < 1) { set_error("%s: source pos-encoding size h=%d, w=%d (both >= 1)", who, pe->src_h, pe->src_w); return DINER_E_INVALID; }
    if (pe->tgt_h < 1 || pe->tgt_w < 1) { set_error("%s: target pos-encoding size h=%d, w=%d (both >= 1)", who, pe->tgt_h, pe->tgt_w); return DINER_E_INVALID; }
    if (scene->C < 8) { set_error("%s: d_latent=%d leaves no latent channel (C = d_latent - 8 >= 8)", who, shape->d_latent); return DINER_E_UNSUPPORTED; }
    if ((int64_t)gen->h * gen->w * (gen->C / 4) > 0x7fffffffLL || (int64_t)scene->h * scene->w * (scene->C / 4) > 0x7fffffffLL)
        return bad("render_points_novel_pe: a latent map of 2^31 or more float4 (the tap offsets are 32-bit)");
    if ((int64_t)pe->src_h * pe->src_w > 0x7fffffffLL || (int64_t)pe->tgt_h * pe->tgt_w > 0x7fffffffLL)
        return bad("render_points_novel_pe: a pos-encoding map of 2^31 or more texels (the tap offsets are 32-bit)");
    if (has_lz && !gen->latent) return bad("render_points_novel_pe: general latent is NULL");
    if (has_lz && (!pe->map || !pe->head || !pe->src_pe || !pe->tgt_pe)) return bad("render_points_novel_pe: NULL map / head / pos-encoding pointer");
    if (!gen->poses || !gen->focal || !gen->c) return bad("render_points_novel_pe: NULL general camera pointer");
    if (!pe->poses || !pe->focal || !pe->c) return bad("render_points_novel_pe: NULL target camera pointer");
    if (!(gen->image_w > 0.f) || !(gen->image_h > 0.f)) return bad("render_points_novel_pe: bad general image shape");
    if (!(pe->image_w > 0.f) || !(pe->image_h > 0.f)) return bad("render_points_novel_pe: bad target image shape");
    if (P < 0) return bad("render_points_novel_pe: bad P");
    if ((P + 63) / 64 > 0x7fffffffLL) { set_error("%s: too many points (%lld)", who, (long long)P); return DINER_E_INVALID; }
    if (!mlp_packed) return bad("render_points_novel_pe: mlp_packed is NULL");
    if (f16 && (uintptr_t)mlp_packed % 16) return bad("render_points_novel_pe: mlp_packed not 16-byte aligned (f16x3)");
    if (has_lz && ((uintptr_t)gen->latent % 16 || (uintptr_t)pe->map % 16 || (uintptr_t)pe->head % 16 || (uintptr_t)pe->src_pe % 16 ||
                   (uintptr_t)pe->tgt_pe % 16))
        return bad("render_points_novel_pe: latent / map / head / pos-encoding not 16-byte aligned");
    if (P == 0 || scene->SB == 0) return DINER_OK;
    if (!xyz_in || !xyz_gen || !xyz_tgt || !viewdirs || !rgbsigma_out) return bad("render_points_novel_pe: NULL points / viewdirs / out");
    return (f16 ? genf16::launch_points_mlp_novel_pe : gen::launch_points_mlp_novel_pe)(
        *scene, index ? *index : k_default_index, *gen, *pe, *shape, mlp_packed, xyz_in, xyz_gen, xyz_tgt, viewdirs, P, rgbsigma_out,
        (hipStream_t)stream);
}

/* ---- the NOVEL point model's training path (train_novel.hip; diner_amd/training_novel.py) ------------------------------------------ */
int diner_train_point_inputs_novel(const DinerScene *scene, const DinerLatentIndex *index, const float *latent_nhwc, const DinerNovelGen *gen,
                                   const float *xyz_in, const float *xyz_gen, const float *viewdirs, int64_t P, int32_t sb, float *in_out,
                                   int64_t ld_in, float *zlat, float *taps, float *gen_taps, void *stream)
{
    const char *who = "train_point_inputs_novel";
    int rc;
    if (!gen) return bad("train_point_inputs_novel: gen is NULL");
    if (index && index->interp == 2) {   /* SpatialEncoder's third index_interp: DinerLatentIndex does not carry the 16-tap lookup */
        set_error("%s: latent index interp=2 (bicubic) is not served: the 4-tap modes only (DINER_INDEX_BILINEAR 0 or DINER_INDEX_NEAREST 1)", who);
        return DINER_E_UNSUPPORTED;
    }
    if ((rc = check_train_gen_inputs(scene, index, 0, 1, sb, ld_in, who))) return rc;
    if (P < 0) return bad("train_point_inputs_novel: bad P");
    if (gen->C != scene->C) { set_error("%s: general latent channels C=%d != latent channels C=%d", who, gen->C, scene->C); return DINER_E_INVALID; }
    if (gen->h < 1 || gen->w < 1) { set_error("%s: general latent size h=%d, w=%d (both >= 1)", who, gen->h, gen->w); return DINER_E_INVALID; }
    if ((int64_t)gen->h * gen->w > 0x7fffffffLL || (int64_t)scene->h * scene->w > 0x7fffffffLL)
        return bad("train_point_inputs_novel: a latent map of 2^31 or more texels (the tap indices are 32-bit)");
    if (!gen->poses || !gen->focal || !gen->c) return bad("train_point_inputs_novel: NULL general camera pointer");
    if (!(gen->image_w > 0.f) || !(gen->image_h > 0.f)) return bad("train_point_inputs_novel: bad general image shape");
    if (!xyz_in || !xyz_gen || !viewdirs || !in_out) return bad("train_point_inputs_novel: NULL pointer");
    if (zlat && (!latent_nhwc || !gen->latent || !taps || !gen_taps)) return bad("train_point_inputs_novel: NULL latent / taps pointer");
    if (P * (int64_t)scene->NV > 0x7fffffffLL) { set_error("%s: too many rows (%lld points, %d views)", who, (long long)P, scene->NV); return DINER_E_INVALID; }
    if (P == 0) return DINER_OK;
    return launch_train_point_inputs_novel(*scene, index ? *index : k_default_index, latent_nhwc, *gen, xyz_in, xyz_gen, viewdirs, P, sb, in_out,
                                           ld_in, zlat, taps, gen_taps, (hipStream_t)stream);
}

int diner_train_novel_gen_scatter(const float *d_zlat, const float *gen_taps, int64_t P, int32_t C, int32_t h, int32_t w, int32_t NV,
                                  float *d_gen_nhwc, void *stream)
{
    if (!d_zlat || !gen_taps || !d_gen_nhwc) return bad("train_novel_gen_scatter: NULL pointer");
    if (P < 0 || C <= 0 || h < 1 || w < 1 || NV < 1) return bad("train_novel_gen_scatter: bad size");
    if ((P + 15) / 16 > 0x7fffffffLL) return bad("train_novel_gen_scatter: too many points");
    if (P == 0) return DINER_OK;
    return launch_train_novel_gen_scatter(d_zlat, gen_taps, P, C, NV, d_gen_nhwc, (hipStream_t)stream);
}

}  // extern "C"
