// Shape-general fused per-point evaluation: the job of points_mlp_kernel (points_mlp.hip) -- multi-view projection, positional
// encodings, bilinear latent gather, the ResnetFC fusion MLP and the sigmoid/relu head -- for any MLP shape the reference's
// constructors accept within the envelope below, described at RUN time by a DinerMlpShape instead of compile-time constants:
//   PixelNeRF.forward            src/models/pixelnerf.py:55-145 (d_in = PE3 (3+6F) + viewdir 3 + PE1 (1+2F))
//   PositionalEncoding.forward   src/models/positional_encoding.py:33-53 (num_freqs F >= 1, include_input)
//   SpatialEncoder.index         src/models/image_encoder.py:97-127 (d_latent = the encoder's channel count)
//   ResnetFC.forward             src/models/resnetfc.py:129-159 (d_hidden, n_blocks, combine_layer, ReLU or Softplus(beta))
//
// Envelope: d_hidden in {32, 64, ..., 512}; d_latent a multiple of 8 up to 1024; n_blocks >= 1; combine_layer >= 0 (>= n_blocks:
// no mean over views, NV must be 1 -- pixelnerf.py:137 reshapes (SB,NV,B,4) to (SB,B,4)); d_in = 7 + 8F <= 512; d_out = 4.
//
// Arithmetic and structure are those of points_mlp_kernel (exact fp32 v_mfma_f32_32x32x2_f32, the same k order, the same bias /
// residual / mean order), so at the standard shape this kernel computes the same values; what changes is that the layer widths are
// loop bounds:
//   * 64 points per workgroup, 8 waves; the output columns of a layer are 32-wide tiles (NT = d_hidden / 32) distributed over the
//     waves by one of three instantiations <RB row blocks, CT column tiles per wave>: <1,1> for NT <= 4, <2,1> for NT <= 8,
//     <2,2> for NT <= 16.  A wave whose tile index passes NT-1 reads the last tile again and discards its result (uniform);
//   * the A operand of every layer is staged in one 128-KiB LDS image [k/8][k%2][row][(k/2)%4] of 512 columns; the latent GEMM
//     (d_latent up to 1024) runs in 512-column pieces: gather a piece, multiply, gather the next;
//   * weights are packed per layer in the B-fragment order of points_mlp.hip (diner_pack_mlp_gen) and streamed from L2 with one
//     k-block of prefetch;
//   * views are processed one after another; the hidden state, `net` and the running view-sum stay in registers.
//
// The device code is points_mlp_gen_kernel.hpp: one kernel template whose first parameter is the lookup mode.  This file holds the host
// side -- the envelope, the packers, the validation and the dispatch -- and instantiates the default mode (bilinear / border); every
// other mode is instantiated in a translation unit of its own.
#include "points_mlp_gen_kernel.hpp"

namespace diner {
namespace gen {

// DINER_OK, or DINER_E_UNSUPPORTED with the reason in diner_last_error()
int check_shape(const DinerMlpShape &m)
{
    if (m.d_out != 4) { set_error("mlp shape: d_out=%d unsupported (PixelNeRF's head is rgb + sigma: 4)", m.d_out); return DINER_E_UNSUPPORTED; }
    if (m.combine_type != DINER_COMBINE_AVERAGE) { set_error("mlp shape: combine_type %d unsupported (only 'average', resnetfc.py:9-14)", m.combine_type); return DINER_E_UNSUPPORTED; }
    if (m.d_hidden < 32 || m.d_hidden > 512 || m.d_hidden % 32) { set_error("mlp shape: d_hidden=%d unsupported (a multiple of 32 in [32, 512])", m.d_hidden); return DINER_E_UNSUPPORTED; }
    if (m.d_latent < 8 || m.d_latent > 1024 || m.d_latent % 8) { set_error("mlp shape: d_latent=%d unsupported (a multiple of 8 in [8, 1024])", m.d_latent); return DINER_E_UNSUPPORTED; }
    if (m.n_blocks < 1 || m.n_blocks > 64) { set_error("mlp shape: n_blocks=%d unsupported (1..64)", m.n_blocks); return DINER_E_UNSUPPORTED; }
    if (m.combine_layer < 0) { set_error("mlp shape: combine_layer=%d unsupported (>= 0)", m.combine_layer); return DINER_E_UNSUPPORTED; }
    if (m.num_freqs < 1 || 7 + 8 * m.num_freqs > KMAX) { set_error("mlp shape: num_freqs=%d unsupported (1..63)", m.num_freqs); return DINER_E_UNSUPPORTED; }
    if (m.d_in != 7 + 8 * m.num_freqs) { set_error("mlp shape: d_in=%d does not match num_freqs=%d (PixelNeRF: d_in = 7 + 8 * num_freqs)", m.d_in, m.num_freqs); return DINER_E_UNSUPPORTED; }
    if (!(m.beta >= 0.0f) || !(m.beta < __builtin_inff())) { set_error("mlp shape: beta must be finite and >= 0 (0 = ReLU)"); return DINER_E_UNSUPPORTED; }
    return DINER_OK;
}

int64_t packed_floats(const DinerMlpShape &m) { return layout_of(m).total; }

// one thread per packed float of one layer
__global__ void pack_layer_kernel(const float *__restrict__ w, int in_dim, int out_dim, int njb, int64_t n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ji = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const int64_t blk = i >> 8;
    const int jb = (int)(blk % njb), tile = (int)(blk / njb);
    const int r = tile * 32 + (lane & 31), k = jb * 8 + ji * 2 + (lane >> 5);
    out[i] = (r < out_dim && k < in_dim) ? w[(int64_t)r * in_dim + k] : 0.0f;
}

__global__ void pack_bias_kernel(const float *__restrict__ b, int n, int npad, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad) out[i] = i < n ? b[i] : 0.0f;
}

static int pack_layer(const float *w, int in_dim, int out_dim, int njb, int tiles, float *out, hipStream_t st)
{
    const int64_t n = (int64_t)tiles * njb * 256;
    hipLaunchKernelGGL(pack_layer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, in_dim, out_dim, njb, n, out);
    return check_launch("pack_layer_kernel");
}

static int pack_bias(const float *b, int n, int npad, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(pack_bias_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, b, n, npad, out);
    return check_launch("pack_bias_kernel");
}

int launch_pack_mlp(const DinerMlpShape &m, const DinerMlpGenRaw &raw, float *out, hipStream_t st)
{
    const Layout L = layout_of(m);
    int rc;
    float *bias = out + L.off_bias;
    if ((rc = pack_layer(raw.lin_in_w, L.din, L.H, L.njb_in, L.NT, out + L.off_in, st))) return rc;
    if ((rc = pack_bias(raw.lin_in_b, L.H, L.H, bias + L.bias_lin_in(), st))) return rc;
    for (int b = 0; b < L.nlz; ++b) {
        if ((rc = pack_layer(raw.lin_z_w[b], L.dlat, L.H, L.njb_lat, L.NT, out + L.off_z + b * L.w_z, st))) return rc;
        if ((rc = pack_bias(raw.lin_z_b[b], L.H, L.H, bias + L.bias_lin_z(b), st))) return rc;
    }
    for (int b = 0; b < L.nb; ++b) {
        if ((rc = pack_layer(raw.fc0_w[b], L.H, L.H, L.H / 8, L.NT, out + L.off_fc0 + b * L.w_h, st))) return rc;
        if ((rc = pack_bias(raw.fc0_b[b], L.H, L.H, bias + L.bias_fc0(b), st))) return rc;
        if ((rc = pack_layer(raw.fc1_w[b], L.H, L.H, L.H / 8, L.NT, out + L.off_fc1 + b * L.w_h, st))) return rc;
        if ((rc = pack_bias(raw.fc1_b[b], L.H, L.H, bias + L.bias_fc1(b), st))) return rc;
    }
    if ((rc = pack_layer(raw.lin_out_w, L.H, 4, L.H / 8, 1, out + L.off_out, st))) return rc;
    return pack_bias(raw.lin_out_b, 4, 32, bias + L.bias_lin_out(), st);
}

template int launch_mode<Default>(const Launch &);   // the three bilinear / border kernels: this file's code object

// What every render call checks before it launches (`who` names the entry point in the messages); DINER_OK: `a` is filled in but for
// the lookup mode and the maps.
static int validate(const char *who, const DinerScene &s, const DinerMlpShape &m, const float *mlp_packed, const float *rays, const float *z,
                    int64_t NR, int K, float *rgbsigma, hipStream_t st, Launch &a)
{
    int rc;
    if ((rc = check_shape(m))) return rc;
    if (m.combine_layer >= m.n_blocks && s.NV != 1) {
        set_error("%s: combine_layer=%d >= n_blocks=%d never averages over views, which the reference supports for NV = 1 "
                  "only (src/models/pixelnerf.py:137 reshapes (SB, NV, B, 4) to (SB, B, 4)); NV=%d", who, m.combine_layer, m.n_blocks, s.NV);
        return DINER_E_UNSUPPORTED;
    }
    if (s.C != m.d_latent) { set_error("%s: latent channels C=%d != d_latent=%d", who, s.C, m.d_latent); return DINER_E_INVALID; }
    if (s.num_freqs != m.num_freqs) { set_error("%s: scene num_freqs=%d != shape num_freqs=%d", who, s.num_freqs, m.num_freqs); return DINER_E_INVALID; }
    const int64_t P = NR * (int64_t)K;
    if ((P + TILE_P - 1) / TILE_P > 0x7fffffffLL) { set_error("%s: too many points (%lld)", who, (long long)P); return DINER_E_INVALID; }
    a = Launch{&s, layout_of(m), 0, 0, mlp_packed, rays, z, NR, K, rgbsigma, nullptr, st};
    return DINER_OK;
}

static bool no_points(const Launch &a) { return a.NR * (int64_t)a.K == 0 || a.s->SB == 0; }

// bicubic_pad >= 0: the bicubic lookup with that DINER_INDEX_PAD_* (ix is then not read)
int launch_points_mlp(const DinerScene &s, const DinerLatentIndex &ix, const DinerMlpShape &m, const float *mlp_packed, const float *rays,
                      const float *z, int64_t NR, int K, float *rgbsigma, hipStream_t st, int bicubic_pad)
{
    Launch a;
    const int rc = validate("render_points_gen", s, m, mlp_packed, rays, z, NR, K, rgbsigma, st, a);
    if (rc || no_points(a)) return rc;
    if (bicubic_pad >= 0) { a.ix_padding = bicubic_pad; return launch_mode<Bc>(a); }
    if (ix.interp == DINER_INDEX_BILINEAR && ix.padding == DINER_INDEX_PAD_BORDER) return launch_mode<Default>(a);
    a.ix_interp = ix.interp; a.ix_padding = ix.padding;
    return launch_mode<Ix>(a);
}

// launch_points_mlp with the lin_z maps of linz_maps_gen.hip (lzmaps; the shape has nlz > 0): every 4-tap lookup mode runs on one kernel
int launch_points_mlp_lz(const DinerScene &s, const DinerLatentIndex &ix, const DinerMlpShape &m, const float *mlp_packed, const float *rays,
                         const float *z, int64_t NR, int K, float *rgbsigma, hipStream_t st, int bicubic_pad, const float *lzmaps)
{
    Launch a;
    const int rc = validate("render_points_gen_lz", s, m, mlp_packed, rays, z, NR, K, rgbsigma, st, a);
    if (rc || no_points(a)) return rc;
    a.lzmaps = lzmaps;
    if (bicubic_pad >= 0) { a.ix_padding = bicubic_pad; return launch_mode<LzBc>(a); }
    a.ix_interp = ix.interp; a.ix_padding = ix.padding;
    return launch_mode<Lz>(a);
}

}  // namespace gen
}  // namespace diner
