// Shape-general fused per-point evaluation in split fp16 ("f16x3"): the job of points_mlp_gen_kernel (points_mlp_gen.hip) -- multi-view
// projection, positional encodings, latent gather, the ResnetFC fusion MLP and the sigmoid/relu head for any MLP shape inside
// gen::check_shape's envelope, described at run time by a DinerMlpShape -- with the arithmetic of points_mlp_f16.hip:
//   PixelNeRF.forward            src/models/pixelnerf.py:55-145
//   PositionalEncoding.forward   src/models/positional_encoding.py:33-53
//   SpatialEncoder.index         src/models/image_encoder.py:97-127
//   ResnetFC.forward             src/models/resnetfc.py:129-159
//
// Arithmetic (one description with points_mlp_f16.hip's header): every GEMM operand is split a = a_hi + a_lo, w = w_hi + w_lo with
// hi = fp16(v), lo = fp16(v - hi); a*w ~= a_hi*w_hi + a_hi*w_lo + a_lo*w_hi as three v_mfma_f32_32x32x16_f16 back to back on one fp32
// accumulator.  The hidden state is carried scaled by 2^-4: lin_in's inputs, the latent (through its tap weights) and every bias are
// pre-scaled, the head multiplies by 16 (all exact).  ReLU commutes with the scale and keeps NaN (v < 0 ? 0 : v); Softplus is
// evaluated as softplus_beta(16 x) / 16 with torch's threshold 20 on the unscaled argument.  An activation beyond the fp16 range
// becomes hi = inf, lo = -inf, the next layer's products inf - inf = NaN, and the sample's rgb-sigma is NaN: compositing raises
// DINER_STATUS_NONFINITE.  Nothing is clamped.  lin_out (d_hidden -> 4) is an fp32 VALU dot product straight from the accumulators.
// Bias / residual / mean-over-views order are those of points_mlp_gen.hip; none of the standard kernel's algebraic shortcuts is used.
//
// Structure: 64 points per workgroup, 8 waves, views one after another, x / net / the running view-sum in registers, the three
// instantiations <RB point blocks of 32, CT feature tiles of 32 per wave> of points_mlp_gen.hip (<1,1> d_hidden <= 128, <2,1> <= 256,
// <2,2> <= 512).  Unlike there the GEMMs are computed TRANSPOSED, X^T = W A^T: the weights are the MFMA's A operand (rows = output
// features) and the activations its B operand (columns = points), so a lane's 16 accumulator registers are 4 runs of 4 consecutive
// features of ONE point.  Two runs of the lane halves h = 0 / 1 (features 8g + 4h + 0..3) are joined by v_permlane32_swap into the 8
// consecutive features of a 16-byte operand slot, so an activation goes back to LDS as 4 ds_write_b128 per tile and part.
//
// LDS A image (128 KiB): [plane = k / 8 (64)][part hi = 0 / lo = 1][point (64)][k % 8] halfs, a 16-byte slot per (plane, part, point).
// The B fragment of k-block kb (16 columns) of lane (point r, half h) is the slot (plane 2 kb + h, part, point): a ds_read_b128 whose 32
// lanes of a half read 512 contiguous bytes, so each of its 16-lane groups covers 256 distinct bytes = all 64 banks once: no
// conflict.  Stores are ds_write_b128 to 128 contiguous bytes per 8-lane group (activations: 32 points of one plane per lane half;
// encodings: the 64 points of one plane; latent: 8 points x 8 planes): no conflict either.  After the image come one Tap per point
// (2 KiB); lin_out's per-wave partial sums reuse the image.  d_latent above 512 runs in 512-column pieces as in points_mlp_gen.hip.
//
// Packed weight image (diner_pack_mlp_gen_f16): halfs lin_in | lin_z[0..nlz) | fc_0[0..nb) | fc_1[0..nb), each
// [feature tile][k-block of 16][part][lane][8]: lane = 32 h + r holds W[n = 32 tile + r][k = 16 kb + 8 h + j], j = 0..7 (zero outside
// the layer), i.e. one global_load_dwordx4 per fragment; then fp32: the biases x 2^-4 (lin_in | lin_z[b] | fc_0[b] | fc_1[b], d_hidden
// each | lin_out padded to 32) and lin_out's weights [4][d_hidden], unscaled.
//
// The device code is points_mlp_gen_f16_kernel.hpp: one kernel template whose first parameter is the lookup mode.  This file holds the host
// side -- the packers, the validation and the dispatch -- and instantiates the default mode (bilinear / border); every other mode is
// instantiated in a translation unit of its own.
#include "points_mlp_gen_f16_kernel.hpp"

namespace diner {
namespace gen {
int check_shape(const DinerMlpShape &);   // points_mlp_gen.hip: the envelope is the same
}
namespace genf16 {

int64_t packed_floats(const DinerMlpShape &m) { return layout_of(m).total; }

// one thread per weight slot of one layer: its hi and lo halfs
__global__ void pack_layer_kernel(const float *__restrict__ w, int in_dim, int out_dim, int nkb, int64_t n, _Float16 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const int64_t blk = i >> 9;
    const int kb = (int)(blk % nkb), tile = (int)(blk / nkb);
    const int r = tile * 32 + (lane & 31), k = kb * 16 + 8 * (lane >> 5) + j;
    const float v = (r < out_dim && k < in_dim) ? w[(int64_t)r * in_dim + k] : 0.0f;
    _Float16 hi, lo;
    split(v, hi, lo);
    out[blk * 1024 + lane * 8 + j] = hi;
    out[blk * 1024 + 512 + lane * 8 + j] = lo;
}

__global__ void pack_vec_kernel(const float *__restrict__ b, int n, int npad, float scale, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad) out[i] = i < n ? b[i] * scale : 0.0f;
}

static int pack_layer(const float *w, int in_dim, int out_dim, int nkb, int tiles, _Float16 *out, hipStream_t st)
{
    const int64_t n = (int64_t)tiles * nkb * 512;
    hipLaunchKernelGGL(pack_layer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, in_dim, out_dim, nkb, n, out);
    return check_launch("pack_layer_kernel (f16)");
}

static int pack_vec(const float *b, int n, int npad, float scale, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(pack_vec_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, b, n, npad, scale, out);
    return check_launch("pack_vec_kernel (f16)");
}

int launch_pack_mlp(const DinerMlpShape &m, const DinerMlpGenRaw &raw, float *out, hipStream_t st)
{
    const Layout L = layout_of(m);
    int rc;
    _Float16 *wh = (_Float16 *)out;
    float *bias = out + L.off_bias;
    if ((rc = pack_layer(raw.lin_in_w, L.din, L.H, L.nkb_in, L.NT, wh + L.off_in, st))) return rc;
    if ((rc = pack_vec(raw.lin_in_b, L.H, L.H, ACT_SCALE, bias + L.bias_lin_in(), st))) return rc;
    for (int b = 0; b < L.nlz; ++b) {
        if ((rc = pack_layer(raw.lin_z_w[b], L.dlat, L.H, L.nkb_lat, L.NT, wh + L.off_z + b * L.w_z, st))) return rc;
        if ((rc = pack_vec(raw.lin_z_b[b], L.H, L.H, ACT_SCALE, bias + L.bias_lin_z(b), st))) return rc;
    }
    for (int b = 0; b < L.nb; ++b) {
        if ((rc = pack_layer(raw.fc0_w[b], L.H, L.H, L.H / 16, L.NT, wh + L.off_fc0 + b * L.w_h, st))) return rc;
        if ((rc = pack_vec(raw.fc0_b[b], L.H, L.H, ACT_SCALE, bias + L.bias_fc0(b), st))) return rc;
        if ((rc = pack_layer(raw.fc1_w[b], L.H, L.H, L.H / 16, L.NT, wh + L.off_fc1 + b * L.w_h, st))) return rc;
        if ((rc = pack_vec(raw.fc1_b[b], L.H, L.H, ACT_SCALE, bias + L.bias_fc1(b), st))) return rc;
    }
    if ((rc = pack_vec(raw.lin_out_b, 4, 32, ACT_SCALE, bias + L.bias_lin_out(), st))) return rc;
    return pack_vec(raw.lin_out_w, 4 * L.H, 4 * L.H, 1.0f, out + L.off_wout, st);
}

template int launch_mode<Default>(const Launch &);   // the three bilinear / border kernels: this file's code object

// What every render call checks before it launches (`who` names the entry point in the messages); DINER_OK: `a` is filled in but for
// the lookup mode and the maps.
static int validate(const char *who, const DinerScene &s, const DinerMlpShape &m, const float *mlp_packed, const float *rays, const float *z,
                    int64_t NR, int K, float *rgbsigma, hipStream_t st, Launch &a)
{
    int rc;
    if ((rc = gen::check_shape(m))) return rc;
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
    const int rc = validate("render_points_gen_f16", s, m, mlp_packed, rays, z, NR, K, rgbsigma, st, a);
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
    const int rc = validate("render_points_gen_lz (f16x3)", s, m, mlp_packed, rays, z, NR, K, rgbsigma, st, a);
    if (rc || no_points(a)) return rc;
    a.lzmaps = lzmaps;
    if (bicubic_pad >= 0) { a.ix_padding = bicubic_pad; return launch_mode<LzBc>(a); }
    a.ix_interp = ix.interp; a.ix_padding = ix.padding;
    return launch_mode<Lz>(a);
}

}  // namespace genf16
}  // namespace diner
