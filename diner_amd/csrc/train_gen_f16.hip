// Shape-general training path in f16x3: the GEMM of train_gen.hip (activation codes, stride-described operands, ragged M, split-K) in
// the fp32-grade fp16 arithmetic of train.hip's gemm_f16x3_kernel, for every (M, N, K) diner_amd/training_gen.py issues:
//   gemm_act_f16x3_kernel  C[m][n] (+)= sum_k actA(A[m][k]) * actB(B[k][n])  (+ bias[n]) (* act'(S[m][n]))
//                          every operand element: activation in fp32, times a power of two (2^exp, or the one that maps *amax into
//                          [2^13, 2^14)), split into fp16 hi + lo; three v_mfma_f32_32x32x16_f16 per product (lo*hi, hi*lo, hi*hi), fp32
//                          accumulation, C divided by the two scales; the derivative in the epilogue is fp32 (act_bwd).
//                          128 x 128 x 32 block tiles, 4 waves as 2 x 2, LDS images double-buffered, 3-stage pipeline.
//                          BPRE: the B operand (a weight) arrives pre-split (split_weight_kernel): its tile is four 16-byte loads per
//                          thread that go to LDS as they are -- no VALU work, no bounds (the planes are zero-padded to whole tiles).
//   split_weight_kernel    fp16 hi / lo planes of a weight matrix of any (N, K), either orientation, made once per parameter version
// plus the C entry points (diner_train_gemm_act_f16x3, diner_train_gemm_act_f16x3_w, diner_train_split_weight).  A translation unit of
// its own (a code object of its own); the tile loads, the split, the scale and the epilogue are the shared ones of train_blocks.hpp.
#include "train_blocks.hpp"

namespace diner {

namespace train_gen_f16 {

using namespace train_blocks;

constexpr int BM = 128, BN = 128, BKH = 32;
constexpr int UNITS_T = (BKH / 8) * 128;   // 16-byte units of one fp16 plane of one operand tile

struct GemmArgs {
    const float *A, *B, *bias, *S;   // BPRE: B = the hi plane, Blo = the lo plane (fp16 [npad][kpad], k contiguous)
    const float *Blo;
    float *C;
    int64_t M;
    int N, K;
    int64_t sam, sak, sbk, sbn;      // element strides of the logical A[m][k], B[k][n]  (BPRE: sbn = kpad in halfs)
    int64_t ldc, lds_;
    int act_a, act_b, act_s;
    float beta;
    int accumulate, atomic;
    int64_t k_chunk;
    const unsigned int *amax_a, *amax_b;
    int exp_a, exp_b;
};

// A pre-split weight tile: 128 rows x 32 halfs x {hi, lo} = 2 x 512 16-byte units, two per plane and thread (pieces 0, 1: hi; 2, 3: lo),
// carried as raw 16-byte words.  The planes are whole tiles (rows padded to 128, k to 32): no bounds, past the last k-step the
// previous step is read again into a buffer nobody reads.
__device__ __forceinline__ void tile_load_w(f32x4 (&v)[4], const float *__restrict__ hi, const float *__restrict__ lo, int64_t kpad, int n0,
                                            int64_t k0, int tid)
{
    const int64_t k = k0 < kpad ? k0 : kpad - BKH;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        const int64_t off = ((int64_t)(n0 + (idx >> 2)) * kpad + k + (idx & 3) * 8) / 2;   // in floats (2 halfs)
        v[i] = *(const f32x4 *)(hi + off);
        v[2 + i] = *(const f32x4 *)(lo + off);
    }
}

__device__ __forceinline__ void tile_store_w(h8 *Thi, h8 *Tlo, const f32x4 (&v)[4], int tid)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, o = unit(idx & 3, idx >> 2);
        *(f32x4 *)&Thi[o] = v[i];
        *(f32x4 *)&Tlo[o] = v[2 + i];
    }
}

// The operand transform happens here, once per staged element, in fp32 and before the scale and the split; out-of-range pieces are
// staged as 0 (not act(0): Softplus(0) != 0).  SP: the instantiation that carries the Softplus code (applied four values at a time,
// right before their split: sixteen results at once do not fit beside the accumulators).
template <bool KC, bool SP>
__device__ __forceinline__ void tile_store(h8 *Thi, h8 *Tlo, const f32x4 (&v)[4], unsigned ok, int act, float beta, float sc, int tid)
{
    const bool relu = act == DINER_ACT_RELU, sp = SP && act == DINER_ACT_SOFTPLUS;
    f32x4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = v[i];
    if (ok != 0xFu) {   // ragged edge of the operand only
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) x[i][j] = ((ok >> i) & 1u) ? v[i][j] : 0.0f;
    }
    auto val = [&](int i, int j) -> float { return sp && ((ok >> i) & 1u) ? softplus(x[i][j], beta) : x[i][j]; };
    if (KC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            put4(Thi, Tlo, idx >> 3, (idx & 7) * 4, val(i, 0), val(i, 1), val(i, 2), val(i, 3), relu, sc);
        }
    } else {
        // The thread holds 4 (k) x 4 (l); row l + c goes to LDS slot slot16(l + c) = (l & ~15) | 4c | (lq4 & 3): the 16 half-cells of a
        // 16-lane group (4 k-quads x 4 l-quads) fall on 16 different bank pairs (row order: 4-way conflicts).  epilogue<PA, PB> undoes it.
        const int kq4 = (tid & 3) | ((tid >> 4) & 4), lq4 = ((tid >> 2) & 15) | ((tid >> 3) & 16);
        const int kq = kq4 * 4, sl = ((lq4 * 4) & ~15) | (lq4 & 3);
#pragma unroll
        for (int c = 0; c < 4; ++c) put4(Thi, Tlo, sl + 4 * c, kq, val(0, c), val(1, c), val(2, c), val(3, c), relu, sc);
    }
}

// AK: A contiguous along k (sak == 1) else along m.  BNC: B contiguous along n (sbn == 1) else along k.  BPRE: B pre-split (then BNC is
// false: the planes are k-contiguous).  SP: Softplus on a staged operand.
// The k-loop is train.hip's 3-stage pipeline: while tile t is multiplied out of LDS buffer t&1, tile t+1 sits in registers (split and
// stored into the other buffer after the MFMAs) and the loads of tile t+2 are issued; each step is one basic block whose global loads
// and split are dealt between the 24 MFMAs (sched_group_barrier).
// Two workgroups per CU (256 VGPRs) where both tiles are staged along k (forward, and dX on the pre-split weight: the step's hot
// forms); an instantiation with a transposing store does not fit 256 registers beside the three load stages (hipcc spills 4 to 30 of them
// to scratch) and is built for one workgroup per CU instead.
template <bool AK, bool BNC, bool BPRE, bool SP>
__global__ __launch_bounds__(256, (AK && !BNC) ? 2 : 1) void gemm_act_f16x3_kernel(GemmArgs g)
{
    __shared__ h8 T[2][4][UNITS_T];  // [buffer][A hi, A lo, B hi, B lo][unit]  (64 KiB)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t m0;
    int n0;
    // split-K launches: re-deal the (tile, chunk) pairs so that one XCD works through whole chunks (its L2 then serves the chunk's operand
    // slices to all of the chunk's tiles) -- train.hip's gemm_f16x3_kernel
    int64_t bx = blockIdx.x, bz = blockIdx.z;
    if (gridDim.z % 8 == 0) {
        const int64_t id = (int64_t)blockIdx.z * gridDim.x + blockIdx.x, xcd = id % 8, j = id / 8;
        bz = (j / gridDim.x) * 8 + xcd;
        bx = j % gridDim.x;
    }
    tile_of(g.M, g.N, BM, BN, bx, m0, n0);
    const int64_t kbeg = bz * g.k_chunk;
    const int64_t kend = kbeg + g.k_chunk < g.K ? kbeg + g.k_chunk : g.K;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    float sa, ia, sb, ib;
    scale_of(g.amax_a, g.exp_a, sa, ia);
    scale_of(g.amax_b, g.exp_b, sb, ib);
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;
    f32x4 ra[2][4], rb[2][4];
    const int r = lane & 31, h = lane >> 5;
    const int64_t steps = (kend - kbeg + BKH - 1) / BKH;
    unsigned oka[2], okb[2] = {0u, 0u};
#define DINER_LOAD_B(SL, K0)                                                                                     \
    if constexpr (BPRE) tile_load_w(rb[SL], g.B, g.Blo, g.sbn, n0, K0, tid);                                     \
    else okb[SL] = tile_load<!BNC>(rb[SL], g.B, g.sbn, g.sbk, n0, g.N, K0, kend, tid);
#define DINER_STORE_B(BUF, SL)                                                                                   \
    if constexpr (BPRE) tile_store_w(T[BUF][2], T[BUF][3], rb[SL], tid);                                         \
    else tile_store<!BNC, SP>(T[BUF][2], T[BUF][3], rb[SL], okb[SL], g.act_b, g.beta, sb, tid);
    oka[0] = tile_load<AK>(ra[0], g.A, g.sam, g.sak, m0, g.M, kbeg, kend, tid);
    DINER_LOAD_B(0, kbeg)
    oka[1] = tile_load<AK>(ra[1], g.A, g.sam, g.sak, m0, g.M, kbeg + BKH, kend, tid);      // all-invalid past kend
    DINER_LOAD_B(1, kbeg + BKH)
    tile_store<AK, SP>(T[0][0], T[0][1], ra[0], oka[0], g.act_a, g.beta, sa, tid);
    DINER_STORE_B(0, 0)
    __syncthreads();
#define DINER_GEMM_STEP(SL)                                                                                      \
    {                                                                                                            \
        const int64_t k2 = kbeg + (t + 2) * BKH;                                                                 \
        oka[SL] = tile_load<AK>(ra[SL], g.A, g.sam, g.sak, m0, g.M, k2, kend, tid);                              \
        DINER_LOAD_B(SL, k2)                                                                                     \
        _Pragma("unroll") for (int ks = 0; ks < BKH / 16; ++ks) {                                                \
            const int u = ks * 2 + h;                                                                            \
            h8 ah[2], al[2], bh[2], bl[2];                                                                       \
            _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                      \
                const int oa = unit(u, wm + 32 * q + r), ob = unit(u, wn + 32 * q + r);                          \
                ah[q] = T[SL][0][oa]; al[q] = T[SL][1][oa];                                                      \
                bh[q] = T[SL][2][ob]; bl[q] = T[SL][3][ob];                                                      \
            }                                                                                                    \
            _Pragma("unroll") for (int ta = 0; ta < 2; ++ta)                                                     \
                _Pragma("unroll") for (int tb = 0; tb < 2; ++tb) {                                               \
                    acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ta], bh[tb], acc[ta][tb], 0, 0, 0);  \
                    acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ta], bl[tb], acc[ta][tb], 0, 0, 0);  \
                    acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ta], bh[tb], acc[ta][tb], 0, 0, 0);  \
                }                                                                                                \
        }                                                                                                        \
        tile_store<AK, SP>(T[1 - SL][0], T[1 - SL][1], ra[1 - SL], oka[1 - SL], g.act_a, g.beta, sa, tid);       \
        DINER_STORE_B(1 - SL, 1 - SL)                                                                            \
        if constexpr (!SP) {                                                                                     \
            /* sched_group_barrier masks: 0x008 MFMA, 0x020 VMEM read, 0x100 DS read, 0x200 DS write, 0x002 VALU */ \
            __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);  /* fragments of the first k-step */              \
            _Pragma("unroll") for (int i_ = 0; i_ < 24; ++i_) {                                                  \
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                               \
                if (i_ < 16 && (i_ & 1) == 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                 \
                if (i_ < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                   \
                __builtin_amdgcn_sched_group_barrier(0x002, BPRE ? 3 : 6, 0);                                    \
                if (i_ >= 8 && (i_ & 1) == 0) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);                 \
            }                                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                   \
        }                                                                                                        \
        __syncthreads();                                                                                         \
    }
    for (int64_t t = 0; t < steps; ++t) {
        DINER_GEMM_STEP(0)
        if (++t >= steps) break;
        DINER_GEMM_STEP(1)
    }
#undef DINER_GEMM_STEP
#undef DINER_LOAD_B
#undef DINER_STORE_B
    epilogue<!AK, BNC && !BPRE>(g, acc, m0, n0, wm, wn, lane, bz, ia * ib,
                                [&](float v, float s) { return g.S ? act_bwd(v, s, g.act_s, g.beta) : v; });
}

// fp16 hi / lo planes of a weight for the BPRE kernel: plane[n][k] = split(B[k][n] * 2^exp) for n < N, k < K, 0 in the padding
// (npad x kpad, whole 128 x 32 tiles); B[k][n] = W[n*ld + k], or W[k*ld + n] when transpose (the dX GEMM's operand)
__global__ __launch_bounds__(256) void split_weight_kernel(const float *__restrict__ W, int N, int K, int64_t ld, int transpose, int exp_,
                                                           _Float16 *__restrict__ hi, _Float16 *__restrict__ lo, int64_t kpad, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t n = i / kpad, k = i - n * kpad;
    float t = 0.0f;
    if (n < N && k < K) t = (transpose ? W[k * ld + n] : W[n * ld + k]) * __uint_as_float((unsigned int)(127 + exp_) << 23);
    const _Float16 hv = (_Float16)t;
    hi[i] = hv;
    lo[i] = (_Float16)(t - (float)hv);
}

template <bool AK, bool BNC, bool BPRE>
static void launch_sp(const GemmArgs &g, dim3 grid, bool sp, hipStream_t st)
{
    if (sp) hipLaunchKernelGGL((gemm_act_f16x3_kernel<AK, BNC, BPRE, true>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((gemm_act_f16x3_kernel<AK, BNC, BPRE, false>), grid, dim3(256), 0, st, g);
}

static int launch(const GemmArgs &g, bool pre, hipStream_t st)
{
    if (g.M == 0 || g.N == 0) return DINER_OK;
    const dim3 grid((unsigned)(((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN)), 1, (unsigned)((g.K + g.k_chunk - 1) / g.k_chunk));
    const bool sp = g.act_a == DINER_ACT_SOFTPLUS || (!pre && g.act_b == DINER_ACT_SOFTPLUS);
    const bool ak = g.sak == 1, bnc = g.sbn == 1;
    if (pre) launch_sp<true, false, true>(g, grid, sp, st);
    else if (ak && bnc) launch_sp<true, true, false>(g, grid, sp, st);
    else if (ak && !bnc) launch_sp<true, false, false>(g, grid, sp, st);
    else if (!ak && bnc) launch_sp<false, true, false>(g, grid, sp, st);
    else launch_sp<false, false, false>(g, grid, sp, st);
    return check_launch("train_gen_f16::gemm_act_f16x3_kernel");
}

static int bad(const char *msg)
{
    set_error("%s", msg);
    return DINER_E_INVALID;
}

static bool act_known(int32_t a) { return a == DINER_ACT_NONE || a == DINER_ACT_RELU || a == DINER_ACT_SOFTPLUS; }
static bool beta_ok(float beta) { return beta > 0.0f && beta < __builtin_inff(); }
static bool exp_ok(int32_t e) { return e >= -60 && e <= 60; }

}  // namespace train_gen_f16
}  // namespace diner

using namespace diner;
using namespace diner::train_gen_f16;

extern "C" {

int diner_train_gemm_act_f16x3(const float *A, const float *B, const float *bias, const float *S, float *C, int64_t M, int32_t N, int32_t K,
                               int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t ldc, int64_t lds, int32_t act_a, int32_t act_b,
                               int32_t act_s, float beta, int32_t accumulate, int32_t atomic, int64_t k_chunk, const void *amax_a,
                               const void *amax_b, int32_t exp_a, int32_t exp_b, void *stream)
{
    if (!A || !B || !C) return bad("train_gemm_act_f16x3: NULL pointer");
    if (!act_known(act_a) || !act_known(act_b) || !act_known(act_s)) {
        set_error("train_gemm_act_f16x3: unknown activation code (act_a %d, act_b %d, act_s %d; DINER_ACT_NONE 0, _RELU 1, _SOFTPLUS 2)",
                  act_a, act_b, act_s);
        return DINER_E_INVALID;
    }
    if ((act_a == DINER_ACT_SOFTPLUS || act_b == DINER_ACT_SOFTPLUS || act_s == DINER_ACT_SOFTPLUS) && !beta_ok(beta))
        return bad("train_gemm_act_f16x3: Softplus needs a finite beta > 0");
    if (M < 0 || N <= 0 || K <= 0 || (N & 3) || k_chunk < 0 || (k_chunk & 31))
        return bad("train_gemm_act_f16x3: bad size (N % 4, k_chunk % 32 must be 0)");
    if (k_chunk > 0 && k_chunk < K && !atomic) return bad("train_gemm_act_f16x3: a split contraction (k_chunk < K) needs atomic = 1");
    if (sak != 1 && sam != 1) return bad("train_gemm_act_f16x3: A must be contiguous along m or k");
    if (sbn != 1 && sbk != 1) return bad("train_gemm_act_f16x3: B must be contiguous along k or n");
    if ((sak == 1 ? (K & 3) || (sam & 3) : (M & 3) || (sak & 3)) || (sbn == 1 ? (sbk & 3) : (K & 3) || (sbn & 3)))
        return bad("train_gemm_act_f16x3: the contiguous extent and the other stride of each operand must be multiples of 4");
    if (((uintptr_t)A & 15) || ((uintptr_t)B & 15)) return bad("train_gemm_act_f16x3: operands must be 16-byte aligned");
    if (!exp_ok(exp_a) || !exp_ok(exp_b)) return bad("train_gemm_act_f16x3: scale exponent out of range");
    const int64_t kc = k_chunk > 0 ? k_chunk : K;
    GemmArgs g{A, B, bias, S, nullptr, C, M, N, K, sam, sak, sbk, sbn, ldc, lds, act_a, act_b, act_s, beta, accumulate, atomic, kc,
               (const unsigned int *)amax_a, (const unsigned int *)amax_b, exp_a, exp_b};
    return launch(g, false, (hipStream_t)stream);
}

int64_t diner_train_split_weight_halfs(int32_t N, int32_t K)
{
    if (N <= 0 || K <= 0) return 0;
    return (((int64_t)N + BN - 1) / BN * BN) * (((int64_t)K + BKH - 1) / BKH * BKH);
}

int diner_train_split_weight(const float *W, int32_t N, int32_t K, int64_t ld, int32_t transpose, int32_t exp, void *hi, void *lo, void *stream)
{
    if (!W || !hi || !lo || N <= 0 || K <= 0 || ld <= 0) return bad("train_split_weight: bad argument");
    if (ld < (transpose ? N : K)) return bad("train_split_weight: ld is smaller than the row length");
    if (!exp_ok(exp)) return bad("train_split_weight: scale exponent out of range");
    if (((uintptr_t)hi & 15) || ((uintptr_t)lo & 15)) return bad("train_split_weight: planes must be 16-byte aligned");
    const int64_t kpad = ((int64_t)K + BKH - 1) / BKH * BKH, total = diner_train_split_weight_halfs(N, K);
    hipLaunchKernelGGL(split_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, N, K, ld, transpose, exp,
                       (_Float16 *)hi, (_Float16 *)lo, kpad, total);
    return check_launch("train_gen_f16::split_weight_kernel");
}

int diner_train_gemm_act_f16x3_w(const float *A, int64_t sam, const void *Bhi, const void *Blo, const float *bias, const float *S, int64_t lds,
                                 float *C, int64_t ldc, int64_t M, int32_t N, int32_t K, int32_t act_a, int32_t act_s, float beta,
                                 int32_t accumulate, const void *amax_a, int32_t exp_a, int32_t exp_b, void *stream)
{
    if (!A || !Bhi || !Blo || !C) return bad("train_gemm_act_f16x3_w: NULL pointer");
    if (!act_known(act_a) || !act_known(act_s)) {
        set_error("train_gemm_act_f16x3_w: unknown activation code (act_a %d, act_s %d; DINER_ACT_NONE 0, _RELU 1, _SOFTPLUS 2)", act_a, act_s);
        return DINER_E_INVALID;
    }
    if ((act_a == DINER_ACT_SOFTPLUS || act_s == DINER_ACT_SOFTPLUS) && !beta_ok(beta))
        return bad("train_gemm_act_f16x3_w: Softplus needs a finite beta > 0");
    if (M < 0 || N <= 0 || K <= 0 || (N & 3) || (K & 3) || (sam & 3)) return bad("train_gemm_act_f16x3_w: bad size (N % 4, K % 4, sam % 4 must be 0)");
    if (((uintptr_t)A & 15) || ((uintptr_t)Bhi & 15) || ((uintptr_t)Blo & 15)) return bad("train_gemm_act_f16x3_w: operands must be 16-byte aligned");
    if (!exp_ok(exp_a) || !exp_ok(exp_b)) return bad("train_gemm_act_f16x3_w: scale exponent out of range");
    const int64_t kpad = ((int64_t)K + BKH - 1) / BKH * BKH;
    GemmArgs g{A, (const float *)Bhi, bias, S, (const float *)Blo, C, M, N, K, sam, 1, 1, kpad, ldc, lds, act_a, DINER_ACT_NONE, act_s, beta,
               accumulate, 0, K, (const unsigned int *)amax_a, nullptr, exp_a, exp_b};
    return launch(g, true, (hipStream_t)stream);
}

}  // extern "C"
