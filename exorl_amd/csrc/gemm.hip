// Grouped MFMA GEMMs for the hidden layers: forward (x W^T), dgrad (dZ W) and wgrad (dZ^T H) of nn.Linear, several
// independent problems per launch. Layout 0 / "row image": element (r, k) at ptr[r * ld + k]; layout 1 / "k image": at ptr[k * ld + r].
//
// Map of the file: the kernel families, when each is taken, and who reaches it in the product.
//
//  fp32-source operands (gemm_grouped; the intrinsic modules in intr.hip, the pixel agents' heads and module layers in pixel_agent.hip, and the
//  actor / critic layers of agent.hip in fp32 precision)
//  * gemm_kernel<PREC, AL, BL, VEC>: 64 x 64 tile, register-staged double buffer, all four layout pairs, any shape (bounds-guarded; VEC = the
//    16-byte loads where pointers and pitches allow). PREC picks the product: exact fp32 (v_mfma_f32_32x32x2_f32), bf16, split bf16 in two
//    (bf16x3) or three (bf16x6) planes made while staging. Taken whenever planes_adapter is not. (bf16x6 state agents whose shapes tile by 128
//    do not come here: agent.hip converts their operands to three planes and calls gemm16_grouped, below.)
//  * planes_adapter: bf16x3 problems with M, N, K >= 256 in one of the three nn.Linear layout pairs, outside a stream capture. Writes zero-padded
//    hi/lo bf16 planes of both operands into a scratch arena and hands them to gemm16_grouped, where (padded to multiples of 128) they take the
//    gemm16p kernels: the same arithmetic at about four times the rate of gemm_kernel. The reward-free agents' updates reach it.
//
//  bf16 operands in memory, plain, as hi/lo planes or as hi/mid/lo planes (gemm16_grouped, gemm16_grouped_mixed; the H x H layers of every actor /
//  critic in agent.hip in bf16, bf16x3 and — at hidden_dim and batch multiples of 128 — bf16x6 precision, and planes_adapter). One ladder,
//  pick16(), first match wins:
//  * three planes (Gemm16Problem::A_mid; exorl_gemm_planes3, agent.hip's bf16x6 route): gemm16p_kernel<AT, BT, 3, 64> or an error — 128 x 64
//    tiles, k32 stages four deep (144 KB of LDS), gemm_kernel<BF16X6>'s six products in three accumulator classes; the three uniform forms, no
//    mixed one. Needs what the next entry needs. The planes come from to_planes3_kernel (fp32 -> three bf16 images, one pass per buffer).
//  * gemm16p_kernel / gemm16p_mixed_kernel: 128 x TN tiles, LDS-DMA stage ring, XCD-local tile blocks, float4 epilogue. Needs M % 128, N % 64,
//    K % 128 = 0, 16-byte aligned operands, lo planes, C and bias, ldc % 4 = 0. TN = 128 when every N allows it and the launch still has 256
//    workgroups, else 64. Every launch of the product at hidden_dim and batch multiples of 128 (the 1024-wide flagship step among them).
//  * gemm16x3_kernel / gemm16x3_mixed_kernel (split planes), gemm16g_kernel / gemm16g_mixed_kernel (plain): 64 x 64 tiles, LDS-DMA, scalar
//    stores. Need M, N % 64 = 0, aligned operands, and K % 64 = 0 (split) or K % 256 = 0 (plain, four-stage ring); nothing of C. E.g.
//    split-bf16 planes at a batch that is a multiple of 64 but not of 128, or any launch whose output is not 16-byte aligned.
//  * gemm16_kernel<AL, BL, BM, NS, GUARD>: BM x 64 tiles (BM = 128 from 256 workgroups), register-staged, bounds-guarded unless M % 128, N % 64,
//    K % 64 = 0. Plain bf16 only, no mixed form; everything else the entry point's alignment rules admit, e.g. plain bf16 at hidden_dim 192,
//    where K is no multiple of 256.
//  The mixed entry (wgrad + dgrad of one backward pass in one launch) has a precondition of its own and otherwise falls back to one
//  gemm16_grouped call per problem; see gemm16_grouped_mixed.
//
// Shared by all of them: 256-thread workgroups of four waves on 32 x 32 MFMA accumulators (v_mfma_f32_32x32x16_bf16, fp32 accumulate), LDS rows
// of 16-byte units XOR-swizzled so the ds_read_b128 fragment reads are bank-conflict free, and — for operands whose reduction index is the slow
// dimension (dgrad B, wgrad A and B) — a transpose on the way in (registers) or out (ds_read_b64_tr_b16) of LDS, so that the three GEMM forms
// share one inner loop per family. Each family's own design notes and measurements stand in front of its kernels.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "kernels.h"

// ---- debug state (no product path sets it), read through tune_variant() / prec_override_mask() here and in pixels.hip, agent.hip, pixel_agent.hip
namespace exorl {
static int g_tune_variant = 0;       // exorl_gemm_tune: the TUNE_* reference-path bits (kernels.h), each read at one decision point; 0 = defaults
// exorl_debug_precision_override (tools/debug/config4_ablation.py): which split-bf16 products run with exact fp32 products instead.
// bits: 1 / 2 forward (row-image A, row-image B) narrow / wide; 4 / 8 wgrad (k-image A and B); 16 / 32 dgrad (row-image A, k-image B);
// "wide" = a problem dimension >= 8192 (the 39200-wide layers of the pixel agents); 64 / 128 / 256 = conv forward / dgrad / wgrad (pixels.hip)
static int g_prec_override = 0;
int tune_variant() { return g_tune_variant; }
int prec_override_mask() { return g_prec_override; }
}  // namespace exorl
extern "C" int exorl_gemm_tune(int32_t variant) {
    exorl::g_tune_variant = variant < 0 ? 0 : variant;
    return 0;
}
extern "C" int exorl_debug_precision_override(int32_t mask) {
    exorl::g_prec_override = mask;
    return 0;
}

namespace exorl {

// Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg): off by default,
// the product path never pays for it.
struct GemmProfile {
    bool on = false;
    std::vector<hipEvent_t> ev;      // pairs
    std::vector<double> flops;
    size_t used = 0;
};
static GemmProfile g_prof;
constexpr size_t PROF_MAX_LAUNCHES = 1 << 15;

// The event pair around one GEMM launch: begin() before it, end() after it, both on the launch stream.
struct ProfBracket {
    bool on = false;
    int begin(hipStream_t s, double flops) {
        on = g_prof.on && g_prof.used < PROF_MAX_LAUNCHES;
        if (!on) return 0;
        if (g_prof.ev.size() < 2 * (g_prof.used + 1)) {
            hipEvent_t a, b;
            EXORL_CHECK_HIP(hipEventCreate(&a));
            EXORL_CHECK_HIP(hipEventCreate(&b));
            g_prof.ev.push_back(a);
            g_prof.ev.push_back(b);
        }
        g_prof.flops.push_back(flops);
        EXORL_CHECK_HIP(hipEventRecord(g_prof.ev[2 * g_prof.used], s));
        return 0;
    }
    int end(hipStream_t s) {
        if (!on) return 0;
        EXORL_CHECK_HIP(hipEventRecord(g_prof.ev[2 * g_prof.used + 1], s));
        g_prof.used += 1;
        return 0;
    }
};

constexpr int GEMM_MAX_GROUP = 32;     // problems per launch of the generic kernel (split-K slabs of one layer share a launch)
struct GemmBatch {
    GemmProblem p[GEMM_MAX_GROUP];
    int relu;
    int accumulate;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int TILE = 64;        // BM = BN
constexpr int ROWB = 128;       // bytes per LDS tile row
constexpr int TILEB = TILE * ROWB;

__device__ __forceinline__ int lds_off(int row, int unit) { return row * ROWB + ((unit ^ ((row >> 1) & 7)) << 4); }

// L == 0: element (r,k) at ptr[r*ld + k]   (k contiguous)
// L == 1: element (r,k) at ptr[k*ld + r]   (r contiguous)
template <int L, bool VEC, int KU>
__device__ __forceinline__ void load_tile(const float* __restrict__ ptr, int64_t ld, int R, int K, int r0, int k0,
                                          int tid, float (&reg)[2][KU]) {
    if constexpr (L == 0) {
        const int unit = tid & 7;
        const int k = k0 + unit * KU;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = r0 + (tid >> 3) + 32 * u;
            const float* src = ptr + (int64_t)row * ld + k;
            if constexpr (VEC) {
#pragma unroll
                for (int c = 0; c < KU / 4; ++c) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (row < R && k + 4 * c + 4 <= K) v = *reinterpret_cast<const float4*>(src + 4 * c);
                    reg[u][4 * c + 0] = v.x; reg[u][4 * c + 1] = v.y; reg[u][4 * c + 2] = v.z; reg[u][4 * c + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < KU; ++j) reg[u][j] = (row < R && k + j < K) ? src[j] : 0.f;
            }
        }
    } else {
        const int row = r0 + 2 * (tid & 31);
        const int k = k0 + (tid >> 5) * KU;
#pragma unroll
        for (int j = 0; j < KU; ++j) {
            const float* src = ptr + (int64_t)(k + j) * ld + row;
            if constexpr (VEC) {
                float2 v = make_float2(0.f, 0.f);
                if (k + j < K && row + 2 <= R) v = *reinterpret_cast<const float2*>(src);
                reg[0][j] = v.x; reg[1][j] = v.y;
            } else {
                reg[0][j] = (k + j < K && row < R) ? src[0] : 0.f;
                reg[1][j] = (k + j < K && row + 1 < R) ? src[1] : 0.f;
            }
        }
    }
}

template <int L, int PREC, int KU>
__device__ __forceinline__ void store_tile(unsigned char* lds, int tid, const float (&reg)[2][KU]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int row, unit;
        if constexpr (L == 0) { row = (tid >> 3) + 32 * u; unit = tid & 7; }
        else                  { row = 2 * (tid & 31) + u;  unit = tid >> 5; }
        uint4 w;
        if constexpr (PREC == EXORL_PREC_BF16X6) {      // three planes: hi, mid = bf16(x - hi), lo = bf16(x - hi - mid): images at +0, +2, +4 tiles
            float md[8], lw[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float r1 = bf16_residual(reg[u][j]);
                md[j] = r1;
                lw[j] = bf16_residual(r1);
            }
            uint4 m2, l2;
            m2.x = pack_bf16(md[0], md[1]); m2.y = pack_bf16(md[2], md[3]); m2.z = pack_bf16(md[4], md[5]); m2.w = pack_bf16(md[6], md[7]);
            l2.x = pack_bf16(lw[0], lw[1]); l2.y = pack_bf16(lw[2], lw[3]); l2.z = pack_bf16(lw[4], lw[5]); l2.w = pack_bf16(lw[6], lw[7]);
            *reinterpret_cast<uint4*>(lds + 2 * TILEB + lds_off(row, unit)) = m2;
            *reinterpret_cast<uint4*>(lds + 4 * TILEB + lds_off(row, unit)) = l2;
        }
        if constexpr (PREC == EXORL_PREC_BF16X3) {      // lo image two tiles after the hi image (A_hi B_hi A_lo B_lo)
            uint4 l;
            l.x = pack_bf16(bf16_residual(reg[u][0]), bf16_residual(reg[u][1])); l.y = pack_bf16(bf16_residual(reg[u][2]), bf16_residual(reg[u][3]));
            l.z = pack_bf16(bf16_residual(reg[u][4]), bf16_residual(reg[u][5])); l.w = pack_bf16(bf16_residual(reg[u][6]), bf16_residual(reg[u][7]));
            *reinterpret_cast<uint4*>(lds + 2 * TILEB + lds_off(row, unit)) = l;
        }
        if constexpr (PREC == EXORL_PREC_F32) {
            w.x = __float_as_uint(reg[u][0]); w.y = __float_as_uint(reg[u][1]);
            w.z = __float_as_uint(reg[u][2]); w.w = __float_as_uint(reg[u][3]);
        } else {
            w.x = pack_bf16(reg[u][0], reg[u][1]); w.y = pack_bf16(reg[u][2], reg[u][3]);
            w.z = pack_bf16(reg[u][4], reg[u][5]); w.w = pack_bf16(reg[u][6], reg[u][7]);
        }
        *reinterpret_cast<uint4*>(lds + lds_off(row, unit)) = w;
    }
}

// measured (round 3): one LDS stage pays for three planes (Proto pixels 9.8 -> 9.5 ms, ICM pixels 27.2 -> 22.8 ms per update in bf16x6) and is
// neutral to slightly worse for two (rnd 1528 -> 1514, icm_apt 1186 -> 1172 update()/s): two planes keep the double buffer
template <int PREC, int AL, int BL, bool VEC>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmBatch gb) {
    constexpr int KU = (PREC == EXORL_PREC_F32) ? 4 : 8;   // k elements per 16-byte unit
    constexpr int KPT = KU * 8;                            // k elements per LDS tile
    constexpr bool X3 = PREC == EXORL_PREC_BF16X3, X6 = PREC == EXORL_PREC_BF16X6;
    constexpr int NT = X6 ? 6 : (X3 ? 4 : 2);              // LDS tiles per stage: [A p0][B p0][A p1][B p1][A p2][B p2]
    // two stages; the three-plane mode needs 96 KB, past the 64 KB a static array may have: dynamic there
    extern __shared__ __attribute__((aligned(16))) unsigned char gk_dyn[];
    __shared__ __attribute__((aligned(16))) unsigned char gk_static[X6 ? 16 : 2 * NT * TILEB];
    unsigned char* const smem_base = X6 ? gk_dyn : gk_static;
    auto smem = [&](int stage, int tile) { return smem_base + (stage * NT + tile) * TILEB; };

    const GemmProblem& P = gb.p[blockIdx.z];
    const int M = P.M, N = P.N, K = P.K;
    const int tiles_n = (N + TILE - 1) / TILE;
    const int tiles_m = (M + TILE - 1) / TILE;
    if ((int)blockIdx.x >= tiles_n * tiles_m) return;
    const int m0 = ((int)blockIdx.x / tiles_n) * TILE;
    const int n0 = ((int)blockIdx.x % tiles_n) * TILE;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int h = lane >> 5;

    float ra[2][KU], rb[2][KU];
    f32x16 acc, acc2, acc3;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; acc2[i] = 0.f; acc3[i] = 0.f; }
    // fp32 operands: one accumulator over a long k is a sum of k terms in sequence, about sqrt(k) ulp off (k = 4100, the inverse model of ICM
    // on a 2050-wide observation: 4.3e-6 of max|g| against float64 where the float32 reference has 1.0e-6). Every F32_SLAB k-tiles (256
    // elements) the accumulator is folded into a total instead; up to k = 256 nothing changes, bit for bit. Measured cost: the fp32 state step
    // (1024^3 layers) 1290 -> 1142 steps/s; the split-bf16 modes do not run this code. A separate variant for k > 1024 alone keeps that rate
    // but sums the pixel agents' 39200-wide layers differently from their 512- and 1024-row weight gradients, and the config-4 sharded run's
    // first actor loss (a cancelling mean behind Adam's +-lr first step) then lands 2.1e-4 off float64 where its test allows 1e-4.
    constexpr bool SLAB = PREC == EXORL_PREC_F32;
    constexpr int F32_SLAB = 8;
    f32x16 total;
#pragma unroll
    for (int i = 0; i < 16; ++i) total[i] = 0.f;

    const int nk = (K + KPT - 1) / KPT;
    load_tile<AL, VEC, KU>(P.A, P.lda, M, K, m0, 0, tid, ra);
    load_tile<BL, VEC, KU>(P.B, P.ldb, N, K, n0, 0, tid, rb);
    store_tile<AL, PREC, KU>(smem(0, 0), tid, ra);
    store_tile<BL, PREC, KU>(smem(0, 1), tid, rb);
    __syncthreads();

    const int arow = wm * 32 + (lane & 31);
    const int brow = wn * 32 + (lane & 31);

    // three planes: ONE LDS stage (48 KB, three workgroups per CU) instead of two (96 KB, one workgroup of four waves per CU — one wave per SIMD
    // with nothing to hide a barrier or an LDS round trip behind); the next tile still travels in registers while this one is multiplied
    constexpr bool SS = X6;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = SS ? 0 : (kt & 1);
        if (kt + 1 < nk) {
            load_tile<AL, VEC, KU>(P.A, P.lda, M, K, m0, (kt + 1) * KPT, tid, ra);
            load_tile<BL, VEC, KU>(P.B, P.ldb, N, K, n0, (kt + 1) * KPT, tid, rb);
        }
        const unsigned char* As = smem(cur, 0);
        const unsigned char* Bs = smem(cur, 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 a = *reinterpret_cast<const uint4*>(As + lds_off(arow, 2 * q + h));
            const uint4 b = *reinterpret_cast<const uint4*>(Bs + lds_off(brow, 2 * q + h));
            if constexpr (PREC == EXORL_PREC_F32) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                              acc, 0, 0, 0);
                if constexpr (X3) {
                    const uint4 al = *reinterpret_cast<const uint4*>(As + 2 * TILEB + lds_off(arow, 2 * q + h));
                    const uint4 bl = *reinterpret_cast<const uint4*>(Bs + 2 * TILEB + lds_off(brow, 2 * q + h));
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bl), acc2, 0, 0, 0);
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, b), acc3, 0, 0, 0);
                }
                if constexpr (X6) {       // acc: hi*hi; acc2: hi*mid + mid*hi (~2^-8 of it); acc3: hi*lo + lo*hi + mid*mid (~2^-16)
                    const uint4 am = *reinterpret_cast<const uint4*>(As + 2 * TILEB + lds_off(arow, 2 * q + h));
                    const uint4 bm = *reinterpret_cast<const uint4*>(Bs + 2 * TILEB + lds_off(brow, 2 * q + h));
                    const uint4 al = *reinterpret_cast<const uint4*>(As + 4 * TILEB + lds_off(arow, 2 * q + h));
                    const uint4 bl = *reinterpret_cast<const uint4*>(Bs + 4 * TILEB + lds_off(brow, 2 * q + h));
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bm), acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, am), __builtin_bit_cast(bf16x8, b), acc2, 0, 0, 0);
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bl), acc3, 0, 0, 0);
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, b), acc3, 0, 0, 0);
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, am), __builtin_bit_cast(bf16x8, bm), acc3, 0, 0, 0);
                }
            }
        }
        if constexpr (SLAB) {
            if ((kt & (F32_SLAB - 1)) == F32_SLAB - 1 && kt + 1 < nk) {
#pragma unroll
                for (int i = 0; i < 16; ++i) { total[i] += acc[i]; acc[i] = 0.f; }
            }
        }
        if constexpr (SS) __syncthreads();             // every wave is done reading the stage before it is overwritten
        if (kt + 1 < nk) {
            store_tile<AL, PREC, KU>(smem(SS ? 0 : cur ^ 1, 0), tid, ra);
            store_tile<BL, PREC, KU>(smem(SS ? 0 : cur ^ 1, 1), tid, rb);
        }
        __syncthreads();
    }

    // epilogue: C/D map of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    if constexpr (SLAB) {
        if (nk > F32_SLAB) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += total[i];
        }
    }
    if constexpr (X3) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = (acc2[i] + acc3[i]) + acc[i];      // cross terms first
    }
    if constexpr (X6) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = (acc3[i] + acc2[i]) + acc[i];      // smallest class first
    }
    const int n = n0 + wn * 32 + (lane & 31);
    if (n < N) {
        const float bias = P.bias ? P.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m < M) {
                float v = acc[r] + bias;
                if (gb.relu) v = fmaxf(v, 0.f);
                float* dst = P.C + (int64_t)m * P.ldc + n;
                if (gb.accumulate) v += *dst;
                *dst = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// bf16-operand variant (fast mode): A and B already live in memory as bf16 (written by the producing kernels:
// trunk_fwd -> h1, head_bwd -> dz2, Adam -> W1 shadow), so staging moves half the bytes and does no conversion.
// The per-CU L2->LDS path (~64 B/clk) bounds these 1024^3 layers, so the tile is BM x 64 with BM = 128 when that
// still yields >= 256 workgroups: (128+64) rows of 128 B per k-tile instead of 2 x (64+64).
// Layout-1 operands (reduction index slow) are transposed in registers: 8 k-rows x 2 columns per thread as
// 4-byte loads, v_perm_b32 splits the low/high bf16 into two 16-byte k-contiguous units.
template <int L, int NU, bool GUARD>
__device__ __forceinline__ void load_tile16(const unsigned short* __restrict__ ptr, int64_t ld, int R, int K, int r0, int k0,
                                            int tid, uint4 (&reg)[NU]) {
    if constexpr (L == 0) {
        const int unit = tid & 7;
        const int k = k0 + unit * 8;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int row = r0 + (tid >> 3) + 32 * u;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (!GUARD || (row < R && k + 8 <= K)) v = *reinterpret_cast<const uint4*>(ptr + (int64_t)row * ld + k);
            reg[u] = v;
        }
    } else {       // raw: reg[2g] = k rows 0..3, reg[2g+1] = k rows 4..7, each dword = {col, col+1}; permuted at store time
#pragma unroll
        for (int g = 0; g < NU / 2; ++g) {
            const int row = r0 + 2 * (tid & 31) + 64 * g;
            const int k = k0 + (tid >> 5) * 8;
            uint32_t d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                d[j] = 0u;
                if (!GUARD || (k + j < K && row + 2 <= R)) d[j] = *reinterpret_cast<const uint32_t*>(ptr + (int64_t)(k + j) * ld + row);
            }
            reg[2 * g] = make_uint4(d[0], d[1], d[2], d[3]);
            reg[2 * g + 1] = make_uint4(d[4], d[5], d[6], d[7]);
        }
    }
}

template <int L, int NU>
__device__ __forceinline__ void store_tile16(unsigned char* lds, int tid, const uint4 (&reg)[NU]) {
    if constexpr (L == 0) {
#pragma unroll
        for (int u = 0; u < NU; ++u)
            *reinterpret_cast<uint4*>(lds + lds_off((tid >> 3) + 32 * u, tid & 7)) = reg[u];
    } else {
#pragma unroll
        for (int g = 0; g < NU / 2; ++g) {
            const uint4 lo = reg[2 * g], hi = reg[2 * g + 1];
            uint4 e, o;      // low halves -> column `row`, high halves -> column `row+1`
            e.x = __builtin_amdgcn_perm(lo.y, lo.x, 0x05040100u); e.y = __builtin_amdgcn_perm(lo.w, lo.z, 0x05040100u);
            e.z = __builtin_amdgcn_perm(hi.y, hi.x, 0x05040100u); e.w = __builtin_amdgcn_perm(hi.w, hi.z, 0x05040100u);
            o.x = __builtin_amdgcn_perm(lo.y, lo.x, 0x07060302u); o.y = __builtin_amdgcn_perm(lo.w, lo.z, 0x07060302u);
            o.z = __builtin_amdgcn_perm(hi.y, hi.x, 0x07060302u); o.w = __builtin_amdgcn_perm(hi.w, hi.z, 0x07060302u);
            const int row = 2 * (tid & 31) + 64 * g, unit = tid >> 5;
            *reinterpret_cast<uint4*>(lds + lds_off(row, unit)) = e;
            *reinterpret_cast<uint4*>(lds + lds_off(row + 1, unit)) = o;
        }
    }
}

struct Gemm16Batch {
    Gemm16Problem p[4];
    int relu;
    int accumulate;
    int swizzle;      // 1: XCD-aware tile order (blocks that share an XCD take neighbouring tiles)
    int a_t[4];       // mixed-layout launch (gemm16g_mixed_kernel): problem i reads A as a k image (layout 1)
    int xcd_map;      // 1: 1-D grid, workgroup id -> (problem, tile) so that each XCD owns a compact block of one problem's output
    int count;
};

// Workgroups are dealt to the 8 XCDs round-robin by linear id and every XCD has its own L2, so what an XCD's tiles touch is
// fetched once per XCD over the fabric. With tile order following the id, an XCD ends up needing every problem's whole B
// operand (PMC: 39 MB of fabric reads for a launch whose operands total 12 MB). This mapping gives XCD x = id & 7 the problem
// x / (8/count) and, inside it, one block of an (sm x sn) split of the output, walked row-major by id >> 3: per XCD only a
// 1/sm slice of A and a 1/sn slice of B of ONE problem.
struct XcdTile { int p, tm, tn; bool ok; };
__device__ __forceinline__ XcdTile xcd_tile(int id, int count, int tiles_m, int tiles_n) {
    const int X = 8 / count;                       // XCDs per problem (count in {1, 2, 4})
    const int sm = X == 8 ? 4 : 2, sn = X == 2 ? 1 : 2;
    const int xcd = id & 7, slot = id >> 3;
    const int xq = xcd % X;
    const int bm = tiles_m / sm, bn = tiles_n / sn;
    XcdTile t;
    t.p = xcd / X;
    t.tm = (xq / sn) * bm + slot / bn;
    t.tn = (xq % sn) * bn + slot % bn;
    t.ok = slot < bm * bn;
    return t;
}

template <int AL, int BL, int BM, int NS, bool GUARD>
__global__ __launch_bounds__(256) void gemm16_kernel(const Gemm16Batch gb) {
    constexpr int KPT = 64;                   // bf16 k per LDS tile (128 B rows)
    constexpr int NUA = BM / 32, NUB = 2;     // 16-byte units per thread
    constexpr int MT = BM / 64;               // 32x32 accumulator tiles per wave along M
    __shared__ __attribute__((aligned(16))) unsigned char smem[2][(BM + 64) * ROWB];

    const Gemm16Problem& P = gb.p[blockIdx.z];
    const int M = P.M, N = P.N, K = P.K;
    const int tiles_n = (N + 63) / 64;
    const int tiles_m = (M + BM - 1) / BM;
    const int ntiles = tiles_n * tiles_m;
    if ((int)blockIdx.x >= ntiles) return;
    int tile = blockIdx.x;
    if (gb.swizzle && (ntiles & 7) == 0) {
        // blocks b, b+8, b+16.. share an XCD (round-robin dispatch): give each XCD a contiguous run of tiles so its
        // private L2 holds one A row-panel set and the B panels instead of the whole of A
        const int per = ntiles >> 3;
        tile = (tile & 7) * per + (tile >> 3);
    }
    const int m0 = (tile / tiles_n) * BM;
    const int n0 = (tile % tiles_n) * 64;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int h = lane >> 5;

    static_assert(NS == 2 || NS == 3, "register stages");
    uint4 ra[NS][NUA], rb[NS][NUB];      // NS register stages: loads run NS-1 k-tiles ahead of their LDS store
    f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    const int nk = (K + KPT - 1) / KPT;
    const int arow = wm * (BM / 2) + (lane & 31);
    const int brow = wn * 32 + (lane & 31);
    auto compute = [&](int cur) {
        const unsigned char* As = smem[cur];
        const unsigned char* Bs = smem[cur] + BM * ROWB;
        uint4 af[MT][4], bfr[4];          // all fragment reads of the k-tile first (one exposed LDS latency), then MFMAs
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bfr[q] = *reinterpret_cast<const uint4*>(Bs + lds_off(brow, 2 * q + h));
#pragma unroll
            for (int t = 0; t < MT; ++t) af[t][q] = *reinterpret_cast<const uint4*>(As + lds_off(arow + 32 * t, 2 * q + h));
        }
        __builtin_amdgcn_sched_barrier(0);      // keep the reads batched: hipcc otherwise sinks each pair to its MFMA
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int t = 0; t < MT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[t][q]),
                                                                 __builtin_bit_cast(bf16x8, bfr[q]), acc[t], 0, 0, 0);
    };
    auto issue = [&](auto sc, int kt) {          // loads of k-tile kt into register stage sc (clamped: never past K)
        constexpr int st = decltype(sc)::value;
        const int k0 = (kt < nk ? kt : nk - 1) * KPT;
        load_tile16<AL, NUA, GUARD>(P.A, P.lda, M, K, m0, k0, tid, ra[st]);
        load_tile16<BL, NUB, GUARD>(P.B, P.ldb, N, K, n0, k0, tid, rb[st]);
    };
    auto commit = [&](auto sc, int buf) {        // register stage sc -> LDS buffer buf
        constexpr int st = decltype(sc)::value;
        store_tile16<AL, NUA>(smem[buf], tid, ra[st]);
        store_tile16<BL, NUB>(smem[buf] + BM * ROWB, tid, rb[st]);
    };
    auto step = [&](auto sc, int kt) {           // k-tile kt lives in LDS[kt&1]; tile kt+1 is in stage (sc+1)%NS
        constexpr int st = decltype(sc)::value;
        issue(sc, kt + NS);                      // stage sc was committed last step: refill it NS tiles ahead
        compute(kt & 1);
        if (kt + 1 < nk) commit(std::integral_constant<int, (st + 1) % NS>{}, (kt & 1) ^ 1);
        __syncthreads();
    };
    // prologue: tiles 0..NS-1 in flight, tile 0 committed
    issue(std::integral_constant<int, 0>{}, 0);
    if constexpr (NS > 1) issue(std::integral_constant<int, 1>{}, 1);
    if constexpr (NS > 2) issue(std::integral_constant<int, 2>{}, 2);
    commit(std::integral_constant<int, 0>{}, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += NS) {
        step(std::integral_constant<int, 0>{}, kt);
        if constexpr (NS > 1) { if (kt + 1 >= nk) break; step(std::integral_constant<int, 1>{}, kt + 1); }
        if constexpr (NS > 2) { if (kt + 2 >= nk) break; step(std::integral_constant<int, 2>{}, kt + 2); }
    }

    const int n = n0 + wn * 32 + (lane & 31);
    if (n < N) {
        const float bias = P.bias ? P.bias[n] : 0.f;
        const bool relu = gb.relu != 0;
        if (gb.accumulate) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * (BM / 2) + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < M) {
                        float* dst = P.C + (int64_t)m * P.ldc + n;
                        float v = acc[t][r] + bias;
                        if (relu) v = fmaxf(v, 0.f);
                        *dst = v + *dst;
                    }
                }
        } else {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * (BM / 2) + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (m < M) {
                        float v = acc[t][r] + bias;
                        if (relu) v = fmaxf(v, 0.f);
                        P.C[(int64_t)m * P.ldc + n] = v;
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant for exactly-tiled problems (M, N, K multiples of 64): the production path of the 1024-wide layers.
// Operand tiles go global -> LDS with `global_load_lds_dwordx4` (no VGPR round trip, no ds_write), four stages deep,
// paced by counted s_waitcnt vmcnt + one raw s_barrier per k-tile (the loads of tiles t+1, t+2 stay in flight
// across the barrier). LDS images are lane-linear per wave-instruction; the bank swizzles are applied to the per-lane
// SOURCE address and again on the fragment read:
//   k-contiguous operand ("row image", [row][64 k]):   unit' = unit ^ ((row>>1)&7), fragments by ds_read_b128
//   reduction-slow operand ("k image", [k][64 rows], a straight copy of memory): unit' = unit ^ 4*((k>>1)&1),
//     fragments by ds_read_b64_tr_b16 (hardware transpose: 4 k-rows x 16 columns per 16-lane group), so dgrad and
//     wgrad need no transposed copies of W1 / dZ / H in memory and no register shuffles.
typedef short v4s16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int G16G_NSTG = 4;
constexpr int G16G_IMG = 64 * ROWB;                // 8 KB per operand image

template <bool AT, bool BT, int NSTG = G16G_NSTG, bool X3 = false>
__device__ __forceinline__ void gemm16g_body(const Gemm16Batch& gb, unsigned char* smem) {
    constexpr int IMG = G16G_IMG;

    const Gemm16Problem& P = gb.p[blockIdx.z];
    const int tiles_n = P.N >> 6, ntiles = tiles_n * (P.M >> 6);
    if ((int)blockIdx.x >= ntiles) return;
    int tile = blockIdx.x;
    if (gb.swizzle && (ntiles & 7) == 0) tile = (tile & 7) * (ntiles >> 3) + (tile >> 3);
    const int m0 = (tile / tiles_n) << 6;
    const int n0 = (tile % tiles_n) << 6;
    const int K = P.K;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int h = lane >> 5;
    const int nk = K >> 6;                         // multiple of NSTG (checked by the launcher)

    constexpr int NIMG = X3 ? 4 : 2;               // images per stage: A_hi B_hi [A_lo B_lo]
    f32x16 acc, acc2, acc3;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; acc2[i] = 0.f; acc3[i] = 0.f; }

    // ---- LDS-DMA source pointers: this wave's two 1-KB pieces per operand image (image rows 16*wave+8j + lane/8);
    // everything per-lane is computed once, the k-loop only adds a constant stride
    const unsigned short* src[8];
    int64_t kstep[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int rr = 16 * wave + 8 * j + (lane >> 3), p = lane & 7;
        const int64_t oa = !AT ? (int64_t)(m0 + rr) * P.lda + 8 * (p ^ ((rr >> 1) & 7)) : (int64_t)rr * P.lda + m0 + 8 * (p ^ (4 * ((rr >> 1) & 1)));
        const int64_t ob = !BT ? (int64_t)(n0 + rr) * P.ldb + 8 * (p ^ ((rr >> 1) & 7)) : (int64_t)rr * P.ldb + n0 + 8 * (p ^ (4 * ((rr >> 1) & 1)));
        src[j] = P.A + oa;
        src[2 + j] = P.B + ob;
        if constexpr (X3) { src[4 + j] = P.A_lo + oa; src[6 + j] = P.B_lo + ob; }
    }
    kstep[0] = AT ? 64 * P.lda : 64;
    kstep[1] = BT ? 64 * P.ldb : 64;
    const int piece = 16 * wave * ROWB;            // wave-uniform LDS offset of this wave's pieces inside an image

    // ---- fragment read offsets (per lane, stage-relative; stage and q enter as immediates)
    const int arow = wm * 32 + (lane & 31), brow = wn * 32 + (lane & 31);
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    auto tr_off = [&](int rbase) {      // k image: k-row 8*(g>>1)+qq, columns rbase + 16*(g&1) + 4*pp ..+3
        const int c = rbase + 16 * (g & 1) + 4 * pp;
        return (8 * (g >> 1) + qq) * ROWB + (((c >> 3) ^ (4 * ((qq >> 1) & 1))) << 4) + ((c & 7) << 1);
    };
    int aoff[4], boff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        aoff[q] = AT ? tr_off(wm * 32) + q * 16 * ROWB : lds_off(arow, 2 * q + h);
        boff[q] = BT ? tr_off(wn * 32) + q * 16 * ROWB : lds_off(brow, 2 * q + h);
    }

    auto fill = [&](auto sc) {                     // issue the 4 DMA pieces of the next k-tile into stage sc
        constexpr int st = decltype(sc)::value;
        unsigned char* base = smem + st * NIMG * IMG + piece;
        __builtin_amdgcn_global_load_lds((const void*)src[0], (lds_void*)(base), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)src[1], (lds_void*)(base + 8 * ROWB), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)src[2], (lds_void*)(base + IMG), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)src[3], (lds_void*)(base + IMG + 8 * ROWB), 16, 0, 0);
        src[0] += kstep[0]; src[1] += kstep[0]; src[2] += kstep[1]; src[3] += kstep[1];
        if constexpr (X3) {
            __builtin_amdgcn_global_load_lds((const void*)src[4], (lds_void*)(base + 2 * IMG), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)src[5], (lds_void*)(base + 2 * IMG + 8 * ROWB), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)src[6], (lds_void*)(base + 3 * IMG), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)src[7], (lds_void*)(base + 3 * IMG + 8 * ROWB), 16, 0, 0);
            src[4] += kstep[0]; src[5] += kstep[0]; src[6] += kstep[1]; src[7] += kstep[1];
        }
    };
    auto frag = [&](const unsigned char* img, bool tr, int off) -> bf16x8 {
        if (!tr) return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(img + off));
        const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)(img + off));
        const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)(img + off + 4 * ROWB));
        typedef short v8s16 __attribute__((ext_vector_type(8)));
        const v8s16 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        return __builtin_bit_cast(bf16x8, v);
    };
    auto step = [&](auto sc, int t) {              // k-tile t sits in stage sc
        constexpr int st = decltype(sc)::value;
        // tile t has landed once at most the fills of the two younger tiles remain outstanding (4 DMA pieces per tile per wave)
        const int younger = nk - 1 - t;            // NSTG - 2 younger tiles may still be in flight
        const int allowed = younger < NSTG - 2 ? younger : NSTG - 2;
#define EXORL_WAITC(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
        if constexpr (X3) {
            switch (allowed) {
                case 0: EXORL_WAITC(0); break;
                case 1: EXORL_WAITC(8); break;
                case 2: EXORL_WAITC(16); break;
                case 3: EXORL_WAITC(24); break;
                case 4: EXORL_WAITC(32); break;
                case 5: EXORL_WAITC(40); break;
                default: EXORL_WAITC(48); break;
            }
        } else {
            switch (allowed) {
                case 0: EXORL_WAITC(0); break;
                case 1: EXORL_WAITC(4); break;
                case 2: EXORL_WAITC(8); break;
                case 3: EXORL_WAITC(12); break;
                case 4: EXORL_WAITC(16); break;
                case 5: EXORL_WAITC(20); break;
                case 6: EXORL_WAITC(24); break;
                case 7: EXORL_WAITC(28); break;
                default: EXORL_WAITC(32); break;
            }
        }
#undef EXORL_WAITC
        __builtin_amdgcn_s_barrier();              // every wave's pieces of tile t are in LDS; stage st-1 is no longer being read
        asm volatile("" ::: "memory");
        if (t + NSTG - 1 < nk) fill(std::integral_constant<int, (st + NSTG - 1) % NSTG>{});
        const unsigned char* As = smem + st * NIMG * IMG;
        const unsigned char* Bs = As + IMG;
        bf16x8 af[4], bfr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            af[q] = frag(As, AT, aoff[q]);
            bfr[q] = frag(Bs, BT, boff[q]);
        }
        if constexpr (X3) {                        // hi*hi + hi*lo + lo*hi, three independent accumulators
            bf16x8 al[4], bl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                al[q] = frag(As + 2 * IMG, AT, aoff[q]);
                bl[q] = frag(Bs + 2 * IMG, BT, boff[q]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[q], bfr[q], acc, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[q], bl[q], acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[q], bfr[q], acc3, 0, 0, 0);
            }
            return;
        }
        __builtin_amdgcn_sched_barrier(0);
        // two independent accumulation chains: PMC shows ~36 % of wave cycles as MFMA issue stalls (SQ_WAIT_INST_ANY)
        // when all four MFMAs of a k-tile chain through one accumulator
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bfr[0], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bfr[1], acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], bfr[2], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[3], bfr[3], acc2, 0, 0, 0);
    };

    static_assert(NSTG >= 2 && NSTG <= 10 && (X3 ? NSTG <= 8 : true), "stage count out of range of the vmcnt table");
#define EXORL_FILL0(I) if constexpr (NSTG > I + 1) { if (I < nk) fill(std::integral_constant<int, I>{}); }
    EXORL_FILL0(0) EXORL_FILL0(1) EXORL_FILL0(2) EXORL_FILL0(3) EXORL_FILL0(4) EXORL_FILL0(5) EXORL_FILL0(6) EXORL_FILL0(7) EXORL_FILL0(8)
#undef EXORL_FILL0
    int t = 0;
#define EXORL_STEP(I) if constexpr (NSTG > I) step(std::integral_constant<int, I>{}, t + I);
    for (; t + NSTG <= nk; t += NSTG) {
        EXORL_STEP(0) EXORL_STEP(1) EXORL_STEP(2) EXORL_STEP(3) EXORL_STEP(4) EXORL_STEP(5) EXORL_STEP(6) EXORL_STEP(7) EXORL_STEP(8) EXORL_STEP(9)
    }
#undef EXORL_STEP
#define EXORL_TAIL(I) if constexpr (NSTG > I + 1) { if (t + I < nk) step(std::integral_constant<int, I>{}, t + I); }     // nk % NSTG tail
    EXORL_TAIL(0) EXORL_TAIL(1) EXORL_TAIL(2) EXORL_TAIL(3) EXORL_TAIL(4) EXORL_TAIL(5) EXORL_TAIL(6) EXORL_TAIL(7) EXORL_TAIL(8)
#undef EXORL_TAIL

#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = X3 ? (acc2[i] + acc3[i]) + acc[i] : acc[i] + acc2[i];      // small terms first
    const int n = n0 + wn * 32 + (lane & 31);
    const float bias = P.bias ? P.bias[n] : 0.f;
    const bool relu = gb.relu != 0;
    float* crow = P.C + (int64_t)(m0 + wm * 32 + 4 * h) * P.ldc + n;
    if (gb.accumulate) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* dst = crow + (int64_t)((r & 3) + 8 * (r >> 2)) * P.ldc;
            float v = acc[r] + bias;
            if (relu) v = fmaxf(v, 0.f);
            *dst = v + *dst;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r] + bias;
            if (relu) v = fmaxf(v, 0.f);
            crow[(int64_t)((r & 3) + 8 * (r >> 2)) * P.ldc] = v;
        }
    }
}

// ---- "p" kernels: 128 x TN workgroup tile (TN = 128 or 64), k32 stages, 4-deep LDS-DMA ring, XCD-local tile blocks -----------
// Why a wave owns 64 x TN/2 of output here: the 64 x 64 kernel above re-reads every operand byte from LDS for 32 x 32 of output per wave, 8 KB
// of ds_read per 4 MFMAs, twice what the CU's 128 B/clk LDS port can feed while the MFMAs run (PMC: the pipe is LDS-bound). A 64 x 64 wave
// tile reuses each fragment twice (16 KB per 16 MFMAs: LDS and MFMA time balance) and halves the L2->LDS bytes per FLOP.
// What round 2's measurements changed (tools/micro/fill_bench.hip): a CU pulls ~115 GB/s from its XCD's L2 on EVERY path (LDS-DMA,
// registers, both) but only 30-40 GB/s from the Infinity Cache, so the ~75 GB/s the kernels above sustain is an L2 miss rate, not a
// DMA limit: with tiles dealt in id order an XCD walks one tile-row of every problem and re-fetches each B strip once per tile.
// Here (a) workgroup id -> tile goes through xcd_tile(): the 32 workgroups of an XCD (one per CU, all resident) form a compact block
// of ONE problem's output (512 x 512 or 512 x 1024), so every operand strip an XCD touches is fetched once and reused 4-8 times while
// the CUs walk k together; (b) the stage is 32 k wide (32 KB for a split-bf16 128 x 128 tile), four stages deep: two to three
// stages are always in flight, which a single workgroup per CU needs to cover the DMA latency (the 2 x 64 KB ring of the round-1
// 128 x 128 kernels, since removed, could keep only one); (c) the k-loop is software-pipelined across the barrier: the fragments of the next k16 are read while the MFMAs of the
// current one issue, the barrier that certifies stage t+1 sits in the middle of step t.
// LDS images per 64-row block and stage (4 KB): "row image" [64 rows][32 k] with 64-byte rows, 16-byte units swizzled by
// (row >> 2) & 3 (the 16 lanes of a ds_read_b128 group then hit 16 distinct bank quads); "k image" [32 k][64 rows] = the first half
// of the 64-k image above (same swizzle, same ds_read_b64_tr_b16 fragments).

template <int I, int N, typename F>
__device__ __forceinline__ void g16p_static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); g16p_static_for<I + 1, N>(f); }
}

// ds_read_b64_tr_b16 through inline asm: the builtin carries no memory operand, so the compiler assumes it may read what an LDS-DMA
// still in flight is writing and puts an s_waitcnt vmcnt(0) in front of it — which also waits for the stage that was issued a moment
// ago, i.e. no prefetch at all for the transposed operands. The asm form is invisible to that pass; its results are fenced by
// g16p_lds_fence() (an lgkmcnt(0) that names them) before the MFMAs of the next region read them. The two 64-bit halves stay separate
// variables until that fence: a register move the compiler makes to pack them earlier would copy registers the LDS has not written yet.
template <int IMM>
__device__ __forceinline__ v4s16 g16p_read_tr(unsigned addr) {
    v4s16 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(IMM));
    return r;
}
struct G16pFrag {
    bf16x8 v;            // MFMA operand (row-image fragments are read straight into it)
    v4s16 lo, hi;        // k-image fragments: the two transposed 64-bit reads, packed into v by the fence
};
__device__ __forceinline__ void g16p_lds_fence(G16pFrag& f) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.lo), "+v"(f.hi));
    typedef short v8s16 __attribute__((ext_vector_type(8)));
    const v8s16 v = {f.lo.x, f.lo.y, f.lo.z, f.lo.w, f.hi.x, f.hi.y, f.hi.z, f.hi.w};
    f.v = __builtin_bit_cast(bf16x8, v);
}

// KS = k per stage (32: 64-byte row-image rows = half cache lines, four stages fit the 128 x 128 split-bf16 tile; 64: whole lines, the
// 64-wide images and swizzle of the gemm16g kernels above), NSTG = ring depth. A stage's slot is refilled with the stage NSTG ahead as soon
// as its last fragments have been read, i.e. behind the barrier that opens the stage's last k16.
// The refill of a stage slot is spread over two consecutive k-regions. Stamps of the in-kernel clock (a diagnostic build removed after
// commit d23b35a) put the k-loop at MFMA cycles + ~60 cycles per DMA piece of the wave: the four waves issue their pieces together, the
// CU's vector-memory path takes them one at a time, and a wave blocked on an issue cannot feed its matrix pipe. Spread over two regions
// the same pieces have twice the MFMAs to hide behind.
// NPL = operand planes: 1 plain bf16; 2 split bf16 (hi, lo: hi*hi + hi*lo + lo*hi); 3 three-plane split (hi, mid, lo: + mid*hi + hi*mid in the
// second accumulator class, hi*lo + lo*hi + mid*mid in a third; Gemm16Problem::A_mid). Three planes at TN = 64, KS = 32, NSTG = 4 are
// (128 + 64) rows x 64 B x 3 x 4 = 144 KB of the 160 KB of LDS, 9 DMA pieces per wave and stage, 12 MFMAs and 9 fragments per k16.
template <bool AT, bool BT, int NPL, int TN, int KS, int NSTG>
__device__ __forceinline__ void gemm16p_body(const Gemm16Batch& gb, unsigned char* smem, int pidx, int m0, int n0) {
    constexpr int NW = 4, NBA = 2, NBB = TN / 64;
    constexpr bool X3 = NPL == 2, X6 = NPL == 3;
    static_assert(NPL >= 1 && NPL <= 3, "operand planes");
    constexpr int WR = 64, WC = TN / 2;                     // wave tile: WR rows x WC columns
    constexpr int WN = TN / WC;                             // waves along N (the rest along M)
    constexpr int BLK = 64 * 2 * KS;                        // one 64-row block of one plane and stage (either image kind)
    constexpr int PLANE = (NBA + NBB) * BLK;                // [A blk0][A blk1][B blk0][B blk1]
    constexpr int STAGE = NPL * PLANE;                      // hi plane, then (mid plane and) lo plane
    constexpr int PPW = KS / 8 / NW;                        // 1-KB DMA pieces per wave and block
    constexpr int NP = (NBA + NBB) * NPL * PPW;             // DMA pieces per wave and stage
    constexpr int NQ = KS / 16;                             // regions (k16) per stage
    constexpr int SA = WR / 32;                             // 32-row sub-tiles of a wave along M
    constexpr int SB = WC / 32;                             // 32-column sub-tiles of a wave along N
    constexpr int NPAIR = SA * SB;                          // 32 x 32 accumulators of a wave
    constexpr int TERMS = X6 ? 6 : (X3 ? 3 : 1);            // plane products formed per accumulator tile
    constexpr int NM = NPAIR * TERMS;                       // MFMAs per region
    constexpr int NF = (SA + SB) * NPL;                     // fragments per region
    constexpr int SMIN = SA < SB ? SA : SB;
    typedef float acc_t __attribute__((ext_vector_type(16)));
    constexpr int FPG = (NF + NM - 2) / (NM - 1);           // fragments read per MFMA gap: all of them behind the first NM-1 MFMAs
    static_assert(NQ % 2 == 0 && NP * (NSTG - 1) <= 63 && NSTG >= 2, "stage geometry");
    const Gemm16Problem& P = gb.p[pidx];
    const int nst = P.K / KS;                               // multiple of NSTG, >= NSTG (launcher)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int h = lane >> 5;
    const int arow0 = (wm * WR) & 63, ablk = (wm * WR) >> 6;        // this wave's rows inside A block ablk
    const int bcol0 = (wn * WC) & 63, bblk = (wn * WC) >> 6;        // this wave's columns inside B block bblk

    // [ua * SB + ub]; accx: the cross terms with the second plane (hi*lo + lo*hi; three planes: hi*mid + mid*hi); accy: three planes' third
    // class hi*lo + lo*hi + mid*mid
    acc_t acc[NPAIR], accx[NPL > 1 ? NPAIR : 1], accy[X6 ? NPAIR : 1];
#pragma unroll
    for (int a = 0; a < NPAIR; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[a][i] = 0.f; if constexpr (NPL > 1) accx[a][i] = 0.f; if constexpr (X6) accy[a][i] = 0.f; }

    // row image: 2*KS-byte rows, 16-byte units swizzled so that the 16 lanes of a ds_read_b128 group hit 16 distinct bank quads
    auto row_off = [](int row, int unit) {
        if constexpr (KS == 32) return row * 64 + ((unit ^ ((row >> 2) & 3)) << 4);
        else return lds_off(row, unit);
    };
    // ---- DMA sources: this wave's pieces (index wave + 4 j) of every block; per-lane addresses carry the LDS swizzle
    const unsigned short* src[NP];
    {
        constexpr int U = KS / 8, RP = 64 / U;              // row image: 16-byte units per row, rows per 1-KB piece
        const int rr = lane / U, ur = lane % U;
        const int r8 = lane >> 3, u8 = lane & 7;            // k image piece: 8 k-rows x 8 units
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int b = 0; b < NBA + NBB; ++b)
#pragma unroll
                for (int j = 0; j < PPW; ++j) {
                    const int pc = wave + NW * j;
                    const bool isA = b < NBA;
                    const bool tr = isA ? AT : BT;
                    const int64_t ld = isA ? P.lda : P.ldb;
                    const int r0 = (isA ? m0 : n0) + 64 * (isA ? b : b - NBA);
                    const int irow = pc * RP + rr;          // row inside the 64-row block
                    const int usrc = KS == 32 ? (ur ^ ((irow >> 2) & 3)) : (ur ^ ((irow >> 1) & 7));
                    const int64_t o = !tr ? (int64_t)(r0 + irow) * ld + 8 * usrc
                                          : (int64_t)(8 * pc + r8) * ld + r0 + 8 * (u8 ^ (4 * ((r8 >> 1) & 1)));
                    // plane order in LDS: hi, [mid,] lo
                    const unsigned short* base = isA ? (pl == 0 ? P.A : (X6 && pl == 1 ? P.A_mid : P.A_lo)) : (pl == 0 ? P.B : (X6 && pl == 1 ? P.B_mid : P.B_lo));
                    src[(pl * (NBA + NBB) + b) * PPW + j] = base + o;
                }
    }
    const int64_t kstepA = AT ? KS * P.lda : KS, kstepB = BT ? KS * P.ldb : KS;

    // ---- fragment offsets inside a stage's hi plane (the next planes: + PLANE each)
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    auto tr_off = [&](int rbase) {      // k image: k-row 8*(g>>1)+qq (+4 for the second half), columns rbase + 16*(g&1) + 4*pp ..+3
        const int c = rbase + 16 * (g & 1) + 4 * pp;
        return (8 * (g >> 1) + qq) * ROWB + (((c >> 3) ^ (4 * ((qq >> 1) & 1))) << 4) + ((c & 7) << 1);
    };
    int aoff[SA][NQ], boff[SB][NQ];                 // [sub-tile][q]
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int u = 0; u < SA; ++u)
            aoff[u][q] = ablk * BLK + (AT ? tr_off(arow0 + u * 32) + q * 16 * ROWB : row_off(arow0 + u * 32 + (lane & 31), 2 * q + h));
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int r0 = bcol0 + u * 32;
            boff[u][q] = (NBA + bblk) * BLK + (BT ? tr_off(r0) + q * 16 * ROWB : row_off(r0 + (lane & 31), 2 * q + h));
        }
    }

    auto fill_one = [&](int st, auto ic) {          // DMA piece I of stage slot st
        constexpr int I = decltype(ic)::value;
        constexpr int j = I % PPW, b = (I / PPW) % (NBA + NBB), pl = I / (PPW * (NBA + NBB));
        __builtin_amdgcn_global_load_lds((const void*)src[I], (lds_void*)(smem + st * STAGE + pl * PLANE + b * BLK + (wave + NW * j) * 1024), 16, 0, 0);
        src[I] += b < NBA ? kstepA : kstepB;
    };
    auto fill = [&](int st) { g16p_static_for<0, NP>([&](auto ic) { fill_one(st, ic); }); };

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;       // LDS byte address of the ring
    auto frag = [&](G16pFrag& f, auto plane, bool tr, int st, int off) {     // plane 0 = hi, 1 = lo (three planes: 1 = mid, 2 = lo)
        constexpr int PL = decltype(plane)::value * PLANE;
        if (!tr) { f.v = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(smem + st * STAGE + PL + off)); return; }
        const unsigned a = lds0 + st * STAGE + off;
        f.lo = g16p_read_tr<PL>(a);
        f.hi = g16p_read_tr<PL + 4 * ROWB>(a);
    };
    struct Frags { G16pFrag ah[SA], bh[SB], al[NPL > 1 ? SA : 1], bl[NPL > 1 ? SB : 1], at[X6 ? SA : 1], bt[X6 ? SB : 1]; };     // planes 0, 1, 2
    // fragment J of a region, in the order the MFMAs want them: per plane A0 B0 A1 B1 ... interleaved, then the rest of the longer list
    auto read_one = [&](Frags& f, int st, auto qc, auto jc) {
        constexpr int J = decltype(jc)::value, q = decltype(qc)::value;
        constexpr int pl = J % NPL, k = J / NPL;                         // k: 0 = A0, 1 = B0, 2 = A1, 3 = B1, ...
        constexpr bool isA = k < 2 * SMIN ? k % 2 == 0 : SA > SB;
        constexpr int u = k < 2 * SMIN ? k / 2 : k - SMIN;
        if constexpr (isA) {
            if constexpr (pl == 0) frag(f.ah[u], std::integral_constant<int, 0>{}, AT, st, aoff[u][q]);
            else if constexpr (pl == 1) frag(f.al[u], std::integral_constant<int, 1>{}, AT, st, aoff[u][q]);
            else frag(f.at[u], std::integral_constant<int, 2>{}, AT, st, aoff[u][q]);
        } else {
            if constexpr (pl == 0) frag(f.bh[u], std::integral_constant<int, 0>{}, BT, st, boff[u][q]);
            else if constexpr (pl == 1) frag(f.bl[u], std::integral_constant<int, 1>{}, BT, st, boff[u][q]);
            else frag(f.bt[u], std::integral_constant<int, 2>{}, BT, st, boff[u][q]);
        }
    };
    auto fence = [&](Frags& f) {               // the asm-issued transposed reads of f have landed (see g16p_read_tr)
        if constexpr (AT) {
#pragma unroll
            for (int u = 0; u < SA; ++u) { g16p_lds_fence(f.ah[u]); if constexpr (NPL > 1) g16p_lds_fence(f.al[u]); if constexpr (X6) g16p_lds_fence(f.at[u]); }
        }
        if constexpr (BT) {
#pragma unroll
            for (int u = 0; u < SB; ++u) { g16p_lds_fence(f.bh[u]); if constexpr (NPL > 1) g16p_lds_fence(f.bl[u]); if constexpr (X6) g16p_lds_fence(f.bt[u]); }
        }
    };
    // MFMA I of a k16. Operands swapped: the accumulator is the TRANSPOSED 32 x 32 block, i.e. lane = output row, registers r..r+3 =
    // four consecutive output columns -> the epilogue stores 16 bytes per lane (16 stores per wave instead of 64)
    auto mfma_one = [&](const Frags& f, auto ic) {
        constexpr int I = decltype(ic)::value;
        constexpr int pair = I / TERMS, term = I % TERMS, ua = pair / SB, ub = pair % SB;
        if constexpr (term == 0) acc[pair] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.bh[ub].v, f.ah[ua].v, acc[pair], 0, 0, 0);
        else if constexpr (term == 1) accx[pair] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.bl[ub].v, f.ah[ua].v, accx[pair], 0, 0, 0);
        else if constexpr (term == 2) accx[pair] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.bh[ub].v, f.al[ua].v, accx[pair], 0, 0, 0);
        // three planes (al / bl hold mid, at / bt hold lo): A_hi B_lo, A_lo B_hi, A_mid B_mid
        else if constexpr (term == 3) accy[pair] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.bt[ub].v, f.ah[ua].v, accy[pair], 0, 0, 0);
        else if constexpr (term == 4) accy[pair] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.bh[ub].v, f.at[ua].v, accy[pair], 0, 0, 0);
        else accy[pair] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.bl[ub].v, f.al[ua].v, accy[pair], 0, 0, 0);
    };
    // One scheduling region = the NM MFMAs of a k16 on `cur`, with the reads of the NEXT k16's fragments (stage slot nst_, region NQn) into
    // `nxt` (FPG per MFMA gap) and, when NFILL > 0, this region's half (chunk) of the DMA issues of stage slot `fst` written out between them; sched_barrier(0)
    // after every piece keeps the machine scheduler from regrouping them (left alone it sinks the reads to just before their use; issued
    // as one block they exceed the 4-bit lgkmcnt and the compiler waits for all of them). The reads complete in the shadow of the matrix
    // pipe, the next region opens with waits that cost nothing.
    auto region = [&](Frags& cur, Frags& nxt, auto has_next, int nst_, auto nq, auto nfill, int fst, auto chunk) {
        constexpr bool HN = decltype(has_next)::value;
        constexpr int NFILL = decltype(nfill)::value;
        constexpr int F0 = decltype(chunk)::value * NP / 2, F1 = (decltype(chunk)::value + 1) * NP / 2;      // this region's share of the refill
        g16p_static_for<0, NM>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            mfma_one(cur, ic);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (HN) g16p_static_for<I * FPG, ((I + 1) * FPG < NF ? (I + 1) * FPG : NF)>([&](auto jc) { read_one(nxt, nst_, nq, jc); });
            constexpr int PPG = (F1 - F0 + NM - 1) / NM;     // DMA pieces per gap
            if constexpr (NFILL > 0)
                g16p_static_for<F0 + I * PPG, (F0 + (I + 1) * PPG < F1 ? F0 + (I + 1) * PPG : F1)>([&](auto pc) { fill_one(fst, pc); });
            __builtin_amdgcn_sched_barrier(0);
        });
        // The fence of the fragments just requested closes the region that issued them — the same place in the instruction stream as the head
        // of the next region, but inside the same basic block. Round 2 had it at the head of the consuming region: wherever a branch or a loop
        // back-edge lay between the two (the nst == NSTG test behind the prologue reads, the group loop) the register allocator was free to
        // resolve the join with v_mov copies of the asm outputs BEFORE the wait, i.e. copies of registers the LDS had not written yet
        // (tools/check_async_reads.py shows them in the round-2 ISA of every SPREAD = 2 kernel with a k-image operand, split-bf16 included;
        // the plain-bf16 launches — 2-4 MFMAs between the reads and the copy — lost that race visibly: DESIGN 4, "the SPREAD = 2 anomaly").
        if constexpr (HN) fence(nxt);
    };
    // a stage has landed for this wave once at most `younger` younger stages' pieces are outstanding (NP per stage)
    auto wait_landed = [&](auto younger) {
        constexpr int y = decltype(younger)::value;
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(y * NP) : "memory");
    };
    Frags fr[2];
    using T = std::true_type;
    using F = std::false_type;
    using NoFill = std::integral_constant<int, 0>;
    using Fill = std::integral_constant<int, NP>;
    // NSTG stages on slots 0..NSTG-1; LAST = the final group (nothing left to refill, no barrier after the last stage). Every condition is
    // a compile-time constant: a run-time branch in here makes the compiler fall back to lgkmcnt(0) / vmcnt(0)
    using C0 = std::integral_constant<int, 0>;
    auto group = [&](auto first, auto last) {
        constexpr bool FIRST = decltype(first)::value, LAST = decltype(last)::value;
        g16p_static_for<0, NSTG>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            // the refill the previous stage began behind its barrier (chunk 0) continues in this stage's first region
            constexpr bool PENDING = s > 0 ? !LAST : !FIRST;
            g16p_static_for<0, NQ - 1>([&](auto qc) {        // all but the last k16 of the stage: read the next k16 of the same stage
                constexpr int q = decltype(qc)::value;
                if constexpr (PENDING && q == 0)
                    region(fr[q & 1], fr[(q + 1) & 1], T{}, s, std::integral_constant<int, q + 1>{}, Fill{}, (s + NSTG - 1) % NSTG, std::integral_constant<int, 1>{});
                else
                    region(fr[q & 1], fr[(q + 1) & 1], T{}, s, std::integral_constant<int, q + 1>{}, NoFill{}, 0, C0{});
            });
            Frags& cur = fr[(NQ - 1) & 1];
            Frags& nxt = fr[NQ & 1];
            if constexpr (!LAST || s < NSTG - 1) {
                // the next stage has landed for this wave when only the stages younger than it are outstanding: NSTG-2 of them in the steady
                // state, NSTG-2-s in the last group (nothing is issued there any more)
                wait_landed(std::integral_constant<int, LAST ? NSTG - 2 - s : NSTG - 2>{});
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's reads of stage s are done: its slot may be refilled
                __builtin_amdgcn_s_barrier();                           // ... by anyone; and the next stage has landed for everyone
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (!LAST) region(cur, nxt, T{}, (s + 1) % NSTG, std::integral_constant<int, 0>{}, Fill{}, s, C0{});
                else region(cur, nxt, T{}, (s + 1) % NSTG, std::integral_constant<int, 0>{}, NoFill{}, 0, C0{});
            } else {
                region(cur, nxt, F{}, 0, std::integral_constant<int, 0>{}, NoFill{}, 0, C0{});
            }
        });
    };

    g16p_static_for<0, NSTG>([&](auto sc) { fill(decltype(sc)::value); });
    wait_landed(std::integral_constant<int, NSTG - 1>{});
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    g16p_static_for<0, NF>([&](auto jc) { read_one(fr[0], 0, std::integral_constant<int, 0>{}, jc); });
    fence(fr[0]);                               // before any control flow (see region())
    if (nst == NSTG) {
        group(T{}, T{});
    } else {
        group(T{}, F{});
        for (int t = NSTG; t + NSTG < nst; t += NSTG) group(F{}, F{});
        group(F{}, T{});
    }

    const bool relu = gb.relu != 0;
    // the accumulator classes of output element (pair, i), smallest class first
    auto total = [&](int pair, int i) {
        if constexpr (X6) return (accy[pair][i] + accx[pair][i]) + acc[pair][i];
        else if constexpr (X3) return accx[pair][i] + acc[pair][i];
        else return acc[pair][i];
    };
    if (P.head_part) {
        // folded scalar head: this wave's share of relu(acc + bias) . head_w for each of its rows; lanes l and l + 32 hold the two column
        // interleaves of one row. Nothing of C is stored.
#pragma unroll
        for (int ta = 0; ta < SA; ++ta) {
            float dot = 0.f;
#pragma unroll
            for (int tb = 0; tb < SB; ++tb) {
                const int nb = n0 + wn * WC + tb * 32 + 4 * h;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 bias = P.bias ? *reinterpret_cast<const float4*>(P.bias + nb + 8 * g4) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 w = *reinterpret_cast<const float4*>(P.head_w + nb + 8 * g4);
                    float4 v;
                    v.x = total(ta * SB + tb, 4 * g4 + 0) + bias.x;
                    v.y = total(ta * SB + tb, 4 * g4 + 1) + bias.y;
                    v.z = total(ta * SB + tb, 4 * g4 + 2) + bias.z;
                    v.w = total(ta * SB + tb, 4 * g4 + 3) + bias.w;
                    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    dot += (v.x * w.x + v.y * w.y) + (v.z * w.z + v.w * w.w);
                }
            }
            dot += __shfl_xor(dot, 32);
            if (h == 0) P.head_part[(int64_t)(m0 + wm * WR + ta * 32 + (lane & 31)) * (P.N / WC) + (n0 / WC + wn)] = dot;
        }
    } else {
#pragma unroll
    for (int ta = 0; ta < SA; ++ta)
#pragma unroll
        for (int tb = 0; tb < SB; ++tb) {
            // lane: output row m0 + .. + (lane & 31); registers 4g..4g+3: columns nb + 8g + 4h .. +3
            const int nb = n0 + wn * WC + tb * 32 + 4 * h;
            float* crow = P.C + (int64_t)(m0 + wm * WR + ta * 32 + (lane & 31)) * P.ldc + nb;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                if (P.n_store && nb + 8 * g4 >= P.n_store) continue;        // columns of the padded operand planes that C does not have
                float4* dst = reinterpret_cast<float4*>(crow + 8 * g4);
                const float4 bias = P.bias ? *reinterpret_cast<const float4*>(P.bias + nb + 8 * g4) : make_float4(0.f, 0.f, 0.f, 0.f);
                float4 v;
                v.x = total(ta * SB + tb, 4 * g4 + 0) + bias.x;
                v.y = total(ta * SB + tb, 4 * g4 + 1) + bias.y;
                v.z = total(ta * SB + tb, 4 * g4 + 2) + bias.z;
                v.w = total(ta * SB + tb, 4 * g4 + 3) + bias.w;
                if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                if (gb.accumulate) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                *dst = v;
            }
        }
    }
}
// workgroup id -> (problem, tile origin): XCD-local blocks when the launcher found the problems uniform, id order otherwise
template <int TN>
__device__ __forceinline__ bool g16p_tile(const Gemm16Batch& gb, int& pidx, int& m0, int& n0) {
    constexpr int SH = TN == 128 ? 7 : 6;
    if (gb.xcd_map) {
        const XcdTile xt = xcd_tile(blockIdx.x, gb.count, gb.p[0].M >> 7, gb.p[0].N >> SH);
        if (!xt.ok) return false;
        pidx = xt.p; m0 = xt.tm << 7; n0 = xt.tn << SH;
        return true;
    }
    pidx = blockIdx.z;
    const int tiles_n = gb.p[pidx].N >> SH, ntiles = tiles_n * (gb.p[pidx].M >> 7);
    if ((int)blockIdx.x >= ntiles) return false;
    m0 = ((int)blockIdx.x / tiles_n) << 7;
    n0 = ((int)blockIdx.x % tiles_n) << SH;
    return true;
}

template <bool AT, bool BT, int NPL, int TN, int KS = 32, int NSTG = 4>
__global__ __launch_bounds__(256) void gemm16p_kernel(const Gemm16Batch gb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_p[];
    int pidx, m0, n0;
    if (!g16p_tile<TN>(gb, pidx, m0, n0)) return;
    gemm16p_body<AT, BT, NPL, TN, KS, NSTG>(gb, smem_p, pidx, m0, n0);
}

template <int NPL, int TN>      // wgrad (A as a k image) and dgrad (A as a row image) of one Linear(H,H) in one launch; B is a k image in both
__global__ __launch_bounds__(256) void gemm16p_mixed_kernel(const Gemm16Batch gb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_p[];
    int pidx, m0, n0;
    if (!g16p_tile<TN>(gb, pidx, m0, n0)) return;
    if (gb.a_t[pidx]) gemm16p_body<true, true, NPL, TN, 32, 4>(gb, smem_p, pidx, m0, n0);
    else gemm16p_body<false, true, NPL, TN, 32, 4>(gb, smem_p, pidx, m0, n0);
}
constexpr int g16p_lds(int npl, int tn, int ks = 32, int nstg = 4) { return nstg * npl * (2 + tn / 64) * 64 * 2 * ks; }
static_assert(g16p_lds(3, 64) == 147456, "three planes, 128 x 64 tile, four k32 stages");

static bool g16p_uniform(const Gemm16Batch& gb, int count, int tn) {       // xcd_tile()'s preconditions
    if (!(count == 1 || count == 2 || count == 4)) return false;
    const int X = 8 / count, sm = X == 8 ? 4 : 2, sn = X == 2 ? 1 : 2;
    for (int i = 0; i < count; ++i) {
        if (gb.p[i].M != gb.p[0].M || gb.p[i].N != gb.p[0].N) return false;
        if ((gb.p[i].M / 128) % sm != 0 || (gb.p[i].N / tn) % sn != 0) return false;
    }
    return true;
}
template <typename K>
static int g16p_launch(K kernel, Gemm16Batch& gb, int count, int npl, int tn, hipStream_t s, int ks = 32, int nstg = 4) {
    const int lds = g16p_lds(npl, tn, ks, nstg);
    static std::vector<const void*> enabled;         // > 64 KB of dynamic LDS needs the opt-in, once per kernel
    if (std::find(enabled.begin(), enabled.end(), (const void*)kernel) == enabled.end()) {
        EXORL_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        enabled.push_back((const void*)kernel);
    }
    gb.count = count;
    gb.xcd_map = g16p_uniform(gb, count, tn) ? 1 : 0;
    int tmax = 0, ttot = 0;
    for (int i = 0; i < count; ++i) { const int t = (gb.p[i].M >> 7) * (gb.p[i].N / tn); tmax = t > tmax ? t : tmax; ttot += t; }
    hipLaunchKernelGGL(kernel, gb.xcd_map ? dim3(ttot, 1, 1) : dim3(tmax, 1, count), dim3(256), lds, s, gb);
    return 0;
}

template <bool AT, bool BT, int NSTG = G16G_NSTG>
__global__ __launch_bounds__(256) void gemm16g_kernel(const Gemm16Batch gb) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[NSTG * 2 * G16G_IMG];
    gemm16g_body<AT, BT, NSTG>(gb, smem);
}

// split-bf16 operands (Gemm16Problem::A_lo / B_lo): 2 stages x 4 images = 64 KB of LDS, two workgroups per CU
template <bool AT, bool BT>
__global__ __launch_bounds__(256) void gemm16x3_kernel(const Gemm16Batch gb) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 4 * G16G_IMG];
    gemm16g_body<AT, BT, 2, true>(gb, smem);
}
__global__ __launch_bounds__(256) void gemm16x3_mixed_kernel(const Gemm16Batch gb) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 4 * G16G_IMG];
    if (gb.a_t[blockIdx.z]) gemm16g_body<true, true, 2, true>(gb, smem);
    else gemm16g_body<false, true, 2, true>(gb, smem);
}

// One launch for the wgrad and dgrad GEMMs of a Linear(H,H) backward: both read dZ (wgrad as a k image, dgrad as a row image)
// and are independent, so 2 x 512 tiles fill the 256 CUs four deep instead of two launches two deep, and one kernel boundary
// (~4.5 us of drain + cache write-back + ramp on this part) disappears. B is a k image in both.
__global__ __launch_bounds__(256) void gemm16g_mixed_kernel(const Gemm16Batch gb) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[G16G_NSTG * 2 * G16G_IMG];
    if (gb.a_t[blockIdx.z]) gemm16g_body<true, true>(gb, smem);
    else gemm16g_body<false, true>(gb, smem);
}

// ---- which bf16 kernel serves a launch (the map at the head of this file, as code) ---------------------------------------------------
// Every entry point gathers the same facts about its problems in one pass (gather16), asks the one ladder (pick16) for a kernel family,
// and launches the instantiation of that family for its operand form (launch16).
enum class Form { row_row, row_k, k_k, mixed };      // (A, B) images; mixed: A per problem (Gemm16Batch::a_t), B a k image
enum class Family { p, x3, g, reg, none };           // none: split-bf16 planes that no kernel can read (missing, misaligned, M/N/K not of 64; three planes: not of 128 x 64 x 128)

struct Facts16 {
    int m_div = 256, n_div = 256, k_div = 256;       // largest power of two, up to 256, that divides every problem's M / N / K
    int k_min = 1 << 30;
    bool ab16 = true;        // A, B 16-byte aligned with pitches that are multiples of 8 bf16: what every LDS-DMA kernel asks of its operands
    bool has_lo = false;     // some problem carries a lo plane: a split-bf16 launch
    bool lo16 = true;        // every problem carries both lo planes, 16-byte aligned
    bool has_mid = false;    // some problem carries a mid plane: a three-plane launch
    bool mid16 = true;       // every problem carries both mid planes, 16-byte aligned
    bool c16 = true;         // C and bias 16-byte aligned, ldc a multiple of 4 floats: the float4 epilogue of the p kernels
    int t64 = 0, t128x64 = 0;      // most 64 x 64 / 128 x 64 tiles (partial ones included) any one problem has: grid.x of the 64-wide kernels
    int t128 = 0;            // 128 x 128 tiles of the whole launch
    double flops = 0;
};
static int pow2_div(int v) { const int d = v & -v; return d == 0 || d > 256 ? 256 : d; }

static Facts16 gather16(const Gemm16Problem* probs, int count, Gemm16Batch& gb) {      // also fills gb.p
    Facts16 f;
    auto al16 = [](const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; };
    for (int i = 0; i < count; ++i) {
        const Gemm16Problem& p = gb.p[i] = probs[i];
        f.m_div = std::min(f.m_div, pow2_div(p.M));
        f.n_div = std::min(f.n_div, pow2_div(p.N));
        f.k_div = std::min(f.k_div, pow2_div(p.K));
        f.k_min = std::min(f.k_min, p.K);
        f.ab16 = f.ab16 && p.lda % 8 == 0 && p.ldb % 8 == 0 && al16(p.A) && al16(p.B);
        f.has_lo = f.has_lo || p.A_lo || p.B_lo;
        f.lo16 = f.lo16 && p.A_lo && p.B_lo && al16(p.A_lo) && al16(p.B_lo);
        f.has_mid = f.has_mid || p.A_mid || p.B_mid;
        f.mid16 = f.mid16 && p.A_mid && p.B_mid && al16(p.A_mid) && al16(p.B_mid);
        f.c16 = f.c16 && p.ldc % 4 == 0 && al16(p.C) && al16(p.bias);
        f.t64 = std::max(f.t64, cdiv(p.M, 64) * cdiv(p.N, 64));
        f.t128x64 = std::max(f.t128x64, cdiv(p.M, 128) * cdiv(p.N, 64));
        f.t128 += (p.M >> 7) * (p.N >> 7);
        f.flops += 2.0 * p.M * (double)p.N * p.K;
    }
    return f;
}

// The ladder. The operand form never changes the family, only which instantiation of it launch16 takes.
struct Pick16 { Family family; int tn; };            // tn: tile width of the p kernels
static Pick16 pick16(const Facts16& f) {
    // 128 x TN tiles on the k32 / k64 stage rings: whole 128-row tiles, K a whole number of rings, float4 stores.
    // TN = 128 only when that still gives every CU a workgroup (4-problem launches of 1024^2 outputs are 256 of them): with fewer, one
    // workgroup per CU leaves the k-tile chain wait -> barrier -> DMA issue -> LDS reads -> MFMA exposed and 128-wide tiles measured slower
    // than narrower ones on the 1024-wide layers (profiles/r02_gemm_shapes_old_vs_new.txt, "128x128 everywhere").
    const bool p_ok = f.ab16 && (!f.has_lo || f.lo16) && f.c16 && f.m_div >= 128 && f.n_div >= 64 && f.k_div >= 128 && f.k_min >= 128;
    // three planes: the 128 x 64 p kernel or nothing (the callers route other shapes to gemm_kernel<EXORL_PREC_BF16X6>)
    if (f.has_mid) return {p_ok && f.mid16 && f.lo16 ? Family::p : Family::none, 64};
    if (p_ok) return {Family::p, f.n_div >= 128 && f.t128 >= 256 ? 128 : 64};
    // 64 x 64 LDS-DMA tiles, scalar epilogue stores (nothing asked of C): split planes two stages deep, plain ones four (K a multiple of 4 x 64)
    if (f.has_lo) return {f.ab16 && f.lo16 && f.m_div >= 64 && f.n_div >= 64 && f.k_div >= 64 ? Family::x3 : Family::none, 0};
    if (f.ab16 && f.m_div >= 64 && f.n_div >= 64 && f.k_div >= 256) return {Family::g, 0};
    return {Family::reg, 0};                         // register-staged, any shape the entry point's alignment rules admit
}

template <Form F, int NPL, int TN>
static int launch16p(Gemm16Batch& gb, int count, hipStream_t s) {
    constexpr bool X3 = NPL == 2;
    // three planes: one instantiation per uniform form (TN = 64, k32 stages, four deep); no caller needs the mixed form (refused at the entry)
    if constexpr (NPL == 3 && (F == Form::mixed || TN != 64)) { set_error("gemm16: no three-plane kernel of this form"); return 2; }
    else if constexpr (F == Form::mixed) return g16p_launch(gemm16p_mixed_kernel<NPL, TN>, gb, count, NPL, TN, s);
    // split planes, both operands row images (the forward launches): 64-wide stages, two deep — whole cache lines per DMA row instead of halves, which
    // halves the requests the XCD L2s serve (critic fwd 21.8 -> 19.5 us, actor fwd 21.1 -> 18.9, critic+target fwd 33.7 -> 32.4)
    else if constexpr (F == Form::row_row && X3) return g16p_launch(gemm16p_kernel<false, false, 2, TN, 64, 2>, gb, count, 2, TN, s, 64, 2);
    // plain bf16 planes take the two-region refill as well (round 3). Round 2 kept them on a one-region refill because the k-image B operand
    // came out wrong, run-to-run different, under the two-region one: that was the pre-fence register copy described in region() — a
    // compiler-placed v_mov of an asm-issued LDS read's destination — not the schedule (tests/test_gpu_ops.py::test_gemm_plain_bf16_k_image_regression).
    else return g16p_launch(gemm16p_kernel<F == Form::k_k, F != Form::row_row, NPL, TN>, gb, count, NPL, TN, s);
}

template <Form F>
static int launch16(Gemm16Batch& gb, int count, const Facts16& f, Pick16 pk, hipStream_t s) {
    constexpr bool MIXED = F == Form::mixed;
    constexpr int AL = F == Form::k_k, BL = F != Form::row_row;      // the uniform forms' layouts
    gb.swizzle = 1;
    const dim3 grid64(f.t64, 1, count), grid128(f.t128x64, 1, count), block(256);
    ProfBracket prof;
    EXORL_TRY(prof.begin(s, f.flops));
    switch (pk.family) {
    case Family::p:
        if (f.has_mid) EXORL_TRY((launch16p<F, 3, 64>(gb, count, s)));
        else if (f.has_lo) EXORL_TRY((pk.tn == 128 ? launch16p<F, 2, 128>(gb, count, s) : launch16p<F, 2, 64>(gb, count, s)));
        else EXORL_TRY((pk.tn == 128 ? launch16p<F, 1, 128>(gb, count, s) : launch16p<F, 1, 64>(gb, count, s)));
        break;
    case Family::x3:
        if constexpr (MIXED) hipLaunchKernelGGL(gemm16x3_mixed_kernel, grid64, block, 0, s, gb);
        else hipLaunchKernelGGL((gemm16x3_kernel<AL != 0, BL != 0>), grid64, block, 0, s, gb);
        break;
    case Family::g:
        if constexpr (MIXED) hipLaunchKernelGGL(gemm16g_mixed_kernel, grid64, block, 0, s, gb);
        else hipLaunchKernelGGL((gemm16g_kernel<AL != 0, BL != 0>), grid64, block, 0, s, gb);
        break;
    case Family::reg:
        if constexpr (!MIXED) {      // no mixed form (gemm16_grouped_mixed refuses)
            // three register stages where every problem tiles exactly, else two with bounds guards; 128-row tiles from 256 workgroups
            const bool exact = f.m_div >= 128 && f.n_div >= 64 && f.k_div >= 64, big = f.t128x64 * count >= 256;
            if (exact && big) hipLaunchKernelGGL((gemm16_kernel<AL, BL, 128, 3, false>), grid128, block, 0, s, gb);
            else if (exact) hipLaunchKernelGGL((gemm16_kernel<AL, BL, 64, 3, false>), grid64, block, 0, s, gb);
            else if (big) hipLaunchKernelGGL((gemm16_kernel<AL, BL, 128, 2, true>), grid128, block, 0, s, gb);
            else hipLaunchKernelGGL((gemm16_kernel<AL, BL, 64, 2, true>), grid64, block, 0, s, gb);
        }
        break;
    case Family::none: break;        // refused by both entry points
    }
    EXORL_LAUNCH_CHECK();
    return prof.end(s);
}

static bool pk3_has_mid(const Gemm16Problem* probs, int count) {
    for (int i = 0; i < count; ++i)
        if (probs[i].A_mid || probs[i].B_mid) return true;
    return false;
}
// How many head_part slots per row a folded-head forward launch of these problems writes; 0 = the launch would not take the p kernels.
int gemm16_head_slots(const Gemm16Problem* probs, int count) {
    if (count < 1 || count > 4) return 0;
    Gemm16Batch gb;
    memset(&gb, 0, sizeof(gb));
    const Pick16 pk = pick16(gather16(probs, count, gb));
    if (pk.family != Family::p || pk3_has_mid(probs, count)) return 0;
    for (int i = 0; i < count; ++i)
        if (probs[i].N != probs[0].N) return 0;
    return probs[0].N / (pk.tn / 2);            // four waves: 2 x 2, each TN / 2 columns wide
}

// bf16-in-memory operands, fp32 output. Requirements (checked): 16-byte aligned rows for layout 0 (ld % 8 == 0,
// K % 8 == 0), 4-byte aligned pairs for layout 1 (ld % 2 == 0, R % 2 == 0).
int gemm16_grouped(int a_layout, int b_layout, const Gemm16Problem* probs, int count, bool relu, bool accumulate, hipStream_t s) {
    EXORL_REQUIRE(count >= 1 && count <= 4, "gemm16_grouped: count %d out of range", count);
    for (int i = 0; i < count; ++i) {
        const Gemm16Problem& p = probs[i];
        EXORL_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "gemm16_grouped: empty problem %d", i);
        auto ok = [](const unsigned short* ptr, int64_t ld, int R, int K, int layout) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
            if (layout == 0) return (a % 16 == 0) && (ld % 8 == 0) && (K % 8 == 0);
            return (a % 4 == 0) && (ld % 2 == 0) && (R % 2 == 0);
        };
        EXORL_REQUIRE(ok(p.A, p.lda, p.M, p.K, a_layout) && ok(p.B, p.ldb, p.N, p.K, b_layout),
                      "gemm16_grouped: problem %d (M=%d N=%d K=%d lda=%lld ldb=%lld) violates the bf16 path's alignment rules "
                      "(hidden_dim and batch must be multiples of 8 in bf16 precision)", i, p.M, p.N, p.K, (long long)p.lda, (long long)p.ldb);
    }
    Gemm16Batch gb;
    memset(&gb, 0, sizeof(gb));
    const Facts16 f = gather16(probs, count, gb);
    const Pick16 pk = pick16(f);
    gb.relu = relu ? 1 : 0;
    gb.accumulate = accumulate ? 1 : 0;
    for (int i = 0; i < count; ++i)
        if (probs[i].head_part)
            EXORL_REQUIRE(probs[i].head_w && a_layout == 0 && b_layout == 0 && !accumulate && gemm16_head_slots(probs, count) > 0,
                          "gemm16_grouped: a folded head needs a forward launch on the 128 x TN kernels (ask gemm16_head_slots first)");
    EXORL_REQUIRE(!f.has_mid || pk.family == Family::p, "gemm16_grouped: three-plane operands need M %% 128 = 0, N %% 64 = 0, K %% 128 = 0 (K >= 128), 16-byte aligned "
                  "hi/mid/lo planes with pitches that are multiples of 8, 16-byte aligned C and bias, ldc %% 4 = 0 (problem 0: M=%d N=%d K=%d)",
                  probs[0].M, probs[0].N, probs[0].K);
    for (int i = 0; i < count; ++i)
        EXORL_REQUIRE(!f.has_mid || !probs[i].head_part, "gemm16_grouped: no folded head on three-plane operands");
    EXORL_REQUIRE(pk.family != Family::none, "gemm16_grouped: split-bf16 operands need M, N, K multiples of 64 and 16-byte aligned hi/lo planes");
    if (a_layout == 0 && b_layout == 0) return launch16<Form::row_row>(gb, count, f, pk, s);
    if (a_layout == 0 && b_layout == 1) return launch16<Form::row_k>(gb, count, f, pk, s);
    if (a_layout == 1 && b_layout == 1) return launch16<Form::k_k>(gb, count, f, pk, s);
    set_error("gemm16_grouped: unsupported layout combination %d %d", a_layout, b_layout);
    return 2;
}

// probs[i] with a_layouts[i] in {0,1}, b_layout 1 for all, no bias/relu/accumulate. Falls back to one launch per layout when a
// problem does not meet the 64 x 64 LDS-DMA kernel's tiling rules.
// That precondition is stricter than the ladder needs: K % 256 is gemm16g's four-stage ring, while the p kernels, which take every
// launch the product makes here, want only K % 128. It is left as it is: lifting it would turn the two launches of a backward pass at a
// batch that is an odd multiple of 128 (the wgrad's K) into one — a change of launch counts, to be measured on its own.
int gemm16_grouped_mixed(const int* a_layouts, const Gemm16Problem* probs, int count, hipStream_t s) {
    EXORL_REQUIRE(count >= 1 && count <= 4, "gemm16_grouped_mixed: count %d out of range", count);
    Gemm16Batch gb;
    memset(&gb, 0, sizeof(gb));
    const Facts16 f = gather16(probs, count, gb);
    EXORL_REQUIRE(!f.has_mid, "gemm16_grouped_mixed: three-plane operands have no mixed wgrad + dgrad form");
    const Pick16 pk = pick16(f);
    bool ok = f.ab16 && f.m_div >= 64 && f.n_div >= 64 && f.k_div >= 256 && pk.family != Family::none;
    for (int i = 0; i < count; ++i) {
        gb.a_t[i] = a_layouts[i] != 0;
        ok = ok && probs[i].M > 0 && !probs[i].bias;
    }
    if (!ok) {
        for (int i = 0; i < count; ++i) EXORL_TRY(gemm16_grouped(a_layouts[i], 1, probs + i, 1, false, false, s));
        return 0;
    }
    EXORL_REQUIRE(pk.family != Family::reg, "gemm16_grouped_mixed: the register-staged kernel has no mixed form");
    return launch16<Form::mixed>(gb, count, f, pk, s);
}

template <int PREC, int AL, int BL>
static int launch_layout(const GemmBatch& gb, int count, int max_tiles, bool vec, hipStream_t s) {
    dim3 grid(max_tiles, 1, count), block(256);
    double flops = 0;
    for (int i = 0; i < count; ++i) flops += 2.0 * gb.p[i].M * (double)gb.p[i].N * gb.p[i].K;
    ProfBracket prof;
    EXORL_TRY(prof.begin(s, flops));
    constexpr size_t dyn = PREC == EXORL_PREC_BF16X6 ? 6 * TILEB : 0;          // 48 KB: one stage of three planes of A and B
    if constexpr (PREC == EXORL_PREC_BF16X6) {
        static bool attr = false;
        if (!attr) {
            EXORL_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_kernel<PREC, AL, BL, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
            EXORL_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_kernel<PREC, AL, BL, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
            attr = true;
        }
    }
    if (vec) hipLaunchKernelGGL((gemm_kernel<PREC, AL, BL, true>), grid, block, dyn, s, gb);
    else     hipLaunchKernelGGL((gemm_kernel<PREC, AL, BL, false>), grid, block, dyn, s, gb);
    EXORL_LAUNCH_CHECK();
    return prof.end(s);
}

template <int PREC>
static int launch_prec(const GemmBatch& gb, int count, int al, int bl, int max_tiles, bool vec, hipStream_t s) {
    if (al == 0 && bl == 0) return launch_layout<PREC, 0, 0>(gb, count, max_tiles, vec, s);
    if (al == 0 && bl == 1) return launch_layout<PREC, 0, 1>(gb, count, max_tiles, vec, s);
    if (al == 1 && bl == 1) return launch_layout<PREC, 1, 1>(gb, count, max_tiles, vec, s);
    if (al == 1 && bl == 0) return launch_layout<PREC, 1, 0>(gb, count, max_tiles, vec, s);
    set_error("gemm: bad layout %d %d", al, bl);
    return 2;
}

static bool aligned_for_vec(const GemmProblem& p, int al, int bl) {
    auto ok = [](const float* ptr, int64_t ld, int R, int K, int layout) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
        if (layout == 0) return (a % 16 == 0) && (ld % 4 == 0) && (K % 4 == 0);
        return (a % 8 == 0) && (ld % 2 == 0) && (R % 2 == 0);
    };
    return ok(p.A, p.lda, p.M, p.K, al) && ok(p.B, p.ldb, p.N, p.K, bl);
}

// ---- fp32-source operands onto the hi/lo-plane kernels (round 3) ------------------------------------------------------------------------
// The callers of gemm_grouped keep fp32 activations and weights (intrinsic modules, the pixel agents' heads and 39200-wide module layers); the
// generic kernel above splits them into hi/lo planes on their way into LDS — 64 x 64 tiles, register staging: ~62 TFLOP/s at 1024^3. The plane
// kernels (gemm16p_*) run the SAME arithmetic (hi*hi + hi*lo + lo*hi, three fp32 accumulators summed small-first) at 230-300 TFLOP/s but want
// bf16 planes in memory, M % 128 = 0, N % 64 = 0, K % 128 = 0. For problems large enough to pay for it this adapter writes zero-padded hi/lo
// planes of both operands into a scratch arena (one elementwise pass each: 8 B per element moved), runs the plane kernels, and — when C does
// not tile — copies the padded result back (bias, ReLU in the GEMM epilogue as always; accumulate in the copy). Groups of more than four
// problems (Disagreement's five models) go in chunks.
struct PlaneArena { unsigned char* buf = nullptr; size_t bytes = 0; };
static PlaneArena g_plane_arena;
// A stream capture may take the adapter only where its caller asks for it (gemm_planes_capture: the joint module + agent graph of
// exorl_agent_enable_graph_intr), and only into an arena that is large enough already: nothing may be allocated while capturing. The caller
// sizes the arena first — a throw-away capture of the same launches with g_plane_probe set records the largest chunk, gemm_planes_reserve
// grows the arena to it — so the captured step takes exactly the kernels the eager step takes. A graph keeps the arena's address: once one
// has captured it, a later growth leaves the old buffer allocated (g_plane_captured) instead of freeing it under the graph.
static bool g_plane_capture_ok = false, g_plane_captured = false;
static size_t* g_plane_probe = nullptr;

__global__ __launch_bounds__(256) void to_planes_kernel(const float* __restrict__ src, int64_t ld, int rows, int cols, unsigned short* __restrict__ hi,
                                                        unsigned short* __restrict__ lo, int rows_p, int cols_p) {
    // 8 consecutive columns per thread: two 16-byte loads (when aligned and in range), one 16-byte store per plane; padding is written as zeros
    const int64_t groups = (int64_t)rows_p * (cols_p / 8);
    const bool vec = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (cols_p / 8)), c0 = (int)(i % (cols_p / 8)) * 8;
        float v[8];
        if (r < rows && vec && c0 + 8 <= cols) {
            const float4 a = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c0), b = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (r < rows && c0 + j < cols) ? src[(int64_t)r * ld + c0 + j] : 0.f;
        }
        uint4 h, l;
        h.x = pack_bf16(v[0], v[1]); h.y = pack_bf16(v[2], v[3]); h.z = pack_bf16(v[4], v[5]); h.w = pack_bf16(v[6], v[7]);
        l.x = pack_bf16(bf16_residual(v[0]), bf16_residual(v[1])); l.y = pack_bf16(bf16_residual(v[2]), bf16_residual(v[3]));
        l.z = pack_bf16(bf16_residual(v[4]), bf16_residual(v[5])); l.w = pack_bf16(bf16_residual(v[6]), bf16_residual(v[7]));
        *reinterpret_cast<uint4*>(hi + (int64_t)r * cols_p + c0) = h;
        *reinterpret_cast<uint4*>(lo + (int64_t)r * cols_p + c0) = l;
    }
}
// three-plane sibling: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); blockIdx.y = image (see to_planes3 in kernels.h)
__global__ __launch_bounds__(256) void to_planes3_kernel(const float* __restrict__ src, int64_t ld, int rows, int cols, unsigned short* __restrict__ hi,
                                                         unsigned short* __restrict__ mid, unsigned short* __restrict__ lo, int rows_p, int cols_p,
                                                         int64_t src_stride, int64_t dst_stride) {
    src += blockIdx.y * src_stride;
    const int64_t dst0 = blockIdx.y * dst_stride;
    const int64_t groups = (int64_t)rows_p * (cols_p / 8);
    const bool vec = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (cols_p / 8)), c0 = (int)(i % (cols_p / 8)) * 8;
        float v[8], m[8], l[8];
        if (r < rows && vec && c0 + 8 <= cols) {
            const float4 a = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c0), b = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (r < rows && c0 + j < cols) ? src[(int64_t)r * ld + c0 + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { m[j] = bf16_residual(v[j]); l[j] = bf16_residual(m[j]); }
        uint4 h, md, lw;
        h.x = pack_bf16(v[0], v[1]); h.y = pack_bf16(v[2], v[3]); h.z = pack_bf16(v[4], v[5]); h.w = pack_bf16(v[6], v[7]);
        md.x = pack_bf16(m[0], m[1]); md.y = pack_bf16(m[2], m[3]); md.z = pack_bf16(m[4], m[5]); md.w = pack_bf16(m[6], m[7]);
        lw.x = pack_bf16(l[0], l[1]); lw.y = pack_bf16(l[2], l[3]); lw.z = pack_bf16(l[4], l[5]); lw.w = pack_bf16(l[6], l[7]);
        const int64_t o = dst0 + (int64_t)r * cols_p + c0;
        *reinterpret_cast<uint4*>(hi + o) = h;
        *reinterpret_cast<uint4*>(mid + o) = md;
        *reinterpret_cast<uint4*>(lo + o) = lw;
    }
}
int to_planes3(const float* src, int64_t ld, int rows, int cols, unsigned short* hi, unsigned short* mid, unsigned short* lo, int rows_p, int cols_p,
               int nb, int64_t src_stride, int64_t dst_stride, hipStream_t s) {
    auto al16 = [](const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; };
    EXORL_REQUIRE(src && hi && mid && lo && rows > 0 && cols > 0 && rows_p >= rows && cols_p >= cols && cols_p % 8 == 0 && nb >= 1 && ld >= cols &&
                  al16(hi) && al16(mid) && al16(lo) && dst_stride % 8 == 0 && (nb == 1 || dst_stride >= (int64_t)rows_p * cols_p),
                  "to_planes3: bad arguments (rows=%d cols=%d rows_p=%d cols_p=%d nb=%d)", rows, cols, rows_p, cols_p, nb);
    const int64_t blocks = ((int64_t)rows_p * (cols_p / 8) + 255) / 256;
    ProfBracket prof;                  // exorl_profile_gemm lists the conversion passes too, with 0 FLOPs (tools/micro/planes_bench.py planes3)
    EXORL_TRY(prof.begin(s, 0.0));
    hipLaunchKernelGGL(to_planes3_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks), nb), dim3(256), 0, s, src, ld, rows, cols, hi, mid, lo, rows_p, cols_p,
                       src_stride, dst_stride);
    EXORL_LAUNCH_CHECK();
    return prof.end(s);
}
// C[m][n] (+)= Cp[m][n] for the unpadded block
__global__ __launch_bounds__(256) void from_padded_kernel(const float* __restrict__ cp, int64_t ldp, float* __restrict__ c, int64_t ldc, int M, int N, int accumulate) {
    const int64_t n = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / N), j = (int)(i % N);
        const float v = cp[(int64_t)m * ldp + j];
        float* d = c + (int64_t)m * ldc + j;
        *d = accumulate ? v + *d : v;
    }
}
__global__ void pad_bias_kernel(const float* __restrict__ b, float* __restrict__ out, int N, int Np) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Np) out[i] = i < N ? b[i] : 0.f;
}

static bool planes_adapter_wants(int al, int bl, const GemmProblem* probs, int count) {
    if (!((al == 0 && bl == 0) || (al == 0 && bl == 1) || (al == 1 && bl == 1))) return false;
    for (int i = 0; i < count; ++i)
        if (probs[i].M < 256 || probs[i].N < 256 || probs[i].K < 256) return false;       // conversion passes + padded tiles must be worth it
    return true;
}

// 0 = done; -1 = not taken (the caller runs the generic kernel); > 0 = error
// C written in place by the plane kernels: whole row tiles, 16-byte rows and bias; a width that is not a multiple of the 128-column tile is
// handled by the epilogue's column guard (n_store) as long as it is a multiple of 4 (round 3: the padded copy + from_padded_kernel pass of the
// 39200-wide module layers was 0.7 ms of an ICM update on pixels and 2.0 ms of a Disagreement update; TUNE_ADAPTER_PADDED brings it back)
static bool adapter_direct(const GemmProblem& p) {
    const bool wide_ok = p.N % 128 == 0 || (p.N % 4 == 0 && !(tune_variant() & TUNE_ADAPTER_PADDED));
    return p.M % 128 == 0 && wide_ok && p.ldc % 4 == 0 && reinterpret_cast<uintptr_t>(p.C) % 16 == 0 &&
           (!p.bias || reinterpret_cast<uintptr_t>(p.bias) % 16 == 0);
}
static int planes_adapter(int al, int bl, const GemmProblem* probs, int count, bool relu, bool accumulate, hipStream_t s) {
    struct Plan { int Mp, Np, Kp; size_t a_hi, a_lo, b_hi, b_lo, cp, bias; bool direct; };
    auto take_all = [](const GemmProblem& p, size_t& need) {
        auto take = [&](size_t bytes) { need += (bytes + 255) & ~(size_t)255; };
        const size_t Mp = round_up(p.M, 128), Np = round_up(p.N, 128), Kp = round_up(p.K, 128);
        take(Mp * Kp * 2); take(Mp * Kp * 2); take(Np * Kp * 2); take(Np * Kp * 2);
        if (!adapter_direct(p)) { take(Mp * Np * 4); if (p.bias) take(Np * 4); }
    };
    {   // inside a stream capture only by request and without touching the allocation: the arena may be re-allocated later, a captured
        // graph would keep the old addresses
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        EXORL_CHECK_HIP(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) {
            if (!g_plane_capture_ok) return -1;
            size_t most = 0;
            for (int c0 = 0; c0 < count; c0 += 4) {
                size_t need = 0;
                for (int i = c0; i < count && i < c0 + 4; ++i) take_all(probs[i], need);
                most = need > most ? need : most;
            }
            if (g_plane_probe && most > *g_plane_probe) *g_plane_probe = most;
            if (most > g_plane_arena.bytes) return -1;
            g_plane_captured = true;
        }
    }
    for (int c0 = 0; c0 < count; c0 += 4) {
        const int nc = count - c0 < 4 ? count - c0 : 4;
        Plan pl[4];
        size_t need = 0;
        auto take = [&](size_t bytes) { const size_t o = need; need += (bytes + 255) & ~(size_t)255; return o; };
        for (int i = 0; i < nc; ++i) {
            const GemmProblem& p = probs[c0 + i];
            Plan& q = pl[i];
            q.Mp = (int)round_up(p.M, 128); q.Np = (int)round_up(p.N, 128); q.Kp = (int)round_up(p.K, 128);
            q.a_hi = take((size_t)q.Mp * q.Kp * 2); q.a_lo = take((size_t)q.Mp * q.Kp * 2);
            q.b_hi = take((size_t)q.Np * q.Kp * 2); q.b_lo = take((size_t)q.Np * q.Kp * 2);
            q.direct = adapter_direct(p);
            q.cp = q.direct ? 0 : take((size_t)q.Mp * q.Np * 4);
            q.bias = (q.direct || !p.bias) ? 0 : take((size_t)q.Np * 4);
        }
        if (need > g_plane_arena.bytes) {
            EXORL_CHECK_HIP(hipDeviceSynchronize());                                // nothing in flight may still read the old arena
            if (g_plane_arena.buf && !g_plane_captured) EXORL_CHECK_HIP(hipFree(g_plane_arena.buf));
            g_plane_captured = false;
            g_plane_arena.buf = nullptr; g_plane_arena.bytes = 0;
            const size_t want = need + need / 8;
            if (hipMalloc((void**)&g_plane_arena.buf, want) != hipSuccess) {
                (void)hipGetLastError();
                if (c0 == 0) return -1;
                set_error("planes_adapter: could not grow the plane arena to %zu bytes", want);
                return 3;
            }
            g_plane_arena.bytes = want;
        }
        unsigned char* base = g_plane_arena.buf;
        Gemm16Problem q16[4];
        for (int i = 0; i < nc; ++i) {
            const GemmProblem& p = probs[c0 + i];
            const Plan& q = pl[i];
            auto u16 = [&](size_t o) { return reinterpret_cast<unsigned short*>(base + o); };
            // storage shapes: layout 0 = [rows = M or N][K]; layout 1 = [K][M or N]
            const int ar = al == 0 ? p.M : p.K, acol = al == 0 ? p.K : p.M, arp = al == 0 ? q.Mp : q.Kp, acp = al == 0 ? q.Kp : q.Mp;
            const int br = bl == 0 ? p.N : p.K, bcol = bl == 0 ? p.K : p.N, brp = bl == 0 ? q.Np : q.Kp, bcp = bl == 0 ? q.Kp : q.Np;
            auto grid = [](int64_t groups) { const int64_t b = (groups + 255) / 256; return (unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); };
            hipLaunchKernelGGL(to_planes_kernel, dim3(grid((int64_t)arp * (acp / 8))), dim3(256), 0, s, p.A, p.lda, ar, acol, u16(q.a_hi), u16(q.a_lo), arp, acp);
            hipLaunchKernelGGL(to_planes_kernel, dim3(grid((int64_t)brp * (bcp / 8))), dim3(256), 0, s, p.B, p.ldb, br, bcol, u16(q.b_hi), u16(q.b_lo), brp, bcp);
            const float* bias = p.bias;
            if (!q.direct && p.bias) {
                hipLaunchKernelGGL(pad_bias_kernel, dim3(cdiv(q.Np, 256)), dim3(256), 0, s, p.bias, reinterpret_cast<float*>(base + q.bias), p.N, q.Np);
                bias = reinterpret_cast<float*>(base + q.bias);
            }
            EXORL_LAUNCH_CHECK();
            Gemm16Problem g{u16(q.a_hi), u16(q.b_hi), q.direct ? p.C : reinterpret_cast<float*>(base + q.cp), bias, q.Mp, q.Np, q.Kp, acp, bcp,
                            q.direct ? p.ldc : (int64_t)q.Np};
            g.A_lo = u16(q.a_lo); g.B_lo = u16(q.b_lo);
            g.n_store = q.direct && p.N % 128 != 0 ? p.N : 0;          // written in place, the tile columns past N skipped in the epilogue
            q16[i] = g;
        }
        bool all_direct = true;
        for (int i = 0; i < nc; ++i) all_direct = all_direct && pl[i].direct;
        // accumulate rides in the GEMM epilogue only when every C of the chunk is written in place; otherwise the copy-back adds
        EXORL_TRY(gemm16_grouped(al, bl, q16, nc, relu, accumulate && all_direct, s));
        for (int i = 0; i < nc; ++i) {
            if (pl[i].direct) {
                EXORL_REQUIRE(!accumulate || all_direct, "planes_adapter: mixed in-place / padded outputs with accumulate");
                continue;
            }
            const GemmProblem& p = probs[c0 + i];
            const int64_t n = (int64_t)p.M * p.N;
            hipLaunchKernelGGL(from_padded_kernel, dim3((unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256)), dim3(256), 0, s,
                               reinterpret_cast<const float*>(base + pl[i].cp), (int64_t)pl[i].Np, p.C, p.ldc, p.M, p.N, accumulate ? 1 : 0);
            EXORL_LAUNCH_CHECK();
        }
    }
    return 0;
}

void gemm_planes_capture(bool allow, size_t* probe) { g_plane_capture_ok = allow; g_plane_probe = probe; }

int gemm_planes_reserve(size_t bytes) {
    if (bytes <= g_plane_arena.bytes) return 0;
    EXORL_CHECK_HIP(hipDeviceSynchronize());
    if (g_plane_arena.buf && !g_plane_captured) EXORL_CHECK_HIP(hipFree(g_plane_arena.buf));
    g_plane_captured = false;
    g_plane_arena.buf = nullptr; g_plane_arena.bytes = 0;
    const size_t want = bytes + bytes / 8;
    if (hipMalloc((void**)&g_plane_arena.buf, want) != hipSuccess) {
        (void)hipGetLastError();
        set_error("gemm_planes_reserve: could not grow the plane arena to %zu bytes", want);
        return 3;
    }
    g_plane_arena.bytes = want;
    return 0;
}

// Launches up to GEMM_MAX_GROUP independent problems (same layouts / epilogue flags) as one grid.
int gemm_grouped(int precision, int a_layout, int b_layout, const GemmProblem* probs, int count, bool relu,
                 bool accumulate, hipStream_t s) {
    EXORL_REQUIRE(count >= 1 && count <= GEMM_MAX_GROUP, "gemm_grouped: count %d out of range", count);
    if (g_prec_override && precision == EXORL_PREC_BF16X3) {
        bool wide = false;
        for (int i = 0; i < count; ++i) wide = wide || probs[i].M >= 8192 || probs[i].N >= 8192 || probs[i].K >= 8192;
        const int form = (a_layout == 0 && b_layout == 0) ? 0 : (a_layout == 1 && b_layout == 1) ? 1 : (a_layout == 0 && b_layout == 1) ? 2 : -1;
        if (form >= 0 && (g_prec_override >> (2 * form + (wide ? 1 : 0))) & 1) precision = EXORL_PREC_F32;
    }
    GemmBatch gb;
    memset(&gb, 0, sizeof(gb));
    int max_tiles = 0;
    bool vec = true;
    for (int i = 0; i < count; ++i) {
        gb.p[i] = probs[i];
        EXORL_REQUIRE(probs[i].M > 0 && probs[i].N > 0 && probs[i].K > 0, "gemm_grouped: empty problem %d", i);
        const int t = cdiv(probs[i].M, TILE) * cdiv(probs[i].N, TILE);
        max_tiles = t > max_tiles ? t : max_tiles;
        vec = vec && aligned_for_vec(probs[i], a_layout, b_layout);
    }
    gb.relu = relu ? 1 : 0;
    gb.accumulate = accumulate ? 1 : 0;
    if (precision == EXORL_PREC_BF16X3 && planes_adapter_wants(a_layout, b_layout, probs, count)) {
        bool mixed = false;          // accumulate with some outputs in place and some padded: keep it simple, generic kernel
        if (accumulate) {
            int direct = 0;
            for (int i = 0; i < count; ++i)
                direct += adapter_direct(probs[i]);
            mixed = direct != 0 && direct != count;
        }
        if (!mixed) {
            const int rc = planes_adapter(a_layout, b_layout, probs, count, relu, accumulate, s);
            if (rc >= 0) return rc;
        }
    }
    if (precision == EXORL_PREC_F32) return launch_prec<EXORL_PREC_F32>(gb, count, a_layout, b_layout, max_tiles, vec, s);
    if (precision == EXORL_PREC_BF16) return launch_prec<EXORL_PREC_BF16>(gb, count, a_layout, b_layout, max_tiles, vec, s);
    if (precision == EXORL_PREC_BF16X3) return launch_prec<EXORL_PREC_BF16X3>(gb, count, a_layout, b_layout, max_tiles, vec, s);
    if (precision == EXORL_PREC_BF16X6) return launch_prec<EXORL_PREC_BF16X6>(gb, count, a_layout, b_layout, max_tiles, vec, s);
    set_error("gemm_grouped: unknown precision %d", precision);
    return 2;
}

}  // namespace exorl

extern "C" int exorl_profile_gemm(int32_t enable) {
    exorl::g_prof.on = enable != 0;
    if (enable) { exorl::g_prof.used = 0; exorl::g_prof.flops.clear(); }
    return 0;
}

// Synchronises, then returns per-launch (algorithmic FLOPs, milliseconds) of the GEMM launches recorded
// since exorl_profile_gemm(1); n_out = number of launches written (<= cap).
extern "C" int exorl_profile_gemm_read(double* flops_out, float* ms_out, int32_t cap, int32_t* n_out) {
    using namespace exorl;
    EXORL_REQUIRE(flops_out && ms_out && n_out, "profile_gemm_read: null argument");
    EXORL_CHECK_HIP(hipDeviceSynchronize());
    int n = 0;
    for (size_t i = 0; i < g_prof.used && n < cap; ++i, ++n) {
        float ms = 0.f;
        EXORL_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
        flops_out[n] = g_prof.flops[i];
        ms_out[n] = ms;
    }
    *n_out = n;
    return 0;
}

// Median duration of an EMPTY start/stop event bracket on `stream`: the fixed cost hipEvent timing adds to every
// bracketed launch (subtracted by bench.py so its per-launch figure is comparable with rocprofv3's kernel durations).
extern "C" int exorl_profile_event_overhead(float* ms_out, void* stream) {
    using namespace exorl;
    EXORL_REQUIRE(ms_out, "profile_event_overhead: null argument");
    hipStream_t s = as_stream(stream);
    const int n = 31;
    hipEvent_t ev[2 * n];
    for (int i = 0; i < 2 * n; ++i) EXORL_CHECK_HIP(hipEventCreate(&ev[i]));
    for (int i = 0; i < n; ++i) {
        EXORL_CHECK_HIP(hipEventRecord(ev[2 * i], s));
        EXORL_CHECK_HIP(hipEventRecord(ev[2 * i + 1], s));
    }
    EXORL_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<float> t(n);
    for (int i = 0; i < n; ++i) EXORL_CHECK_HIP(hipEventElapsedTime(&t[i], ev[2 * i], ev[2 * i + 1]));
    for (int i = 0; i < 2 * n; ++i) (void)hipEventDestroy(ev[i]);
    std::sort(t.begin(), t.end());
    *ms_out = t[n / 2];
    return 0;
}

extern "C" int exorl_gemm_bf16(int32_t a_layout, int32_t b_layout, int32_t M, int32_t N, int32_t K, const uint16_t* A,
                               int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                               int32_t relu, int32_t accumulate, void* stream) {
    exorl::Gemm16Problem p{A, B, C, bias, M, N, K, lda, ldb, ldc};
    return exorl::gemm16_grouped(a_layout, b_layout, &p, 1, relu != 0, accumulate != 0, exorl::as_stream(stream));
}

extern "C" int exorl_gemm_planes(int32_t count, const int32_t* a_layouts, int32_t b_layout, int32_t M, int32_t N, int32_t K,
                                 const uint16_t* const* A_hi, const uint16_t* const* A_lo, int64_t lda, const uint16_t* const* B_hi,
                                 const uint16_t* const* B_lo, int64_t ldb, float* const* C, int64_t ldc, int32_t relu, void* stream) {
    using namespace exorl;
    EXORL_REQUIRE(count >= 1 && count <= 4 && a_layouts && A_hi && B_hi && C, "gemm_planes: bad arguments");
    Gemm16Problem p[4];
    bool mixed = false;
    for (int i = 0; i < count; ++i) {
        p[i] = Gemm16Problem{A_hi[i], B_hi[i], C[i], nullptr, M, N, K, lda, ldb, ldc};
        if (A_lo && A_lo[i]) { p[i].A_lo = A_lo[i]; p[i].B_lo = B_lo ? B_lo[i] : nullptr; }
        mixed = mixed || a_layouts[i] != a_layouts[0];
    }
    if (mixed) {
        EXORL_REQUIRE(b_layout == 1 && !relu, "gemm_planes: mixed A layouts go with B as a k image and no epilogue (wgrad + dgrad)");
        int at[4];
        for (int i = 0; i < count; ++i) at[i] = a_layouts[i];
        return gemm16_grouped_mixed(at, p, count, as_stream(stream));
    }
    return gemm16_grouped(a_layouts[0], b_layout, p, count, relu != 0, false, as_stream(stream));
}

extern "C" int exorl_gemm_planes3(int32_t count, const int32_t* a_layouts, int32_t b_layout, int32_t M, int32_t N, int32_t K,
                                  const uint16_t* const* A_hi, const uint16_t* const* A_mid, const uint16_t* const* A_lo, int64_t lda,
                                  const uint16_t* const* B_hi, const uint16_t* const* B_mid, const uint16_t* const* B_lo, int64_t ldb, float* const* C,
                                  int64_t ldc, int32_t relu, void* stream) {
    using namespace exorl;
    EXORL_REQUIRE(count >= 1 && count <= 4 && a_layouts && A_hi && A_mid && A_lo && B_hi && B_mid && B_lo && C, "gemm_planes3: bad arguments");
    EXORL_REQUIRE(M > 0 && N > 0 && K > 0 && lda > 0 && ldb > 0 && ldc >= N, "gemm_planes3: bad shape M=%d N=%d K=%d lda=%lld ldb=%lld ldc=%lld", M, N, K,
                  (long long)lda, (long long)ldb, (long long)ldc);
    Gemm16Problem p[4];
    for (int i = 0; i < count; ++i) {
        EXORL_REQUIRE(a_layouts[i] == a_layouts[0], "gemm_planes3: three-plane operands have no mixed wgrad + dgrad form (one A layout per launch)");
        EXORL_REQUIRE(A_hi[i] && A_mid[i] && A_lo[i] && B_hi[i] && B_mid[i] && B_lo[i] && C[i], "gemm_planes3: problem %d has a null plane or output", i);
        p[i] = Gemm16Problem{A_hi[i], B_hi[i], C[i], nullptr, M, N, K, lda, ldb, ldc};
        p[i].A_mid = A_mid[i]; p[i].B_mid = B_mid[i]; p[i].A_lo = A_lo[i]; p[i].B_lo = B_lo[i];
    }
    return gemm16_grouped(a_layouts[0], b_layout, p, count, relu != 0, false, as_stream(stream));
}

extern "C" int exorl_gemm(int32_t precision, int32_t a_layout, int32_t b_layout, int32_t M, int32_t N, int32_t K,
                          const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                          const float* bias, int32_t relu, int32_t accumulate, void* stream) {
    exorl::GemmProblem p{A, B, C, bias, M, N, K, lda, ldb, ldc};
    return exorl::gemm_grouped(precision, a_layout, b_layout, &p, 1, relu != 0, accumulate != 0, exorl::as_stream(stream));
}
