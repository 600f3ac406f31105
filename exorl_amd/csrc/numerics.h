// Device primitives the numeric contracts rest on, one definition each: the block reduction, the draws on a Philox block and the fp32 ->
// bf16 plane split. Kernels in different sources that must agree bit for bit (the action-noise stream, the derived weight images) agree
// because they call the same function here.
#pragma once
#include "common.h"

namespace exorl {

// ---- block reduction: every v[i] becomes its sum over the workgroup, waves added in wave order (at most 16 waves) ----------------
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float (*sm)[16]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float s = wave_sum(v[i]);
        if (lane == 0) sm[i][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float t = 0.f;
        for (int w = 0; w < nw; ++w) t += sm[i][w];
        v[i] = t;
    }
    __syncthreads();
}

// ---- draws on a Philox block {element, purpose, counter lo, counter hi} keyed by the seed ------------------------------------------
// The purpose word keeps two noise sources that share a seed and a counter apart: two purposes that collide would correlate them
// silently. This enum is the one place a new purpose is added. (The replay sampler is not part of this table: its block is laid out
// {sample, counter lo, counter hi, 0}, replay.hip.)
enum PhiloxPurpose : uint32_t {
    PHILOX_ACTION_NOISE = 0,         // TruncatedNormal / tanh-Gaussian action noise: every agent's draws, exorl_debug_philox_normal
    PHILOX_CQL_UNIFORM = 1,          // CQL's uniform random actions
    PHILOX_PROTO_CATEGORICAL = 7,    // Proto's categorical draw of queue candidates
    PHILOX_SMM_EPSILON = 11,         // SMM's VAE epsilon
    PHILOX_AUG_SHIFT = 13,           // RandomShiftsAug's per-image shifts
};
constexpr uint32_t PHILOX_PURPOSES[] = {PHILOX_ACTION_NOISE, PHILOX_CQL_UNIFORM, PHILOX_PROTO_CATEGORICAL, PHILOX_SMM_EPSILON, PHILOX_AUG_SHIFT};
constexpr bool philox_purposes_distinct() {
    for (size_t i = 0; i < sizeof(PHILOX_PURPOSES) / sizeof(uint32_t); ++i)
        for (size_t j = 0; j < i; ++j)
            if (PHILOX_PURPOSES[i] == PHILOX_PURPOSES[j]) return false;
    return true;
}
static_assert(philox_purposes_distinct(), "two Philox purposes share a word");
static_assert(PHILOX_ACTION_NOISE == 0 && PHILOX_CQL_UNIFORM == 1 && PHILOX_PROTO_CATEGORICAL == 7 && PHILOX_SMM_EPSILON == 11 &&
              PHILOX_AUG_SHIFT == 13, "the purpose words are part of the streams the tests and the oracle restate");

constexpr float PHILOX_UNIT = 2.3283064365386963e-10f;      // 2^-32: a 32-bit word -> [0, 1)

__device__ __forceinline__ void philox_block(uint32_t (&c)[4], uint64_t seed, uint64_t counter, uint32_t elem, PhiloxPurpose purpose) {
    c[0] = elem; c[1] = purpose; c[2] = (uint32_t)counter; c[3] = (uint32_t)(counter >> 32);
    Philox::gen(c, seed);
}

// standard normal (Box-Muller on words 0 and 1; u1 in (0, 1])
__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t counter, uint32_t elem, PhiloxPurpose purpose = PHILOX_ACTION_NOISE) {
    uint32_t c[4];
    philox_block(c, seed, counter, elem, purpose);
    const float u1 = ((float)c[0] + 1.0f) * PHILOX_UNIT;
    const float u2 = (float)c[1] * PHILOX_UNIT;
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.283185307179586f * u2);
}
// uniform on [0, 1) from word 0
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t counter, uint32_t elem, PhiloxPurpose purpose) {
    uint32_t c[4];
    philox_block(c, seed, counter, elem, purpose);
    return (float)c[0] * PHILOX_UNIT;
}
// uniform on [-1, 1)
__device__ __forceinline__ float philox_uniform_pm1(uint64_t seed, uint64_t counter, uint32_t elem, PhiloxPurpose purpose) {
    return -1.0f + 2.0f * philox_uniform(seed, counter, elem, purpose);
}
// integer on [0, n) from one word of a block (multiply-shift); the augmentation shifts take words 0 and 1 of one block
__device__ __forceinline__ int philox_below(uint32_t word, int n) { return (int)(((uint64_t)word * (uint64_t)n) >> 32); }

// ---- fp32 -> bf16 planes: x = hi + lo (+ third) with hi = bf16(x), lo = bf16(x - hi), third = bf16(x - hi - lo) -------------------
// bits of bf16(x)
__device__ __forceinline__ unsigned short bf16_bits(float x) {
    __bf16 b = (__bf16)x;
    return __builtin_bit_cast(unsigned short, b);
}
// x - bf16(x): what the next plane holds; bf16_residual(bf16_residual(x)) feeds the third
__device__ __forceinline__ float bf16_residual(float x) { return x - (float)(__bf16)x; }
// bits of the lo plane. The same value as bf16_bits(bf16_residual(x)), hi widened by a shift instead of a conversion: the two spellings
// compile to different instructions in the row kernels of fused.hip, so both stay, side by side
__device__ __forceinline__ unsigned short bf16_lo_bits(float x) { return bf16_bits(x - __uint_as_float((unsigned)bf16_bits(x) << 16)); }
__device__ __forceinline__ ushort4 bf16_bits4(const float4& v) { ushort4 q; q.x = bf16_bits(v.x); q.y = bf16_bits(v.y); q.z = bf16_bits(v.z); q.w = bf16_bits(v.w); return q; }
__device__ __forceinline__ ushort4 bf16_lo_bits4(const float4& v) { ushort4 q; q.x = bf16_lo_bits(v.x); q.y = bf16_lo_bits(v.y); q.z = bf16_lo_bits(v.z); q.w = bf16_lo_bits(v.w); return q; }
// two neighbours as one 32-bit word (a in the low half): the two-element vector conversion
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, v);
}

}  // namespace exorl
