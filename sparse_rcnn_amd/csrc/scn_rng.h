// The counter-based generator of the sample conversion's draws: Philox4x32-10 (Salmon et al., "Parallel random numbers: as
// easy as 1, 2, 3", SC'11; the Random123 constants).  One definition for host and device, plain 32 x 32 -> 64 multiplies.
//
//   key     = (seed lo32, seed hi32)
//   counter = (index, stream, sample counter lo32, sample counter hi32)
//
// so a value is a function of (seed, sample counter, stream, index) and of nothing else -- not of the launch shape, the
// order of the calls or any state.  Streams (include/scn_mi355x.h SCN_RNG_*): 0 the host's draws (distortion matrix, mirror,
// angle, sub-pixel offset), 1 the random cut-out, 2 / 3 the per-point colour / normal noise (index = kept row), 4 / 5 the
// common colour / normal noise (index 0).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SCN_RNG_HD __host__ __device__ inline
#else
#define SCN_RNG_HD inline
#endif

struct scn_rng_words { uint32_t w[4]; };

SCN_RNG_HD scn_rng_words scn_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;                                // the Weyl sequence of the key, bumped after every round
        k1 += 0xBB67AE85u;
    }
    scn_rng_words r;
    r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
    return r;
}

SCN_RNG_HD scn_rng_words scn_rng_draw(uint64_t seed, uint64_t counter, uint32_t stream, uint32_t index) {
    return scn_philox4x32_10(index, stream, (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ((w >> 9) + 0.5) * 2^-23: a 23-bit integer plus a half is exact in fp32, the result lies in (0, 1) and is never 0.
SCN_RNG_HD float scn_rng_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }

#if defined(__HIPCC__)
// Three standard normals of one draw (Box-Muller; the second sine is not used).  The accurate logf / sqrtf / sincospif:
// every operation is rounded once and nothing is contracted, so every kernel that calls this gets the same bits.
__device__ __forceinline__ void scn_rng_normal3(const scn_rng_words& d, float z[3]) {
#pragma clang fp contract(off)
    const float r0 = sqrtf(-2.f * logf(scn_rng_uniform(d.w[0])));
    const float r1 = sqrtf(-2.f * logf(scn_rng_uniform(d.w[2])));
    float s0, c0, s1, c1;
    sincospif(2.f * scn_rng_uniform(d.w[1]), &s0, &c0);
    sincospif(2.f * scn_rng_uniform(d.w[3]), &s1, &c1);
    z[0] = r0 * c0;
    z[1] = r0 * s0;
    z[2] = r1 * c1;
}

// A noise value, sigma * z, and a feature with it, v + sigma * z: a multiply and an add, each rounded once.  Written with plain
// operators under contract(off) on purpose: HIP's __fmul_rn / __fadd_rn are `x * y` / `x + y` compiled where contraction is
// allowed, and the pair of them fuses into ONE fma -- a bit off what the add of a stored sigma * z gives.
__device__ __forceinline__ float scn_rng_noise(float sigma, float z) {
#pragma clang fp contract(off)
    return sigma * z;
}
__device__ __forceinline__ float scn_rng_add_noise(float v, float sigma, float z) {
#pragma clang fp contract(off)
    const float nz = sigma * z;
    return v + nz;
}
#endif
