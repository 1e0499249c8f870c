// Device-side draws of the sample conversion (scn_rng.h: Philox4x32-10, a pure function of seed / sample counter / stream /
// index).
//
//   scn_philox_words_host  the generator compiled for the host: what C callers and the CPU tests check the header with.
//   scn_philox_fill        the words, or sigma * normal triples, of a run of indices as a tensor -- exactly what the fused
//                          pack kernel (scn_sample.hip, k_sample_pack<true>) adds without ever storing it.
//   scn_sample_cut_start   random_cut_out's start positions (ndsis/data/sparse_augmentation.py:50-78) in ONE launch of ONE
//                          workgroup: per dimension, in the drawn order, a pass over the voxels for min / max / count of
//                          the ones the dimensions before left alive, then the draw.  "Alive" is recomputed from the starts
//                          decided so far; nothing is stored per point.  200 000 voxels are 2.4 MB per pass.
#include "scn_common.h"
#include "scn_rng.h"

#include <limits.h>

using scn::S;

namespace {

__global__ __launch_bounds__(256) void k_philox_fill(unsigned long long seed, unsigned long long counter, unsigned stream,
                                                     unsigned first, long long n, int mode, float sigma, void* out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const scn_rng_words d = scn_rng_draw(seed, counter, stream, first + (unsigned)i);
        if (mode == 0) {
            unsigned* o = (unsigned*)out + 4 * i;                                 // (4-byte stores: `out` owes no alignment)
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = d.w[k];
        } else {
            float z[3];
            scn_rng_normal3(d, z);
            float* o = (float*)out + 3 * i;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = scn_rng_noise(sigma, z[k]);
        }
    }
}

constexpr int kCutThreads = 1024, kCutWaves = kCutThreads / 64;

// a[d] of three values without an indexed private array (which the compiler would move to LDS, 12 bytes per thread)
// a start position as int32: lo - border and the drawn start are formed in 64 bits and saturate instead of wrapping
__device__ __forceinline__ int sat_i32(long long v) { return v < INT_MIN ? INT_MIN : (v > INT_MAX ? INT_MAX : (int)v); }
__device__ __forceinline__ int pick3(int a0, int a1, int a2, int d) { return d == 0 ? a0 : (d == 1 ? a1 : a2); }

// One workgroup.  Pass k (k = 0 .. 3) counts the voxels inside the windows of the dimensions decided before it and, for
// k < 3, takes min / max of dimension order[k] over them; thread 0 then decides that dimension's start.  The pass that finds
// no voxel alive -- or pass 3 -- ends the loop: its count is the "alive" output and k the number of dimensions processed.
__global__ __launch_bounds__(kCutThreads) void k_sample_cut_start(const int* __restrict__ discrete, long long n, int z0, int z1,
                                                                   int z2, int b0, int b1, int b2, unsigned long long seed,
                                                                   unsigned long long counter, int* __restrict__ out8) {
    __shared__ int s_lo[kCutWaves], s_hi[kCutWaves], s_cnt[kCutWaves];
    __shared__ int s_start[3], s_on[3], s_order[3], s_stop;
    const int size[3] = {z0, z1, z2};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        const scn_rng_words d = scn_rng_draw(seed, counter, SCN_RNG_CUT, 0);
        const int i = (int)(((unsigned long long)d.w[0] * 3ull) >> 32), j = (int)(((unsigned long long)d.w[1] * 2ull) >> 32);
        const int r0 = i == 0 ? 1 : 0, r1 = i == 2 ? 1 : 2;                      // [0, 1, 2] without element i ...
        s_order[0] = i;
        s_order[1] = j ? r1 : r0;                                                // ... then element j of the rest: one is left
        s_order[2] = j ? r0 : r1;
        for (int k = 0; k < 3; ++k) { s_start[k] = 0; s_on[k] = 0; }
        s_stop = 0;
    }
    __syncthreads();
    int processed = 0, alive = 0;
    for (int k = 0; k < 4; ++k) {
        const int dim = k < 3 ? s_order[k] : 0;
        int st[3], on[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) { st[d] = s_start[d]; on[d] = s_on[d]; }
        int lo = INT_MAX, hi = INT_MIN, cnt = 0;
        for (long long p = threadIdx.x; p < n; p += kCutThreads) {
            int v[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) v[d] = discrete[3 * p + d];
            bool in = true;
#pragma unroll
            for (int d = 0; d < 3; ++d) {                                        // (64-bit: col - start of any two int32 values)
                const long long moved = (long long)v[d] - st[d];
                in = in && (!on[d] || (moved >= 0 && moved < size[d]));
            }
            if (in) {
                const int c = pick3(v[0], v[1], v[2], dim);
                lo = min(lo, c);
                hi = max(hi, c);
                ++cnt;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o));
            hi = max(hi, __shfl_xor(hi, o));
            cnt += __shfl_xor(cnt, o);
        }
        if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; s_cnt[wave] = cnt; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kCutWaves; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); cnt += s_cnt[w]; }
            alive = cnt;
            processed = k;
            if (k == 3 || cnt == 0) {
                s_stop = 1;
            } else {
                const int sz = pick3(z0, z1, z2, dim), bd = pick3(b0, b1, b2, dim);
                const long long min_start = (long long)lo - bd;
                const long long max_start = (long long)hi + 1 - sz + bd;
                if (max_start <= min_start) {
                    s_start[dim] = sat_i32(min_start);                              // empty range: no draw, nothing filtered
                } else {
                    const scn_rng_words d = scn_rng_draw(seed, counter, SCN_RNG_CUT, 1);
                    const unsigned long long span = (unsigned long long)(max_start - min_start);
                    const unsigned wk = pick3((int)d.w[0], (int)d.w[1], (int)d.w[2], k);
                    s_start[dim] = sat_i32(min_start + (long long)(((unsigned long long)wk * span) >> 32));
                    s_on[dim] = 1;
                }
            }
        }
        __syncthreads();
        if (s_stop) break;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { out8[d] = s_start[d]; out8[3 + d] = s_order[d]; }
        out8[6] = alive;
        out8[7] = processed;
    }
}

}  // namespace

extern "C" int scn_philox_words_host(uint64_t seed, uint64_t counter, uint32_t stream, uint32_t index, uint32_t* out4) {
    SCN_REQUIRE(out4);
    const scn_rng_words d = scn_rng_draw(seed, counter, stream, index);
    for (int k = 0; k < 4; ++k) out4[k] = d.w[k];
    return SCN_OK;
}

extern "C" int scn_philox_fill(uint64_t seed, uint64_t counter, uint32_t stream, int64_t first_index, int64_t n, int mode,
                               float sigma, void* out, scn_stream_t stream_handle) {
    SCN_REQUIRE(n >= 0 && first_index >= 0 && (mode == 0 || mode == 1));
    if (first_index > 4294967296LL || n > 4294967296LL - first_index)
        return scn::fail(SCN_ESIZE, "scn_philox_fill%s: indices %lld + %lld leave the 32-bit index word", "", first_index, n);
    if (n == 0) return SCN_OK;
    SCN_REQUIRE(out);
    hipLaunchKernelGGL(k_philox_fill, dim3(scn::ew_grid(n, 256)), dim3(256), 0, S(stream_handle), (unsigned long long)seed,
                       (unsigned long long)counter, (unsigned)stream, (unsigned)first_index, (long long)n, mode, sigma, out);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_sample_cut_start(const int32_t* discrete, int64_t n, const int32_t* size_host, const int32_t* border_host,
                                    uint64_t seed, uint64_t counter, int32_t* out8, scn_stream_t stream) {
    SCN_REQUIRE(n >= 1 && n < 2147483647LL && discrete && size_host && border_host && out8);
    SCN_REQUIRE(size_host[0] >= 1 && size_host[1] >= 1 && size_host[2] >= 1);
    SCN_REQUIRE(border_host[0] >= 0 && border_host[1] >= 0 && border_host[2] >= 0);
    SCN_REQUIRE(border_host[0] <= size_host[0] && border_host[1] <= size_host[1] && border_host[2] <= size_host[2]);
    hipLaunchKernelGGL(k_sample_cut_start, dim3(1), dim3(kCutThreads), 0, S(stream), discrete, (long long)n, size_host[0],
                       size_host[1], size_host[2], border_host[0], border_host[1], border_host[2], (unsigned long long)seed,
                       (unsigned long long)counter, out8);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}
