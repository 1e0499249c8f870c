// Training-sample conversion on the device: what ndsis/data/sparse_augmentation.py `convert_sample` (:250-313) does after
// augment_coords -- get_masks (:208-234), get_bbox (:188-205), get_semantic_segmentation_labels (:237-247), augment_features
// (:152-185).  The coordinate part is scn_vox_* (scn_elem.hip); the random draws are inputs.
//
//   scn_sample_stats  one pass over the N stored points: per instance slot 0 .. I the number of points, the number the
//                     cut-out keeps, and min / max of the kept points' final voxel coordinates.  Integers only: every
//                     workgroup collects in an LDS table, then merges it into the global one with integer atomics, so the
//                     result is exact and the same from run to run whatever the order.
//   scn_sample_pack   one pass over the M kept rows: features, segmentation labels, and the kept instances' point masks as
//                     bits in loss.PackedMasks' layout (a wave's 64 rows are two words; the rows of one instance are
//                     combined with a ballot before one integer OR per word).
// The selection between the two (ratio of two exact counts > threshold, boxes, labels) is a few hundred values: the host
// does it from one copy of the stats table (sparse_rcnn_amd/sample.py).
#include "scn_common.h"
#include "scn_rng.h"

#include <limits.h>

using scn::S;

namespace {

constexpr int kStatCols = 8;                          // total, inside, min x y z, max x y z

__device__ __forceinline__ int stat_identity(int col) { return col < 2 ? 0 : (col < 5 ? INT_MAX : INT_MIN); }

__global__ void k_sample_stats_init(int slots, int* __restrict__ stats, int* __restrict__ n_bad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < slots * kStatCols) stats[t] = stat_identity(t % kStatCols);
    if (t == 0) *n_bad = 0;
}

__global__ __launch_bounds__(256) void k_sample_stats(const int* __restrict__ discrete, const int* __restrict__ table,
                                                      const long long* __restrict__ ids, long long n, int slots, int s0,
                                                      int s1, int s2, int* __restrict__ stats, int* __restrict__ n_bad) {
    extern __shared__ int tab[];                       // [slots][kStatCols]
    for (int t = threadIdx.x; t < slots * kStatCols; t += blockDim.x) tab[t] = stat_identity(t % kStatCols);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int st[3] = {s0, s1, s2};
    int bad = 0;
    // (the loop condition is the wave's first point: uniform, so the ballots below see the whole wave)
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i - lane < n; i += (long long)gridDim.x * blockDim.x) {
        const bool valid = i < n;
        int sid = -2, inside = 0, v[3] = {0, 0, 0};
        if (valid) {
            const long long id = ids[i];
            sid = (id >= 0 && id < slots) ? (int)id : -1;
            inside = table[i] >= 0;
            if (inside) {
#pragma unroll
                for (int d = 0; d < 3; ++d) v[d] = discrete[3 * i + d] - st[d];
            }
        }
        const unsigned long long vm = __ballot(valid);
        const int lead = __ffsll((long long)vm) - 1;
        const int sid_lead = __shfl(sid, lead);
        if (__ballot(valid && sid != sid_lead) == 0) {
            // mesh order: the 64 points of a wave mostly belong to ONE instance -> reduce in registers, one lane updates
            const unsigned long long im = __ballot(inside);
            int mn[3], mx[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                mn[d] = inside ? v[d] : INT_MAX;
                mx[d] = inside ? v[d] : INT_MIN;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    mn[d] = min(mn[d], __shfl_xor(mn[d], o));
                    mx[d] = max(mx[d], __shfl_xor(mx[d], o));
                }
            }
            if (lane == lead) {
                if (sid_lead < 0) {
                    bad += __popcll(vm);
                } else {
                    int* row = tab + sid_lead * kStatCols;
                    atomicAdd(row, __popcll(vm));
                    if (im) {
                        atomicAdd(row + 1, __popcll(im));
#pragma unroll
                        for (int d = 0; d < 3; ++d) {
                            atomicMin(row + 2 + d, mn[d]);
                            atomicMax(row + 5 + d, mx[d]);
                        }
                    }
                }
            }
        } else if (valid) {
            if (sid < 0) {
                ++bad;
            } else {
                int* row = tab + sid * kStatCols;
                atomicAdd(row, 1);
                if (inside) {
                    atomicAdd(row + 1, 1);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        atomicMin(row + 2 + d, v[d]);
                        atomicMax(row + 5 + d, v[d]);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < slots * kStatCols; t += blockDim.x) {
        const int col = t % kStatCols, val = tab[t];
        if (val == stat_identity(col)) continue;
        if (col < 2) atomicAdd(stats + t, val);
        else if (col < 5) atomicMin(stats + t, val);
        else atomicMax(stats + t, val);
    }
    if (bad) atomicAdd(n_bad, bad);
}

struct PackArgs {
    const int* rows; long long m;
    const float* colors; const float* normals; const long long* ids; int slots;
    float r[9];
    const float* cnoise; int cnoise_pp; const float* nnoise; int nnoise_pp;
    int use_color, use_ones, use_normal, c;
    float* feats;
    const long long* seg_table; long long* seg;
    const int* slot_of; long long w; unsigned* words;
};

// Where the noise comes from is a compile-time variant of ONE kernel body.  kDrawn = false: the tensors above, the kernel
// scn_sample_pack has always launched (its argument block is PackArgs and nothing else).  kDrawn = true: the noise of kept
// row p is drawn in place (scn_rng.h: streams 2 / 3 with index p, or the common draw of streams 4 / 5 with index 0) and
// added as v + sigma * z, each rounded once -- the bits scn_sample_pack gives when fed what scn_philox_fill writes.
template <bool kDrawn> struct PackArgsT : PackArgs {};
template <> struct PackArgsT<true> : PackArgs {
    unsigned long long seed, counter;
    float csigma, nsigma;                              // 0 = no noise, no generator call
    int ccommon, ncommon;
};

template <bool kDrawn>
__global__ __launch_bounds__(256) void k_sample_pack(PackArgsT<kDrawn> a) {
    const int lane = threadIdx.x & 63;
    [[maybe_unused]] float ccz[3] = {0.f, 0.f, 0.f}, ncz[3] = {0.f, 0.f, 0.f};
    if constexpr (kDrawn) {
        if (a.feats && a.use_color && a.csigma != 0.f && a.ccommon) scn_rng_normal3(scn_rng_draw(a.seed, a.counter, SCN_RNG_COLOR_COMMON, 0), ccz);
        if (a.feats && a.use_normal && a.nsigma != 0.f && a.ncommon) scn_rng_normal3(scn_rng_draw(a.seed, a.counter, SCN_RNG_NORMAL_COMMON, 0), ncz);
    }
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p - lane < a.m; p += (long long)gridDim.x * blockDim.x) {
        int slot = -1;
        if (p < a.m) {
            const long long r = a.rows[p];
            if (a.feats) {
                float* f = a.feats + p * a.c;
                if (a.use_color) {
                    [[maybe_unused]] float z[3] = {ccz[0], ccz[1], ccz[2]};
                    if constexpr (kDrawn) {
                        if (a.csigma != 0.f && !a.ccommon) scn_rng_normal3(scn_rng_draw(a.seed, a.counter, SCN_RNG_COLOR, (uint32_t)p), z);
                    }
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float v = a.colors[3 * r + d];
                        if constexpr (kDrawn) f[d] = a.csigma != 0.f ? scn_rng_add_noise(v, a.csigma, z[d]) : v;
                        else f[d] = a.cnoise ? __fadd_rn(v, a.cnoise[a.cnoise_pp ? 3 * p + d : d]) : v;
                    }
                    f += 3;
                }
                if (a.use_ones) *f++ = 1.f;
                if (a.use_normal) {
                    const float x = a.normals[3 * r], y = a.normals[3 * r + 1], z = a.normals[3 * r + 2];
                    [[maybe_unused]] float nz[3] = {ncz[0], ncz[1], ncz[2]};
                    if constexpr (kDrawn) {
                        if (a.nsigma != 0.f && !a.ncommon) scn_rng_normal3(scn_rng_draw(a.seed, a.counter, SCN_RNG_NORMAL, (uint32_t)p), nz);
                    }
#pragma unroll
                    for (int d = 0; d < 3; ++d) {          // the association of k_vox_project: torch's CPU matmul for K = 3
                        const float v = fmaf(z, a.r[6 + d], fmaf(y, a.r[3 + d], __fmul_rn(x, a.r[d])));
                        if constexpr (kDrawn) f[d] = a.nsigma != 0.f ? scn_rng_add_noise(v, a.nsigma, nz[d]) : v;
                        else f[d] = a.nnoise ? __fadd_rn(v, a.nnoise[a.nnoise_pp ? 3 * p + d : d]) : v;
                    }
                }
            }
            if (a.ids) {
                const long long id = a.ids[r];
                const int sid = (id >= 0 && id < a.slots) ? (int)id : a.slots - 1;    // (outside 0 .. I: "no instance"; counted by the stats)
                if (a.seg) a.seg[p] = a.seg_table[sid];
                if (a.slot_of) slot = a.slot_of[sid];
            }
        }
        // rows p - lane .. p - lane + 63 are words (p - lane) / 32 and the next one of every instance's mask row
        unsigned long long todo = __ballot(slot >= 0);
        while (todo) {
            const int sl = __shfl(slot, __ffsll((long long)todo) - 1);
            const unsigned long long mk = __ballot(slot == sl);
            unsigned* word = a.words + (long long)sl * a.w + ((p - lane) >> 5);
            if (lane == 0 && (unsigned)mk) atomicOr(word, (unsigned)mk);
            if (lane == 32 && (unsigned)(mk >> 32)) atomicOr(word + 1, (unsigned)(mk >> 32));
            todo &= ~mk;
        }
    }
}

}  // namespace

extern "C" int scn_sample_stats(const int32_t* discrete, const int32_t* table, const int64_t* instance_ids, int64_t n,
                                int n_instances, const int32_t* start_host, int32_t* stats, int32_t* n_bad_ids,
                                scn_stream_t stream) {
    SCN_REQUIRE(n >= 1 && n < 2147483647LL && discrete && table && instance_ids && start_host && stats && n_bad_ids);
    SCN_REQUIRE(n_instances >= 0);
    if (n_instances > SCN_SAMPLE_MAX_INSTANCES)
        return scn::fail(SCN_ESIZE, "scn_sample_stats%s: %lld instances, the LDS table holds %lld", "", n_instances,
                         SCN_SAMPLE_MAX_INSTANCES);
    const int slots = n_instances + 1;
    hipLaunchKernelGGL(k_sample_stats_init, dim3((slots * kStatCols + 255) / 256), dim3(256), 0, S(stream), slots, stats, n_bad_ids);
    SCN_LAUNCH_CHECK();
    int64_t blocks = scn::cdiv(n, 2048);               // >= 8 points per thread before a workgroup's table is merged
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(k_sample_stats, dim3((unsigned)blocks), dim3(256), (size_t)slots * kStatCols * sizeof(int), S(stream),
                       discrete, table, (const long long*)instance_ids, (long long)n, slots, start_host[0], start_host[1],
                       start_host[2], stats, n_bad_ids);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

// The argument checks and the launch of both pack entry points; `a` arrives with its noise source filled in.
template <bool kDrawn>
static int sample_pack_run(PackArgsT<kDrawn>& a, const char* who, const int32_t* rows, int64_t m, const float* colors,
                           const float* normals, const int64_t* instance_ids, int n_instances, const float* rotation_host,
                           int use_color, int use_ones, int use_normal, float* features, const int64_t* seg_table,
                           int64_t* seg_labels, const int32_t* slot_of_instance, int64_t n_kept, uint32_t* mask_words,
                           scn_stream_t stream) {
    SCN_REQUIRE(m >= 0 && m < 2147483647LL && n_kept >= 0 && n_instances >= 0);
    if (n_instances > SCN_SAMPLE_MAX_INSTANCES)
        return scn::fail(SCN_ESIZE, "%s: %lld instances, at most %lld", who, n_instances, SCN_SAMPLE_MAX_INSTANCES);
    if (m == 0) return SCN_OK;                         // no kept row: no feature, no label, no mask word
    const int c = (use_color ? 3 : 0) + (use_ones ? 1 : 0) + (use_normal ? 3 : 0);
    SCN_REQUIRE(rows && (c == 0 || features));
    SCN_REQUIRE(!use_color || colors);
    SCN_REQUIRE(!use_normal || (normals && rotation_host));
    SCN_REQUIRE((seg_labels == nullptr) == (seg_table == nullptr));
    SCN_REQUIRE(n_kept == 0 || (slot_of_instance && mask_words));
    SCN_REQUIRE((!seg_labels && n_kept == 0) || instance_ids);
    a.rows = rows; a.m = m; a.colors = colors; a.normals = normals;
    a.ids = (seg_labels || n_kept) ? (const long long*)instance_ids : nullptr;
    a.slots = n_instances + 1;
    for (int k = 0; k < 9; ++k) a.r[k] = use_normal ? rotation_host[k] : 0.f;
    a.use_color = use_color ? 1 : 0; a.use_ones = use_ones ? 1 : 0; a.use_normal = use_normal ? 1 : 0; a.c = c;
    a.feats = c ? features : nullptr;
    a.seg_table = (const long long*)seg_table; a.seg = (long long*)seg_labels;
    a.slot_of = n_kept ? slot_of_instance : nullptr;
    a.w = (m + 31) / 32; a.words = mask_words;
    if (n_kept) SCN_HIP(hipMemsetAsync(mask_words, 0, (size_t)n_kept * (size_t)a.w * sizeof(uint32_t), S(stream)));
    if (!a.feats && !a.ids) return SCN_OK;
    hipLaunchKernelGGL(k_sample_pack<kDrawn>, dim3(scn::ew_grid(m, 256)), dim3(256), 0, S(stream), a);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_sample_pack(const int32_t* rows, int64_t m, const float* colors, const float* normals,
                               const int64_t* instance_ids, int n_instances, const float* rotation_host,
                               const float* color_noise, int color_noise_per_point, const float* normal_noise,
                               int normal_noise_per_point, int use_color, int use_ones, int use_normal, float* features,
                               const int64_t* seg_table, int64_t* seg_labels, const int32_t* slot_of_instance, int64_t n_kept,
                               uint32_t* mask_words, scn_stream_t stream) {
    PackArgsT<false> a;
    a.cnoise = use_color ? color_noise : nullptr; a.cnoise_pp = color_noise_per_point ? 1 : 0;
    a.nnoise = use_normal ? normal_noise : nullptr; a.nnoise_pp = normal_noise_per_point ? 1 : 0;
    return sample_pack_run<false>(a, "scn_sample_pack", rows, m, colors, normals, instance_ids, n_instances, rotation_host,
                                  use_color, use_ones, use_normal, features, seg_table, seg_labels, slot_of_instance, n_kept,
                                  mask_words, stream);
}

extern "C" int scn_sample_pack_drawn(const int32_t* rows, int64_t m, const float* colors, const float* normals,
                                     const int64_t* instance_ids, int n_instances, const float* rotation_host, uint64_t seed,
                                     uint64_t counter, float color_sigma, int color_common, float normal_sigma,
                                     int normal_common, int use_color, int use_ones, int use_normal, float* features,
                                     const int64_t* seg_table, int64_t* seg_labels, const int32_t* slot_of_instance,
                                     int64_t n_kept, uint32_t* mask_words, scn_stream_t stream) {
    SCN_REQUIRE(color_sigma == color_sigma && normal_sigma == normal_sigma);      // a NaN sigma is no amount of noise
    PackArgsT<true> a;
    a.cnoise = nullptr; a.cnoise_pp = 0; a.nnoise = nullptr; a.nnoise_pp = 0;
    a.seed = seed; a.counter = counter;
    a.csigma = use_color ? color_sigma : 0.f; a.nsigma = use_normal ? normal_sigma : 0.f;
    a.ccommon = color_common ? 1 : 0; a.ncommon = normal_common ? 1 : 0;
    return sample_pack_run<true>(a, "scn_sample_pack_drawn", rows, m, colors, normals, instance_ids, n_instances,
                                 rotation_host, use_color, use_ones, use_normal, features, seg_table, seg_labels,
                                 slot_of_instance, n_kept, mask_words, stream);
}
