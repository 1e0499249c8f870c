// Global-norm gradient clipping over a list of fp32 segments: the step executor's SCN_OP_GRAD_NORM and SCN_OP_GRAD_SCALE
// (include/scn_mi355x.h; library-internal, scn_common.h: reached through scn_exec_run, not entry points of the C ABI).
// torch.nn.utils.clip_grad_norm_ with norm_type 2 on the device: no host wait, a fixed summation order, a handful of launches.
//
// Norm: S = sum of squares, accumulated in DOUBLE from the first element (the pass is bandwidth-bound -- 4 B read per element --
// so the fp64 FMAs are hidden; fp32 squares overflow above 1.8e19).  The order is fixed: each workgroup owns one 4096-element
// chunk of one segment (k_adam's deal, scn_optim.hip) and writes ONE double to the pass's shared scratch -- per thread its
// elements in ascending order, the 64 lanes of a wave by a shuffle tree, the 4 waves in wave order -- and a final launch of one
// workgroup adds the partial sums: thread t those at t, t + 256, ... in ascending order, then the 256 sums by the same tree.  No
// atomics, no arrival counter: same bits run to run.  The final launch writes the 4-float record {total_norm, clip_coef,
// nonfinite, 0}; the coefficient is torch's fp32 expression (contraction is off in this file, `/` is correctly rounded).
//
// Scale: g *= record[1] in place; a workgroup that reads 1.0f returns before it touches the gradient (x * 1.0f is x on every
// bit pattern), so the unclipped step costs the norm's one read and nothing else.
//
// The segment table travels BY VALUE in the kernel arguments (at most 80 segments per launch); a segment whose pointer is
// 16-byte aligned after a scalar head of at most 3 elements runs 16-byte accesses, which is every 4-byte aligned pointer.
#include "scn_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                   // float4 per thread in flight
constexpr int kChunk = kThreads * 4 * kUnroll;               // elements per workgroup: 4096
constexpr int kMaxSegs = 80;                                 // segments per launch (the arguments stay below 4 KB)

struct Seg {                                                 // 24 B
    float* g;
    int64_t n;
    int32_t block0;                                          // first workgroup of this segment in the launch
    int32_t head;                                            // scalar elements before the 16-byte aligned body
};

struct Batch {
    Seg seg[kMaxSegs];
    int32_t nseg;
    int32_t part0;                                           // index of this launch's first partial sum
};
static_assert(sizeof(Batch) < 4000, "kernel arguments");

__device__ __forceinline__ Seg find_seg(const Batch& b, int blk) {
    int lo = 0, hi = b.nseg - 1;                             // last segment whose block0 <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b.seg[mid].block0 <= blk) lo = mid; else hi = mid - 1;
    }
    return b.seg[lo];
}

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double wave_sum[kThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += wave_sum[w];
    }
    return s;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(kThreads) void k_grad_sumsq(const Batch b, double* __restrict__ partial) {
    const int blk = blockIdx.x;
    const Seg s = find_seg(b, blk);
    const int64_t chunk = blk - s.block0;
    const int t = threadIdx.x;
    const int64_t h = s.head < s.n ? s.head : s.n;
    const int64_t nv = (s.n - h) >> 2;                       // float4 groups of the aligned body
    const int64_t last = nv > 0 ? (nv - 1) / (kChunk / 4) : 0;
    double acc = 0.0;
    if (chunk == 0 && t < h) acc += sq(s.g[t]);
    if (chunk == last && h + 4 * nv + t < s.n) acc += sq(s.g[h + 4 * nv + t]);
    const float4* G = reinterpret_cast<const float4*>(s.g + h);
    const int64_t v0 = chunk * (kChunk / 4) + t;
    float4 r[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
        const int64_t i = v0 + k * kThreads;
        r[k] = i < nv ? G[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
        acc += sq(r[k].x);
        acc += sq(r[k].y);
        acc += sq(r[k].z);
        acc += sq(r[k].w);
    }
    const double sum = block_sum(acc);
    if (t == 0) partial[b.part0 + blk] = sum;
}

__global__ __launch_bounds__(kThreads) void k_grad_norm_record(const double* __restrict__ partial, int64_t n_partial, float gs_abs,
                                                               float max_norm, float* __restrict__ record) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_partial; i += kThreads) acc += partial[i];
    const double S = block_sum(acc);
    if (threadIdx.x != 0) return;
    const float total = (float)(sqrt(S) * (double)gs_abs);
    float c = max_norm / (total + 1e-6f);                    // torch: max_norm / (total_norm + 1e-6), clamp(max=1.0): a NaN stays
    c = c > 1.f ? 1.f : c;
    record[0] = total;
    record[1] = c;
    record[2] = isfinite(S) ? 0.f : 1.f;
    record[3] = 0.f;
}

__global__ __launch_bounds__(kThreads) void k_grad_scale(const Batch b, const float* __restrict__ record) {
    const float coef = record[1];
    if (coef == 1.0f) return;                                // not clipped: the gradient is not touched
    const int blk = blockIdx.x;
    const Seg s = find_seg(b, blk);
    const int64_t chunk = blk - s.block0;
    const int t = threadIdx.x;
    const int64_t h = s.head < s.n ? s.head : s.n;
    const int64_t nv = (s.n - h) >> 2;
    const int64_t last = nv > 0 ? (nv - 1) / (kChunk / 4) : 0;
    if (chunk == 0 && t < h) s.g[t] = s.g[t] * coef;
    if (chunk == last && h + 4 * nv + t < s.n) s.g[h + 4 * nv + t] = s.g[h + 4 * nv + t] * coef;
    float4* G = reinterpret_cast<float4*>(s.g + h);
    const int64_t v0 = chunk * (kChunk / 4) + t;
    float4 r[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
        const int64_t i = v0 + k * kThreads;
        if (i < nv) r[k] = G[i];
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
        const int64_t i = v0 + k * kThreads;
        if (i < nv) {
            r[k].x = r[k].x * coef;
            r[k].y = r[k].y * coef;
            r[k].z = r[k].z * coef;
            r[k].w = r[k].w * coef;
            G[i] = r[k];
        }
    }
}

inline int seg_head(const float* g) { return (int)((16 - ((uintptr_t)g & 15)) & 15) / 4; }

inline int64_t seg_blocks(int64_t n, int head) {
    const int64_t h = head < n ? head : n;
    const int64_t nv = (n - h) >> 2;
    return nv > 0 ? (nv + kChunk / 4 - 1) / (kChunk / 4) : 1;
}

// Nothing is launched for a bad table.
int check_table(const char* op, void* const* grads, const int64_t* prefix, int64_t T) {
    if (T < 0) return scn::fail(SCN_EINVAL, "%s: %lld segments", op, T);
    if (T > 0 && (!grads || !prefix)) return scn::fail(SCN_EINVAL, "%s: no gradient table or no count prefix", op);
    for (int64_t i = 0; i < T; ++i) {
        const int64_t n = prefix[i + 1] - prefix[i];
        if (n < 0) return scn::fail(SCN_EINVAL, "%s: segment %lld has n = %lld < 0", op, i, n);
        if (n > 0 && !grads[i]) return scn::fail(SCN_EINVAL, "%s: segment %lld has a null pointer", op, i);
        if ((uintptr_t)grads[i] & 3) return scn::fail(SCN_EINVAL, "%s: segment %lld: the pointer is not 4-byte aligned", op, i);
        if (n > ((int64_t)1 << 40)) return scn::fail(SCN_EINVAL, "%s: segment %lld is too large (%lld elements)", op, i, n);
    }
    return SCN_OK;
}

// Walks the table in launches of at most kMaxSegs segments; `each(batch, blocks)` launches one.
template <typename F>
int for_batches(void* const* grads, const int64_t* prefix, int64_t T, F each) {
    Batch b;
    int nb = 0;
    int64_t blocks = 0, part = 0;
    auto flush = [&]() -> int {
        if (nb == 0) return SCN_OK;
        b.nseg = nb;
        b.part0 = (int32_t)part;
        const int rc = each(b, blocks);
        part += blocks;
        nb = 0;
        blocks = 0;
        return rc;
    };
    for (int64_t i = 0; i < T; ++i) {
        const int64_t n = prefix[i + 1] - prefix[i];
        if (n == 0) continue;
        float* g = (float*)grads[i];
        const int head = seg_head(g);
        const int64_t sb = seg_blocks(n, head);
        if (part + blocks + sb > ((int64_t)1 << 31) - 1)     // (part0 is an int32; a table of 8e12 elements)
            return scn::fail(SCN_EINVAL, "%sgradient clipping: the table is too large (segment %lld)", "", i);
        if (nb == kMaxSegs || blocks + sb > ((int64_t)1 << 30)) {
            const int rc = flush();
            if (rc) return rc;
        }
        Seg& d = b.seg[nb++];
        d.g = g;
        d.n = n;
        d.block0 = (int32_t)blocks;
        d.head = head;
        blocks += sb;
    }
    return flush();
}

}  // namespace

// Workgroups of the partial-sum launches of a count prefix, counted without the pointers: a segment's 16-byte form never takes
// more workgroups than its scalar count ceil(n / 4096).  -1: a negative count or no prefix.
int64_t scn::grad_norm_blocks(const int64_t* prefix, int64_t T) {
    if (T < 0 || (T > 0 && !prefix)) return -1;
    int64_t blocks = 0;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t n = prefix[i + 1] - prefix[i];
        if (n < 0) return -1;
        blocks += (n + kChunk - 1) / kChunk;
    }
    return blocks;
}

int scn::grad_norm(void* const* grads, const int64_t* prefix, int64_t T, float grad_scale, float max_norm, float* record,
                   void* scratch, int64_t scratch_bytes, scn_stream_t stream) {
    static const char* op = "SCN_OP_GRAD_NORM";
    if (!record || ((uintptr_t)record & 3)) return scn::fail(SCN_EINVAL, "%s: y names no 4-byte aligned record buffer", op);
    const int rc0 = check_table(op, grads, prefix, T);
    if (rc0) return rc0;
    const int64_t need = scn::grad_norm_blocks(prefix, T) * (int64_t)sizeof(double);
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < need)
        return scn::fail(SCN_EINVAL, "%s: the scratch holds %lld bytes, the partial sums take %lld", op, scratch_bytes, need);
    double* partial = (double*)scratch;
    int64_t n_partial = 0;
    const int rc = for_batches(grads, prefix, T, [&](const Batch& b, int64_t blocks) -> int {
        hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)blocks), dim3(kThreads), 0, scn::S(stream), b, partial);
        SCN_LAUNCH_CHECK();
        n_partial += blocks;
        return SCN_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_grad_norm_record, dim3(1), dim3(kThreads), 0, scn::S(stream), (const double*)partial, n_partial,
                       fabsf(grad_scale), max_norm, record);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

int scn::grad_scale(void* const* grads, const int64_t* prefix, int64_t T, const float* record, scn_stream_t stream) {
    static const char* op = "SCN_OP_GRAD_SCALE";
    if (!record || ((uintptr_t)record & 3)) return scn::fail(SCN_EINVAL, "%s: x1 names no 4-byte aligned record buffer", op);
    const int rc0 = check_table(op, grads, prefix, T);
    if (rc0) return rc0;
    return for_batches(grads, prefix, T, [&](const Batch& b, int64_t blocks) -> int {
        hipLaunchKernelGGL(k_grad_scale, dim3((unsigned)blocks), dim3(kThreads), 0, scn::S(stream), b, record);
        SCN_LAUNCH_CHECK();
        return SCN_OK;
    });
}
