// Adam / AdamW parameter update over a list of fp32 segments (include/scn_mi355x.h: scn_adam_many).
//
// The arithmetic mirrors torch.optim.Adam's single-tensor, non-capturable path (torch/optim/adam.py::_single_tensor_adam)
// operation by operation, with torch's GPU forms of each operation: the two-branch lerp, `alpha * (b * c)` for addcmul, the
// division by a host scalar as a multiplication by its reciprocal (rounded to float once), `a + alpha * (b / c)` for addcdiv -- each
// `a + alpha * x` as the one fused multiply-add torch's compiled kernels make of it.  Implicit FMA contraction is off in this
// file, and `/` and sqrtf are correctly rounded (hipcc's default for fp32; NOT __fsqrt_rn, which the HIP headers map to the
// approximate native square root), so every step rounds exactly as written.
//
// The update is bandwidth-bound (28 B per parameter: p, g, m, v read, p, m, v written).  One launch covers up to
// kMaxSegs segments; the segment table travels BY VALUE in the kernel arguments, so there is no upload, no staging buffer
// and no host wait.  Each workgroup owns one chunk of one segment (a search over the segments' first-block indices finds
// it); a segment whose four pointers share their offset modulo 16 bytes runs 16-byte loads after a scalar head of at most
// 3 elements, any other segment (views at arbitrary float offsets) runs scalar.
#include "scn_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                   // float4 per thread in flight per stream
constexpr int kChunk = kThreads * 4 * kUnroll;               // elements per workgroup: 4096
constexpr int kMaxSegs = 80;                                 // segments per launch (the arguments stay below 4 KB)
constexpr int kMaxConsts = 4;                                // distinct per-segment constant sets per launch

struct Seg {                                                 // 48 B
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int32_t block0;                                          // first workgroup of this segment in the launch
    int16_t head;                                            // scalar elements before the 16-byte aligned body; -1: scalar only
    int16_t cset;                                            // index into Batch::cst
};

struct Cst {
    float neg_step_size;                                     // -lr / (1 - beta1^t)
    float inv_bc2;                                           // 1 / sqrt(1 - beta2^t)
    float wd;                                                // coupled weight decay (0: none)
    float decay;                                             // decoupled: p *= decay (1: none)
};

struct Batch {
    Seg seg[kMaxSegs];
    Cst cst[kMaxConsts];
    int32_t nseg;
    float gs, w1, b2, omb2, eps;                             // grad scale, 1 - beta1, beta2, 1 - beta2, eps
};
static_assert(sizeof(Batch) < 4000, "kernel arguments");

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const Cst& c, float gs, float w1, float b2,
                                      float omb2, float eps) {
    // torch's GPU kernels are compiled with FMA contraction: `a + alpha * b` in add / lerp / addcmul / addcdiv is one fused
    // multiply-add there, and is written as one here (__fmaf_rn); nothing else contracts in this file
    g = g * gs;
    if (c.wd != 0.f) g = __fmaf_rn(c.wd, p, g);             // grad.add(param, alpha=weight_decay)
    p = p * c.decay;                                         // param.mul_(1 - lr * weight_decay); exact when decay == 1
    m = (w1 < 0.5f) ? __fmaf_rn(w1, g - m, m)                // exp_avg.lerp_(grad, 1 - beta1), torch's two branches
                    : __fmaf_rn(-(g - m), 1.f - w1, g);
    v = __fmaf_rn(omb2, g * g, v * b2);                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) * c.inv_bc2 + eps;          // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = __fmaf_rn(c.neg_step_size, m / denom, p);            // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ void adam_at(const Seg& s, int64_t i, const Cst& c, const Batch& b) {
    float p = s.p[i], m = s.m[i], v = s.v[i];
    adam1(p, s.g[i], m, v, c, b.gs, b.w1, b.b2, b.omb2, b.eps);
    s.p[i] = p;
    s.m[i] = m;
    s.v[i] = v;
}

__global__ __launch_bounds__(kThreads) void k_adam(const Batch b) {
    const int blk = blockIdx.x;
    int lo = 0, hi = b.nseg - 1;                             // last segment whose block0 <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (b.seg[mid].block0 <= blk) lo = mid; else hi = mid - 1;
    }
    const Seg s = b.seg[lo];
    const Cst c = b.cst[s.cset];
    const int64_t chunk = blk - s.block0;
    const int t = threadIdx.x;
    if (s.head < 0) {
        const int64_t beg = chunk * kChunk;
        const int64_t end = beg + kChunk < s.n ? beg + kChunk : s.n;
        for (int64_t i = beg + t; i < end; i += kThreads) adam_at(s, i, c, b);
        return;
    }
    const int64_t h = s.head < s.n ? s.head : s.n;
    const int64_t nv = (s.n - h) >> 2;                       // float4 groups of the aligned body
    const int64_t last = nv > 0 ? (nv - 1) / (kChunk / 4) : 0;
    if (chunk == 0 && t < h) adam_at(s, t, c, b);
    if (chunk == last && h + 4 * nv + t < s.n) adam_at(s, h + 4 * nv + t, c, b);
    float4* P = reinterpret_cast<float4*>(s.p + h);
    const float4* G = reinterpret_cast<const float4*>(s.g + h);
    float4* M = reinterpret_cast<float4*>(s.m + h);
    float4* V = reinterpret_cast<float4*>(s.v + h);
    const int64_t v0 = chunk * (kChunk / 4) + t;
    float4 rp[kUnroll], rg[kUnroll], rm[kUnroll], rv[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
        const int64_t i = v0 + k * kThreads;
        if (i < nv) {
            rp[k] = P[i];
            rg[k] = G[i];
            rm[k] = M[i];
            rv[k] = V[i];
        }
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
        const int64_t i = v0 + k * kThreads;
        if (i < nv) {
            adam1(rp[k].x, rg[k].x, rm[k].x, rv[k].x, c, b.gs, b.w1, b.b2, b.omb2, b.eps);
            adam1(rp[k].y, rg[k].y, rm[k].y, rv[k].y, c, b.gs, b.w1, b.b2, b.omb2, b.eps);
            adam1(rp[k].z, rg[k].z, rm[k].z, rv[k].z, c, b.gs, b.w1, b.b2, b.omb2, b.eps);
            adam1(rp[k].w, rg[k].w, rm[k].w, rv[k].w, c, b.gs, b.w1, b.b2, b.omb2, b.eps);
            P[i] = rp[k];
            M[i] = rm[k];
            V[i] = rv[k];
        }
    }
}

int64_t seg_blocks(int64_t n, int head) {
    if (head < 0) return (n + kChunk - 1) / kChunk;
    const int64_t h = head < n ? head : n;
    const int64_t nv = (n - h) >> 2;
    return nv > 0 ? (nv + kChunk / 4 - 1) / (kChunk / 4) : 1;
}

int seg_head(const scn_adam_segment& s) {
    const uintptr_t a = (uintptr_t)s.p & 15;
    if (((uintptr_t)s.g & 15) != a || ((uintptr_t)s.m & 15) != a || ((uintptr_t)s.v & 15) != a) return -1;
    return (int)((16 - a) & 15) / 4;
}

// Validates everything first (nothing is launched for a bad table), then walks the batches; stream == NULL with
// `launches` set: count only.
int adam_run(const scn_adam_segment* segs, int n_segs, double grad_scale, double beta1, double beta2, double eps,
             scn_stream_t stream, int* launches, bool launch) {
    SCN_REQUIRE(n_segs >= 0 && (segs != nullptr || n_segs == 0));
    SCN_REQUIRE(isfinite(grad_scale) && isfinite(beta1) && isfinite(beta2) && isfinite(eps));
    for (int i = 0; i < n_segs; ++i) {
        const scn_adam_segment& s = segs[i];
        if (s.n < 0) return scn::fail(SCN_EINVAL, "scn_adam_many: segment %s%lld has n = %lld < 0", "", i, s.n);
        if (s.n > 0 && (!s.p || !s.g || !s.m || !s.v))
            return scn::fail(SCN_EINVAL, "scn_adam_many: segment %s%lld has a null pointer", "", i);
        if (((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 3)
            return scn::fail(SCN_EINVAL, "scn_adam_many: segment %s%lld: a pointer is not 4-byte aligned", "", i);
        if (!isfinite(s.step_size) || !isfinite(s.inv_bc2_sqrt) || !(s.inv_bc2_sqrt > 0.f) || !isfinite(s.weight_decay) ||
            !isfinite(s.decay))
            return scn::fail(SCN_EINVAL, "scn_adam_many: segment %s%lld: step_size / inv_bc2_sqrt / weight_decay / decay "
                             "not finite (or inv_bc2_sqrt <= 0)", "", i);
    }
    Batch b;
    b.gs = (float)grad_scale;
    b.w1 = (float)(1.0 - beta1);                              // torch: lerp weight 1 - beta1 in double, rounded to float
    b.b2 = (float)beta2;
    b.omb2 = (float)(1.0 - beta2);
    b.eps = (float)eps;
    int nb = 0, nc = 0, count = 0;
    int64_t blocks = 0;
    auto flush = [&]() -> int {
        if (nb == 0) return SCN_OK;
        b.nseg = nb;
        ++count;
        if (launch) {
            hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, b);
            SCN_LAUNCH_CHECK();
        }
        nb = nc = 0;
        blocks = 0;
        return SCN_OK;
    };
    for (int i = 0; i < n_segs; ++i) {
        const scn_adam_segment& s = segs[i];
        if (s.n == 0) continue;
        Cst c;
        c.neg_step_size = -s.step_size;
        c.inv_bc2 = s.inv_bc2_sqrt;
        c.wd = s.weight_decay;
        c.decay = s.decay;
        const int head = seg_head(s);
        const int64_t sb = seg_blocks(s.n, head);
        if (sb > (int64_t)1 << 30)
            return scn::fail(SCN_EINVAL, "scn_adam_many: segment %s%lld is too large (%lld elements)", "", i, s.n);
        int ci = -1;
        for (int k = 0; k < nc; ++k)
            if (!memcmp(&b.cst[k], &c, sizeof(Cst))) ci = k;
        if (nb == kMaxSegs || (ci < 0 && nc == kMaxConsts) || blocks + sb > ((int64_t)1 << 31) - 1) {
            const int rc = flush();
            if (rc) return rc;
            ci = -1;
        }
        if (ci < 0) {
            b.cst[nc] = c;
            ci = nc++;
        }
        Seg& d = b.seg[nb++];
        d.p = s.p;
        d.g = s.g;
        d.m = s.m;
        d.v = s.v;
        d.n = s.n;
        d.block0 = (int32_t)blocks;
        d.head = (int16_t)head;
        d.cset = (int16_t)ci;
        blocks += sb;
    }
    const int rc = flush();
    if (launches) *launches = count;
    return rc;
}

}  // namespace

extern "C" int64_t scn_adam_segment_bytes(void) { return (int64_t)sizeof(scn_adam_segment); }

extern "C" int scn_adam_launches(const scn_adam_segment* segs, int n_segs, int* launches) {
    SCN_REQUIRE(launches != nullptr);
    return adam_run(segs, n_segs, 1.0, 0.9, 0.999, 1e-8, nullptr, launches, false);
}

extern "C" int scn_adam_many(const scn_adam_segment* segs, int n_segs, double grad_scale, double beta1, double beta2,
                             double eps, scn_stream_t stream) {
    return adam_run(segs, n_segs, grad_scale, beta1, beta2, eps, stream, nullptr, true);
}
