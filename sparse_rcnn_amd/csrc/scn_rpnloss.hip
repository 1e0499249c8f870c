// The RPN loss of the reference (ndsis/modules/loss.py RpnLoss + BatchwiseBboxTargetSelector, ndsis/utils/bbox.py select_bbox +
// bbox_transform) on the device (include/scn_mi355x.h: scn_rpn_targets, scn_rpn_sample_batchwise, scn_rpn_loss,
// scn_rpn_loss_scale).
//
//   k_rpn_targets     IoU of every inside anchor against every ground-truth box of its sample, max + argmax (ties: lowest box),
//                     bbox_transform of the matched box.  The boxes of one sample are staged in LDS in chunks of kBoxChunk, each
//                     thread keeps kAnchorsPerThread anchors in registers.  The IoU is evaluated in the reference's operation
//                     order with round-to-nearest intrinsics (as k_nms in scn_elem.hip), so max_overlap is bit-equal to it.
//   k_sample_*        the batch-wide subsample: counts, then a radix select of the min_count smallest keys of the larger set
//                     (two 16-bit digits), then the weights.  key = a keyed 32-bit bijection of the flat index (4 rounds of
//                     xor-with-round-key + a bijective mixer), so keys never tie and exactly min_count members are drawn.
//   k_rpn_loss        BCE-with-logits over the scores, smooth-L1 over the deltas, both gradients for an upstream gradient of 1;
//                     the sums are reduced in double, per thread, per block (fixed tree), then one finishing block in block
//                     order: no float atomics, bitwise reproducible.
#include "scn_common.h"

#include <math.h>

#pragma clang fp contract(off)

using scn::S;

namespace {

constexpr int kTgtThreads = 256;
constexpr int kAnchorsPerThread = 2;
constexpr int kBoxChunk = 512;                               // boxes per LDS stage: 512 x 7 floats = 14 KB
constexpr int kMaxSamplesPerLaunch = 32;                     // box offsets travel in the kernel arguments

struct BoxOffsets {
    int64_t off[kMaxSamplesPerLaunch + 1];
};

__device__ __forceinline__ float volume3(float a, float b, float c) {   // size.prod(-1), left to right
    return (a * b) * c;
}

__global__ __launch_bounds__(kTgtThreads) void k_rpn_targets(const float* __restrict__ anchors, int64_t n,
                                                             const float* __restrict__ gt, const BoxOffsets offs, int b0,
                                                             float* __restrict__ max_ov, long long* __restrict__ argmax,
                                                             float* __restrict__ tgt) {
    __shared__ float sb[kBoxChunk][7];                       // start xyz, stop xyz, volume
    const int lb = blockIdx.y, b = b0 + lb;
    const int64_t g0 = offs.off[lb], G = offs.off[lb + 1] - g0;
    float as[kAnchorsPerThread][3], ae[kAnchorsPerThread][3], area[kAnchorsPerThread], best[kAnchorsPerThread];
    int64_t arg[kAnchorsPerThread];
    int64_t idx[kAnchorsPerThread];
#pragma unroll
    for (int p = 0; p < kAnchorsPerThread; ++p) {
        idx[p] = (int64_t)blockIdx.x * (kTgtThreads * kAnchorsPerThread) + p * kTgtThreads + threadIdx.x;
        const int64_t i = idx[p] < n ? idx[p] : 0;
        float pos[3], sz[3];
        for (int d = 0; d < 3; ++d) {
            pos[d] = anchors[i * 6 + d];
            sz[d] = anchors[i * 6 + 3 + d];
            const float half = sz[d] / 2.f;              // calc_start_end: size / 2, position -+ half
            as[p][d] = (pos[d] - half);
            ae[p][d] = (pos[d] + half);
        }
        area[p] = volume3(sz[0], sz[1], sz[2]);                  // the anchor's own size, not end - start
        best[p] = -INFINITY;
        arg[p] = 0;
    }
    for (int64_t c0 = 0; c0 < G; c0 += kBoxChunk) {
        const int cn = (int)(G - c0 < kBoxChunk ? G - c0 : kBoxChunk);
        __syncthreads();
        for (int j = threadIdx.x; j < cn; j += kTgtThreads) {
            const float* B = gt + (g0 + c0 + j) * 6;
            float v[6];
            for (int d = 0; d < 6; ++d) v[d] = B[d];
            for (int d = 0; d < 6; ++d) sb[j][d] = v[d];
            sb[j][6] = volume3((v[3] - v[0]), (v[4] - v[1]), (v[5] - v[2]));
        }
        __syncthreads();
        for (int j = 0; j < cn; ++j) {
            float bx[7];
            for (int d = 0; d < 7; ++d) bx[d] = sb[j][d];
#pragma unroll
            for (int p = 0; p < kAnchorsPerThread; ++p) {
                float inter = 1.f;                               // prod over the dims of clamp(min_end - max_start, 0)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float lo = fmaxf(as[p][d], bx[d]), hi = fminf(ae[p][d], bx[3 + d]);
                    const float e = fmaxf((hi - lo), 0.f);
                    inter = d == 0 ? e : (inter * e);
                }
                const float uni = (area[p] + bx[6]) - inter;
                const float q = (inter / uni);
                // overlaps.max(1): the first maximum wins; a NaN (0 / 0) wins over any number, as torch's max does
                if (q > best[p] || (q != q && best[p] == best[p])) {
                    best[p] = q;
                    arg[p] = c0 + j;
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < kAnchorsPerThread; ++p) {
        if (idx[p] >= n) continue;
        const int64_t i = idx[p];
        const int64_t o = (int64_t)b * n + i;
        float gs[3] = {0.f, 0.f, 0.f}, ge[3] = {0.f, 0.f, 0.f};      // no boxes: select_bbox's zero box
        if (G > 0) {
            const float* B = gt + (g0 + arg[p]) * 6;
            for (int d = 0; d < 3; ++d) {
                gs[d] = B[d];
                ge[d] = B[3 + d];
            }
        }
        max_ov[o] = G > 0 ? best[p] : 0.f;
        argmax[o] = G > 0 ? (long long)arg[p] : -1ll;
        float* T = tgt + o * 6;
        for (int d = 0; d < 3; ++d) {                        // bbox_transform_position_size (bbox.py:109-137,337-364)
            const float apos = anchors[i * 6 + d], asz = anchors[i * 6 + 3 + d];
            const float gsz = (ge[d] - gs[d]);
            const float gpos = gs[d] + 0.5f * gsz;
            const float den = (asz + 1e-14f);
            T[d] = (gpos - apos) / den;
            T[3 + d] = (float)log((double)(gsz / den + 1e-14f));   // (log in double: rounded once)
        }
    }
}

// ---- batch-wide sampling -----------------------------------------------------------------------------------------------
constexpr int kBins = 65536;
constexpr int kSampThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kBinsPerScanThread = kBins / kScanThreads;     // 64

struct SampleWs {                                            // include/scn_mi355x.h: zero before the first use, left zero
    unsigned int hist1[2][kBins];                            // [pos, neg][key >> 16]
    unsigned int hist2[kBins];                               // [key & 0xffff] of the larger set within bin b1
    unsigned long long acc[2];                               // pos / neg counts
    // written by k_sample_scan1 / _scan2 every call (no zero needed)
    long long n_pos, n_neg;
    int larger;                                              // 0: the positives are subsampled, 1: the negatives
    int k;                                                   // min_count
    unsigned int b1, r1;                                     // digit 1 of the k-th smallest key, 0-based rank inside it
    unsigned int thr;                                        // the k-th smallest key
    int pad;
};

struct Keys {
    unsigned int rk[4];
};

__device__ __forceinline__ unsigned int mix32(unsigned int x) {  // a bijection of the 32-bit integers
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ unsigned int sample_key(unsigned int i, const Keys& k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) i = mix32(i ^ k.rk[r]);
    return i;
}

// 0: positive, 1: negative, -1: neither (between the thresholds, or NaN)
__device__ __forceinline__ int sample_class(float ov, float pos_thr, float neg_thr) {
    return ov >= pos_thr ? 0 : (ov < neg_thr ? 1 : -1);
}

__global__ __launch_bounds__(kSampThreads) void k_sample_hist1(const float* __restrict__ ov, int64_t n, float pos_thr,
                                                               float neg_thr, const Keys keys, SampleWs* __restrict__ ws) {
    unsigned long long np = 0, nn = 0;
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (int64_t i = (int64_t)blockIdx.x * kSampThreads + threadIdx.x, base = (int64_t)blockIdx.x * kSampThreads; base < n;
         i += (int64_t)gridDim.x * kSampThreads, base += (int64_t)gridDim.x * kSampThreads) {
        const int c = i < n ? sample_class(ov[i], pos_thr, neg_thr) : -1;
        const unsigned long long bp = __ballot(c == 0), bn = __ballot(c == 1);
        if (lane0) {
            np += __popcll(bp);
            nn += __popcll(bn);
        }
        if (c >= 0) atomicAdd(&ws->hist1[c][sample_key((unsigned int)i, keys) >> 16], 1u);
    }
    if (lane0) {
        if (np) atomicAdd(&ws->acc[0], np);
        if (nn) atomicAdd(&ws->acc[1], nn);
    }
}

// One block: the digit of a 65536-bin histogram that holds the element of 0-based rank r.  -> (*bin, rank inside it)
__device__ void scan_find(const unsigned int* __restrict__ h, unsigned int r, unsigned int* bin, unsigned int* rin) {
    __shared__ unsigned int part[kScanThreads];
    const int t = threadIdx.x;
    unsigned int s = 0;
    for (int q = 0; q < kBinsPerScanThread; ++q) s += h[t * kBinsPerScanThread + q];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {       // inclusive scan (Hillis-Steele)
        const unsigned int v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const unsigned int hi = part[t], lo = hi - s;
    if (r >= lo && r < hi) {
        unsigned int cum = lo;
        for (int q = 0; q < kBinsPerScanThread; ++q) {
            const unsigned int c = h[t * kBinsPerScanThread + q];
            if (r < cum + c) {
                *bin = (unsigned int)(t * kBinsPerScanThread + q);
                *rin = r - cum;
                break;
            }
            cum += c;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kScanThreads) void k_sample_scan1(SampleWs* __restrict__ ws, long long* __restrict__ counts) {
    const long long np = (long long)ws->acc[0], nn = (long long)ws->acc[1];
    const int larger = np > nn ? 0 : 1;                      // pos == neg: the reference's else branch (negatives drawn)
    const long long k = np < nn ? np : nn;
    if (threadIdx.x == 0) {
        ws->n_pos = np;
        ws->n_neg = nn;
        ws->larger = larger;
        ws->k = (int)k;
        if (counts) {
            counts[0] = np;
            counts[1] = nn;
        }
    }
    if (k > 0) scan_find(ws->hist1[larger], (unsigned int)(k - 1), &ws->b1, &ws->r1);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * kBins; i += kScanThreads) (&ws->hist1[0][0])[i] = 0u;   // left zero for the next call
    if (threadIdx.x == 0) ws->acc[0] = ws->acc[1] = 0ull;
}

__global__ __launch_bounds__(kSampThreads) void k_sample_hist2(const float* __restrict__ ov, int64_t n, float pos_thr,
                                                               float neg_thr, const Keys keys, SampleWs* __restrict__ ws) {
    if (ws->k == 0) return;
    const int larger = ws->larger;
    const unsigned int b1 = ws->b1;
    for (int64_t i = (int64_t)blockIdx.x * kSampThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSampThreads) {
        if (sample_class(ov[i], pos_thr, neg_thr) != larger) continue;
        const unsigned int key = sample_key((unsigned int)i, keys);
        if ((key >> 16) == b1) atomicAdd(&ws->hist2[key & 0xffffu], 1u);
    }
}

__global__ __launch_bounds__(kScanThreads) void k_sample_scan2(SampleWs* __restrict__ ws) {
    __shared__ unsigned int b2, r2;
    if (ws->k > 0) {
        scan_find(ws->hist2, ws->r1, &b2, &r2);              // (keys are distinct: r2 == 0)
        if (threadIdx.x == 0) ws->thr = (ws->b1 << 16) | b2;
        __syncthreads();
        for (int i = threadIdx.x; i < kBins; i += kScanThreads) ws->hist2[i] = 0u;
    }
}

__global__ __launch_bounds__(kSampThreads) void k_sample_weights(const float* __restrict__ ov, int64_t n, float pos_thr,
                                                                 float neg_thr, float min_inverse_weight, const Keys keys,
                                                                 const SampleWs* __restrict__ ws, float* __restrict__ label,
                                                                 float* __restrict__ score_w, float* __restrict__ bbox_w) {
    const int larger = ws->larger, k = ws->k;
    const unsigned int thr = ws->thr;
    const long long den_s = 2ll * k > 1 ? 2ll * k : 1ll;     // max(1, 2 * min_count)
    const float inv_s = 1.f / (float)den_s;
    const float den_b = fmaxf((float)ws->n_pos, min_inverse_weight);   // labels.sum().clamp(min=1 / max_weight)
    for (int64_t i = (int64_t)blockIdx.x * kSampThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSampThreads) {
        const int c = sample_class(ov[i], pos_thr, neg_thr);
        const bool drawn = c == larger && k > 0 && sample_key((unsigned int)i, keys) <= thr;
        const bool kept = c >= 0 && c != larger;             // the smaller set, whole
        const float lab = c == 0 ? 1.f : 0.f;
        label[i] = lab;
        score_w[i] = (kept || drawn) ? inv_s : 0.f;
        bbox_w[i] = (lab / den_b);
    }
}

unsigned long long splitmix64(unsigned long long& s) {
    unsigned long long z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// ---- loss ----------------------------------------------------------------------------------------------------------------
constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 512;

int loss_blocks(int64_t n) {                                 // a function of n only: the same reduction tree on every device
    const int64_t b = scn::cdiv(n, (int64_t)kLossThreads * 4);
    return (int)(b < 1 ? 1 : (b > kLossMaxBlocks ? kLossMaxBlocks : b));
}

__device__ __forceinline__ void block_sum2(double& a, double& b) {   // fixed tree over the block; thread 0 holds the result
    __shared__ double sa[kLossThreads], sbb[kLossThreads];
    sa[threadIdx.x] = a;
    sbb[threadIdx.x] = b;
    __syncthreads();
    for (int off = kLossThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            sa[threadIdx.x] += sa[threadIdx.x + off];
            sbb[threadIdx.x] += sbb[threadIdx.x + off];
        }
        __syncthreads();
    }
    a = sa[0];
    b = sbb[0];
}

__global__ __launch_bounds__(kLossThreads) void k_rpn_loss(const float* __restrict__ score, const float* __restrict__ bbox,
                                                           const float* __restrict__ label, const float* __restrict__ score_w,
                                                           const float* __restrict__ tgt, const float* __restrict__ bbox_w,
                                                           int64_t n, float half_s2, float inv_s2, float half_inv_s2,
                                                           float* __restrict__ dscore, float* __restrict__ dbbox,
                                                           double* __restrict__ partial) {
    double ls = 0.0, lb = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLossThreads) {
        // binary_cross_entropy_with_logits: ((1 - t) * x - log_sigmoid(x)) * w;  d/dx = (sigmoid(x) - t) * w
        const float x = score[i], t = label[i], w = score_w[i];
        const float lsig = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
        ls += (double)(((1.f - t) * x - lsig) * w);
        const float sig = 1.f / (1.f + expf(-x));
        dscore[i] = (sig - t) * w;
        // smooth L1 (loss.py:240-252): |d| < 1 / sigma^2 ? d^2 sigma^2 / 2 : |d| - 0.5 / sigma^2, weighted per anchor
        const float wb = bbox_w[i];
        for (int c = 0; c < 6; ++c) {
            const float d = (bbox[i * 6 + c] - tgt[i * 6 + c]);
            const float a = fabsf(d);
            const bool m = a < inv_s2;
            const float in = m ? (d * d) * half_s2 : a - half_inv_s2;
            lb += (double)(wb * in);
            // autograd of the reference's expression: 2 * ((w * m) * sigma^2 / 2 * d) + (w * (1 - m)) * sign(d)
            const float g = (wb * half_s2) * d;
            dbbox[i * 6 + c] = m ? (g + g) : (d > 0.f ? wb : (d < 0.f ? -wb : 0.f));
        }
    }
    block_sum2(ls, lb);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ls;
        partial[2 * blockIdx.x + 1] = lb;
    }
}

__global__ __launch_bounds__(kLossThreads) void k_rpn_loss_finish(const double* __restrict__ partial, int nb,
                                                                  float* __restrict__ score_loss, float* __restrict__ bbox_loss) {
    double ls = 0.0, lb = 0.0;
    for (int b = threadIdx.x; b < nb; b += kLossThreads) {
        ls += partial[2 * b];
        lb += partial[2 * b + 1];
    }
    block_sum2(ls, lb);
    if (threadIdx.x == 0) {
        *score_loss = (float)ls;
        *bbox_loss = (float)lb;
    }
}

__global__ __launch_bounds__(kLossThreads) void k_rpn_loss_scale(const float* __restrict__ dscore, const float* __restrict__ dbbox,
                                                                 int64_t n, const float* __restrict__ gs, const float* __restrict__ gb,
                                                                 float* __restrict__ out_s, float* __restrict__ out_b) {
    const float s = gs ? *gs : 0.f, b = gb ? *gb : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < 7 * n; i += (int64_t)gridDim.x * kLossThreads) {
        if (i < n) {
            if (out_s) out_s[i] = (dscore[i] * s);
        } else if (out_b) {
            out_b[i - n] = (dbbox[i - n] * b);
        }
    }
}

}  // namespace

extern "C" int scn_rpn_targets(const float* anchors, int64_t n_anchors, const float* gt_boxes, const int64_t* box_offsets,
                               int batch, float* max_overlap, int64_t* argmax, float* bbox_target, scn_stream_t stream) {
    SCN_REQUIRE(n_anchors >= 0 && batch >= 0 && box_offsets);
    if (batch == 0) return SCN_OK;
    SCN_REQUIRE(box_offsets[0] >= 0);
    for (int b = 0; b < batch; ++b) SCN_REQUIRE(box_offsets[b + 1] >= box_offsets[b]);
    if (n_anchors == 0) return SCN_OK;
    SCN_REQUIRE(anchors && max_overlap && argmax && bbox_target && (gt_boxes || box_offsets[batch] == box_offsets[0]));
    const int gx = (int)scn::cdiv(n_anchors, (int64_t)kTgtThreads * kAnchorsPerThread);
    for (int b0 = 0; b0 < batch; b0 += kMaxSamplesPerLaunch) {
        const int nb = batch - b0 < kMaxSamplesPerLaunch ? batch - b0 : kMaxSamplesPerLaunch;
        BoxOffsets o;
        for (int q = 0; q <= kMaxSamplesPerLaunch; ++q) o.off[q] = box_offsets[b0 + (q <= nb ? q : nb)];
        hipLaunchKernelGGL(k_rpn_targets, dim3(gx, nb), dim3(kTgtThreads), 0, S(stream), anchors, n_anchors, gt_boxes, o, b0,
                           max_overlap, (long long*)argmax, bbox_target);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

extern "C" int64_t scn_rpn_sample_workspace_bytes(void) { return (int64_t)sizeof(SampleWs); }

extern "C" int scn_rpn_sample_batchwise(const float* overlaps, int64_t n, float positive_overlap, float negative_overlap,
                                        float min_inverse_weight, uint64_t seed, uint64_t counter, void* workspace,
                                        float* label, float* score_weight, float* bbox_weight, int64_t* counts,
                                        scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && n <= 0x7fffffffLL && workspace && ((uintptr_t)workspace & 7) == 0);
    SCN_REQUIRE(negative_overlap <= positive_overlap && min_inverse_weight == min_inverse_weight);
    SCN_REQUIRE(n == 0 || (overlaps && label && score_weight && bbox_weight));
    Keys keys;
    unsigned long long s = seed ^ (counter * 0xd1b54a32d192ed03ull);
    s = splitmix64(s) ^ counter;
    for (int r = 0; r < 4; ++r) keys.rk[r] = (unsigned int)(splitmix64(s) >> 32);
    SampleWs* ws = (SampleWs*)workspace;
    const int g = scn::ew_grid(n, kSampThreads);
    if (n > 0) {
        hipLaunchKernelGGL(k_sample_hist1, dim3(g), dim3(kSampThreads), 0, S(stream), overlaps, n, positive_overlap,
                           negative_overlap, keys, ws);
        SCN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_sample_scan1, dim3(1), dim3(kScanThreads), 0, S(stream), ws, (long long*)counts);
    SCN_LAUNCH_CHECK();
    if (n == 0) return SCN_OK;
    hipLaunchKernelGGL(k_sample_hist2, dim3(g), dim3(kSampThreads), 0, S(stream), overlaps, n, positive_overlap,
                       negative_overlap, keys, ws);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_scan2, dim3(1), dim3(kScanThreads), 0, S(stream), ws);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sample_weights, dim3(g), dim3(kSampThreads), 0, S(stream), overlaps, n, positive_overlap,
                       negative_overlap, min_inverse_weight, keys, (const SampleWs*)ws, label, score_weight, bbox_weight);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int64_t scn_rpn_loss_scratch_bytes(int64_t n) { return (int64_t)loss_blocks(n) * 2 * (int64_t)sizeof(double); }

extern "C" int scn_rpn_loss(const float* score, const float* bbox, const float* label, const float* score_weight,
                            const float* bbox_target, const float* bbox_weight, int64_t n, float sigma, void* scratch,
                            float* score_loss, float* bbox_loss, float* dscore, float* dbbox, scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && sigma > 0.f && sigma < INFINITY && scratch && ((uintptr_t)scratch & 7) == 0 && score_loss && bbox_loss);
    SCN_REQUIRE(n == 0 || (score && bbox && label && score_weight && bbox_target && bbox_weight && dscore && dbbox));
    const double s2 = (double)sigma * (double)sigma;         // the reference's python floats: sigma ** 2, then / 2 and 1 / ...
    const int nb = loss_blocks(n);
    hipLaunchKernelGGL(k_rpn_loss, dim3(nb), dim3(kLossThreads), 0, S(stream), score, bbox, label, score_weight, bbox_target,
                       bbox_weight, n, (float)(s2 / 2.), (float)(1. / s2), (float)(0.5 / s2), dscore, dbbox, (double*)scratch);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rpn_loss_finish, dim3(1), dim3(kLossThreads), 0, S(stream), (const double*)scratch, nb, score_loss,
                       bbox_loss);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_rpn_loss_scale(const float* dscore, const float* dbbox, int64_t n, const float* grad_score_loss,
                                  const float* grad_bbox_loss, float* out_dscore, float* out_dbbox, scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && (!out_dscore || (dscore && grad_score_loss)) && (!out_dbbox || (dbbox && grad_bbox_loss)));
    if (n == 0 || (!out_dscore && !out_dbbox)) return SCN_OK;
    hipLaunchKernelGGL(k_rpn_loss_scale, dim3(scn::ew_grid(7 * n, kLossThreads)), dim3(kLossThreads), 0, S(stream), dscore, dbbox,
                       n, out_dscore ? grad_score_loss : nullptr, out_dbbox ? grad_bbox_loss : nullptr, out_dscore, out_dbbox);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}
