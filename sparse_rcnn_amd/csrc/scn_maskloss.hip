// The mask loss of the reference (ndsis/modules/model.py OverlapCalculator, TrainSelector, SparseMaskLossSelector;
// ndsis/modules/loss.py MaskLoss) on the device (include/scn_mi355x.h: scn_mask_overlap_draw, scn_mask_loss,
// scn_mask_loss_bwd, scn_mask_pack).
//
//   k_mask_overlap_draw  one workgroup per sample: the IoU of every proposal against every ground-truth box of the sample
//                        (boxes staged in LDS 512 at a time), max + first-index argmax, in bbox_overlap_prediction's operation
//                        order with every operation rounded once (as k_rpn_targets), so the overlaps and the >= threshold
//                        decisions are bit-equal to the reference.  Then the draw: every positive gets a key = a keyed 32-bit
//                        bijection of (sample, index); the rank of a key among the sample's positive keys is counted in LDS,
//                        and the min(num_positive, #positives) smallest keys fill the first slots in key order.  Keys never
//                        tie, so the draw is uniform without replacement and a function of (seed, counter) only.
//   k_mask_loss_boxes    one workgroup per forward box: its rows (box-major CSR: found by two binary searches in box_of), the
//                        logit column of the associated instance's label, the instance's mask bit, BCE-with-logits summed
//                        in double in a fixed order (per thread, then a fixed tree), and sigmoid(x) - t per row.
//   k_mask_loss_finish   one block: valid = rows > 0 and a ground truth, optional class weights, the weighted mean (double,
//                        fixed order), and every box's gradient factor w_b / (rows_b * W).  Reruns are bitwise identical.
//   k_mask_loss_bwd      dlogits = g * (sigmoid(x) - t) * factor in the label column, zero elsewhere (as k_mask_gather_bwd).
//   k_mask_pack          bool [G_s][N_s] per sample -> uint32 words [G_s][ceil(N_s / 32)], bit p % 32 of word p / 32.
#include "scn_common.h"

#include <math.h>

#pragma clang fp contract(off)

using scn::S;

namespace {

constexpr int kMaxSamplesPerLaunch = 32;                     // per-sample tables travel in the kernel arguments
constexpr int kDrawThreads = 256;
constexpr int kMaxProposals = 1024;                          // per sample
constexpr int kPropPerThread = kMaxProposals / kDrawThreads;
constexpr int kBoxChunk = 512;                               // ground-truth boxes per LDS stage (14 KB)

struct DrawTable {
    int64_t pred_off[kMaxSamplesPerLaunch + 1];              // proposals of sample s: rows pred_off[s] .. pred_off[s+1]-1
    int64_t gt_off[kMaxSamplesPerLaunch + 1];                // ground-truth boxes of sample s
    int64_t fwd_off[kMaxSamplesPerLaunch + 1];               // forward boxes of sample s: cap_s slots, then G_s boxes
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

__device__ __forceinline__ unsigned int draw_key(unsigned int i, const Keys& k) {
#pragma unroll
    for (int r = 0; r < 4; ++r) i = mix32(i ^ k.rk[r]);
    return i;
}

__device__ __forceinline__ float volume3(float a, float b, float c) {   // size.prod(-1), left to right
    return (a * b) * c;
}

__global__ __launch_bounds__(kDrawThreads) void k_mask_overlap_draw(
    const float* __restrict__ pred, const float* __restrict__ gt, const DrawTable tab, int b0, float* __restrict__ max_ov,
    long long* __restrict__ argmax, int given, float pos_thr, int num_pos, const Keys keys, float* __restrict__ fwd,
    long long* __restrict__ assoc, long long* __restrict__ pred_sel, long long* __restrict__ n_drawn) {
    __shared__ float sb[kBoxChunk][7];                       // start xyz, stop xyz, volume
    __shared__ unsigned int skey[kMaxProposals];
    __shared__ int spos[kMaxProposals];
    __shared__ int sslot[kMaxProposals];
    __shared__ long long sarg[kMaxProposals];
    __shared__ int snpos;
    const int ls = blockIdx.x, s = b0 + ls;
    const int64_t p0 = tab.pred_off[ls], P = tab.pred_off[ls + 1] - p0;
    const int64_t g0 = tab.gt_off[ls], G = tab.gt_off[ls + 1] - g0;
    float as[kPropPerThread][3], ae[kPropPerThread][3], area[kPropPerThread], best[kPropPerThread];
    int64_t arg[kPropPerThread];
#pragma unroll
    for (int q = 0; q < kPropPerThread; ++q) {
        const int64_t i = q * kDrawThreads + threadIdx.x;
        float sz[3];
        for (int d = 0; d < 3; ++d) {
            as[q][d] = ae[q][d] = 0.f;
            if (i < P) {
                as[q][d] = pred[(p0 + i) * 6 + d];
                ae[q][d] = pred[(p0 + i) * 6 + 3 + d];
            }
            sz[d] = (ae[q][d] - as[q][d]);                   // prepare_overlap_from_start_end: end - start
        }
        area[q] = volume3(sz[0], sz[1], sz[2]);
        best[q] = -INFINITY;
        arg[q] = 0;
    }
    if (!given) {
        for (int64_t c0 = 0; c0 < G; c0 += kBoxChunk) {
            const int cn = (int)(G - c0 < kBoxChunk ? G - c0 : kBoxChunk);
            __syncthreads();
            for (int j = threadIdx.x; j < cn; j += kDrawThreads) {
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
                for (int q = 0; q < kPropPerThread; ++q) {
                    const float o = scn_box_iou(as[q], ae[q], area[q], bx);
                    // overlaps.max(1): the first maximum wins; a NaN (0 / 0) wins over any number, as torch's max does
                    if (o > best[q] || (o != o && best[q] == best[q])) {
                        best[q] = o;
                        arg[q] = c0 + j;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kPropPerThread; ++q) {
        const int64_t i = q * kDrawThreads + threadIdx.x;
        if (i >= P) continue;
        if (given) {
            best[q] = max_ov[p0 + i];
            arg[q] = argmax[p0 + i];
        } else {
            if (G == 0) {                                    // max_with_default: 0 and 0
                best[q] = 0.f;
                arg[q] = 0;
            }
            if (max_ov) max_ov[p0 + i] = best[q];
            if (argmax) argmax[p0 + i] = (long long)arg[q];
        }
    }
    if (!fwd) return;
    // ---- the draw ----
    if (threadIdx.x == 0) snpos = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPropPerThread; ++q) {
        const int i = q * kDrawThreads + threadIdx.x;
        const bool pos = i < P && best[q] >= pos_thr;        // (NaN: not positive)
        spos[i] = pos ? 1 : 0;
        sarg[i] = (long long)arg[q];
        skey[i] = draw_key(((unsigned int)s << 16) | (unsigned int)i, keys);
        if (pos) atomicAdd(&snpos, 1);
    }
    __syncthreads();
    const int npos = snpos;
    const int cap = (int)(tab.fwd_off[ls + 1] - tab.fwd_off[ls] - G);
    const int nd = npos < num_pos ? npos : num_pos;         // (cap >= nd: checked on the host)
#pragma unroll
    for (int q = 0; q < kPropPerThread; ++q) {
        const int i = q * kDrawThreads + threadIdx.x;
        if (i >= P || !spos[i]) continue;
        const unsigned int k = skey[i];
        int rank = 0;                                        // (keys are distinct: ranks are too)
        for (int j = 0; j < P; ++j) rank += (spos[j] && skey[j] < k) ? 1 : 0;
        if (rank < nd) sslot[rank] = i;
    }
    __syncthreads();
    const int64_t f0 = tab.fwd_off[ls];
    for (int q = threadIdx.x; q < cap + G; q += kDrawThreads) {
        float* F = fwd + (f0 + q) * 6;
        if (q < cap) {
            const int i = q < nd ? sslot[q] : -1;
            if (i >= 0) {
                const float* B = pred + (p0 + i) * 6;
                for (int d = 0; d < 6; ++d) F[d] = B[d];
            } else {
                for (int d = 0; d < 6; ++d) F[d] = 0.f;      // start = stop = 0: selects no point
            }
            assoc[f0 + q] = i >= 0 ? sarg[i] : -1ll;
            if (pred_sel) pred_sel[f0 - tab.gt_off[ls] + q] = i;   // (slots before this sample: f0 - its ground truths)
        } else {
            const int64_t g = q - cap;
            const float* B = gt + (g0 + g) * 6;
            for (int d = 0; d < 6; ++d) F[d] = B[d];
            assoc[f0 + q] = g;
        }
    }
    if (n_drawn && threadIdx.x == 0) n_drawn[s] = nd;
}

// ---- loss ----------------------------------------------------------------------------------------------------------------
constexpr int kLossThreads = 256;

struct LossTable {
    int64_t box_off[kMaxSamplesPerLaunch + 1];               // forward boxes of sample s (global box indices)
    int64_t gt_off[kMaxSamplesPerLaunch + 1];                // labels of sample s
    int64_t word_off[kMaxSamplesPerLaunch + 1];              // mask words of sample s: [G_s][ceil(N_s / 32)]
    int64_t pt_off[kMaxSamplesPerLaunch + 1];                // point rows of sample s
};

struct LossScratch {                                         // carved out of the caller's scratch (scn_mask_loss_scratch_bytes)
    double* sum;                                             // [n_boxes] BCE sum of the box
    long long* rows;                                         // [n_boxes]
    float* factor;                                           // [n_boxes] w_b / (rows_b * W), 0 for a dropped box
    int* label;                                              // [n_boxes] the logit column, -1: dropped
    float* draw;                                             // [m] sigmoid(x) - t
};

__host__ __device__ inline LossScratch carve(void* p, int64_t n_boxes, int64_t m) {
    char* c = (char*)p;
    LossScratch s;
    s.sum = (double*)c;
    c += 8 * n_boxes;
    s.rows = (long long*)c;
    c += 8 * n_boxes;
    s.factor = (float*)c;
    c += 4 * n_boxes;
    s.label = (int*)c;
    c += 4 * n_boxes;
    s.draw = (float*)c;
    return s;
}

__device__ __forceinline__ int64_t lower_bound(const int* __restrict__ a, int64_t n, int v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double block_sum(double a) {     // fixed tree over the block; every thread gets the result
    __shared__ double sa[kLossThreads];
    sa[threadIdx.x] = a;
    __syncthreads();
    for (int off = kLossThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sa[threadIdx.x] += sa[threadIdx.x + off];
        __syncthreads();
    }
    const double r = sa[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kLossThreads) void k_mask_loss_boxes(
    const float* __restrict__ logits, int64_t m, int k, const int* __restrict__ src_row, const int* __restrict__ box_of,
    const long long* __restrict__ assoc, const long long* __restrict__ labels, const unsigned int* __restrict__ words,
    const LossTable tab, int nb, LossScratch sc) {
    __shared__ long long srange[2];
    const int64_t b = tab.box_off[0] + blockIdx.x;
    int ls = 0;
    while (ls + 1 < nb && tab.box_off[ls + 1] <= b) ++ls;
    if (threadIdx.x == 0) srange[0] = lower_bound(box_of, m, (int)b);
    if (threadIdx.x == 64) srange[1] = lower_bound(box_of, m, (int)(b + 1));
    __syncthreads();
    const int64_t lo = srange[0], hi = srange[1];
    const int64_t G = tab.gt_off[ls + 1] - tab.gt_off[ls];
    const int64_t N = tab.pt_off[ls + 1] - tab.pt_off[ls], W = (N + 31) / 32;
    const long long a = assoc[b];
    long long lab = -1;
    if (a >= 0 && a < G) {
        lab = labels[tab.gt_off[ls] + a];
        if (lab < 0 || lab >= k) lab = -1;                   // (a label outside the logit columns: the box is dropped)
    }
    double acc = 0.0;
    if (lab < 0) {
        for (int64_t r = lo + threadIdx.x; r < hi; r += kLossThreads) sc.draw[r] = 0.f;
    } else {
        const unsigned int* mw = words + tab.word_off[ls] + a * W;
        for (int64_t r = lo + threadIdx.x; r < hi; r += kLossThreads) {
            const float x = logits[r * k + lab];
            const int64_t p = (int64_t)src_row[r] - tab.pt_off[ls];
            const float t = (p >= 0 && p < N) ? (float)((mw[p >> 5] >> (p & 31)) & 1u) : 0.f;
            // binary_cross_entropy_with_logits: (1 - t) * x - log_sigmoid(x);  d/dx = sigmoid(x) - t
            const float lsig = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
            acc += (double)((1.f - t) * x - lsig);
            const float sig = 1.f / (1.f + expf(-x));
            sc.draw[r] = (sig - t);
        }
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) {
        sc.sum[b] = acc;
        sc.rows[b] = hi - lo;
        sc.label[b] = (int)lab;
    }
}

__global__ __launch_bounds__(kLossThreads) void k_mask_loss_finish(int64_t n_boxes, const float* __restrict__ class_weights,
                                                                   float* __restrict__ loss, LossScratch sc) {
    double w_sum = 0.0, l_sum = 0.0;
    for (int64_t b = threadIdx.x; b < n_boxes; b += kLossThreads) {
        const int lab = sc.label[b];
        const long long n = sc.rows[b];
        if (lab < 0 || n <= 0) continue;                     // the reference's NaN (mean over no point): dropped
        const double w = class_weights ? (double)class_weights[lab] : 1.0;
        w_sum += w;
        l_sum += w * (sc.sum[b] / (double)n);
    }
    w_sum = block_sum(w_sum);
    l_sum = block_sum(l_sum);
    if (threadIdx.x == 0) *loss = w_sum != 0.0 ? (float)(l_sum / w_sum) : 0.f;
    for (int64_t b = threadIdx.x; b < n_boxes; b += kLossThreads) {
        const int lab = sc.label[b];
        const long long n = sc.rows[b];
        float f = 0.f;
        if (lab >= 0 && n > 0 && w_sum != 0.0) {
            const double w = class_weights ? (double)class_weights[lab] : 1.0;
            f = (float)(w / ((double)n * w_sum));
        }
        sc.factor[b] = f;
    }
}

__global__ __launch_bounds__(kLossThreads) void k_mask_loss_bwd(const float* __restrict__ g, int64_t m, int k,
                                                                const int* __restrict__ box_of, LossScratch sc,
                                                                float* __restrict__ dlogits) {
    const float gv = *g;
    for (int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x; i < m * k; i += (int64_t)gridDim.x * kLossThreads) {
        const int64_t r = i / k;
        const int c = (int)(i - r * k);
        const int b = box_of[r];
        dlogits[i] = c == sc.label[b] ? (gv * (sc.draw[r] * sc.factor[b])) : 0.f;
    }
}

// ---- packing -------------------------------------------------------------------------------------------------------------
struct PackTable {
    const unsigned char* mask[kMaxSamplesPerLaunch];
    int64_t n_points[kMaxSamplesPerLaunch];
    int64_t word_off[kMaxSamplesPerLaunch + 1];              // relative to the launch's first word
};

__global__ __launch_bounds__(256) void k_mask_pack(const PackTable tab, int nb, unsigned int* __restrict__ out) {
    const int64_t total = tab.word_off[nb];
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (int64_t)gridDim.x * 256) {
        int s = 0;
        while (s + 1 < nb && tab.word_off[s + 1] <= w) ++s;
        const int64_t N = tab.n_points[s], W = (N + 31) / 32;
        const int64_t local = w - tab.word_off[s], g = local / W, p0 = (local - g * W) * 32;
        const unsigned char* row = tab.mask[s] + g * N;
        unsigned int v = 0u;
        for (int j = 0; j < 32; ++j)
            if (p0 + j < N && row[p0 + j]) v |= 1u << j;
        out[w] = v;
    }
}

unsigned long long splitmix64(unsigned long long& s) {
    unsigned long long z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

extern "C" int scn_mask_overlap_draw(const float* pred_boxes, const int64_t* pred_offsets, const float* gt_boxes,
                                     const int64_t* gt_offsets, int batch, float* max_overlap, int64_t* argmax,
                                     int overlaps_given, float positive_threshold, int num_positive, uint64_t seed,
                                     uint64_t counter, const int64_t* fwd_offsets, float* fwd_boxes, int64_t* gt_association,
                                     int64_t* pred_selection, int64_t* n_drawn, scn_stream_t stream) {
    SCN_REQUIRE(batch >= 0 && batch < 65536 && pred_offsets && gt_offsets);
    if (batch == 0) return SCN_OK;
    SCN_REQUIRE(pred_offsets[0] == 0 && gt_offsets[0] == 0);
    for (int b = 0; b < batch; ++b) {
        SCN_REQUIRE(pred_offsets[b + 1] >= pred_offsets[b] && pred_offsets[b + 1] - pred_offsets[b] <= kMaxProposals);
        SCN_REQUIRE(gt_offsets[b + 1] >= gt_offsets[b]);
    }
    const bool draw = fwd_boxes != nullptr;
    SCN_REQUIRE(!overlaps_given || (max_overlap && argmax));
    SCN_REQUIRE(pred_offsets[batch] == 0 || pred_boxes);
    SCN_REQUIRE(overlaps_given || gt_offsets[batch] == gt_offsets[0] || gt_boxes);
    if (draw) {
        SCN_REQUIRE(fwd_offsets && fwd_offsets[0] == 0 && gt_association && num_positive >= 0);
        SCN_REQUIRE(gt_offsets[batch] == gt_offsets[0] || gt_boxes);
        for (int b = 0; b < batch; ++b) {         // cap_s = min(num_positive, P_s) slots, then the G_s boxes
            const int64_t P = pred_offsets[b + 1] - pred_offsets[b], G = gt_offsets[b + 1] - gt_offsets[b];
            SCN_REQUIRE(fwd_offsets[b + 1] - fwd_offsets[b] == (P < num_positive ? P : num_positive) + G);
        }
    }
    Keys keys;
    unsigned long long st = seed ^ (counter * 0xd1b54a32d192ed03ull) ^ 0x6d61736bull;   // ("mask": not the RPN draw's keys)
    st = splitmix64(st) ^ counter;
    for (int r = 0; r < 4; ++r) keys.rk[r] = (unsigned int)(splitmix64(st) >> 32);
    for (int b0 = 0; b0 < batch; b0 += kMaxSamplesPerLaunch) {
        const int nb = batch - b0 < kMaxSamplesPerLaunch ? batch - b0 : kMaxSamplesPerLaunch;
        DrawTable t;
        for (int q = 0; q <= kMaxSamplesPerLaunch; ++q) {
            const int b = b0 + (q <= nb ? q : nb);
            t.pred_off[q] = pred_offsets[b];
            t.gt_off[q] = gt_offsets[b];
            t.fwd_off[q] = draw ? fwd_offsets[b] : 0;
        }
        hipLaunchKernelGGL(k_mask_overlap_draw, dim3(nb), dim3(kDrawThreads), 0, S(stream), pred_boxes, gt_boxes, t, b0,
                           max_overlap, (long long*)argmax, overlaps_given ? 1 : 0, positive_threshold, num_positive, keys,
                           fwd_boxes, (long long*)gt_association, (long long*)pred_selection, (long long*)n_drawn);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

extern "C" int64_t scn_mask_loss_scratch_bytes(int64_t n_boxes, int64_t m) {
    if (n_boxes < 0 || m < 0) return -1;
    return 24 * n_boxes + 4 * m + 8;
}

extern "C" int scn_mask_loss(const float* logits, int64_t m, int k, const int32_t* src_row, const int32_t* box_of,
                             const int64_t* gt_association, const int64_t* box_offsets, const int64_t* labels,
                             const int64_t* gt_offsets, const uint32_t* mask_words, const int64_t* word_offsets,
                             const int64_t* point_offsets, int batch, const float* class_weights, void* scratch, float* loss,
                             scn_stream_t stream) {
    SCN_REQUIRE(m >= 0 && m < 0x7fffffffLL && k > 0 && batch >= 0 && loss && scratch && ((uintptr_t)scratch & 7) == 0);
    SCN_REQUIRE(batch == 0 || (box_offsets && gt_offsets && word_offsets && point_offsets));
    const int64_t n_boxes = batch ? box_offsets[batch] - box_offsets[0] : 0;
    SCN_REQUIRE(batch == 0 || box_offsets[0] == 0);
    SCN_REQUIRE(n_boxes < 0x7fffffffLL);
    for (int b = 0; b < batch; ++b) {
        const int64_t G = gt_offsets[b + 1] - gt_offsets[b], N = point_offsets[b + 1] - point_offsets[b];
        SCN_REQUIRE(box_offsets[b + 1] >= box_offsets[b] && G >= 0 && N >= 0);
        SCN_REQUIRE(word_offsets[b + 1] - word_offsets[b] == G * ((N + 31) / 32));
    }
    SCN_REQUIRE(m == 0 || (logits && src_row && box_of));
    SCN_REQUIRE(n_boxes == 0 || gt_association);
    SCN_REQUIRE(batch == 0 || gt_offsets[batch] == gt_offsets[0] || labels);
    SCN_REQUIRE(batch == 0 || word_offsets[batch] == word_offsets[0] || mask_words);
    const LossScratch sc = carve(scratch, n_boxes, m);
    for (int b0 = 0; b0 < batch; b0 += kMaxSamplesPerLaunch) {
        const int nb = batch - b0 < kMaxSamplesPerLaunch ? batch - b0 : kMaxSamplesPerLaunch;
        LossTable t;
        for (int q = 0; q <= kMaxSamplesPerLaunch; ++q) {
            const int b = b0 + (q <= nb ? q : nb);
            t.box_off[q] = box_offsets[b];
            t.gt_off[q] = gt_offsets[b];
            t.word_off[q] = word_offsets[b];
            t.pt_off[q] = point_offsets[b];
        }
        const int64_t boxes = t.box_off[nb] - t.box_off[0];
        if (boxes == 0) continue;
        hipLaunchKernelGGL(k_mask_loss_boxes, dim3((unsigned)boxes), dim3(kLossThreads), 0, S(stream), logits, m, k, src_row,
                           box_of, (const long long*)gt_association, (const long long*)labels, mask_words, t, nb, sc);
        SCN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mask_loss_finish, dim3(1), dim3(kLossThreads), 0, S(stream), n_boxes, class_weights, loss, sc);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_mask_loss_bwd(const float* grad_loss, const void* scratch, int64_t n_boxes, int64_t m, int k,
                                 const int32_t* box_of, float* dlogits, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && m >= 0 && k > 0 && scratch && ((uintptr_t)scratch & 7) == 0);
    if (m == 0) return SCN_OK;
    SCN_REQUIRE(grad_loss && box_of && dlogits);
    const LossScratch sc = carve((void*)scratch, n_boxes, m);
    hipLaunchKernelGGL(k_mask_loss_bwd, dim3(scn::ew_grid(m * k, kLossThreads)), dim3(kLossThreads), 0, S(stream), grad_loss,
                       m, k, box_of, sc, dlogits);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_mask_pack(const uint8_t* const* masks, const int64_t* n_gt, const int64_t* n_points, int batch,
                             uint32_t* out_words, scn_stream_t stream) {
    SCN_REQUIRE(batch >= 0 && (batch == 0 || (masks && n_gt && n_points)));
    int64_t w0 = 0;
    for (int b0 = 0; b0 < batch; b0 += kMaxSamplesPerLaunch) {
        const int nb = batch - b0 < kMaxSamplesPerLaunch ? batch - b0 : kMaxSamplesPerLaunch;
        PackTable t;
        t.word_off[0] = 0;
        for (int q = 0; q < kMaxSamplesPerLaunch; ++q) {
            const int b = b0 + q;
            t.mask[q] = q < nb ? masks[b] : nullptr;
            t.n_points[q] = q < nb ? n_points[b] : 0;
            if (q < nb) SCN_REQUIRE(n_gt[b] >= 0 && n_points[b] >= 0 && (n_gt[b] * n_points[b] == 0 || masks[b]));
            t.word_off[q + 1] = t.word_off[q] + (q < nb ? n_gt[b] * ((n_points[b] + 31) / 32) : 0);
        }
        if (t.word_off[nb] > 0) {
            SCN_REQUIRE(out_words);
            hipLaunchKernelGGL(k_mask_pack, dim3(scn::ew_grid(t.word_off[nb], 256)), dim3(256), 0, S(stream), t, nb,
                               out_words + w0);
            SCN_LAUNCH_CHECK();
        }
        w0 += t.word_off[nb];
    }
    return SCN_OK;
}
