// The evaluation of the reference (ndsis/training/evaluation.py; ndsis/utils/mask.py mask_iou_matrix_split_combine,
// mask_confusion_pair; ndsis/utils/bbox.py bbox_overlap_prediction) on the device (include/scn_mi355x.h: scn_eval_*).
// Every integer below is exact and every float is ONE correctly rounded fp32 division of two exact integers (or, for boxes,
// the reference's operation order rounded once per operation), so results are bit-equal to the reference and run-to-run
// identical; where work is split across workgroups the partial results are combined with integer atomics.
//
//   k_eval_mask_bits       one thread per selected row (RoiSelection, box-major, ascending point row): bit = sigmoid(logit of
//                          the box's class) > threshold, OR-ed into the box's word with an integer atomic (words pre-zeroed).
//   k_eval_pack_threshold  dense fp32 [P][N] > threshold: a wave reads 64 consecutive floats of a row, one ballot = 2 words.
//   k_eval_mask_tile       popcount "GEMM": a workgroup owns 64 predictions x 64 ground truths x a range of 32-word chunks,
//                          stages both in LDS (rows padded to 36 words: the 128-bit LDS reads of 16 rows cover the 64 banks
//                          once), every thread keeps a 4 x 4 tile of int counters; integer atomicAdd into `inter`.
//   k_eval_rowcount        |mask| of every packed row: one wave per row.
//   k_eval_mask_finish     iou = float(inter) / float(|pred| + |gt| - inter) (0 / 0 = NaN), and the [[tp, fp], [fn, tn]] of the
//                          pairing prediction i <-> ground truth i.
//   k_eval_bbox_iou        one thread per (prediction, ground truth): scn_box_iou (shared with k_mask_overlap_draw).
//   k_eval_match           PrecisionRecallCurve.calc_tp_indicator: one wave per problem, lanes over the ground truths, the walk
//                          over the predictions sequential.
//   k_eval_confusion       LDS histogram of pred * C + gt per workgroup, integer atomics to the int64 result.
#include "scn_common.h"

#include <math.h>

#pragma clang fp contract(off)

using scn::S;

namespace {

constexpr int kMaxSamples = 32;                              // per-sample tables travel in the kernel arguments

struct EvalTable {
    int64_t pred_off[kMaxSamples + 1];                       // predictions of sample s (rows of |pred|, score, class)
    int64_t gt_off[kMaxSamples + 1];                         // ground truths of sample s
    int64_t pair_off[kMaxSamples + 1];                       // first element of sample s's [P_s][G_s] matrix
    int64_t pword_off[kMaxSamples];                          // first word of sample s's packed predictions [P_s][W_s]
    int64_t gword_off[kMaxSamples];                          // ... ground truths [G_s][W_s]
    int64_t n_points[kMaxSamples];                           // N_s; W_s = ceil(N_s / 32)
};

// ---- packing ------------------------------------------------------------------------------------------------------------------
__global__ void k_eval_mask_bits(const float* __restrict__ logits, long long m, int k, const int* __restrict__ src_row,
                                 const int* __restrict__ box_of, const long long* __restrict__ class_of_box, int num_valid,
                                 float thr, const long long* __restrict__ bit_base, long long n_boxes, long long n_words,
                                 unsigned int* __restrict__ words) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < m; r += (long long)gridDim.x * blockDim.x) {
        const int box = box_of[r];
        if (box < 0 || box >= n_boxes) continue;
        const long long cls = class_of_box[box];
        const bool valid = cls >= 0 && (num_valid == 0 || cls < num_valid) && cls < k;     // as k_mask_scatter
        if (!valid) continue;
        if (!(scn_mask_sigmoid(logits[r * k + cls]) > thr)) continue;
        const long long bit = bit_base[box] + src_row[r];
        const long long w = bit >> 5;
        if (bit < 0 || w >= n_words) continue;               // (a selection that does not match the layout writes nothing)
        atomicOr(&words[w], 1u << (unsigned)(bit & 31));
    }
}

constexpr int kPackThreads = 256;

__global__ __launch_bounds__(kPackThreads) void k_eval_pack_threshold(const float* __restrict__ x, long long p, long long n,
                                                                      float thr, unsigned int* __restrict__ words) {
    const long long w = (n + 31) >> 5, chunks = (n + 63) >> 6;               // 64 columns per wave step
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)kPackThreads + threadIdx.x) >> 6;
    const long long n_waves = (long long)gridDim.x * (kPackThreads / 64);
    for (long long u = wave; u < p * chunks; u += n_waves) {                 // (uniform per wave)
        const long long row = u / chunks, c = u - row * chunks;
        const long long col = c * 64 + lane;
        const bool on = col < n && x[row * n + col] > thr;
        const unsigned long long b = __ballot(on);
        if (lane == 0) words[row * w + 2 * c] = (unsigned int)b;
        if (lane == 32 && 2 * c + 1 < w) words[row * w + 2 * c + 1] = (unsigned int)(b >> 32);
    }
}

// ---- mask IoU -----------------------------------------------------------------------------------------------------------------
constexpr int kTile = 64, kChunk = 32, kLd = kChunk + 4, kTileThreads = 256;

struct TileTable {
    EvalTable t;
    int tile_off[kMaxSamples + 1];                           // first workgroup (before the word split) of sample s
    int n_split;                                             // workgroups along the word axis
};

__global__ __launch_bounds__(kTileThreads) void k_eval_mask_tile(const unsigned int* __restrict__ pw,
                                                                 const unsigned int* __restrict__ gw, const TileTable tab,
                                                                 int nb, int* __restrict__ inter) {
    __shared__ __attribute__((aligned(16))) unsigned int sp[kTile][kLd];
    __shared__ __attribute__((aligned(16))) unsigned int sg[kTile][kLd];
    const int tile = blockIdx.x / tab.n_split, split = blockIdx.x - tile * tab.n_split;
    int s = 0;
    while (s + 1 < nb && tab.tile_off[s + 1] <= tile) ++s;
    const long long P = tab.t.pred_off[s + 1] - tab.t.pred_off[s], G = tab.t.gt_off[s + 1] - tab.t.gt_off[s];
    const long long W = (tab.t.n_points[s] + 31) >> 5;
    const int tg = (int)((G + kTile - 1) / kTile), lt = tile - tab.tile_off[s];
    const long long p0 = (long long)(lt / tg) * kTile, g0 = (long long)(lt % tg) * kTile;
    const long long n_chunks = (W + kChunk - 1) / kChunk, per = (n_chunks + tab.n_split - 1) / tab.n_split;
    const long long c_lo = split * per, c_hi = c_lo + per < n_chunks ? c_lo + per : n_chunks;
    const unsigned int* PW = pw + tab.t.pword_off[s];
    const unsigned int* GW = gw + tab.t.gword_off[s];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;                  // ground truths tx + 16 j, predictions 4 ty + i
    const int lw = threadIdx.x & 31, lr = threadIdx.x >> 5;                  // loader: word lw of rows lr + 8 q
    int acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    for (long long c = c_lo; c < c_hi; ++c) {
        const long long k = c * kChunk + lw;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTile / 8; ++q) {
            const int r = lr + 8 * q;
            sp[r][lw] = (p0 + r < P && k < W) ? PW[(p0 + r) * W + k] : 0u;
            sg[r][lw] = (g0 + r < G && k < W) ? GW[(g0 + r) * W + k] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < kChunk; k4 += 4) {
            uint4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const uint4*>(&sp[4 * ty + i][k4]);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const uint4*>(&sg[tx + 16 * j][k4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] += __popc(a[i].x & b[j].x) + __popc(a[i].y & b[j].y) + __popc(a[i].z & b[j].z) +
                                 __popc(a[i].w & b[j].w);
        }
    }
    int* out = inter + tab.t.pair_off[s];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long p = p0 + 4 * ty + i, g = g0 + tx + 16 * j;
            if (p < P && g < G && acc[i][j]) atomicAdd(&out[p * G + g], acc[i][j]);
        }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// rows 0 .. n_pred-1: predictions, then the ground truths; one wave per row
__global__ __launch_bounds__(256) void k_eval_rowcount(const unsigned int* __restrict__ pw, const unsigned int* __restrict__ gw,
                                                       const EvalTable tab, int nb, int* __restrict__ pred_cnt,
                                                       int* __restrict__ gt_cnt) {
    const long long n_pred = tab.pred_off[nb] - tab.pred_off[0], n_gt = tab.gt_off[nb] - tab.gt_off[0];
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * 256ll + threadIdx.x) >> 6, n_waves = (long long)gridDim.x * 4;
    for (long long row = wave; row < n_pred + n_gt; row += n_waves) {
        const bool is_gt = row >= n_pred;
        const long long r = (is_gt ? row - n_pred + tab.gt_off[0] : row + tab.pred_off[0]);
        const int64_t* off = is_gt ? tab.gt_off : tab.pred_off;
        int s = 0;
        while (s + 1 < nb && off[s + 1] <= r) ++s;
        const long long W = (tab.n_points[s] + 31) >> 5;
        const unsigned int* base = (is_gt ? gw + tab.gword_off[s] : pw + tab.pword_off[s]) + (r - off[s]) * W;
        int v = 0;
        for (long long k = lane; k < W; k += 64) v += __popc(base[k]);
        v = wave_sum(v);
        if (lane == 0) (is_gt ? gt_cnt : pred_cnt)[r] = v;
    }
}

__global__ void k_eval_mask_finish(const int* __restrict__ inter, const int* __restrict__ pred_cnt,
                                   const int* __restrict__ gt_cnt, const EvalTable tab, int nb, float* __restrict__ iou,
                                   long long* __restrict__ conf) {
    const long long e0 = tab.pair_off[0], e1 = tab.pair_off[nb];
    for (long long e = e0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; e < e1; e += (long long)gridDim.x * blockDim.x) {
        int s = 0;
        while (s + 1 < nb && tab.pair_off[s + 1] <= e) ++s;
        const long long G = tab.gt_off[s + 1] - tab.gt_off[s];
        const long long le = e - tab.pair_off[s], p = le / G, g = le - p * G;
        const int in = inter[e], pc = pred_cnt[tab.pred_off[s] + p], gc = gt_cnt[tab.gt_off[s] + g];
        const long long uni = (long long)pc + gc - in;       // (64-bit: |pred| + |gt| may pass 2^31)
        if (iou) iou[e] = ((float)in / (float)uni);          // 0 / 0: NaN, as the reference's inter / union
        if (conf && p == g) {                                // mask_confusion_pair: [[tp, fp], [fn, tn]]
            long long* c = conf + (tab.pred_off[s] + p) * 4;
            c[0] = in;
            c[1] = pc - in;
            c[2] = gc - in;
            c[3] = tab.n_points[s] - uni;
        }
    }
}

// ---- box IoU ------------------------------------------------------------------------------------------------------------------
__global__ void k_eval_bbox_iou(const float* __restrict__ pred, const float* __restrict__ gt, const EvalTable tab, int nb,
                                float* __restrict__ iou) {
    const long long e0 = tab.pair_off[0], e1 = tab.pair_off[nb];
    for (long long e = e0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; e < e1; e += (long long)gridDim.x * blockDim.x) {
        int s = 0;
        while (s + 1 < nb && tab.pair_off[s + 1] <= e) ++s;
        const long long G = tab.gt_off[s + 1] - tab.gt_off[s];
        const long long le = e - tab.pair_off[s], p = le / G, g = le - p * G;
        const float* A = pred + (tab.pred_off[s] + p) * 6;
        const float* B = gt + (tab.gt_off[s] + g) * 6;
        float as[3], ae[3], bx[7];
        for (int d = 0; d < 3; ++d) {
            as[d] = A[d];
            ae[d] = A[3 + d];
        }
        for (int d = 0; d < 6; ++d) bx[d] = B[d];
        const float area = ((ae[0] - as[0]) * (ae[1] - as[1])) * (ae[2] - as[2]);
        bx[6] = ((bx[3] - bx[0]) * (bx[4] - bx[1])) * (bx[5] - bx[2]);
        iou[e] = scn_box_iou(as, ae, area, bx);
    }
}

// ---- matching -----------------------------------------------------------------------------------------------------------------
constexpr int kMatchMaxGt = 64 * 64;                         // one 64-bit "taken / not mine" mask per lane

// problem q = (sample, class or -1, threshold).  flags[q][i] for the P_s predictions of its sample: -1 not part of the problem,
// 0 false positive, 1 true positive.
__global__ __launch_bounds__(256) void k_eval_match(const float* __restrict__ iou, const long long* __restrict__ pred_off,
                                                    const long long* __restrict__ gt_off, const long long* __restrict__ pair_off,
                                                    const unsigned char* __restrict__ keep,
                                                    const long long* __restrict__ pred_class,
                                                    const long long* __restrict__ gt_class, const int* __restrict__ prob_sample,
                                                    const long long* __restrict__ prob_class, const float* __restrict__ prob_thr,
                                                    const long long* __restrict__ prob_out, int n_prob,
                                                    signed char* __restrict__ flags, int* __restrict__ num_gt) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_prob) return;                                 // (whole waves; no barrier below)
    const int s = prob_sample[q];
    const long long cls = prob_class[q];
    const float thr = prob_thr[q];
    const long long p0 = pred_off[s], P = pred_off[s + 1] - p0, g0 = gt_off[s], G = gt_off[s + 1] - g0;
    const float* M = iou + pair_off[s];
    signed char* F = flags + prob_out[q];
    unsigned long long open = 0;                             // bit t: ground truth lane + 64 t is mine and not yet matched
    int mine = 0;
    for (int t = 0; lane + 64 * t < G; ++t) {
        const long long g = lane + 64 * t;
        if (cls < 0 || gt_class[g0 + g] == cls) {
            open |= 1ull << t;
            ++mine;
        }
    }
    int remaining = wave_sum(mine);
    if (lane == 0) num_gt[q] = remaining;
    for (long long i = 0; i < P; ++i) {
        const bool in = (!keep || keep[p0 + i]) && (cls < 0 || pred_class[p0 + i] == cls);   // (uniform over the wave)
        if (!in) {
            if (lane == 0) F[i] = -1;
            continue;
        }
        bool tp = false;
        if (remaining > 0) {
            float best = -INFINITY;
            int arg = 0x7fffffff;
            bool nan = false;
            for (int t = 0; lane + 64 * t < G; ++t) {
                if (!((open >> t) & 1ull)) continue;
                const int g = lane + 64 * t;
                const float v = M[i * G + g];
                nan |= v != v;
                if (v > best) {                              // ascending g: the first maximum of the lane stays
                    best = v;
                    arg = g;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {         // (max, first index) over the wave
                const float ob = __shfl_xor(best, off, 64);
                const int oa = __shfl_xor(arg, off, 64);
                if (ob > best || (ob == best && oa < arg)) {
                    best = ob;
                    arg = oa;
                }
            }
            // a NaN among the remaining ground truths: torch's max returns it, NaN >= threshold is false
            if (!__any(nan) && arg != 0x7fffffff && best >= thr) {
                tp = true;
                if ((arg & 63) == lane) open &= ~(1ull << (arg >> 6));
                --remaining;
            }
        }
        if (lane == 0) F[i] = tp ? 1 : 0;
    }
}

// ---- confusion ----------------------------------------------------------------------------------------------------------------
constexpr int kConfMaxClasses = 64, kConfThreads = 256;

__global__ __launch_bounds__(kConfThreads) void k_eval_confusion(const long long* __restrict__ pred,
                                                                 const long long* __restrict__ gt, long long n, int c,
                                                                 unsigned long long* __restrict__ out,
                                                                 unsigned long long* __restrict__ n_bad) {
    __shared__ unsigned int hist[kConfMaxClasses * kConfMaxClasses];
    for (int i = threadIdx.x; i < c * c; i += kConfThreads) hist[i] = 0;
    __syncthreads();
    unsigned int bad = 0;
    // a workgroup sees fewer than 2^32 rows: 2048 workgroups share at most 2^40 (checked on the host)
    for (long long r = blockIdx.x * (long long)kConfThreads + threadIdx.x; r < n; r += (long long)gridDim.x * kConfThreads) {
        const long long g = gt[r], p = pred[r];
        if (g < 0 || g >= c) continue;
        if (p < 0 || p >= c) {
            ++bad;
            continue;
        }
        atomicAdd(&hist[(int)p * c + (int)g], 1u);
    }
    if (bad && n_bad) atomicAdd(n_bad, (unsigned long long)bad);
    __syncthreads();
    for (int i = threadIdx.x; i < c * c; i += kConfThreads)
        if (hist[i]) atomicAdd(&out[i], (unsigned long long)hist[i]);
}

int fill_table(EvalTable& t, const int64_t* pred_off, const int64_t* gt_off, const int64_t* pair_off, const int64_t* pword_off,
               const int64_t* gword_off, const int64_t* n_points, int b0, int nb) {
    for (int i = 0; i <= nb; ++i) {
        t.pred_off[i] = pred_off[b0 + i];
        t.gt_off[i] = gt_off[b0 + i];
        t.pair_off[i] = pair_off[b0 + i];
        if (i && (t.pred_off[i] < t.pred_off[i - 1] || t.gt_off[i] < t.gt_off[i - 1] ||
                  t.pair_off[i] - t.pair_off[i - 1] != (t.pred_off[i] - t.pred_off[i - 1]) * (t.gt_off[i] - t.gt_off[i - 1])))
            return 0;
    }
    for (int i = 0; i < nb; ++i) {
        t.pword_off[i] = pword_off ? pword_off[b0 + i] : 0;
        t.gword_off[i] = gword_off ? gword_off[b0 + i] : 0;
        t.n_points[i] = n_points ? n_points[b0 + i] : 0;
        if (t.n_points[i] < 0 || t.pword_off[i] < 0 || t.gword_off[i] < 0) return 0;
    }
    return 1;
}

}  // namespace

extern "C" int scn_eval_mask_bits(const float* logits, int64_t m, int k, const int32_t* src_row, const int32_t* box_of,
                                  const int64_t* class_of_box, int num_valid, float mask_threshold, const int64_t* bit_base,
                                  int64_t n_boxes, int64_t n_words, uint32_t* out_words, scn_stream_t stream) {
    SCN_REQUIRE(m >= 0 && k >= 1 && num_valid >= 0 && n_boxes >= 0 && n_words >= 0);
    if (n_words == 0) return SCN_OK;
    SCN_REQUIRE(out_words);
    SCN_HIP(hipMemsetAsync(out_words, 0, (size_t)n_words * 4, S(stream)));
    if (m == 0) return SCN_OK;
    SCN_REQUIRE(logits && src_row && box_of && class_of_box && bit_base);
    hipLaunchKernelGGL(k_eval_mask_bits, dim3(scn::ew_grid(m, 256)), dim3(256), 0, S(stream), logits, (long long)m, k, src_row,
                       box_of, (const long long*)class_of_box, num_valid, mask_threshold, (const long long*)bit_base,
                       (long long)n_boxes, (long long)n_words, out_words);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_eval_pack_threshold(const float* masks, int64_t p, int64_t n, float mask_threshold, uint32_t* out_words,
                                       scn_stream_t stream) {
    SCN_REQUIRE(p >= 0 && n >= 0);
    if (p == 0 || n == 0) return SCN_OK;
    SCN_REQUIRE(masks && out_words);
    hipLaunchKernelGGL(k_eval_pack_threshold, dim3(scn::ew_grid(p * ((n + 63) / 64) * 64, kPackThreads)), dim3(kPackThreads), 0,
                       S(stream), masks, (long long)p, (long long)n, mask_threshold, out_words);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_eval_mask_iou(const uint32_t* pred_words, const int64_t* pred_word_offsets, const uint32_t* gt_words,
                                 const int64_t* gt_word_offsets, const int64_t* pred_offsets, const int64_t* gt_offsets,
                                 const int64_t* pair_offsets, const int64_t* n_points, int batch, int32_t* inter,
                                 int32_t* pred_count, int32_t* gt_count, float* iou, int64_t* pair_confusion,
                                 scn_stream_t stream) {
    SCN_REQUIRE(batch >= 0);
    if (batch == 0) return SCN_OK;
    SCN_REQUIRE(pred_word_offsets && gt_word_offsets && pred_offsets && gt_offsets && pair_offsets && n_points);
    const int64_t n_pred = pred_offsets[batch] - pred_offsets[0], n_gt = gt_offsets[batch] - gt_offsets[0];
    const int64_t n_pair = pair_offsets[batch] - pair_offsets[0];
    SCN_REQUIRE(n_pred >= 0 && n_gt >= 0 && n_pair >= 0);
    SCN_REQUIRE((n_pred == 0 || pred_count) && (n_gt == 0 || gt_count) && (n_pair == 0 || inter));
    SCN_REQUIRE((n_pred == 0 || pred_words) && (n_gt == 0 || gt_words));
    if (n_pair) SCN_HIP(hipMemsetAsync(inter + pair_offsets[0], 0, (size_t)n_pair * 4, S(stream)));
    for (int b0 = 0; b0 < batch; b0 += kMaxSamples) {
        const int nb = batch - b0 < kMaxSamples ? batch - b0 : kMaxSamples;
        TileTable tt;
        SCN_REQUIRE(fill_table(tt.t, pred_offsets, gt_offsets, pair_offsets, pred_word_offsets, gt_word_offsets, n_points, b0,
                               nb));
        int64_t tiles = 0, max_chunks = 1;
        for (int i = 0; i < nb; ++i) {
            const int64_t P = tt.t.pred_off[i + 1] - tt.t.pred_off[i], G = tt.t.gt_off[i + 1] - tt.t.gt_off[i];
            SCN_REQUIRE(tt.t.n_points[i] < (1ll << 31));     // counts are int32
            if (pair_confusion) SCN_REQUIRE(P == G);
            tt.tile_off[i] = (int)tiles;
            tiles += scn::cdiv(P, kTile) * scn::cdiv(G, kTile);
            const int64_t ch = scn::cdiv(scn::cdiv(tt.t.n_points[i], 32), kChunk);
            if (P && G && ch > max_chunks) max_chunks = ch;
            SCN_REQUIRE(tiles < (1 << 24));
        }
        tt.tile_off[nb] = (int)tiles;
        const int64_t rows = (tt.t.pred_off[nb] - tt.t.pred_off[0]) + (tt.t.gt_off[nb] - tt.t.gt_off[0]);
        if (rows) {
            hipLaunchKernelGGL(k_eval_rowcount, dim3(scn::ew_grid(rows * 64, 256)), dim3(256), 0, S(stream), pred_words,
                               gt_words, tt.t, nb, pred_count, gt_count);
            SCN_LAUNCH_CHECK();
        }
        const int64_t pairs = tt.t.pair_off[nb] - tt.t.pair_off[0];
        if (!tiles || !pairs) continue;
        // fill the chip (4 workgroups per CU) by splitting the word axis; every split gets at least 4 chunks
        int64_t split = scn::cdiv(4 * (int64_t)scn::cu_budget(), tiles);
        if (split > scn::cdiv(max_chunks, 4)) split = scn::cdiv(max_chunks, 4);
        if (split < 1) split = 1;
        tt.n_split = (int)split;
        hipLaunchKernelGGL(k_eval_mask_tile, dim3((unsigned)(tiles * split)), dim3(kTileThreads), 0, S(stream), pred_words,
                           gt_words, tt, nb, inter);
        SCN_LAUNCH_CHECK();
        if (iou || pair_confusion) {
            hipLaunchKernelGGL(k_eval_mask_finish, dim3(scn::ew_grid(pairs, 256)), dim3(256), 0, S(stream), inter, pred_count,
                               gt_count, tt.t, nb, iou, (long long*)pair_confusion);
            SCN_LAUNCH_CHECK();
        }
    }
    return SCN_OK;
}

extern "C" int scn_eval_bbox_iou(const float* pred_boxes, const int64_t* pred_offsets, const float* gt_boxes,
                                 const int64_t* gt_offsets, const int64_t* pair_offsets, int batch, float* iou,
                                 scn_stream_t stream) {
    SCN_REQUIRE(batch >= 0);
    if (batch == 0) return SCN_OK;
    SCN_REQUIRE(pred_offsets && gt_offsets && pair_offsets);
    for (int b0 = 0; b0 < batch; b0 += kMaxSamples) {
        const int nb = batch - b0 < kMaxSamples ? batch - b0 : kMaxSamples;
        EvalTable t;
        SCN_REQUIRE(fill_table(t, pred_offsets, gt_offsets, pair_offsets, nullptr, nullptr, nullptr, b0, nb));
        const int64_t pairs = t.pair_off[nb] - t.pair_off[0];
        if (!pairs) continue;
        SCN_REQUIRE(pred_boxes && gt_boxes && iou);
        hipLaunchKernelGGL(k_eval_bbox_iou, dim3(scn::ew_grid(pairs, 256)), dim3(256), 0, S(stream), pred_boxes, gt_boxes, t, nb,
                           iou);
        SCN_LAUNCH_CHECK();
    }
    return SCN_OK;
}

extern "C" int scn_eval_match(const float* iou, const int64_t* pred_offsets, const int64_t* gt_offsets,
                              const int64_t* pair_offsets, int batch, int64_t max_gt, const uint8_t* keep,
                              const int64_t* pred_class, const int64_t* gt_class, const int32_t* problem_sample,
                              const int64_t* problem_class, const float* problem_threshold, const int64_t* problem_out,
                              int n_problems, int any_class_problem, int8_t* flags, int32_t* num_gt, scn_stream_t stream) {
    SCN_REQUIRE(batch >= 0 && n_problems >= 0 && max_gt >= 0);
    if (n_problems == 0) return SCN_OK;
    SCN_REQUIRE(batch > 0 && max_gt <= kMatchMaxGt);
    SCN_REQUIRE(pred_offsets && gt_offsets && pair_offsets && problem_sample && problem_class && problem_threshold &&
                problem_out && flags && num_gt);
    SCN_REQUIRE(!any_class_problem || (pred_class && gt_class));
    hipLaunchKernelGGL(k_eval_match, dim3((n_problems + 3) / 4), dim3(256), 0, S(stream), iou, (const long long*)pred_offsets,
                       (const long long*)gt_offsets, (const long long*)pair_offsets, keep, (const long long*)pred_class,
                       (const long long*)gt_class, problem_sample, (const long long*)problem_class, problem_threshold,
                       (const long long*)problem_out, n_problems, flags, num_gt);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_eval_confusion(const int64_t* pred, const int64_t* gt, int64_t n, int num_classes, int64_t* confusion,
                                  int64_t* n_bad_pred, scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && n < (1ll << 40) && num_classes >= 1 && num_classes <= kConfMaxClasses && confusion);
    SCN_HIP(hipMemsetAsync(confusion, 0, (size_t)num_classes * num_classes * 8, S(stream)));
    if (n_bad_pred) SCN_HIP(hipMemsetAsync(n_bad_pred, 0, 8, S(stream)));
    if (n == 0) return SCN_OK;
    SCN_REQUIRE(pred && gt);
    hipLaunchKernelGGL(k_eval_confusion, dim3(scn::ew_grid(n, kConfThreads)), dim3(kConfThreads), 0, S(stream),
                       (const long long*)pred, (const long long*)gt, (long long)n, num_classes, (unsigned long long*)confusion,
                       (unsigned long long*)n_bad_pred);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}
