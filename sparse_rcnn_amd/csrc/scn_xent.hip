// Weighted cross entropy with an ignored label (nn.CrossEntropyLoss(weight, ignore_index, reduction='mean'): the reference's
// ClassLoss and SegmentationLoss, ndsis/modules/loss.py:94-97, 255-268) and the row softmax / argmax of its two predictors
// (model.py:785-793, 885-893) on the device (include/scn_mi355x.h: scn_xent_fwd, scn_xent_bwd, scn_softmax_argmax).
//
// All three kernels share one row layout.  A row of c <= 256 logits is held in registers by L = 1, 2, 4 or 8 neighbouring
// lanes (c <= 32, 64, 128, 256), each lane owning one contiguous chunk of at most 32 columns, read with 16-byte loads where
// c % 4 == 0 and the base is 16-byte aligned.  The logits are read once per kernel; max, sum of exponentials, the target's
// logit and the argmax come out of the registers (xor butterflies over the L lanes: a fixed order).
//
//   k_xent_rows    per valid row w_t * (logsumexp(x) - x_t) and w_t, accumulated in double per thread over a grid-stride
//                  loop, then a fixed tree over the block: one (loss, weight, bad-target) partial per block.
//   k_xent_finish  one block: the partials in a fixed order, loss = L / W (0 when W == 0), W kept for the backward pass,
//                  the count of out-of-range targets.  Up to 2048 rows x lanes a single k_xent_rows block does this itself.
//   k_xent_bwd     recomputes the row's softmax from the logits (the forward pass keeps nothing per row) and writes
//                  g * w_t * (softmax - onehot) / W, or zeros for a dropped row.
//   k_softmax_argmax   probabilities (optional) and the first index of the row's maximum, taken on the logits.
//   k_loss_combine / k_loss_combine_bwd   the reference's `Loss` container (loss.py:101-191): the five 0-dim loss terms times
//                  exp(-log-weight), summed in fp32 in the reference's order, plus the used log-weights; root and weight
//                  gradients and the reporting record in the same launch.  One wave; lane i < 5 owns term i.
// No float atomics; two runs on the same inputs are bitwise identical.
#include "scn_common.h"

#include <math.h>

#pragma clang fp contract(off)

using scn::S;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxClasses = 256;
constexpr int kChunk = 32;                                   // columns a lane holds at most (8 x 16 bytes)
constexpr int kSingleBlockRows = 2048;                       // rows x lanes-per-row up to which the forward pass is ONE launch

struct Scratch {                                             // scn_xent_scratch_bytes
    double part_l[kMaxBlocks];
    double part_w[kMaxBlocks];
    long long part_bad[kMaxBlocks];
    double w_sum;                                            // sum of the valid rows' weights: read by k_xent_bwd
};

struct RowShape {
    int c;
    int lanes;                                               // L: lanes per row
    int per;                                                 // columns per lane, a multiple of 4
};

RowShape row_shape(int c) {
    RowShape s;
    s.c = c;
    s.lanes = c <= 32 ? 1 : c <= 64 ? 2 : c <= 128 ? 4 : 8;
    s.per = (int)(scn::cdiv(scn::cdiv(c, s.lanes), 4) * 4);
    return s;
}

int grid_for(int64_t n, int lanes) {
    int64_t g = scn::cdiv(n, kThreads / lanes);
    if (g > kMaxBlocks) g = kMaxBlocks;
    return (int)(g < 1 ? 1 : g);
}

// The lane's chunk of row `row`: x[j] = column col0 + j, -inf outside the row.
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float* __restrict__ logits, int64_t row, int c, int col0, int per, bool active,
                                           float (&x)[kChunk]) {
    const float* R = logits + row * c;
#pragma unroll
    for (int q = 0; q < kChunk / 4; ++q) {
        const int col = col0 + 4 * q;
        if (VEC) {
            float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            if (active && 4 * q < per && col < c) v = *reinterpret_cast<const float4*>(R + col);
            x[4 * q + 0] = v.x;
            x[4 * q + 1] = v.y;
            x[4 * q + 2] = v.z;
            x[4 * q + 3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                x[4 * q + e] = (active && 4 * q + e < per && col + e < c) ? R[col + e] : -INFINITY;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_chunk(float* __restrict__ out, int64_t row, int c, int col0, int per,
                                            const float (&y)[kChunk]) {
    float* R = out + row * c;
#pragma unroll
    for (int q = 0; q < kChunk / 4; ++q) {
        const int col = col0 + 4 * q;
        if (VEC) {
            if (4 * q < per && col < c)
                *reinterpret_cast<float4*>(R + col) = make_float4(y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < per && col + e < c) R[col + e] = y[4 * q + e];
        }
    }
}

__device__ __forceinline__ float group_max(float v, int lanes) {
    for (int off = 1; off < lanes; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ float group_sum(float v, int lanes) {   // a butterfly: every lane adds the same pairs
    for (int off = 1; off < lanes; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// max, e[j] = exp(x[j] - max) in place, and the row's sum of them.
__device__ __forceinline__ void row_softmax_terms(float (&x)[kChunk], int lanes, float& mx, float& sum) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) m = fmaxf(m, x[j]);
    m = group_max(m, lanes);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
        x[j] = x[j] == -INFINITY ? 0.f : expf(x[j] - m);     // (the padding, and a -inf logit: probability 0)
        s += x[j];
    }
    mx = m;
    sum = group_sum(s, lanes);
}

__device__ __forceinline__ double block_sum(double a) {     // fixed tree over the block; every thread gets the result
    __shared__ double sa[kThreads];
    sa[threadIdx.x] = a;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sa[threadIdx.x] += sa[threadIdx.x + off];
        __syncthreads();
    }
    const double r = sa[0];
    __syncthreads();
    return r;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_xent_rows(const float* __restrict__ logits, int64_t n, const RowShape sh,
                                                        const long long* __restrict__ targets,
                                                        const float* __restrict__ weights, long long ignore_index,
                                                        Scratch* __restrict__ sc, float* __restrict__ loss,
                                                        long long* __restrict__ n_bad) {
    const int rpb = kThreads / sh.lanes;
    const int sub = (int)threadIdx.x % sh.lanes, col0 = sub * sh.per;
    double acc_l = 0.0, acc_w = 0.0;
    long long bad = 0;
    for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < n; r0 += (int64_t)gridDim.x * rpb) {
        const int64_t row = r0 + (int)threadIdx.x / sh.lanes;
        const bool active = row < n;
        float x[kChunk];
        load_chunk<VEC>(logits, row, sh.c, col0, sh.per, active, x);
        const long long t = active ? targets[row] : ignore_index;
        const bool in_range = t >= 0 && t < sh.c;
        const bool valid = active && in_range && t != ignore_index;
        float xt = 0.f;                                      // the target's logit: held by exactly one lane of the group
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (valid && j < sh.per && col0 + j == (int)t) xt = x[j];   // (j >= per: the neighbour lane's column)
        xt = group_sum(xt, sh.lanes);
        float m, s;
        row_softmax_terms(x, sh.lanes, m, s);
        if (sub == 0) {
            if (valid) {
                const double w = weights ? (double)weights[t] : 1.0;
                acc_l += w * (((double)m - (double)xt) + (double)logf(s));
                acc_w += w;
            } else if (active && !in_range && t != ignore_index) {
                ++bad;
            }
        }
    }
    acc_l = block_sum(acc_l);
    acc_w = block_sum(acc_w);
    const double nb = block_sum((double)bad);                // (counts below 2^53: exact)
    if (threadIdx.x == 0) {
        if (loss) {                                          // a grid of one block (small n): it finishes the loss itself
            sc->w_sum = acc_w;
            *loss = acc_w != 0.0 ? (float)(acc_l / acc_w) : 0.f;
            if (n_bad) *n_bad = (long long)nb;
        } else {
            sc->part_l[blockIdx.x] = acc_l;
            sc->part_w[blockIdx.x] = acc_w;
            sc->part_bad[blockIdx.x] = (long long)nb;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_xent_finish(int blocks, Scratch* __restrict__ sc, float* __restrict__ loss,
                                                          long long* __restrict__ n_bad) {
    double l = 0.0, w = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kThreads) {
        l += sc->part_l[i];
        w += sc->part_w[i];
        b += (double)sc->part_bad[i];
    }
    l = block_sum(l);
    w = block_sum(w);
    b = block_sum(b);
    if (threadIdx.x == 0) {
        sc->w_sum = w;
        *loss = w != 0.0 ? (float)(l / w) : 0.f;             // no valid row: 0 (torch: NaN), see the header
        if (n_bad) *n_bad = (long long)b;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_xent_bwd(const float* __restrict__ g, const float* __restrict__ logits, int64_t n,
                                                       const RowShape sh, const long long* __restrict__ targets,
                                                       const float* __restrict__ weights, long long ignore_index,
                                                       const Scratch* __restrict__ sc, float* __restrict__ dlogits) {
    const int rpb = kThreads / sh.lanes;
    const int sub = (int)threadIdx.x % sh.lanes, col0 = sub * sh.per;
    const double w_sum = sc->w_sum;
    const double gv = (double)*g;
    for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < n; r0 += (int64_t)gridDim.x * rpb) {
        const int64_t row = r0 + (int)threadIdx.x / sh.lanes;
        const bool active = row < n;
        const long long t = active ? targets[row] : ignore_index;
        const bool valid = active && t >= 0 && t < sh.c && t != ignore_index && w_sum != 0.0;
        float x[kChunk];
        // (a dropped row's logits are not needed, but the group's shuffles want every lane: load under the same predicate)
        load_chunk<VEC>(logits, row, sh.c, col0, sh.per, valid, x);
        float m, s;
        row_softmax_terms(x, sh.lanes, m, s);
        float coef = 0.f;
        if (valid) coef = (float)(gv * (weights ? (double)weights[t] : 1.0) / w_sum);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const float p = x[j] / s;
            x[j] = valid ? coef * (p - (col0 + j == (int)t ? 1.f : 0.f)) : 0.f;
        }
        if (active) store_chunk<VEC>(dlogits, row, sh.c, col0, sh.per, x);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_softmax_argmax(const float* __restrict__ logits, int64_t n, const RowShape sh,
                                                             float* __restrict__ prob, long long* __restrict__ indices) {
    const int rpb = kThreads / sh.lanes;
    const int sub = (int)threadIdx.x % sh.lanes, col0 = sub * sh.per;
    for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < n; r0 += (int64_t)gridDim.x * rpb) {
        const int64_t row = r0 + (int)threadIdx.x / sh.lanes;
        const bool active = row < n;
        float x[kChunk];
        load_chunk<VEC>(logits, row, sh.c, col0, sh.per, active, x);
        float best = -INFINITY;                              // comparisons only: exact
        int arg = sh.c;
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (col0 + j < sh.c && j < sh.per && (x[j] > best || arg == sh.c)) {
                best = x[j];
                arg = col0 + j;
            }
        for (int off = 1; off < sh.lanes; off <<= 1) {       // the first index of the maximum across the group
            const float ob = __shfl_xor(best, off, 64);
            const int oa = __shfl_xor(arg, off, 64);
            if (oa < sh.c && (arg == sh.c || ob > best || (ob == best && oa < arg))) {
                best = ob;
                arg = oa;
            }
        }
        if (active && sub == 0) indices[row] = arg;
        if (prob) {
            float m, s;
            row_softmax_terms(x, sh.lanes, m, s);
#pragma unroll
            for (int j = 0; j < kChunk; ++j) x[j] = x[j] / s;
            if (active) store_chunk<VEC>(prob, row, sh.c, col0, sh.per, x);
        }
    }
}

bool vec_ok(const void* a, const void* b, int c) {
    return c % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

}  // namespace

extern "C" int64_t scn_xent_scratch_bytes(int64_t n, int c) {
    if (n < 0 || c < 1 || c > kMaxClasses) return -1;
    return (int64_t)sizeof(Scratch);
}

extern "C" int scn_xent_fwd(const float* logits, int64_t n, int c, const int64_t* targets, const float* weights,
                            int64_t ignore_index, void* scratch, float* loss, int64_t* n_bad_targets, scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && n < (1ll << 40) && c >= 1 && c <= kMaxClasses);
    SCN_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0 && loss);
    SCN_REQUIRE(n == 0 || (logits && targets));
    Scratch* sc = (Scratch*)scratch;
    const RowShape sh = row_shape(c);
    int blocks = 0;
    if (n > 0) {
        // up to kSingleBlockRows rows one block walks them all and finishes the loss in the same launch: at the class sizes
        // (96 and 480 rows) the launches, not the rows, are the cost
        const bool single = n * sh.lanes <= kSingleBlockRows;
        blocks = single ? 1 : grid_for(n, sh.lanes);
        float* l1 = single ? loss : nullptr;
        long long* b1 = single ? (long long*)n_bad_targets : nullptr;
        if (vec_ok(logits, logits, c))
            hipLaunchKernelGGL(k_xent_rows<true>, dim3(blocks), dim3(kThreads), 0, S(stream), logits, n, sh,
                               (const long long*)targets, weights, (long long)ignore_index, sc, l1, b1);
        else
            hipLaunchKernelGGL(k_xent_rows<false>, dim3(blocks), dim3(kThreads), 0, S(stream), logits, n, sh,
                               (const long long*)targets, weights, (long long)ignore_index, sc, l1, b1);
        SCN_LAUNCH_CHECK();
        if (single) return SCN_OK;
    }
    hipLaunchKernelGGL(k_xent_finish, dim3(1), dim3(kThreads), 0, S(stream), blocks, sc, loss, (long long*)n_bad_targets);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_xent_bwd(const float* grad_loss, const float* logits, int64_t n, int c, const int64_t* targets,
                            const float* weights, int64_t ignore_index, const void* scratch, float* dlogits,
                            scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && n < (1ll << 40) && c >= 1 && c <= kMaxClasses);
    SCN_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0);
    if (n == 0) return SCN_OK;
    SCN_REQUIRE(grad_loss && logits && targets && dlogits);
    const RowShape sh = row_shape(c);
    const int blocks = grid_for(n, sh.lanes);
    if (vec_ok(logits, dlogits, c))
        hipLaunchKernelGGL(k_xent_bwd<true>, dim3(blocks), dim3(kThreads), 0, S(stream), grad_loss, logits, n, sh,
                           (const long long*)targets, weights, (long long)ignore_index, (const Scratch*)scratch, dlogits);
    else
        hipLaunchKernelGGL(k_xent_bwd<false>, dim3(blocks), dim3(kThreads), 0, S(stream), grad_loss, logits, n, sh,
                           (const long long*)targets, weights, (long long)ignore_index, (const Scratch*)scratch, dlogits);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_softmax_argmax(const float* logits, int64_t n, int c, float* probabilities, int64_t* indices,
                                  scn_stream_t stream) {
    SCN_REQUIRE(n >= 0 && n < (1ll << 40) && c >= 1 && c <= kMaxClasses);
    if (n == 0) return SCN_OK;
    SCN_REQUIRE(logits && indices);
    const RowShape sh = row_shape(c);
    const int blocks = grid_for(n, sh.lanes);
    if (vec_ok(logits, probabilities, c))
        hipLaunchKernelGGL(k_softmax_argmax<true>, dim3(blocks), dim3(kThreads), 0, S(stream), logits, n, sh, probabilities,
                           (long long*)indices);
    else
        hipLaunchKernelGGL(k_softmax_argmax<false>, dim3(blocks), dim3(kThreads), 0, S(stream), logits, n, sh, probabilities,
                           (long long*)indices);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

// ---- the loss container (ndsis/modules/loss.py Loss.forward :101-191) ---------------------------------------------------
namespace {

constexpr int kTerms = SCN_LOSS_TERMS;

struct CombineArgs {                                         // device pointers, carried in the kernel arguments
    const float* term[kTerms];                               // NULL: the term is absent
    const float* log_weight[kTerms];
    float* weight_grad[kTerms];                              // NULL: not wanted
};

// The reference's crossing (loss.py:111-114): the rpn_score term is scaled by loss_rpn_bbox_weight, the rpn_bbox term by
// loss_rpn_class_weight.
__device__ __forceinline__ int weight_of_term(int i) { return i == 0 ? 1 : i == 1 ? 0 : i; }

struct LaneTerm {
    bool present;
    float t, w, c, p;                                        // term, its log-weight, exp(-w), t * c
    float* wg;
};

// Lane `lane` < 5 loads its term; the selects walk the argument struct with constant indices (no scratch copy of it).
__device__ __forceinline__ LaneTerm load_term(const CombineArgs& a, int lane) {
    const float *tp = nullptr, *wp = nullptr;
    float* gp = nullptr;
#pragma unroll
    for (int k = 0; k < kTerms; ++k)
        if (lane == k) {
            tp = a.term[k];
            wp = a.log_weight[weight_of_term(k)];
            gp = a.weight_grad[weight_of_term(k)];
        }
    LaneTerm r;
    r.present = lane < kTerms && tp != nullptr;
    r.t = r.present ? *tp : 0.f;
    r.w = r.present ? *wp : 0.f;
    r.c = r.present ? expf(-r.w) : 0.f;
    r.p = r.t * r.c;
    r.wg = r.present ? gp : nullptr;
    return r;
}

__global__ __launch_bounds__(64) void k_loss_combine(const CombineArgs a, float scale, float* __restrict__ record,
                                                     float* __restrict__ root_grad, double* __restrict__ running) {
    const int lane = (int)threadIdx.x;
    const LaneTerm r = load_term(a, lane);
    float loss = 0.f, extra = 0.f, nans = 0.f;               // the reference starts both sums from default_loss = 0
    float mine = 0.f;                                        // record entry `lane` (lanes 0 .. 7)
#pragma unroll
    for (int k = 0; k < kTerms; ++k) {                       // every lane adds the same values in the reference's order
        const bool pk = __shfl((int)r.present, k, 64) != 0;
        const float pv = __shfl(r.p, k, 64), wv = __shfl(r.w, k, 64), tv = __shfl(r.t, k, 64);
        if (pk) {
            loss = loss + pv;
            extra = extra + wv;
            if (tv != tv) nans += 1.f;
        }
        if (lane == 2 + k) mine = tv;                        // (0 where the term is absent)
    }
    const float combined = loss + extra;
    if (lane == 0) mine = loss;
    if (lane == 1) mine = combined;
    if (lane == 2 + kTerms) mine = nans;
    if (lane < SCN_LOSS_RECORD) record[lane] = mine;
    if (lane < kTerms) {
        if (root_grad) root_grad[lane] = scale * r.c;
        if (r.wg) *r.wg = *r.wg + scale * (1.f - r.p);
    }
    if (running) {                                           // double sums of the record's entries, then the call count
        if (lane < SCN_LOSS_RECORD) running[lane] = running[lane] + (double)mine;
        if (lane == SCN_LOSS_RECORD) running[lane] = running[lane] + 1.0;
    }
}

__global__ __launch_bounds__(64) void k_loss_combine_bwd(const CombineArgs a, const float* __restrict__ grad,
                                                         float* __restrict__ term_grad, float* __restrict__ weight_grad) {
    const int lane = (int)threadIdx.x;
    const LaneTerm r = load_term(a, lane);
    const float g = *grad;
    if (lane < kTerms) {
        if (term_grad) term_grad[lane] = r.present ? g * r.c : 0.f;
        if (weight_grad) weight_grad[weight_of_term(lane)] = r.present ? g * (1.f - r.p) : 0.f;
    }
}

int combine_args(CombineArgs& a, const float* const* terms, const float* const* log_weights, float* const* weight_grad) {
    for (int k = 0; k < kTerms; ++k) {
        a.term[k] = terms[k];
        a.log_weight[k] = log_weights[k];
        a.weight_grad[k] = weight_grad ? weight_grad[k] : nullptr;
        if (!a.log_weight[k] || ((uintptr_t)a.log_weight[k] & 3) || ((uintptr_t)a.term[k] & 3) ||
            ((uintptr_t)a.weight_grad[k] & 3))
            return 1;
    }
    return 0;
}

}  // namespace

extern "C" int scn_loss_combine(const float* const* terms, const float* const* log_weights, float scale, float* record,
                                float* root_grad, float* const* weight_grad, double* running, scn_stream_t stream) {
    SCN_REQUIRE(terms && log_weights && record && ((uintptr_t)record & 3) == 0 && ((uintptr_t)root_grad & 3) == 0);
    SCN_REQUIRE(((uintptr_t)running & 7) == 0 && isfinite(scale));
    CombineArgs a;
    SCN_REQUIRE(combine_args(a, terms, log_weights, weight_grad) == 0);
    hipLaunchKernelGGL(k_loss_combine, dim3(1), dim3(64), 0, S(stream), a, scale, record, root_grad, running);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_loss_combine_bwd(const float* grad, const float* const* terms, const float* const* log_weights,
                                    float* term_grad, float* weight_grad, scn_stream_t stream) {
    SCN_REQUIRE(grad && terms && log_weights && ((uintptr_t)grad & 3) == 0);
    SCN_REQUIRE(((uintptr_t)term_grad & 3) == 0 && ((uintptr_t)weight_grad & 3) == 0);
    CombineArgs a;
    SCN_REQUIRE(combine_args(a, terms, log_weights, nullptr) == 0);
    hipLaunchKernelGGL(k_loss_combine_bwd, dim3(1), dim3(64), 0, S(stream), a, grad, term_grad, weight_grad);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}
