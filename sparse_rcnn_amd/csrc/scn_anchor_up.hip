// The permutation half of the reference's up-sampling RPN heads (ndsis/modules/anchor_network.py:127-219
// `AnchorNetworkUpsample`; anchor.py:167-192 `rpn_permuter` + `rpn_bbox_score_splitter`) -- include/scn_mi355x.h:
// scn_anchor_up_fwd, scn_anchor_up_bwd.  fp32 only.  Both kernels only copy.
//
// A ConvTranspose3d with kernel = stride has no overlap between taps: the heads of one anchor level are ONE row GEMM
// P = X @ Wm + bias_cols over the level's channels-last slab X [B X Y Z, C] (rpn.AnchorNetworkUpsample packs Wm) and this
// scatter.  Column col0_g + ((a s1 + b) s2 + c) (A_g 7) + co of P's row (sample, x, y, z) is, for co = anchor 7 + k, component
// k (0..5 box deltas, 6 the score) of anchor `anchor` of group g at the fine cell (x s0 + a, y s1 + b, z s2 + c).
//
// All-anchor order (anchor.py:82-101): groups in level order, then group order; inside a group the fine cells row-major over
// (X s0, Y s1, Z s2), z fastest; the anchor index minor.  dest[all-anchor index] = the anchor's rank among the inside
// anchors of ALL levels, -1 outside; the same for every sample.  Outputs rpn_bbox [B, N_in, 2, 3] and rpn_score [B, N_in],
// written in place: there is no [B, N_all, 7] intermediate, no concatenation over groups and no index_select.
//
// Lane mapping.  One thread per element of P (forward) / dP (backward), a workgroup owning ROWS consecutive rows: a wave
// reads (writes) contiguous stretches of a P row.  Inside a tap the A_g 7 columns are the 7-float records of neighbouring
// anchors -- neighbouring dest values, 24 of every 28 bytes adjacent in rpn_bbox -- and the next tap in z is the next fine cell.
// Records are 28 bytes: no 16-byte accesses.  No LDS.  Row offsets are 64-bit.
//
// Backward: a gather -- EVERY element of dP is written exactly once (the groups' columns tile [0, ncol), checked on the host):
// the incoming value where dest >= 0, 0 where it is -1 or where the gradient is absent.  No atomics: reruns are bit-identical.
// A dest value outside [-1, n_inside) is treated as -1: no kernel reads or writes outside its buffers.
#include "scn_common.h"

namespace {

struct Group {
    int s0, s1, s2, a7;          // extra stride; A_g * 7 columns per tap
    int col0;                    // first column of the group's s0 s1 s2 A_g 7
    int64_t first;               // first index in the all-anchor order
};

struct Level {
    Group g[SCN_ANCHOR_UP_MAX_GROUPS];
    int n_groups, ncol;
    int X, Y, Z;
    int64_t cells, rows;         // X Y Z; batch * cells
    int64_t n_inside;
};

constexpr int THREADS = 256;

// all-anchor index and component of column `col` of row `cell` (inside one sample; cells < 2^31: 32-bit arithmetic)
__device__ __forceinline__ int64_t locate(const Level& lv, int cell, int col, int& k) {
    int gi = 0;
    while (gi + 1 < lv.n_groups && col >= lv.g[gi + 1].col0) ++gi;
    const Group& g = lv.g[gi];
    const int r = col - g.col0;
    const int tap = r / g.a7, co = r - tap * g.a7;
    const int anchor = co / 7;
    k = co - anchor * 7;
    const int ab = tap / g.s2, c = tap - ab * g.s2;
    const int a = ab / g.s1, b = ab - a * g.s1;
    const int xy = cell / lv.Z, z = cell - xy * lv.Z;
    const int x = xy / lv.Y, y = xy - x * lv.Y;
    const int64_t fine = ((int64_t)(x * g.s0 + a) * ((int64_t)lv.Y * g.s1) + (y * g.s1 + b)) * ((int64_t)lv.Z * g.s2) + (z * g.s2 + c);
    return g.first + fine * (g.a7 / 7) + anchor;
}

template <bool BWD>
__global__ __launch_bounds__(THREADS) void k_anchor_up(const float* __restrict__ src_a, const float* __restrict__ src_b,
                                                       const int32_t* __restrict__ dest, Level lv, int rows_per_block,
                                                       float* __restrict__ out_a, float* __restrict__ out_b) {
    // forward: src_a = P, out_a = rpn_bbox, out_b = rpn_score;  backward: src_a = d_bbox, src_b = d_score, out_a = dP
    for (int64_t row0 = (int64_t)blockIdx.x * rows_per_block; row0 < lv.rows; row0 += (int64_t)gridDim.x * rows_per_block) {
        const int64_t left = lv.rows - row0;
        const int nrow = left < rows_per_block ? (int)left : rows_per_block;
        const int n = nrow * lv.ncol;
        const int64_t sample0 = row0 / lv.cells, cell0 = row0 - sample0 * lv.cells;      // the one 64-bit split, per block of rows
        for (int i = threadIdx.x; i < n; i += THREADS) {
            const int lr = i / lv.ncol, col = i - lr * lv.ncol;
            const int64_t row = row0 + lr;
            int64_t sample = sample0, c0 = cell0 + lr;
            while (c0 >= lv.cells) { c0 -= lv.cells; ++sample; }
            const int cell = (int)c0;
            int k;
            const int64_t d = dest[locate(lv, cell, col, k)];
            const bool in = d >= 0 && d < lv.n_inside;
            const int64_t e = row * lv.ncol + col;
            const int64_t rec = sample * lv.n_inside + d;
            if (!BWD) {
                if (in) {
                    const float v = src_a[e];
                    if (k < 6) out_a[rec * 6 + k] = v;
                    else out_b[rec] = v;
                }
            } else {
                float v = 0.f;
                if (in) {
                    if (k < 6) { if (src_a) v = src_a[rec * 6 + k]; }
                    else if (src_b) v = src_b[rec];
                }
                out_a[e] = v;
            }
        }
    }
}

// Validates everything that is on the host and fills `lv`; touches no device memory.
int level_of(int batch, const int64_t* size_host, int ncol, const int64_t* groups_host, int n_groups, int64_t n_all,
             int64_t n_inside, Level& lv) {
    SCN_REQUIRE(size_host && groups_host);
    SCN_REQUIRE(batch >= 0 && ncol >= 7 && n_groups >= 1 && n_groups <= SCN_ANCHOR_UP_MAX_GROUPS);
    SCN_REQUIRE(n_all >= 0 && n_inside >= 0 && n_inside <= n_all && n_all < ((int64_t)1 << 31));
    for (int d = 0; d < 3; ++d) SCN_REQUIRE(size_host[d] >= 1 && size_host[d] <= 65536);
    lv.X = (int)size_host[0]; lv.Y = (int)size_host[1]; lv.Z = (int)size_host[2];
    lv.cells = (int64_t)lv.X * lv.Y * lv.Z;
    lv.rows = lv.cells * batch;
    lv.n_groups = n_groups;
    lv.ncol = ncol;
    lv.n_inside = n_inside;
    SCN_REQUIRE(lv.cells < ((int64_t)1 << 31) && lv.rows < ((int64_t)1 << 40));
    int64_t col = 0;
    for (int i = 0; i < n_groups; ++i) {
        const int64_t* h = groups_host + 6 * i;          // (s0, s1, s2, A_g, first column, first all-anchor index)
        for (int d = 0; d < 3; ++d) SCN_REQUIRE(h[d] >= 1 && h[d] <= 64);
        SCN_REQUIRE(h[3] >= 1 && h[3] <= 64);
        const int64_t taps = h[0] * h[1] * h[2], ncols = taps * h[3] * 7;
        SCN_REQUIRE(h[4] == col);                        // the groups' columns tile [0, ncol) in group order
        SCN_REQUIRE(ncols <= ncol - col);
        const int64_t fine = lv.cells * taps;            // fine cells of the group, per sample
        SCN_REQUIRE(fine < ((int64_t)1 << 31));
        SCN_REQUIRE(h[5] >= 0 && h[5] <= n_all && fine * h[3] <= n_all - h[5]);
        Group& g = lv.g[i];
        g.s0 = (int)h[0]; g.s1 = (int)h[1]; g.s2 = (int)h[2]; g.a7 = (int)h[3] * 7;
        g.col0 = (int)col; g.first = h[5];
        col += ncols;
    }
    SCN_REQUIRE(col == ncol);
    return SCN_OK;
}

int rows_per_block(int ncol) {                           // about 8 passes of the workgroup per block of rows, n < 2^31
    int r = (8 * THREADS) / ncol;
    return r < 1 ? 1 : r;
}

}  // namespace

extern "C" int scn_anchor_up_fwd(const float* P, int batch, const int64_t* size_host, int ncol, const int64_t* groups_host,
                                 int n_groups, const int32_t* dest, int64_t n_all, int64_t n_inside, float* rpn_bbox,
                                 float* rpn_score, scn_stream_t stream) {
    Level lv;
    if (int rc = level_of(batch, size_host, ncol, groups_host, n_groups, n_all, n_inside, lv)) return rc;
    if (lv.rows == 0 || n_inside == 0) return SCN_OK;
    SCN_REQUIRE(P && dest && rpn_bbox && rpn_score);
    const int rpb = rows_per_block(ncol);
    int64_t grid = scn::cdiv(lv.rows, rpb);
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(k_anchor_up<false>, dim3((unsigned)grid), dim3(THREADS), 0, scn::S(stream), P, (const float*)nullptr,
                       dest, lv, rpb, rpn_bbox, rpn_score);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_anchor_up_bwd(const float* d_bbox, const float* d_score, int batch, const int64_t* size_host, int ncol,
                                 const int64_t* groups_host, int n_groups, const int32_t* dest, int64_t n_all,
                                 int64_t n_inside, float* dP, scn_stream_t stream) {
    Level lv;
    if (int rc = level_of(batch, size_host, ncol, groups_host, n_groups, n_all, n_inside, lv)) return rc;
    if (lv.rows == 0) return SCN_OK;
    SCN_REQUIRE(dest && dP);
    const int rpb = rows_per_block(ncol);
    int64_t grid = scn::cdiv(lv.rows, rpb);
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(k_anchor_up<true>, dim3((unsigned)grid), dim3(THREADS), 0, scn::S(stream), d_bbox, d_score, dest, lv, rpb,
                       dP, (float*)nullptr);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}
