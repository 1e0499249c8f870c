// Dense RoiAlign (ndsis/modules/roi_select_dense.py:28-141 `RoiAlign` / `RoiAlignInner`, trilinear, clip_boxes=True) and the
// unclamped dense 2^3/2 max pool (torch.nn.MaxPool3d(2)) behind it, on channels-last slabs (include/scn_mi355x.h:
// scn_roialign_fwd, scn_roialign_bwd, scn_dense_maxpool_fwd, scn_dense_maxpool_bwd), fp32 slabs or bf16-STORED slabs (the
// _bf16 forms): one set of kernels, templated on the element type.  A bf16 lane is 16 bytes = 8 channels; its elements are
// widened exactly when they are read, every product and sum is the fp32 kernel's in the same order, and the result is rounded
// to bf16 once, at the store (round to nearest even) -- a _bf16 call gives the fp32 call's output on the widened inputs,
// rounded once, bit for bit.  The tables are the same buffer, filled by the same two kernels.
//
// Layout.  F [B X Y Z, C], row ((b X + x) Y + y) Z + z -- the slab of a fully active grid, what rpn.DenseRpn keeps.
// Out [R ex ey ez, C], row ((r ex + i) ey + j) ez + k -- the slab of the fully active grid (ex, ey, ez) with batch R.  Lanes
// run along C (4 fp32 channels per lane when C is a multiple of 4, 8 bf16 channels), so every corner read and every output write is one
// contiguous row segment (C = 32: 128 B, eight lanes of 16 B).
//
// Coordinate table.  The sample positions depend on (box, axis, sample) only: k_roialign_table computes the R (ex + ey + ez)
// triples (floor cell, ceil cell, weight of the ceil cell) once, with the reference's expression rounded once per operation
// (no contraction):  step = (stop - start) / (e - 1);  c = min(i * step + start, stop);  lo = floor(c);  hi = ceil(c);
// w = c - lo.  The forward's corner weight is (wx * wy) * wz.  The cells are clamped to [0, size - 1] when they are stored:
// for the boxes the entry points accept (clipped to the volume) that changes nothing, and for any others no kernel reads or
// writes outside its buffers.  k_roialign_cells inverts the table for the backward: per (box, axis, cell) the first sample that
// touches the cell (lo == cell or hi == cell) and how many do -- the samples of an axis are monotone, so they are consecutive.
// The caller keeps both tables between the forward and the backward.
//
// No LDS staging of a box's sub-volume: the 8 corner rows of neighbouring samples are the same or adjacent rows, the whole
// volume at the class branch's width (12 crops of 32 x 32 x 16 cells x 32 channels: 25 MB) stays in L2 / Infinity Cache, and
// the kernel's traffic is its output (R x 4096 rows written once) -- see DESIGN 4.13 for the measured rates.
//
// Backward: a gather, no atomics, bit-identical from run to run.  One workgroup owns a (sample, x, y) column of cells: it
// first notes in LDS, for up to 128 boxes of the sample at a time, each box's x and y sample ranges on this column (empty: the
// box is skipped by the whole workgroup).  One thread owns (cell, channel group) and sums, IN THIS
// ORDER: the boxes of the cell's sample in ascending box index; within a box the x samples i that touch the cell's x
// (lo == x or hi == x) ascending, within i the y samples j ascending, within j the z samples k ascending, nested:
//     sk = sum_k az * dOut[r, i, j, k];   sj = sum_j ay * sk;   si = sum_i ax * sj;   dF[cell] = sum_r si
// where the axis weight of a sample on a cell is (lo == cell ? 1 - w : 0) + (hi == cell ? w : 0) -- both terms when the
// coordinate is an integer (w = 0, weight exactly 1).  Every cell of dF is written; a cell no sample touches gets 0.
//
// Max pool: Y = the plain maximum of the 8 children, no clamp (scn_pool_fwd computes max(0, children): SparseConvNet's rule);
// children scanned in (x, y, z) order, z fastest, a later child replaces the maximum only when it is greater or NaN, so on a
// tie the first child wins -- nn.MaxPool3d's rule.  The forward stores that child's index 0..7 as a byte; the backward
// sends dY to that child alone and writes 0 to the other seven.
//
// RoiAlign + max pool in one pass (scn_roialign_pool_fwd / _bwd; the class head without an input convolution cuts 8^3 boxes at
// the RPN stack's full width): the un-pooled samples and their gradient are never written.  The forward evaluates a
// pooled cell's 8 children with the forward's own sample function and keeps the maximum by the rule above -- Y and argmax are the
// pair's, bit for bit; the backward is the gather above with dOut[r, i, j, k] read as dY[r, i/2, j/2, k/2] where argmax names
// child (i & 1, j & 1, k & 1) and as 0 elsewhere -- the pair's dF as numbers.  Behind them scn_box_flatten_fwd / _bwd: the
// reference's channel-major Reshaper of the box grids with the ReLU that follows it.
#include "scn_common.h"

namespace {

struct Geo {
    int X, Y, Z, ex, ey, ez, E, S, batch;      // E = ex + ey + ez samples, S = X + Y + Z cells per box in the tables
};

struct Tables {                                // one device buffer: lo | hi | w over n_boxes * E, first | count over n_boxes * S
    int32_t *lo, *hi;
    float* w;
    int32_t *first, *count;
};

Tables tables(void* table, int64_t n_boxes, const Geo& g) {
    Tables t;
    t.lo = static_cast<int32_t*>(table);
    t.hi = t.lo + n_boxes * g.E;
    t.w = reinterpret_cast<float*>(t.hi + n_boxes * g.E);
    t.first = t.hi + 2 * n_boxes * g.E;
    t.count = t.first + n_boxes * g.S;
    return t;
}

__global__ void k_roialign_table(const float* __restrict__ boxes, int64_t n_boxes, Geo g, Tables tb) {
#pragma clang fp contract(off)
    const int64_t n = n_boxes * g.E;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / g.E;
        int i = (int)(t - r * g.E);
        int axis = 0, e = g.ex, size = g.X;
        if (i >= g.ex + g.ey) { axis = 2; i -= g.ex + g.ey; e = g.ez; size = g.Z; }
        else if (i >= g.ex) { axis = 1; i -= g.ex; e = g.ey; size = g.Y; }
        const float start = boxes[r * 6 + axis], stop = boxes[r * 6 + 3 + axis];
        const float step = __fdiv_rn(__fsub_rn(stop, start), (float)(e - 1));
        const float c = fminf(__fadd_rn(__fmul_rn((float)i, step), start), stop);
        const float fl = floorf(c), ce = ceilf(c);
        // (a NaN or out-of-range coordinate: the comparisons below send it to cell 0 / size - 1; never outside the volume)
        tb.lo[t] = fl >= 0.f ? (fl <= (float)(size - 1) ? (int)fl : size - 1) : 0;
        tb.hi[t] = ce >= 0.f ? (ce <= (float)(size - 1) ? (int)ce : size - 1) : 0;
        tb.w[t] = __fsub_rn(c, fl);
    }
}

// per (box, axis, cell): the first sample that touches the cell and the number of CONSECUTIVE samples from there that do
__global__ void k_roialign_cells(int64_t n_boxes, Geo g, Tables tb) {
    const int64_t n = n_boxes * g.S;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / g.S;
        int cell = (int)(t - r * g.S);
        int off = 0, e = g.ex;
        if (cell >= g.X + g.Y) { cell -= g.X + g.Y; off = g.ex + g.ey; e = g.ez; }
        else if (cell >= g.X) { cell -= g.X; off = g.ex; e = g.ey; }
        const int32_t *l = tb.lo + r * g.E + off, *h = tb.hi + r * g.E + off;
        int first = 0, count = 0;
        for (int i = 0; i < e; ++i) {
            const bool touch = l[i] == cell || h[i] == cell;
            if (touch && count == 0) first = i;
            if (touch && i == first + count) ++count;
        }
        tb.first[t] = first;
        tb.count[t] = count;
    }
}

template <typename T, int V> struct Vec;         // one lane's V channels of a row of T, held as fp32
template <> struct Vec<float, 1> {
    float v;
    __device__ static Vec load(const float* p) { return {*p}; }
    __device__ void store(float* p) const { *p = v; }
    __device__ static Vec zero() { return {0.f}; }
    __device__ void fma(float a, const Vec& x) { v += a * x.v; }
    __device__ Vec stored() const { return *this; }          // (what a store followed by a load gives: fp32 rows keep every bit)
    // one corner of a forward sample.  Spelled out, not left to -ffp-contract: the scalar form has always rounded the product
    // (the compiler packs this multiply with the weight's), the 16-byte forms have always fused it; pinned so that every
    // kernel that evaluates a sample -- whatever is inlined around it -- gives the same bits
    __device__ void corner(float a, const Vec& x) {
#pragma clang fp contract(off)
        v = v + a * x.v;
    }
};
template <> struct Vec<float, 4> {
    float4 v;
    __device__ static Vec load(const float* p) { return {*reinterpret_cast<const float4*>(p)}; }
    __device__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
    __device__ static Vec zero() { return {make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ void fma(float a, const Vec& x) { v.x += a * x.v.x; v.y += a * x.v.y; v.z += a * x.v.z; v.w += a * x.v.w; }
    __device__ Vec stored() const { return *this; }
    __device__ void corner(float a, const Vec& x) {
        v.x = __builtin_fmaf(a, x.v.x, v.x); v.y = __builtin_fmaf(a, x.v.y, v.y);
        v.z = __builtin_fmaf(a, x.v.z, v.z); v.w = __builtin_fmaf(a, x.v.w, v.w);
    }
};
// 8 bf16 bit patterns in one 16-byte lane: widened exactly by load, rounded to nearest even by store (the only rounding)
__device__ __forceinline__ unsigned f32_to_bf16(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
template <> struct Vec<uint16_t, 8> {
    float v[8];
    __device__ static Vec load(const uint16_t* p) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
        Vec r;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            r.v[2 * l] = __uint_as_float(w[l] << 16);
            r.v[2 * l + 1] = __uint_as_float(w[l] & 0xffff0000u);
        }
        return r;
    }
    __device__ void store(uint16_t* p) const {
        unsigned w[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) w[l] = f32_to_bf16(v[2 * l]) | (f32_to_bf16(v[2 * l + 1]) << 16);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __device__ static Vec zero() {
        Vec r;
#pragma unroll
        for (int l = 0; l < 8; ++l) r.v[l] = 0.f;
        return r;
    }
    __device__ void fma(float a, const Vec& x) {
#pragma unroll
        for (int l = 0; l < 8; ++l) v[l] += a * x.v[l];
    }
    __device__ void corner(float a, const Vec& x) {
#pragma unroll
        for (int l = 0; l < 8; ++l) v[l] = __builtin_fmaf(a, x.v[l], v[l]);
    }
    __device__ Vec stored() const {                           // rounded to bf16 once, widened again
        Vec r;
#pragma unroll
        for (int l = 0; l < 8; ++l) r.v[l] = __uint_as_float(f32_to_bf16(v[l]) << 16);
        return r;
    }
};

// The RoiAlign sample of one lane: the 8 corners in (x, y, z) order, z fastest, each weighted (wx * wy) * wz -- the ONE
// evaluation behind k_roialign_fwd and k_roialign_pool_fwd, so the two cannot drift.  `base` = the box's first table entry.
template <typename T, int V>
__device__ __forceinline__ Vec<T, V> roialign_sample(const T* __restrict__ F, const Tables& tb, int64_t base, const Geo& g,
                                                      int b, const int xs[2], const float wxs[2], int j, int k, int c, int q) {
    const int64_t ty = base + g.ex + j, tz = base + g.ex + g.ey + k;
    const int ys[2] = {tb.lo[ty], tb.hi[ty]}, zs[2] = {tb.lo[tz], tb.hi[tz]};
    float wys[2], wzs[2];
    {
#pragma clang fp contract(off)
        wys[1] = tb.w[ty]; wys[0] = 1.f - wys[1];
        wzs[1] = tb.w[tz]; wzs[0] = 1.f - wzs[1];
    }
    Vec<T, V> acc = Vec<T, V>::zero();
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                float wt;
                {
#pragma clang fp contract(off)
                    wt = (wxs[a] * wys[bb]) * wzs[cc];
                }
                const int64_t cell = (((int64_t)b * g.X + xs[a]) * g.Y + ys[bb]) * g.Z + zs[cc];
                acc.corner(wt, Vec<T, V>::load(F + cell * c + q * V));
            }
    return acc;
}

// the x cells and weights of sample i of the box whose table starts at `base`: uniform over a workgroup
__device__ __forceinline__ void x_sample(const Tables& tb, int64_t base, int i, int xs[2], float wxs[2]) {
#pragma clang fp contract(off)
    xs[0] = tb.lo[base + i]; xs[1] = tb.hi[base + i];
    wxs[1] = tb.w[base + i]; wxs[0] = 1.f - wxs[1];
}

// one workgroup per (box, x sample): the x cells and weights are uniform; its ey * ez rows x C / V lanes in 32-bit arithmetic
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_roialign_fwd(const T* __restrict__ F, Tables tb, const int32_t* __restrict__ sample_of_box, int cv, Geo g,
               T* __restrict__ Out) {
    const int c = cv * V;
    const int i = (int)(blockIdx.x % (unsigned)g.ex);
    const int64_t r = blockIdx.x / (unsigned)g.ex;
    const int64_t base = r * g.E;
    int b = sample_of_box[r];
    b = b < 0 ? 0 : (b >= g.batch ? g.batch - 1 : b);
    int xs[2];
    float wxs[2];
    x_sample(tb, base, i, xs, wxs);
    const unsigned items = (unsigned)g.ey * g.ez * cv;
    T* out_plane = Out + (r * g.ex + i) * (int64_t)g.ey * g.ez * c;
    for (unsigned t = threadIdx.x; t < items; t += blockDim.x) {
        const unsigned row = t / (unsigned)cv, q = t - row * cv;
        const unsigned j = row / (unsigned)g.ez, k = row - j * g.ez;
        roialign_sample<T, V>(F, tb, base, g, b, xs, wxs, (int)j, (int)k, c, (int)q).store(out_plane + (int64_t)row * c + q * V);
    }
}

// RoiAlign and the 2^3 max pool in one pass: one workgroup per (box, pooled x), its ey/2 * ez/2 pooled rows x C / V lanes.  A
// thread evaluates its 8 children (x, y, z order, z fastest: the max pool's scan) with roialign_sample, rounds each to the
// storage type once (`stored`: what the un-fused pair writes and reads back between its two kernels), keeps the maximum by the
// max pool's rule (a later child replaces it only when greater or NaN) and writes the value and the child's index.
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_roialign_pool_fwd(const T* __restrict__ F, Tables tb, const int32_t* __restrict__ sample_of_box, int cv, Geo g,
                    T* __restrict__ Y, uint8_t* __restrict__ arg) {
    const int c = cv * V;
    const int ox = g.ex / 2, oy = g.ey / 2, oz = g.ez / 2;
    const int io = (int)(blockIdx.x % (unsigned)ox);
    const int64_t r = blockIdx.x / (unsigned)ox;
    const int64_t base = r * g.E;
    int b = sample_of_box[r];
    b = b < 0 ? 0 : (b >= g.batch ? g.batch - 1 : b);
    int xs[2][2];
    float wxs[2][2];
    x_sample(tb, base, 2 * io, xs[0], wxs[0]);
    x_sample(tb, base, 2 * io + 1, xs[1], wxs[1]);
    const unsigned items = (unsigned)oy * oz * cv;
    for (unsigned t = threadIdx.x; t < items; t += blockDim.x) {
        const unsigned row = t / (unsigned)cv, q = t - row * cv;
        const unsigned jo = row / (unsigned)oz, ko = row - jo * oz;
        Vec<T, V> best;
        float* m = reinterpret_cast<float*>(&best);
        uint8_t am[V];
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            const int dx = ch >> 2, dy = (ch >> 1) & 1, dz = ch & 1;
            const Vec<T, V> v = roialign_sample<T, V>(F, tb, base, g, b, xs[dx], wxs[dx], (int)(2 * jo) + dy, (int)(2 * ko) + dz,
                                                      c, (int)q).stored();
            const float* vf = reinterpret_cast<const float*>(&v);
#pragma unroll
            for (int l = 0; l < V; ++l)
                if (ch == 0 || vf[l] > m[l] || vf[l] != vf[l]) { m[l] = vf[l]; am[l] = (uint8_t)ch; }
        }
        const int64_t o = (((r * ox + io) * oy + jo) * oz + ko) * c + q * V;
        best.store(Y + o);
#pragma unroll
        for (int l = 0; l < V; ++l) arg[o + l] = am[l];
    }
}

__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* a, int64_t n, int v) {
    int64_t l = 0, h = n;
    while (l < h) {
        const int64_t m = (l + h) >> 1;
        if (a[m] < v) l = m + 1; else h = m;
    }
    return l;
}

__device__ __forceinline__ float axis_weight(int l, int h, float wv, int cell) {
#pragma clang fp contract(off)
    return (l == cell ? 1.f - wv : 0.f) + (h == cell ? wv : 0.f);
}

constexpr int BWD_THREADS = 128;      // = the boxes whose x / y ranges one pass holds in LDS

// grid (batch * X * Y, ceil(Z * cv / 128)): workgroup = one (sample, x, y) column, thread = one (z, channel group) of it.
// POOL (the backward of k_roialign_pool_fwd): dOut is dY [R ex/2 ey/2 ez/2, C] and `arg` the forward's child bytes; the term of
// sample (i, j, k) is dY[r, i/2, j/2, k/2] where arg names child (i & 1, j & 1, k & 1) and 0 elsewhere -- the same ordered sums
// with the un-pooled gradient never written.  A lane none of whose channels chose the child adds only zeros: it skips the read.
template <typename T, int V, bool POOL>
__global__ void __launch_bounds__(BWD_THREADS)
k_roialign_bwd(const T* __restrict__ dOut, const uint8_t* __restrict__ arg, Tables tb, const int32_t* __restrict__ sample_of_box,
               int64_t n_boxes, int cv, Geo g, T* __restrict__ dF) {
    __shared__ int s_x0[BWD_THREADS], s_nx[BWD_THREADS], s_y0[BWD_THREADS], s_ny[BWD_THREADS];
    __shared__ int64_t s_range[2];
    const int c = cv * V;
    const unsigned col = blockIdx.x;
    const int y = (int)(col % (unsigned)g.Y), x = (int)((col / (unsigned)g.Y) % (unsigned)g.X);
    const int b = (int)(col / ((unsigned)g.Y * g.X));
    const unsigned item = blockIdx.y * BWD_THREADS + threadIdx.x;
    const bool active = item < (unsigned)g.Z * cv;
    const int z = active ? (int)(item / (unsigned)cv) : 0;
    const int q = active ? (int)(item - (unsigned)z * cv) : 0;
    if (threadIdx.x < 2) s_range[threadIdx.x] = lower_bound_i32(sample_of_box, n_boxes, b + (int)threadIdx.x);
    __syncthreads();
    const int64_t r0 = s_range[0], r1 = s_range[1];
    Vec<T, V> total = Vec<T, V>::zero();
    for (int64_t c0 = r0; c0 < r1; c0 += BWD_THREADS) {
        const int n_here = (int)(r1 - c0 < BWD_THREADS ? r1 - c0 : BWD_THREADS);
        __syncthreads();                                    // (the previous pass has been read)
        if ((int)threadIdx.x < n_here) {
            const int64_t rs = (c0 + threadIdx.x) * g.S;
            s_x0[threadIdx.x] = tb.first[rs + x];
            s_nx[threadIdx.x] = tb.count[rs + x];
            s_y0[threadIdx.x] = tb.first[rs + g.X + y];
            s_ny[threadIdx.x] = tb.count[rs + g.X + y];
        }
        __syncthreads();
        for (int e = 0; e < n_here; ++e) {
            const int nx = s_nx[e], ny = s_ny[e];
            if (nx == 0 || ny == 0 || !active) continue;
            const int64_t r = c0 + e;
            const int k0 = tb.first[r * g.S + g.X + g.Y + z], nk = tb.count[r * g.S + g.X + g.Y + z];
            if (nk == 0) continue;
            const int x0 = s_x0[e], y0 = s_y0[e];
            const int32_t *lx = tb.lo + r * g.E, *hx = tb.hi + r * g.E;
            const int32_t *ly = lx + g.ex, *hy = hx + g.ex, *lz = ly + g.ey, *hz = hy + g.ey;
            const float *wx = tb.w + r * g.E, *wy = wx + g.ex, *wz = wy + g.ey;
            Vec<T, V> si = Vec<T, V>::zero();
            for (int i = x0; i < x0 + nx; ++i) {
                const float ax = axis_weight(lx[i], hx[i], wx[i], x);
                Vec<T, V> sj = Vec<T, V>::zero();
                for (int j = y0; j < y0 + ny; ++j) {
                    const float ay = axis_weight(ly[j], hy[j], wy[j], y);
                    Vec<T, V> sk = Vec<T, V>::zero();
                    if constexpr (POOL) {
                        const int64_t prow = (((int64_t)r * (g.ex / 2) + (i >> 1)) * (g.ey / 2) + (j >> 1)) * (g.ez / 2);
                        const int cij = ((i & 1) << 2) | ((j & 1) << 1);
                        for (int k = k0; k < k0 + nk; ++k) {
                            const int64_t o = (prow + (k >> 1)) * c + q * V;
                            const int mine = cij | (k & 1);
                            uint8_t am[V];
                            __builtin_memcpy(am, arg + o, V);
                            bool any = false;
#pragma unroll
                            for (int l = 0; l < V; ++l) any |= am[l] == mine;
                            if (!any) continue;
                            Vec<T, V> gv = Vec<T, V>::load(dOut + o);
                            float* gf = reinterpret_cast<float*>(&gv);
#pragma unroll
                            for (int l = 0; l < V; ++l) gf[l] = am[l] == mine ? gf[l] : 0.f;
                            sk.fma(axis_weight(lz[k], hz[k], wz[k], z), gv);
                        }
                    } else {
                        const T* row = dOut + ((((int64_t)r * g.ex + i) * g.ey + j) * g.ez) * c + q * V;
                        for (int k = k0; k < k0 + nk; ++k)
                            sk.fma(axis_weight(lz[k], hz[k], wz[k], z), Vec<T, V>::load(row + (int64_t)k * c));
                    }
                    sj.fma(ay, sk);
                }
                si.fma(ax, sj);
            }
            total.fma(1.f, si);
        }
    }
    if (active) total.store(dF + ((int64_t)col * g.Z + z) * c + q * V);
}

// one workgroup per (box, output x): its oy * oz rows x C / V lanes
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_dense_maxpool_fwd(const T* __restrict__ X, int cv, int ox, int oy, int oz, T* __restrict__ Y,
                    uint8_t* __restrict__ arg) {
    const int c = cv * V;
    const unsigned i = blockIdx.x % (unsigned)ox;
    const int64_t r = blockIdx.x / (unsigned)ox;
    const unsigned items = (unsigned)oy * oz * cv;
    for (unsigned t = threadIdx.x; t < items; t += blockDim.x) {
        const unsigned row_in = t / (unsigned)cv, q = t - row_in * cv;
        const unsigned j = row_in / (unsigned)oz, k = row_in - j * oz;
        Vec<T, V> best;                                    // (the maximum is one of the inputs: storing it rounds nothing)
        float* m = reinterpret_cast<float*>(&best);
        uint8_t am[V];
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            const int dx = ch >> 2, dy = (ch >> 1) & 1, dz = ch & 1;
            const int64_t in_row = ((r * (2 * ox) + 2 * i + dx) * (2 * oy) + 2 * j + dy) * (2 * oz) + 2 * k + dz;
            const Vec<T, V> v = Vec<T, V>::load(X + in_row * c + q * V);
            const float* vf = reinterpret_cast<const float*>(&v);
#pragma unroll
            for (int l = 0; l < V; ++l)
                if (ch == 0 || vf[l] > m[l] || vf[l] != vf[l]) { m[l] = vf[l]; am[l] = (uint8_t)ch; }
        }
        const int64_t o = (((r * ox + i) * oy + j) * oz + k) * c + q * V;
        best.store(Y + o);
#pragma unroll
        for (int l = 0; l < V; ++l) arg[o + l] = am[l];
    }
}

// one workgroup per (box, input x): its 2 oy * 2 oz rows x C / V lanes
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_dense_maxpool_bwd(const T* __restrict__ dY, const uint8_t* __restrict__ arg, int cv, int ox, int oy, int oz,
                    T* __restrict__ dX) {
    const int c = cv * V;
    const unsigned x = blockIdx.x % (unsigned)(2 * ox);
    const int64_t r = blockIdx.x / (unsigned)(2 * ox);
    const unsigned items = (unsigned)(2 * oy) * (2 * oz) * cv;
    for (unsigned t = threadIdx.x; t < items; t += blockDim.x) {
        const unsigned row_in = t / (unsigned)cv, q = t - row_in * cv;
        const unsigned y = row_in / (unsigned)(2 * oz), z = row_in - y * (2 * oz);
        const int mine = (int)(((x & 1) << 2) | ((y & 1) << 1) | (z & 1));
        const int64_t o = (((r * ox + (x >> 1)) * oy + (y >> 1)) * oz + (z >> 1)) * c + q * V;
        const int64_t in = (((r * (2 * ox) + x) * (2 * oy) + y) * (2 * oz) + z) * c + q * V;
        Vec<T, V> g = Vec<T, V>::load(dY + o);
        float* gf = reinterpret_cast<float*>(&g);
#pragma unroll
        for (int l = 0; l < V; ++l) gf[l] = arg[o + l] == mine ? gf[l] : 0.f;
        g.store(dX + in);
    }
}

int read_geo(const int64_t* size_host, const int64_t* extract_host, int batch, int64_t n_boxes, Geo* g) {
    SCN_REQUIRE(size_host && extract_host);
    for (int d = 0; d < 3; ++d) {
        SCN_REQUIRE(size_host[d] >= 1 && size_host[d] <= (1 << 16));
        SCN_REQUIRE(extract_host[d] >= 2 && extract_host[d] <= (1 << 10));
    }
    SCN_REQUIRE(batch >= 1 && (int64_t)batch * size_host[0] * size_host[1] < (1ll << 31));      // one workgroup per column
    SCN_REQUIRE(n_boxes * extract_host[0] < (1ll << 31));                                        // one workgroup per (box, i)
    *g = Geo{(int)size_host[0], (int)size_host[1], (int)size_host[2], (int)extract_host[0], (int)extract_host[1],
             (int)extract_host[2], (int)(extract_host[0] + extract_host[1] + extract_host[2]),
             (int)(size_host[0] + size_host[1] + size_host[2]), batch};
    return SCN_OK;
}

// 16-byte lanes need 16-byte aligned rows: every pointer aligned and C a multiple of 4; anything else takes the scalar form
bool wide(int c, const void* a, const void* b) {
    return c % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}

// bf16 rows have the 16-byte form only (8 channels per lane): the storage rule of modules.py -- a slab is bf16-stored only
// when its width is a multiple of 8
bool lanes_bf16(int c, const void* a, const void* b) {
    return c % 8 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}
#define SCN_REQUIRE_BF16_LANES(c, a, b)                                                                                     \
    do {                                                                                                                    \
        if (!lanes_bf16(c, a, b)) {                                                                                         \
            snprintf(scn::g_err, sizeof(scn::g_err), "%s: bf16 rows need c %% 8 == 0 (got %d) and 16-byte aligned feature " \
                     "pointers", __func__, (int)(c));                                                                       \
            return SCN_EINVAL;                                                                                              \
        }                                                                                                                   \
    } while (0)

int pool_geo(const int64_t* extent_host, int64_t n_boxes, int c, int* o) {
    SCN_REQUIRE(extent_host && n_boxes >= 0 && c >= 1);
    for (int d = 0; d < 3; ++d) {
        SCN_REQUIRE(extent_host[d] >= 2 && extent_host[d] <= (1 << 10) && extent_host[d] % 2 == 0);
        o[d] = (int)(extent_host[d] / 2);
    }
    SCN_REQUIRE(n_boxes * extent_host[0] < (1ll << 31));                                          // one workgroup per (box, x)
    return SCN_OK;
}

// The launches behind the entry points: rows of T in lanes of W elements when `wd` (16 bytes), else of N (fp32: 4 and 1, the
// scalar form; bf16: 8 and 8 -- the entry point has refused every other row)
// (argmax == nullptr: the plain forward into Out [R ex ey ez, C]; else the fused one: Out is Y [R ex/2 ey/2 ez/2, C])
template <typename T, int W, int N>
int roialign_fwd(const T* F, const Geo& g, int c, bool wd, const float* boxes, const int32_t* sample_of_box, int64_t n_boxes,
                 void* table, T* Out, uint8_t* argmax, scn_stream_t stream) {
    const Tables tb = tables(table, n_boxes, g);
    hipLaunchKernelGGL(k_roialign_table, dim3(scn::ew_grid(n_boxes * g.E, 256)), dim3(256), 0, scn::S(stream), boxes, n_boxes, g, tb);
    SCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_roialign_cells, dim3(scn::ew_grid(n_boxes * g.S, 256)), dim3(256), 0, scn::S(stream), n_boxes, g, tb);
    SCN_LAUNCH_CHECK();
    if (argmax) {
        const dim3 grid((unsigned)(n_boxes * (g.ex / 2)));
        if (wd)
            hipLaunchKernelGGL((k_roialign_pool_fwd<T, W>), grid, dim3(256), 0, scn::S(stream), F, tb, sample_of_box, c / W, g, Out, argmax);
        else
            hipLaunchKernelGGL((k_roialign_pool_fwd<T, N>), grid, dim3(256), 0, scn::S(stream), F, tb, sample_of_box, c / N, g, Out, argmax);
        SCN_LAUNCH_CHECK();
        return SCN_OK;
    }
    const dim3 grid((unsigned)(n_boxes * g.ex));
    if (wd)
        hipLaunchKernelGGL((k_roialign_fwd<T, W>), grid, dim3(256), 0, scn::S(stream), F, tb, sample_of_box, c / W, g, Out);
    else
        hipLaunchKernelGGL((k_roialign_fwd<T, N>), grid, dim3(256), 0, scn::S(stream), F, tb, sample_of_box, c / N, g, Out);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

// (argmax == nullptr: dOut is the un-pooled gradient; else dOut is dY and the kernel masks it by argmax)
template <typename T, int W, int N>
int roialign_bwd(const T* dOut, const uint8_t* argmax, const void* table, const int32_t* sample_of_box, int64_t n_boxes, int batch,
                 const Geo& g, int c, bool wd, T* dF, scn_stream_t stream) {
    const Tables tb = tables(const_cast<void*>(table), n_boxes, g);
    const int cv = wd ? c / W : c / N;
    SCN_REQUIRE(scn::cdiv((int64_t)g.Z * cv, BWD_THREADS) <= 65535);
    const dim3 grid((unsigned)(batch * g.X * g.Y), (unsigned)scn::cdiv((int64_t)g.Z * cv, BWD_THREADS));
#define SCN_ROIALIGN_BWD(V, POOL)                                                                                           \
    hipLaunchKernelGGL((k_roialign_bwd<T, V, POOL>), grid, dim3(BWD_THREADS), 0, scn::S(stream), dOut, argmax, tb, sample_of_box, \
                       n_boxes, cv, g, dF)
    if (argmax) {
        if (wd) SCN_ROIALIGN_BWD(W, true); else SCN_ROIALIGN_BWD(N, true);
    } else {
        if (wd) SCN_ROIALIGN_BWD(W, false); else SCN_ROIALIGN_BWD(N, false);
    }
#undef SCN_ROIALIGN_BWD
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

template <typename T, int W, int N>
int maxpool_fwd(const T* X, int64_t n_boxes, const int* o, int c, bool wd, T* Y, uint8_t* argmax, scn_stream_t stream) {
    const dim3 grid((unsigned)(n_boxes * o[0]));
    if (wd)
        hipLaunchKernelGGL((k_dense_maxpool_fwd<T, W>), grid, dim3(256), 0, scn::S(stream), X, c / W, o[0], o[1], o[2], Y, argmax);
    else
        hipLaunchKernelGGL((k_dense_maxpool_fwd<T, N>), grid, dim3(256), 0, scn::S(stream), X, c / N, o[0], o[1], o[2], Y, argmax);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

template <typename T, int W, int N>
int maxpool_bwd(const T* dY, const uint8_t* argmax, int64_t n_boxes, const int* o, int c, bool wd, T* dX, scn_stream_t stream) {
    const dim3 grid((unsigned)(n_boxes * 2 * o[0]));
    if (wd)
        hipLaunchKernelGGL((k_dense_maxpool_bwd<T, W>), grid, dim3(256), 0, scn::S(stream), dY, argmax, c / W, o[0], o[1], o[2], dX);
    else
        hipLaunchKernelGGL((k_dense_maxpool_bwd<T, N>), grid, dim3(256), 0, scn::S(stream), dY, argmax, c / N, o[0], o[1], o[2], dX);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

}  // namespace

extern "C" int scn_roialign_fwd(const float* F, int batch, const int64_t* size_host, int c, const float* boxes,
                                const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table,
                                float* Out, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1);
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(F && boxes && sample_of_box && table && Out);
    return roialign_fwd<float, 4, 1>(F, g, c, wide(c, F, Out), boxes, sample_of_box, n_boxes, table, Out, nullptr, stream);
}

extern "C" int scn_roialign_fwd_bf16(const uint16_t* F, int batch, const int64_t* size_host, int c, const float* boxes,
                                     const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table,
                                     uint16_t* Out, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1);
    SCN_REQUIRE_BF16_LANES(c, F, Out);
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(F && boxes && sample_of_box && table && Out);
    return roialign_fwd<uint16_t, 8, 8>(F, g, c, true, boxes, sample_of_box, n_boxes, table, Out, nullptr, stream);
}

extern "C" int scn_roialign_bwd(const float* dOut, const void* table, const int32_t* sample_of_box, int64_t n_boxes, int batch,
                                const int64_t* size_host, int c, const int64_t* extract_host, float* dF,
                                scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1 && dF);
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    const int64_t cells = (int64_t)batch * g.X * g.Y * g.Z;
    if (n_boxes == 0) {
        SCN_HIP(hipMemsetAsync(dF, 0, (size_t)cells * c * sizeof(float), scn::S(stream)));
        return SCN_OK;
    }
    SCN_REQUIRE(dOut && table && sample_of_box);
    return roialign_bwd<float, 4, 1>(dOut, nullptr, table, sample_of_box, n_boxes, batch, g, c, wide(c, dOut, dF), dF, stream);
}

extern "C" int scn_roialign_bwd_bf16(const uint16_t* dOut, const void* table, const int32_t* sample_of_box, int64_t n_boxes,
                                     int batch, const int64_t* size_host, int c, const int64_t* extract_host, uint16_t* dF,
                                     scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1 && dF);
    SCN_REQUIRE_BF16_LANES(c, dOut, dF);
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    const int64_t cells = (int64_t)batch * g.X * g.Y * g.Z;
    if (n_boxes == 0) {
        SCN_HIP(hipMemsetAsync(dF, 0, (size_t)cells * c * sizeof(uint16_t), scn::S(stream)));      // (+0 in bf16 too)
        return SCN_OK;
    }
    SCN_REQUIRE(dOut && table && sample_of_box);
    return roialign_bwd<uint16_t, 8, 8>(dOut, nullptr, table, sample_of_box, n_boxes, batch, g, c, true, dF, stream);
}

extern "C" int scn_dense_maxpool_fwd(const float* X, int64_t n_boxes, const int64_t* extent_host, int c, float* Y,
                                     uint8_t* argmax, scn_stream_t stream) {
    int o[3];
    if (int rc = pool_geo(extent_host, n_boxes, c, o)) return rc;
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(X && Y && argmax);
    return maxpool_fwd<float, 4, 1>(X, n_boxes, o, c, wide(c, X, Y), Y, argmax, stream);
}

extern "C" int scn_dense_maxpool_fwd_bf16(const uint16_t* X, int64_t n_boxes, const int64_t* extent_host, int c, uint16_t* Y,
                                          uint8_t* argmax, scn_stream_t stream) {
    int o[3];
    if (int rc = pool_geo(extent_host, n_boxes, c, o)) return rc;
    SCN_REQUIRE_BF16_LANES(c, X, Y);
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(X && Y && argmax);
    return maxpool_fwd<uint16_t, 8, 8>(X, n_boxes, o, c, true, Y, argmax, stream);
}

extern "C" int scn_dense_maxpool_bwd(const float* dY, const uint8_t* argmax, int64_t n_boxes, const int64_t* extent_host, int c,
                                     float* dX, scn_stream_t stream) {
    int o[3];
    if (int rc = pool_geo(extent_host, n_boxes, c, o)) return rc;
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(dY && argmax && dX);
    return maxpool_bwd<float, 4, 1>(dY, argmax, n_boxes, o, c, wide(c, dY, dX), dX, stream);
}

extern "C" int scn_dense_maxpool_bwd_bf16(const uint16_t* dY, const uint8_t* argmax, int64_t n_boxes, const int64_t* extent_host,
                                          int c, uint16_t* dX, scn_stream_t stream) {
    int o[3];
    if (int rc = pool_geo(extent_host, n_boxes, c, o)) return rc;
    SCN_REQUIRE_BF16_LANES(c, dY, dX);
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(dY && argmax && dX);
    return maxpool_bwd<uint16_t, 8, 8>(dY, argmax, n_boxes, o, c, true, dX, stream);
}

// ---- RoiAlign + max pool in one pass (the class head without an input convolution cuts at the RPN stack's full width) ----
namespace {

int even_extract(const int64_t* extract_host) {
    SCN_REQUIRE(extract_host);
    for (int d = 0; d < 3; ++d) SCN_REQUIRE(extract_host[d] >= 2 && extract_host[d] % 2 == 0);
    return SCN_OK;
}

}  // namespace

extern "C" int scn_roialign_pool_fwd(const float* F, int batch, const int64_t* size_host, int c, const float* boxes,
                                     const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table,
                                     float* Y, uint8_t* argmax, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1);
    if (int rc = even_extract(extract_host)) return rc;
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(F && boxes && sample_of_box && table && Y && argmax);
    return roialign_fwd<float, 4, 1>(F, g, c, wide(c, F, Y), boxes, sample_of_box, n_boxes, table, Y, argmax, stream);
}

extern "C" int scn_roialign_pool_fwd_bf16(const uint16_t* F, int batch, const int64_t* size_host, int c, const float* boxes,
                                          const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host,
                                          void* table, uint16_t* Y, uint8_t* argmax, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1);
    SCN_REQUIRE_BF16_LANES(c, F, Y);
    if (int rc = even_extract(extract_host)) return rc;
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(F && boxes && sample_of_box && table && Y && argmax);
    return roialign_fwd<uint16_t, 8, 8>(F, g, c, true, boxes, sample_of_box, n_boxes, table, Y, argmax, stream);
}

extern "C" int scn_roialign_pool_bwd(const float* dY, const uint8_t* argmax, const void* table, const int32_t* sample_of_box,
                                     int64_t n_boxes, int batch, const int64_t* size_host, int c, const int64_t* extract_host,
                                     float* dF, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1 && dF);
    if (int rc = even_extract(extract_host)) return rc;
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    const int64_t cells = (int64_t)batch * g.X * g.Y * g.Z;
    if (n_boxes == 0) {
        SCN_HIP(hipMemsetAsync(dF, 0, (size_t)cells * c * sizeof(float), scn::S(stream)));
        return SCN_OK;
    }
    SCN_REQUIRE(dY && argmax && table && sample_of_box);
    return roialign_bwd<float, 4, 1>(dY, argmax, table, sample_of_box, n_boxes, batch, g, c, wide(c, dY, dF), dF, stream);
}

extern "C" int scn_roialign_pool_bwd_bf16(const uint16_t* dY, const uint8_t* argmax, const void* table,
                                          const int32_t* sample_of_box, int64_t n_boxes, int batch, const int64_t* size_host,
                                          int c, const int64_t* extract_host, uint16_t* dF, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && c >= 1 && dF);
    SCN_REQUIRE_BF16_LANES(c, dY, dF);
    if (int rc = even_extract(extract_host)) return rc;
    Geo g;
    if (int rc = read_geo(size_host, extract_host, batch, n_boxes, &g)) return rc;
    const int64_t cells = (int64_t)batch * g.X * g.Y * g.Z;
    if (n_boxes == 0) {
        SCN_HIP(hipMemsetAsync(dF, 0, (size_t)cells * c * sizeof(uint16_t), scn::S(stream)));      // (+0 in bf16 too)
        return SCN_OK;
    }
    SCN_REQUIRE(dY && argmax && table && sample_of_box);
    return roialign_bwd<uint16_t, 8, 8>(dY, argmax, table, sample_of_box, n_boxes, batch, g, c, true, dF, stream);
}

// ---- the reference's Reshaper behind the box grids: [R V, C] rows -> [R, C V] channel-major vectors, with the ReLU that
// follows it in linear_layer folded in (`relu`).  One element per thread both ways: the side it WRITES is contiguous, the side
// it reads is a box's own V x C block (a few KB: cached). ----
namespace {

__global__ void k_box_flatten_fwd(const float* __restrict__ X, int64_t n, int64_t v, int c, int relu, float* __restrict__ Y) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / (v * c), e = t - r * (v * c);
        const int64_t ch = e / v, s = e - ch * v;
        const float x = X[(r * v + s) * c + ch];
        Y[t] = relu ? (x > 0.f || x != x ? x : 0.f) : x;      // (NaN stays NaN, as nn.ReLU keeps it)
    }
}

__global__ void k_box_flatten_bwd(const float* __restrict__ X, const float* __restrict__ dY, int64_t n, int64_t v, int c,
                                  int relu, float* __restrict__ dX) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / c, ch = t - row * c;
        const int64_t r = row / v, s = row - r * v;
        const float g = dY[(r * c + ch) * v + s];
        dX[t] = !relu || X[t] > 0.f ? g : 0.f;
    }
}

}  // namespace

extern "C" int scn_box_flatten_fwd(const float* X, int64_t n_boxes, int64_t v, int c, int relu, float* Y, scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && v >= 1 && c >= 1 && v * c < (1ll << 31));
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(X && Y);
    const int64_t n = n_boxes * v * c;
    hipLaunchKernelGGL(k_box_flatten_fwd, dim3(scn::ew_grid(n, 256)), dim3(256), 0, scn::S(stream), X, n, v, c, relu, Y);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}

extern "C" int scn_box_flatten_bwd(const float* X, const float* dY, int64_t n_boxes, int64_t v, int c, int relu, float* dX,
                                   scn_stream_t stream) {
    SCN_REQUIRE(n_boxes >= 0 && v >= 1 && c >= 1 && v * c < (1ll << 31));
    if (n_boxes == 0) return SCN_OK;
    SCN_REQUIRE(dY && dX && (X || !relu));
    const int64_t n = n_boxes * v * c;
    hipLaunchKernelGGL(k_box_flatten_bwd, dim3(scn::ew_grid(n, 256)), dim3(256), 0, scn::S(stream), X, dY, n, v, c, relu, dX);
    SCN_LAUNCH_CHECK();
    return SCN_OK;
}
