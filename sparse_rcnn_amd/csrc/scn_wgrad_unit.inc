// Body of one k_wgrad_direct work unit, included into the standalone kernel (k_wgrad_direct) and into every case of the
// grouped kernel (k_wgrad_group), so that both compile the same text in the kernel's own scope: as a __device__ function
// the same code came out with 20-30 % more registers (4 x 4 blocks: 230 -> 290, one workgroup per CU instead of two).
// In scope: TA, TB, QUAD, EDGE, IDENT, HB (constants); X_0, cin, dY_0, cout, in_rows, out_rows, plan (DPlan or GJob),
// slabs, relu_in, db_slabs, db_mask, cout_pad, more (WdOps or GJob); unit and zb (the standalone grid's blockIdx.x / .z).
{
    typedef typename Frag<TA>::type fa_t;
    typedef typename Frag<TB>::type fb_t;
    constexpr bool PACKED = HB && !EDGE;                         // bf16 rows kept packed in the ring
    typedef typename RawFrag<TA, PACKED>::type ra_t;
    typedef typename RawFrag<TB, PACKED>::type rb_t;
    constexpr int ES = HB ? 2 : 4;                               // bytes per stored element
    constexpr int WI = 16 * TA, WJ = 16 * TB;                   // wave block
    constexpr int CBI = QUAD ? 2 * WI : WI, CBJ = QUAD ? 2 * WJ : WJ;
    constexpr int NACC = TA * TB;
    extern __shared__ __attribute__((aligned(16))) float red[];     // K mode: 4 partial blocks + 4 x 64 bias sums

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if WD_TIMELINE
    const long long wd_t0 = wall_clock64();
#endif
    const int i = lane & 15, kq = lane >> 4;
    // offset of this unit: unit_start is non-decreasing, so o = #{o' : unit >= unit_start[o'+1]} -- one ballot instead
    // of a serial scalar search (every workgroup pays its prologue; with ~1000 short workgroups it adds up)
    const int ov = wd_offset_of(plan, unit, lane);                               // (virtual) offset of this unit
    const int prob = ov / plan.n_real;                                            // which operand pair (scalar)
    const int o = ov - prob * plan.n_real;
    const float* X = prob ? (const float*)more.X[prob] : X_0;
    const float* dY = prob ? (const float*)more.dY[prob] : dY_0;
    const int s_unit = unit - plan.unit_start[ov];
    const int bi = zb / plan.nbj, bj = zb % plan.nbj;
    const int wi = QUAD ? (wave >> 1) : 0, wj = QUAD ? (wave & 1) : 0;
    const int ci0 = bi * CBI + wi * WI, co0 = bj * CBJ + wj * WJ;       // first channel of the wave block

    long long p_lo, p_hi;
    wd_range(plan, ov, o, prob, p_lo, p_hi);
    const long long p0 = p_lo + (long long)s_unit * plan.per;
    const long long p1 = p0 + plan.per < p_hi ? p0 + plan.per : p_hi;
    // this wave's rule range [q0, q1): K mode = a quarter of the unit (multiple of 16 rules), QUAD = the whole unit
    long long q0 = p0, q1 = p1;
    if (!QUAD) {
        const long long quarter = ((p1 - p0 + 63) / 64) * 16;
        q0 = p0 + wave * quarter;
        q1 = q0 + quarter < p1 ? q0 + quarter : p1;
    }
    // rules of this wave, relative to q0: nfull whole blocks of 16 (pipelined, unmasked) + one masked tail block
    const int nrel = __builtin_amdgcn_readfirstlane(q1 > q0 ? (int)(q1 - q0) : 0);
    const int nfull = nrel / 16;
    const int* inq = IDENT ? nullptr : in_rows + q0;
    const int* outq = IDENT ? nullptr : out_rows + q0;
    const int lane_r = 4 * kq;
    const int q0i = (int)q0;                                   // identity list: rule index == row index (< 2^31)

    // channel offsets of this lane inside a row: T consecutive floats starting at ci0 + TA*i (resp. co0 + TB*i)
    const int ca = ci0 + TA * i, cbn = co0 + TB * i;
    bool a_ok[TA], b_ok[TB];
#pragma unroll
    for (int t = 0; t < TA; ++t) a_ok[t] = !EDGE || ca + t < cin;
#pragma unroll
    for (int t = 0; t < TB; ++t) b_ok[t] = !EDGE || cbn + t < cout;
    const bool do_db = db_slabs != nullptr && ((db_mask >> o) & 1u) && bi == 0 && wi == 0;

    f32x4 acc[TA][TB];
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float dbacc[TB];
#pragma unroll
    for (int t = 0; t < TB; ++t) dbacc[t] = 0.f;

    // A block = 16 rules = 4 MFMA steps; lane group kq owns rules qb + 4*kq + s, s = step.
    // Three named register sets (0,1,2) rotate through: indices of block b+3.., rows of block b+2.., MFMAs of block b.
    // The instruction budget matters as much as the latency: a 16x16x4 fp32 MFMA is 32 cycles = 8 VALU slots, and at
    // TA = TB = 2 a block has only 16 of them.  So: the block offset of the index loads is SCALAR (saddr + lane offset +
    // immediate, zero VALU), a row address is ONE v_mad_i64_i32 (row * stride + per-lane base), ReLU is one v_max
    // against 0 or -inf, and rule masking exists only in the peeled tail block.  (First version: ~110 VALU per block,
    // VALU-issue-bound at 1/3 of the MFMA rate.)
    const char* xlane = (const char*)X + (long long)ca * ES;
    const char* ylane = (const char*)dY + (long long)cbn * ES;
    const int xstride = ES * cin, ystride = ES * cout;         // int: row * stride is one v_mad_i64_i32
    const int relu_lo = (relu_in & 1) ? 0 : (int)0x80000000;
    // EDGE with whole fragments (relu_in bit 1, set by the host when Cin % TA == 0, Cout % TB == 0 and rows are 16-byte
    // aligned -- the reference's 48 / 80 / 112-channel layers on 64-wide blocks): a lane's T channels are all inside the
    // layer or all outside, so the row piece is still ONE vector load, from a clamped lane offset, zeroed at use
    const bool evec = EDGE && !HB && (relu_in & 2);
    const char* xlane_e = (const char*)X + (long long)(a_ok[0] ? ca : 0) * ES;
    const char* ylane_e = (const char*)dY + (long long)(b_ok[0] ? cbn : 0) * ES;
    const int last_full = nfull > 0 ? (nfull - 1) * 16 : 0;        // prefetches past the end re-read the last whole block
#define WD_IDX(IN, OUT, QB)                                                                          \
    {                                                                                                \
        const int qs_ = (QB) < last_full ? (QB) : last_full;           /* scalar */                  \
        _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                                           \
            IN[s_] = IDENT ? q0i + qs_ + lane_r + s_ : inq[qs_ + lane_r + s_];                       \
            OUT[s_] = (IDENT || WD_EXP) ? q0i + qs_ + lane_r + s_ : outq[qs_ + lane_r + s_];         \
        }                                                                                            \
    }
#define WD_ROWS(A, B, IN, OUT)                                                                       \
    _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                                               \
        if (EDGE) {                  /* element loads; channels past the end read channel 0 (zeroed at use) */ \
            if constexpr (!HB) {                                                                     \
                if (evec) {              /* whole fragments in or out: one vector load per row piece */ \
                    A[s_] = *(const ra_t*)(xlane_e + (long long)IN[s_] * xstride);                   \
                    B[s_] = *(const rb_t*)(ylane_e + (long long)OUT[s_] * ystride);                  \
                    continue;                                                                        \
                }                                                                                    \
            }                                                                                        \
            if (HB) {                                                                                \
                const unsigned short* xr_ = (const unsigned short*)X + (long long)IN[s_] * cin;      \
                const unsigned short* yr_ = (const unsigned short*)dY + (long long)OUT[s_] * cout;   \
                _Pragma("unroll") for (int t_ = 0; t_ < TA; ++t_)                                    \
                    A[s_][t_] = __uint_as_float((unsigned)xr_[a_ok[t_] ? ca + t_ : 0] << 16);       \
                _Pragma("unroll") for (int t_ = 0; t_ < TB; ++t_)                                    \
                    B[s_][t_] = __uint_as_float((unsigned)yr_[b_ok[t_] ? cbn + t_ : 0] << 16);       \
            } else {                                                                                 \
                const float* xr_ = X + (long long)IN[s_] * cin;                                      \
                const float* yr_ = dY + (long long)OUT[s_] * cout;                                   \
                _Pragma("unroll") for (int t_ = 0; t_ < TA; ++t_) A[s_][t_] = xr_[a_ok[t_] ? ca + t_ : 0]; \
                _Pragma("unroll") for (int t_ = 0; t_ < TB; ++t_) B[s_][t_] = yr_[b_ok[t_] ? cbn + t_ : 0]; \
            }                                                                                        \
        } else if (WD_EXP == 1) {                                                                    \
            A[s_] = *(const ra_t*)(xlane + (long long)IN[s_] * xstride);                             \
            _Pragma("unroll") for (int t_ = 0; t_ < (int)(sizeof(rb_t) / 4); ++t_)                   \
                ((float*)&B[s_])[t_] = __int_as_float(0x3f800000 | (OUT[s_] & 0xffff));              \
        } else if (WD_EXP == 2) {                                                                    \
            A[s_] = *(const ra_t*)(xlane + (long long)IN[s_] * xstride);                             \
            B[s_] = *(const rb_t*)((const char*)red + (((OUT[s_] & 15) * 16 + i) * (int)sizeof(rb_t)));  \
        } else {                                                                                     \
            A[s_] = *(const ra_t*)(xlane + (long long)IN[s_] * xstride);                             \
            B[s_] = *(const rb_t*)(ylane + (long long)OUT[s_] * ystride);                            \
        }                                                                                            \
    }
    // MASK: rules at or past `nrel` contribute nothing (tail block only)
#define WD_MFMA(A, B, QB, MASK)                                                                      \
    _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                                               \
        const bool v_ = !(MASK) || (QB) + lane_r + s_ < nrel;                                        \
        fa_t a_ = widen<TA, PACKED>(A[s_]);                                                          \
        fb_t b_ = widen<TB, PACKED>(B[s_]);                                                          \
        _Pragma("unroll") for (int t_ = 0; t_ < TA; ++t_) {                                          \
            /* ReLU as ONE integer max on the bit pattern (fmaxf costs a canonicalising v_max x,x more; inline asm \
               hides the VALU->MFMA hazard from the compiler): negative floats are negative ints */  \
            float x_ = __int_as_float(max(__float_as_int(a_[t_]), relu_lo));                         \
            if ((MASK) || EDGE) x_ = (v_ && a_ok[t_]) ? x_ : 0.f;                                    \
            a_[t_] = x_;                                                                             \
        }                                                                                            \
        if ((MASK) || EDGE) {                                                                        \
            _Pragma("unroll") for (int t_ = 0; t_ < TB; ++t_) b_[t_] = (v_ && b_ok[t_]) ? b_[t_] : 0.f; \
        }                                                                                            \
        if (do_db) { _Pragma("unroll") for (int t_ = 0; t_ < TB; ++t_) dbacc[t_] += b_[t_]; }         \
        _Pragma("unroll") for (int ta_ = 0; ta_ < TA; ++ta_)                                         \
            _Pragma("unroll") for (int tb_ = 0; tb_ < TB; ++tb_)                                     \
                acc[ta_][tb_] = MFMA16(a_[ta_], b_[tb_], acc[ta_][tb_]);                             \
    }

    int in0[4], out0[4], in1[4], out1[4], in2[4], out2[4];
    ra_t a0[4], a1[4], a2[4];
    rb_t b0[4], b1[4], b2[4];
    // Ring depth: 3 sets (rows two blocks ahead) for the small wave blocks; 2 sets (one block ahead) at TA = TB = 4,
    // where a block is 64 MFMAs = 2048 cycles and the third set would cost the second resident wave per SIMD
    // (64 accumulators + 3 x 32 row registers + indices > 256 registers).
    constexpr bool DEEP = WD_DEEP_ALL || TA * TB < 16;
    if (DEEP && nfull > 0) {
        // (the prologue's issue order is pinned too: the loop header's wait counts are the merge of both ways in)
        WD_IDX(in0, out0, 0);
        WD_IDX(in1, out1, 16);
        __builtin_amdgcn_sched_barrier(0);
        WD_IDX(in2, out2, 32);
        __builtin_amdgcn_sched_barrier(0);
        WD_ROWS(a0, b0, in0, out0);
        WD_IDX(in0, out0, 48);
        __builtin_amdgcn_sched_barrier(0);
        WD_ROWS(a1, b1, in1, out1);
        WD_IDX(in1, out1, 64);
        // steady state, block b (set b%3 holds its rows): queue rows of b+2 (indices arrived), indices of b+5, multiply b.
        // The scheduling barriers keep each phase's address arithmetic in its phase: hoisted to the loop top it made
        // every iteration wait for the newest index loads (s_waitcnt vmcnt(0)) and serialised the pipeline.
        int qb = 0, b = 0;
        for (; b + 3 <= nfull; b += 3, qb += 48) {
            __builtin_amdgcn_sched_barrier(0);
            WD_ROWS(a2, b2, in2, out2);
            WD_IDX(in2, out2, qb + 80);
            WD_MFMA(a0, b0, qb, false);
            __builtin_amdgcn_sched_barrier(0);
            WD_ROWS(a0, b0, in0, out0);
            WD_IDX(in0, out0, qb + 96);
            WD_MFMA(a1, b1, qb + 16, false);
            __builtin_amdgcn_sched_barrier(0);
            WD_ROWS(a1, b1, in1, out1);
            WD_IDX(in1, out1, qb + 112);
            WD_MFMA(a2, b2, qb + 32, false);
        }
        __builtin_amdgcn_sched_barrier(0);
        // remainder: 0, 1 or 2 whole blocks; their rows are already queued (sets 0 and 1)
        if (b < nfull) { WD_MFMA(a0, b0, qb, false); }
        if (b + 1 < nfull) { WD_MFMA(a1, b1, qb + 16, false); }
    }
    if (!DEEP && nfull > 0) {
        WD_IDX(in0, out0, 0);
        __builtin_amdgcn_sched_barrier(0);
        WD_IDX(in1, out1, 16);
        __builtin_amdgcn_sched_barrier(0);
        WD_ROWS(a0, b0, in0, out0);
        WD_IDX(in0, out0, 32);
        // block b: set b%2 holds its rows; queue rows of b+1, indices of b+3, multiply b
        int qb = 0, b = 0;
        for (; b + 2 <= nfull; b += 2, qb += 32) {
            __builtin_amdgcn_sched_barrier(0);
            WD_ROWS(a1, b1, in1, out1);
            WD_IDX(in1, out1, qb + 48);
            WD_MFMA(a0, b0, qb, false);
            __builtin_amdgcn_sched_barrier(0);
            WD_ROWS(a0, b0, in0, out0);
            WD_IDX(in0, out0, qb + 64);
            WD_MFMA(a1, b1, qb + 16, false);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (b < nfull) { WD_MFMA(a0, b0, qb, false); }
    }
    if (nrel > nfull * 16) {        // tail block: clamped indices, masked values, no pipelining (once per wave)
        const int qt = nfull * 16;
#pragma unroll
        for (int s_ = 0; s_ < 4; ++s_) {
            int r_ = qt + lane_r + s_;
            r_ = r_ < nrel ? r_ : nrel - 1;
            in2[s_] = IDENT ? q0i + r_ : inq[r_];
            out2[s_] = IDENT ? q0i + r_ : outq[r_];
        }
        WD_ROWS(a2, b2, in2, out2);
        WD_MFMA(a2, b2, qt, true);
    }
#undef WD_IDX
#undef WD_ROWS
#undef WD_MFMA

#if WD_TIMELINE
    const long long wd_t1 = wall_clock64();
#endif
    float* slab = slabs + ((long long)unit * (plan.nbi * plan.nbj) + zb) * (CBI * CBJ);
    float* dbr = red + (QUAD ? 0 : 4 * NACC * 4 * 64);                  // [4 waves][64 columns]

    // ---- K mode: add the four waves' partial blocks in wave order.  Every wave stores its whole block to LDS
    // ([wave][element][lane], conflict-free) and then OWNS a quarter of the elements: it adds the four copies of its
    // quarter in wave order and writes those rows of the slab -- the epilogue is spread over the 4 waves and never holds
    // more than one quarter in registers (a first version had wave 0 add everything: 200+ VGPRs, one wave per SIMD).
    // acc[a][b][j] is row TA*(4kq+j)+a, column TB*i+b of the wave block.
    if (!QUAD) {
        float* mine = red + wave * (NACC * 4 * 64);
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) mine[((a * TB + b) * 4 + j) * 64 + lane] = acc[a][b][j];
        __syncthreads();
        // the 4 TA (a, j) pairs in order p = 4 a + j, TA consecutive ones per wave (TA = 4: a = wave; TA = 2: a = wave / 2,
        // j = 2 (wave & 1) + jj -- the owners of rounds 1-2; TA = 3: three pairs that may straddle two a)
#pragma unroll
        for (int jj = 0; jj < TA; ++jj) {
            const int p_own = wave * TA + jj;
            const int a_own = p_own >> 2, jx = p_own & 3;
            fb_t v;
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const float* src = red + ((a_own * TB + b) * 4 + jx) * 64 + lane;
                v[b] = ((src[0] + src[NACC * 4 * 64]) + src[2 * NACC * 4 * 64]) + src[3 * NACC * 4 * 64];
            }
            const int r = TA * (4 * kq + jx) + a_own;
            *(fb_t*)(slab + r * CBJ + TB * i) = v;
        }
    } else {
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = wi * WI + TA * (4 * kq + j) + a;
                fb_t v;
#pragma unroll
                for (int b = 0; b < TB; ++b) v[b] = acc[a][b][j];
                *(fb_t*)(slab + r * CBJ + wj * WJ + TB * i) = v;
            }
    }

    // ---- bias gradient: lanes (i, kq) hold column sums of their own rules -> add the 4 kq groups, then the waves ------
    if (db_slabs != nullptr && ((db_mask >> o) & 1u) && bi == 0) {
#pragma unroll
        for (int t = 0; t < TB; ++t) {
            float v = dbacc[t];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            dbacc[t] = v;
        }
        if (!QUAD) {
            if (kq == 0) {
#pragma unroll
                for (int t = 0; t < TB; ++t) dbr[wave * 64 + TB * i + t] = dbacc[t];
            }
            __syncthreads();
            if (wave == 0 && kq == 0) {
#pragma unroll
                for (int t = 0; t < TB; ++t) {
                    const int c = TB * i + t;
                    const float v = ((dbr[c] + dbr[64 + c]) + dbr[128 + c]) + dbr[192 + c];
                    if (co0 + c < cout_pad) db_slabs[(long long)unit * cout_pad + co0 + c] = v;
                }
            }
        } else if (wi == 0 && kq == 0) {
#pragma unroll
            for (int t = 0; t < TB; ++t)
                if (cbn + t < cout_pad) db_slabs[(long long)unit * cout_pad + cbn + t] = dbacc[t];
        }
    }
#if WD_TIMELINE
    if (lane == 0) {
        const long long slot = (((long long)blockIdx.x + (long long)gridDim.x * blockIdx.z) * 4 + wave) & 65535;
        wd_stamps[slot * 4 + 0] = wd_t0; wd_stamps[slot * 4 + 1] = wd_t1; wd_stamps[slot * 4 + 2] = wall_clock64();
        wd_stamps[slot * 4 + 3] = nrel;
    }
#endif
}
