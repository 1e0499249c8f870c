/*
 * scn_mi355x.h -- C ABI of libscn_mi355x.so: the MI355X-native (gfx950) replacement for the
 * native boundary of `sparseconvnet` (SCN), the un-vendored third-party package in which the
 * reference's sparse-convolution hot path runs.
 *
 * What it replaces.  The reference (LeonhardFeiner/sparse_rcnn) reaches native code only through
 * `import sparseconvnet as scn` (ndsis/modules/module_factory.py:5, model.py:6,
 * custom_operations.py:4, roi_select_sparse.py:3).  Upstream, every scn Python layer forwards to
 * a pybind11 module `sparseconvnet.SCN` (`Metadata_3`, `<Op>_updateOutput`, `<Op>_backward`); that
 * module is NOT under /root/reference and cannot be cited by line, so each entry point below cites
 * the REFERENCE call site whose work it performs.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no C++/torch types.  Every pointer is a DEVICE pointer
 *     unless its name ends in `_host`.  `stream` is a hipStream_t passed as void*.
 *   - Ownership: the caller owns every buffer (feature slabs, hash tables, rule tables, scratch).
 *     The library allocates nothing and keeps no state besides the last-error string, so the
 *     caller's stream-ordered allocator (PyTorch's caching allocator in the Python host layer)
 *     governs lifetime.  Data-dependent sizes use two phases: a *_scan/_build call that returns
 *     the size through a `_host` out-parameter (it synchronises `stream` once; documented per
 *     function), then the caller allocates and calls the matching *_fill.
 *   - Every function returns 0 on success or an SCN_E* code; scn_last_error_string() describes
 *     the last failure on the calling thread.  Nothing aborts.
 *   - Threading: functions are re-entrant; work is enqueued on `stream` and is asynchronous
 *     except where a `_host` out-parameter is documented to synchronise.
 *   - Feature slabs are row-major fp32 [rows][channels], channels contiguous.
 *   - Coordinates on device are int32 [n][4] = (x, y, z, batch); hash keys pack 16 bits per field.
 *   - Rule tables are int32 [n_off][n_out]: table[o][r] = input row feeding output row r through
 *     kernel offset o, or -1.  Compacted rules are two int32 arrays (in_rows, out_rows), offset-major,
 *     output row ascending inside an offset (the canonical order), with an int64
 *     prefix[n_off+1].
 */
#ifndef SCN_MI355X_H
#define SCN_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCN_OK 0
#define SCN_EINVAL 1      /* bad argument (null pointer, negative size, unsupported shape) */
#define SCN_ESIZE 2       /* size-constraint violation, e.g. (out-1)*stride+filter != in */
#define SCN_EHASH 3       /* hash table too small / coordinate outside the 16-bit key range */
#define SCN_EHIP 4        /* a HIP runtime call failed; see scn_last_error_string() */

/* History of the ABI (scn_abi_version() returns the value the library was BUILT with: a caller compares it with the
 * SCN_ABI_VERSION of the header it was compiled against):
 *   1  rounds 1-2: 78 entry points
 *   2  round 3: + 23 entry points (step executor: scn_exec_op / scn_exec_level structs, scn_exec_run*; deferred
 *      weight-gradient sums; bf16 elementwise forms; segment pooling; scn_tiles_build_x) -- shipped with the value still 1
 *   3  round 4: SCN_PYRAMID_FUSED (scn_pyramid_build_ex flag, larger scn_pyramid_workspace_bytes), hash slot function
 *      changed (tables built by version <= 2 libraries are not probe-compatible; no table outlives a Metadata, so only a
 *      caller that kept raw tables across a library upgrade is affected); + scn_exec_timing_enable / _collect, scn_pad_params_many, scn_conv_tiles_split_count, scn_dedup_launch_div, scn_child_table_div (107 entry points);
 *      scn_pool_fwd / _bwd (+ _bf16): `average` carries the pool volume above bit 8 (0 = the 2^3 of every configuration) */
/*   4  round 5: + scn_debug_set / scn_debug_get (developer switches no longer follow the ambient environment per launch);
 *      scn_exec_timing_collect forgets only the records it returned; + scn_nms_bits / scn_nms_scratch_bytes, scn_dilate_gather_fwd / _bwd,
 *      scn_parent_lookup_div, scn_topk_boxes / scn_topk_scratch_bytes, scn_cell_map (117 entry points) */
/*   5  round 6: + scn_conv_tiles_chain / scn_conv_tiles_chain_counts, scn_wgrad_tiles32 / _scratch_bytes (121 entry points); scn_tiles_build_x: bits 8-10 of `with_x`
 *      = log2 of the row bins in the sort key of a 27-offset table (0: as before); scn_pyramid_build_ex with
 *      SCN_PYRAMID_XCD_ORDER sorts level 0 by (row bin, mask); switches SCN_TS_PROG, SCN_TS_NO_CHAIN, SCN_TB_NO_BINS;
 *      additive within 5: + scn_adam_many / scn_adam_launches / scn_adam_segment_bytes, struct scn_adam_segment (124 entry
 *      points);
 *      additive within 5: + scn_rpn_targets, scn_rpn_sample_workspace_bytes / scn_rpn_sample_batchwise,
 *      scn_rpn_loss_scratch_bytes / scn_rpn_loss, scn_rpn_loss_scale (130 entry points);
 *      additive within 5: + scn_mask_overlap_draw, scn_mask_loss_scratch_bytes / scn_mask_loss, scn_mask_loss_bwd,
 *      scn_mask_pack (135 entry points);
 *      additive within 5: + scn_xent_scratch_bytes / scn_xent_fwd, scn_xent_bwd, scn_softmax_argmax (139 entry points);
 *      additive within 5: + scn_eval_mask_bits, scn_eval_pack_threshold, scn_eval_mask_iou, scn_eval_bbox_iou, scn_eval_match,
 *      scn_eval_confusion (145 entry points);
 *      additive within 5: + scn_sample_stats, scn_sample_pack (147 entry points);
 *      additive within 5: + scn_wgrad_step_begin / _hold / _flush / _discard, scn_wgrad_group_counts; switch
 *      SCN_EXEC_GROUP_STEP (152 entry points);
 *      additive within 5: + scn_roialign_fwd / _bwd, scn_dense_maxpool_fwd / _bwd (156 entry points);
 *      additive within 5: + scn_anchor_up_fwd / _bwd (158 entry points);
 *      additive within 5: + scn_philox_words_host, scn_philox_fill, scn_sample_pack_drawn, scn_sample_cut_start (162 entry
 *      points);
 *      additive within 5: + scn_roialign_fwd_bf16 / _bwd_bf16, scn_dense_maxpool_fwd_bf16 / _bwd_bf16 (166 entry points);
 *      additive within 5: + scn_relu_fwd_bf16 / _bwd_bf16 (168 entry points);
 *      additive within 5: + scn_wgrad_plan_describe (169 entry points);
 *      additive within 5: + scn_roialign_pool_fwd / _bwd, their _bf16 forms, scn_box_flatten_fwd / _bwd (175 entry points);
 *      additive within 5: + scn_loss_combine / scn_loss_combine_bwd (177 entry points);
 *      additive within 5: + scn_conv_tiles_plan_describe (178 entry points);
 *      additive within 5: + the executor op SCN_OP_ADD_RELU, no new entry point (178 entry points);
 *      additive within 5: + the executor ops SCN_OP_BN_STATS / _BN_FWD / _BN_BWD and the op flag SCN_XF_BN_TRAINING;
 *                           SCN_OP_WGRAD_SUBM with b < 0 is scn_wgrad_rules(_bf16); no new entry point (178 entry points);
 *      additive within 5: + scn_conv_tiles_bf16_plan_describe (179 entry points);
 *      additive within 5: + the switches SCN_WGRAD_STEP_OVERLAP and SCN_EXEC_HOLD_LEAVES, no new entry point (179 entry
 *      points);
 *      additive within 5: + the executor ops SCN_OP_GRAD_NORM / SCN_OP_GRAD_SCALE (global-norm gradient clipping), no new entry
 *                           point (179 entry points) */
#define SCN_ABI_VERSION 5

/* flags for the gather-GEMM entry points */
#define SCN_F_RELU_IN 1      /* use max(X,0) as the input slab (fuses scn.ReLU before a conv, module_factory.py:88,173-176) */
#define SCN_F_W_TRANSPOSED 2 /* use W[o]^T: W is [n_off][cout][cin] seen from this call (backward-data) */
#define SCN_F_OFF_REVERSE 4  /* weight index n_off-1-o for table row o (SubM backward-data: R_o^T = R_{k^3-1-o}) */
#define SCN_F_RESIDUAL_LAST 8 /* scn_conv_tiles: add `residual` AFTER the ReLU-backward mask (gradient of a residual block:
                                dX = mask(conv^T dY1) + dY), default is before */
#define SCN_F_SPLIT_SUM 16    /* scn_conv_tiles: launch the tile kernel only; the caller runs scn_conv_tiles_finish next
                               * (lets a profiler bracket the two kernels separately; results are identical) */
#define SCN_F_TILE_ORDER_X 64 /* scn_conv_tiles_bf16: `tile_order` was built by scn_tiles_build_x(with_x): hand the tiles out by
                               * spatial bin, bin x to the workgroups of XCD x (same results, L2-local row gathers) */
#define SCN_F_GEMM_V1 32      /* scn_gemm_table / scn_gemm_rules: run the register-only kernels (operands straight from
                               * global memory) where the LDS-tiled ones would be taken; same bits -- the tests' cross-check */

typedef void* scn_stream_t;

int scn_abi_version(void);
const char* scn_last_error_string(void);

/* Developer switches (round 5; no reference counterpart -- A/B and cross-check knobs of this library's own kernel variants,
 * e.g. SCN_TS_NO_TAIL, SCN_TB_STREAM, SCN_PYRAMID_V1: the list is scn_debug.hip's table).  The environment is read ONCE, at
 * the first use of any switch; afterwards a switch changes only through scn_debug_set (value NULL: unset).  The product path
 * never scans the environment per launch (rounds 1-4: ~300 getenv calls per step).  Unknown name: SCN_EINVAL. */
int scn_debug_set(const char* name, const char* value);
int scn_debug_get(const char* name, int* is_set, int64_t* value);

/* ------------------------------------------------------------------------------------------
 * Index path: scn.Metadata / InputLayer rules / rulebooks
 * ---------------------------------------------------------------------------------------- */

/* Power-of-two slot count the hash tables for n keys must have. */
int64_t scn_hash_capacity(int64_t n);

/* int64 [n][4] coords (x,y,z,batch) as the reference hands them over (ndsis/data/data.py:95-98, consumed at
 * custom_operations.py:72-80) -> int32 [n][4].  *bad_host receives the number of rows with a field outside
 * [0,65535] (synchronises stream); such input is rejected with SCN_EHASH.  bad_host == NULL: asynchronous form --
 * nothing is copied back and the stream is not synchronised; *scratch1 (device) holds the count once the stream gets
 * there and the caller checks it behind its own event. */
int scn_coords_to_i32(const int64_t* coords, int64_t n, int32_t* out, int32_t* scratch1, int64_t* bad_host,
                      scn_stream_t stream);

/* Scratch bytes scn_dedup_build needs for n items. */
int64_t scn_dedup_scratch_bytes(int64_t n);

/* Row numbering by first occurrence (InputLayer rules: custom_operations.py:72-80 with mode 0-4;
 * strided-conv output sites: module_factory.py:232-234).  Key of item i = (batch, x>>shift, y>>shift, z>>shift).
 *   table_keys[cap], table_rows[cap]  hash of the distinct keys -> row id (kept by the caller as the grid of
 *                                     this spatial size; used later by scn_subm_table)
 *   item_row[n]      row id of every item        (InputLayer: point -> voxel row;  Convolution: fine row -> coarse row)
 *   row_count[n]     multiplicity of each row, first *n_rows_host entries valid (may be NULL)
 *   row_first[n]     smallest item index of each row (may be NULL)
 *   row_coords[n][4] coordinates (shifted) of each row
 *   n_rows_host      number of distinct rows (synchronises stream once) */
int scn_dedup_build(const int32_t* coords, int64_t n, int shift, uint64_t* table_keys, int32_t* table_rows,
                    int64_t cap, int32_t* item_row, int32_t* row_count, int32_t* row_first, int32_t* row_coords,
                    void* scratch, int64_t* n_rows_host, scn_stream_t stream);

/* scn_dedup_build without the host synchronisation: the row count goes to n_rows_dev (device int64[1]) in stream
 * order; the caller copies it back behind its own event and may queue work that does not need it meanwhile. */
int scn_dedup_launch(const int32_t* coords, int64_t n, int shift, uint64_t* table_keys, int32_t* table_rows,
                    int64_t cap, int32_t* item_row, int32_t* row_count, int32_t* row_first, int32_t* row_coords,
                    void* scratch, int64_t* n_rows_dev, scn_stream_t stream);

/* Submanifold neighbour table for filter k (odd; reference uses 1 and 3: module_factory.py:383-385,404-406):
 * table[o][r] = row of coords[r] + delta_o or -1, o = ((dx+h)k + (dy+h))k + (dz+h). */
int scn_subm_table(const int32_t* coords, int64_t n, const uint64_t* table_keys, const int32_t* table_rows,
                   int64_t cap, int k, int32_t* table, scn_stream_t stream);

/* Children table of a size=stride=2 Convolution (module_factory.py:232-234): child[o][c] = fine row with parent c
 * and offset o = ((x&1)*2 + (y&1))*2 + (z&1), or -1.  Also writes fine_off[n_fine] = that offset. */
int scn_child_table(const int32_t* fine_coords, const int32_t* parent, int64_t n_fine, int64_t n_coarse,
                    int32_t* child, int32_t* fine_off, scn_stream_t stream);
/* The same two steps for ANY filter_size = filter_stride = (sx, sy, sz) -- `get_downsampler(stride=...)` /
 * `get_upsampler` hand an int or one entry per axis to scn.Convolution / scn.Deconvolution (module_factory.py:221-258; every
 * shipped configuration uses 2): coarse site = (x / sx, y / sy, z / sz), numbered by first occurrence like scn_dedup_launch;
 * child table [sx sy sz][n_coarse] with offset o = ((x % sx) sy + y % sy) sz + z % sz, which is the 2^3 numbering for 2. */
int scn_dedup_launch_div(const int32_t* coords, int64_t n, int sx, int sy, int sz, uint64_t* table_keys, int32_t* table_rows,
                         int64_t cap, int32_t* item_row, int32_t* row_count, int32_t* row_first, int32_t* row_coords,
                         void* scratch, int64_t* n_rows_dev, scn_stream_t stream);
int scn_child_table_div(const int32_t* fine_coords, const int32_t* parent, int64_t n_fine, int64_t n_coarse, int sx, int sy,
                        int sz, int32_t* child, int32_t* fine_off, scn_stream_t stream);
/* The first of the two steps when the coarse grid ALREADY EXISTS on the Metadata (SparseConvNet keys its grids by spatial size:
 * 64 -> 16 by one stride-4 layer after 64 -> 32 -> 16 by two stride-2 layers lands in the same grid): parent[i] = the existing
 * grid's row of (x / sx, y / sy, z / sz), -1 where that site is not in the grid; *n_missing_dev = how many were not (the
 * caller refuses those: upstream would grow the grid under the tensors that live on it).  scn_child_table_div then builds
 * the child table against that numbering (n_coarse may exceed n_fine there). */
int scn_parent_lookup_div(const int32_t* fine_coords, int64_t n_fine, int sx, int sy, int sz, const uint64_t* table_keys,
                          const int32_t* table_rows, int64_t cap, int32_t* parent, int64_t* n_missing_dev, scn_stream_t stream);

/* Compaction of a rule table into (in,out) pairs -- wave ballot + prefix sum.
 * Phase 1: counts; block_sums must hold scn_rules_blocks(n_off, n_out) int32; writes prefix (device, int64[n_off+1])
 * and copies it to prefix_host (synchronises stream once).  prefix_host == NULL: asynchronous form -- no copy, no
 * synchronisation; the caller reads `prefix` back when it needs the sizes (the forward pass never does: only
 * scn_wgrad_rules / scn_gemm_rules take compacted rules). */
int64_t scn_rules_blocks(int n_off, int64_t n_out);
int scn_rules_scan(const int32_t* table, int n_off, int64_t n_out, int32_t* block_sums, int64_t* prefix,
                   int64_t* prefix_host, scn_stream_t stream);
/* Phase 2: in_rows/out_rows (and seg_of = offset index of each pair, may be NULL) of prefix_host[n_off] entries. */
int scn_rules_fill(const int32_t* table, int n_off, int64_t n_out, const int32_t* block_sums, int32_t* in_rows,
                   int32_t* out_rows, int32_t* seg_of, scn_stream_t stream);

/* All index structures of one forward pass of an n_levels U-Net in one call (what the reference's scn.Metadata builds
 * lazily on the host while InputLayer / SubmanifoldConvolution / Convolution run: custom_operations.py:67-86,
 * module_factory.py:232-234,404-406): InputLayer rules, and per level the SubM-k^3 table + rule scan + tiles and the
 * size=stride=2 coarse sites + child table + rule scan + tiles.  Same kernels, same order and bit-identical results as
 * the step-by-step entry points above; buffers are carved out of `workspace` (256-byte aligned, at least
 * scn_pyramid_workspace_bytes(n_points, n_levels, k) bytes), whose layout comes back in `desc` (HOST int64
 * [SCN_PYRAMID_DESC_LEN], offsets in bytes):
 *   desc[0] n_levels  [1] n_points  [2] bytes used  [3] out-of-range coordinate count
 *   desc[4] item_row int32[n_points]  [5] row_count int32 (first n_0 valid)  [6] row_first int32  [7] int32 coords [n_points][4]
 *   level l at L = desc + 8 + l*SCN_PYRAMID_LEVEL_STRIDE:
 *     L[0] rows n_l  [1] hash capacity  [2] coords int32[n][4]  [3] hash keys u64[cap]  [4] hash rows int32[cap]
 *     L[5] table int32[k^3][n]  [6] scan block sums int32[L[7]]  [8] prefix int64[k^3+1] (device)
 *     L[9] perm  [10] tstab  [11] tile_mask  [12] tile_order  [13] number of tiles
 *     strided rulebook l -> l+1:  L[14] parent int32[n_l]  [15] fine_off int32[n_l]  [16] child int32[8][n_{l+1}]
 *     L[17] block sums int32[L[18]]  [19] prefix int64[9] (device)  L[20..23] perm, tstab, tile_mask, tile_order  [24] tiles
 *     L[25..25+k^3] SubM rule prefix (host copy)   L[53..61] strided rule prefix (host copy)
 *     L[64] / L[65] compacted SubM rules in_rows / out_rows int32[prefix[k^3]]   L[66] / L[67] the strided ones
 * The call synchronises `stream` (row counts of the levels, rule-list sizes) and holds no interpreter state: a helper
 * thread may run it for the next batch while the caller queues the current one. */
#define SCN_PYRAMID_MAX_LEVELS 8
#define SCN_PYRAMID_LEVEL_STRIDE 72
#define SCN_PYRAMID_DESC_LEN (8 + SCN_PYRAMID_MAX_LEVELS * SCN_PYRAMID_LEVEL_STRIDE)
int64_t scn_pyramid_workspace_bytes(int64_t n_points, int n_levels, int k);
int scn_pyramid_build(const int64_t* coords, int64_t n_points, int n_levels, int k, void* workspace,
                      int64_t workspace_bytes, int64_t* desc, scn_stream_t stream);
/* The same build with options.  SCN_PYRAMID_TWO_QUEUES: the SubM work of every level (neighbour table, rule scan, mask sort,
 * tiles) goes to a library-owned side stream beside the chain that numbers the levels on `stream`; `stream` is ordered behind
 * the side stream before the call returns.  Shorter when the build has the GPU to itself (0.95 vs 1.18 ms at 150 k points,
 * four levels), slightly in the way when it runs next to another batch's matrix kernels -- so the inline callers (a forward
 * that builds its own index structures, the ROI batch) ask for it and the pipelined prefetch does not.  Same structures. */
#define SCN_PYRAMID_TWO_QUEUES 1
#define SCN_PYRAMID_XCD_ORDER 2   /* the SubM tiles of every level also get the XCD-local hand-out order (scn_tiles_build_x) */
/* SCN_PYRAMID_FUSED (round 4, k = 3): the same structures, bit for bit, from a build that never waits for the device before
 * its end: level sizes stay in device memory (every index kernel reads its row count from the word the numbering kernel
 * wrote; grids and buffer offsets by the upper bound n_l <= n_points), the levels run side by side inside each launch,
 * flag / scan / fill of the numbering is one look-back pass, and ONE device -> host copy brings back every size
 * (14 + n_levels - 1 launches and one host wait; the builder above: ~136 launches, one wait per level + one).  Only the
 * hash tables differ (every level gets the capacity of n_points).  Overrides SCN_PYRAMID_TWO_QUEUES. */
#define SCN_PYRAMID_FUSED 4
int scn_pyramid_build_ex(const int64_t* coords, int64_t n_points, int n_levels, int k, void* workspace,
                         int64_t workspace_bytes, int64_t* desc, int flags, scn_stream_t stream);

/* Sparse ROI crop (roi_select_sparse.py:157-180 get_inside_indicator / select_features / select_coords / roi_cut) as
 * count -> scan -> scatter; no [boxes][points] object is ever built.  boxes int32 [bb][8] =
 * (start x,y,z,sample ; stop x,y,z,sample+1), half-open.  The result is the reference's selection order: box-major,
 * ascending point row.
 *   scn_roi_units(n)        number of 256-point units of n points
 *   scn_roi_count           unit_offsets int32 [bb * scn_roi_units(n) + bb]: after the call, for every (box, unit) the
 *                           start of its run relative to the box's first output row (+ bb box totals behind them);
 *                           prefix (device int64 [bb+1]): first output row of every box, prefix[bb] = M.
 *                           prefix_host != NULL: copied back (synchronises stream once); NULL: asynchronous.
 *   scn_roi_fill            src_row[M] (point row), box_of[M], out_coords int64 [M][4] = (x,y,z of the point, box) --
 *                           select_coords' extended coordinates (may be NULL).
 *   scn_roi_inside          the dense bool matrix roi_cut also returns (:180), rebuilt from the list ON REQUEST:
 *                           inside_u8 [bb][n] zero-filled, then 1 at (box_of[m], src_row[m]). */
int64_t scn_roi_units(int64_t n);
int scn_roi_count(const int32_t* coords, int64_t n, const int32_t* boxes, int bb, int32_t* unit_offsets, int64_t* prefix,
                  int64_t* prefix_host, scn_stream_t stream);
int scn_roi_fill(const int32_t* coords, int64_t n, const int32_t* boxes, int bb, const int32_t* unit_offsets,
                 const int64_t* prefix, int32_t* src_row, int32_t* box_of, int64_t* out_coords, scn_stream_t stream);
int scn_roi_inside(const int32_t* src_row, const int32_t* box_of, int64_t m, int64_t n, int bb, uint8_t* inside_u8,
                   scn_stream_t stream);
/* out_coords[m] = (x,y,z of coords[src_row[m]], box_of[m]) as int64 rows (select_coords, roi_select_sparse.py:136-149) */
int scn_roi_coords(const int32_t* coords, const int32_t* src_row, const int32_t* box_of, int64_t m, int64_t* out_coords,
                   scn_stream_t stream);
/* BBoxTransformerSlice (roi_select_bbox_transform.py:56-70,87-97): boxes fp32 [bb][2][3] -> optional Divider
 * (box / resize, fp32, per axis; :15-21) -> floor(start), ceil(stop) (ndsis/utils/bbox.py:87-106) -> optional clip of
 * start to [0,S-1] / stop to [1,S] (bbox.py:62-84) -> sample interval appended -> int32 [bb][8] as scn_roi_count expects.
 * resize3_or_null: device float[3]. */
int scn_roi_boxes(const float* boxes, const int32_t* box_sample, int bb, const int32_t* spatial_size3_or_null,
                  const float* resize3_or_null, int32_t* out, scn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Feature path: gather-GEMM-scatter on fp32 MFMA
 * ---------------------------------------------------------------------------------------- */

/* Output-stationary gather GEMM:   Y[r] = residual[r] + bias + sum_o  in(X[table[o][r]]) . W[o']
 * (SubmanifoldConvolution fwd, module_factory.py:404-406; Convolution fwd via the child table, :232-234;
 *  NetworkInNetwork fwd with table == NULL (identity, n_off = 1), :366-367; and the backward-data of
 *  SubM / Deconvolution / NiN with SCN_F_W_TRANSPOSED).
 * W is [n_off][cin][cout] row-major as stored by the layer; with SCN_F_W_TRANSPOSED the call sees it as
 * [n_off][cout_of_call][cin_of_call]^T, i.e. pass the layer's weight unchanged and swap cin/cout.
 * bias, residual may be NULL.  relu_mask (may be NULL, [n_out][cout]): elements of Y are zeroed where relu_mask <= 0
 * (fuses the ReLU backward that follows a backward-data GEMM). */
int scn_gemm_table(const float* X, int64_t n_in, int cin, const int32_t* table, int n_off, int64_t n_out,
                   const float* W, const float* bias, const float* residual, const float* relu_mask, float* Y,
                   int cout, int flags, scn_stream_t stream);

/* Mask-sorted row tiles of a rule table (input of scn_conv_tiles).  Rows are regrouped by their offset mask
 * (bit o set <=> table[o][r] >= 0) with a stable radix sort; nt = ceil(n/16) tiles of 16 sorted rows.
 *   perm      int32 [nt*16]          sorted position -> original row (-1 padding)
 *   tstab     int32 [nt][n_off][16]  tstab[t][o][i] = table[o][perm[16t+i]]
 *   tile_mask uint32 [nt]            OR of the row masks of the tile
 *   tile_order int32 [nt]            tile ids by offset count descending (hand-out order of scn_conv_tiles) */
int64_t scn_tiles_scratch_bytes(int n_off, int64_t n);
int scn_tiles_build(const int32_t* table, int n_off, int64_t n, int32_t* perm, int32_t* tstab, uint32_t* tile_mask,
                    int32_t* tile_order, void* scratch, scn_stream_t stream);
/* The same build with a second hand-out order behind the first (with_x != 0): tile_order then holds scn_tiles_order_ints(n, 1)
 * = 2 NT + 16 ints -- [NT] tile ids by offset count descending (as above), [NT] tile ids by (spatial bin, offset count
 * descending) where the bin of a tile is (its first row * 8 / n) (rows are numbered in the order the points arrive, so a row
 * range is a region of the scene), [9] bin starts in that second list (bin_start[8] = NT).  scn_conv_tiles_bf16 with
 * SCN_F_TILE_ORDER_X hands the tiles of bin x to the workgroups of XCD x: their row gathers then meet in one L2 (the bf16 tile
 * kernel waits for L2 misses at the fine levels: 87 -> 71 us per launch at 600 k voxels, 24.5 -> 21.5 at 150 k; the fp32
 * kernel is bound by its matrix pipe and loses to the shorter per-bin lists, so it keeps the first order).
 * Round 6 (ABI 5): `with_x` bit 0 = the second order; bits 8-10 = lb, log2 of the ROW BINS in the sort key of a 27-offset table
 * (0 = the plain mask sort; lb <= 5): rows are sorted by (row * 2^lb / n, offset mask), so a tile's 16 rows come from one
 * region of the scene -- what the bf16 builds use at level 0 with lb = 3 (600 k voxels: 71 -> 53 us per launch; results are
 * independent of the row order inside the tile tables).  scn_tiles_order_ints takes bit 0 only. */
int64_t scn_tiles_order_ints(int64_t n, int with_x);
int scn_tiles_build_x(const int32_t* table, int n_off, int64_t n, int32_t* perm, int32_t* tstab, uint32_t* tile_mask,
                      int32_t* tile_order, int with_x, void* scratch, scn_stream_t stream);

/* Stable LSD radix sort of (uint32 key, int32 value) pairs on the low `bits` key bits -- the primitive behind
 * scn_tiles_build (rows by offset mask, tiles by offset count); exported so that it can be checked on its own.  It takes
 * the place of the hash-map iteration order upstream leaves undefined (canonical orders are sorted orders).
 * vals == NULL: values are the input positions.  Outputs must not alias the inputs.  ceil(bits/9) passes of <= 512 bins;
 * n <= 4096 runs as one launch out of LDS. */
int64_t scn_sort_pairs_scratch_bytes(int64_t n);
int scn_sort_pairs(const uint32_t* keys, const int32_t* vals, int64_t n, int bits, uint32_t* keys_out,
                   int32_t* vals_out, void* scratch, scn_stream_t stream);

/* THE HOT KERNEL.  Output-stationary convolution over mask-sorted tiles, accumulators in registers, weights in LDS:
 *     Y[r] = residual[r] + bias + sum_o in(X[table[o][r]]) . W[o']          (same result as scn_gemm_table)
 * Serves SubmanifoldConvolution fwd / backward-data (module_factory.py:404-406), Convolution fwd (:232-234) and
 * Deconvolution backward-data (:256-258).  n_off <= 27.  Per-row accumulation order is fixed (offsets ascending). */
int64_t scn_conv_tiles_scratch_bytes(int cin, int64_t n_out, int cout);   /* K-chunk slabs */
/* Layers with more than 32 input channels split K over workgroups.  `arrival` (int32, at least
 * scn_conv_tiles_arrival_counters(cin, n_out, cout) entries; may be shared by every call on one stream) lets the kernel add
 * the K-chunk partial sums itself: the wave that arrives last at a (tile, column chunk) adds them in ascending K-chunk
 * order.  CONTRACT: all entries are ZERO when the call is made; the kernel leaves them zero.  arrival == NULL (or
 * SCN_F_SPLIT_SUM): the partial sums are added by a second launch instead -- same association, same bits. */
int64_t scn_conv_tiles_arrival_counters(int cin, int64_t n_out, int cout);
int scn_conv_tiles(const float* X, int64_t n_in, int cin, const int32_t* tstab, const uint32_t* tile_mask, const int32_t* perm,
                   const int32_t* tile_order, int n_off, int64_t n_out, const float* W, const float* bias, const float* residual,
                   const float* relu_mask, float* Y, int cout, int flags, void* scratch, int32_t* arrival,
                   scn_stream_t stream);
/* CHAINED launch (round 6): 2-4 DEPENDENT convolutions over the same tiles -- the SubM 3^3 launches of a level's residual
 * units (module_factory.py:127-183 builds x + SubM3(ReLU(SubM3(ReLU(x)))); two units per level, :513-530), forward or
 * backward-data -- as ONE launch.  Role r reads what role r-1 wrote (X, residual or relu_mask of role r may be Y of an
 * earlier role); the workgroups of role r are placed on the CUs role r-1 leaves, stage their weights there and wait for
 * role r-1 to complete before their first row gather (scn_conv_ts.hip, "CHAIN").  Same arithmetic per role as n_roles
 * scn_conv_tiles calls: same bits.  Shapes the chained kernel does not cover (channel counts that are no multiple of 32,
 * levels on the four-waves-per-tile loop, SCN_TS_NO_CHAIN=1) run as n_roles plain calls.  All roles share n_in, cin, the
 * tile structures, n_out, cout, SCN_F_W_TRANSPOSED and SCN_F_OFF_REVERSE; `flags` may differ in the other bits. */
typedef struct scn_conv_role {
    const void* X; const void* W; const void* bias; const void* residual; const void* relu_mask; void* Y;
    int32_t flags; int32_t reserved;
} scn_conv_role;
int scn_conv_tiles_chain(int n_roles, const scn_conv_role* roles, int64_t n_in, int cin, const int32_t* tstab,
                         const uint32_t* tile_mask, const int32_t* perm, const int32_t* tile_order, int n_off, int64_t n_out,
                         int cout, void* scratch, int32_t* arrival, scn_stream_t stream);
/* out[0] = chained launches, out[1] = roles they carried, since the last reset (fp32 and bf16 together). */
void scn_conv_tiles_chain_counts(int64_t out[2], int reset);
/* Which kernel variant the scn_conv_tiles calls of this process took since the last reset: out[0] = launches on the fast path
 * (raw-buffer gathers: 16-byte rows, < 2^23 rows, < 4 GB slabs), out[1] = launches that fell back to the general kernel
 * (same results, 64-bit addressing), out[2] = launches with the in-launch K reduction, out[3] = launches that left the K
 * reduction to a second launch.  reset != 0 zeroes the counters after reading.  (bench.py reports it as `fast_path`: a
 * workload that outgrows the fast path's limits changes kernels, and the JSON line says so.) */
void scn_conv_tiles_path_counts(int64_t out[4], int reset);
/* Launches (a subset of out[0]) that took the four-waves-per-tile loop of latency-bound levels: fewer (tile, slice) pairs
 * than half the chip's waves -- the coarse levels of the reference's six-level plan (scannet_config/run.py:539-549: 2 983 /
 * 734 / 180 rows), deep levels of an ROI batch.  Same arithmetic per product, an element's sum associated by wave share. */
int64_t scn_conv_tiles_split_count(int reset);
/* Which path a scn_conv_tiles call takes (host only: launches nothing, allocates nothing; tests and tools).  The launcher
 * takes every decision from the function that fills this report, under the developer switches set at the time of the call.
 *   with_arrival: the call passes an `arrival` array.
 *   xw_ptr_bits: bits 0-3 = the low 4 bits of X | W; bits 4-7 = the low 4 bits of W alone (a subset of bits 0-3: the
 *   weight staging of a column-contiguous W depends on W's alignment only, the row gathers on both).
 *   epilogue_ptr_bits: the low 4 bits of Y | bias | residual | relu_mask | scratch.
 *   out[0]  stream: 1 = the call runs on the opt-in weight-streaming kernel (SCN_TS_STREAM=1, scn_conv_tss.hip); the other
 *           fields then describe the k_conv_ts launch the call would make without the switch
 *   out[1]  FULLK (raw-buffer fast path; 0: the general kernel)  out[2] WT (SCN_F_W_TRANSPOSED)
 *   out[3]  VECN (16-byte weight staging along Cout)  out[4] PART (Cin no multiple of 32)
 *   out[5]  TAIL (dead halves skipped, slices weighted)  out[6] a K-chunk tail of <= 16 channels exists  out[7] a column tail
 *   out[8]  FUSED (in-launch K reduction)  out[9] the four-waves-per-tile loop  out[10] PROG: offsets staged before the barrier
 *   out[11] K-chunks  out[12] column chunks
 *   out[13] the largest number of workgroups a (column chunk, K-chunk) slice gets  out[14] workgroups of the launch
 *   out[15] 1: the K-chunk sum of the call (its second launch, or scn_conv_tiles_finish) moves 16 bytes per thread, 0: 4
 * n_out == 0 (the launcher returns without a launch): all zero.  SCN_EINVAL for arguments the launcher rejects and for
 * pointer bits that are not 4-byte aligned. */
int scn_conv_tiles_plan_describe(int64_t n_in, int cin, int n_off, int64_t n_out, int cout, int flags, int with_arrival,
                                 int xw_ptr_bits, int epilogue_ptr_bits, int64_t out[16]);
/* Second half of a scn_conv_tiles call made with SCN_F_SPLIT_SUM: adds the K-chunk slabs (no-op when cin <= 32: the
 * tile kernel has written Y).  Same arguments as that call. */
int scn_conv_tiles_finish(int cin, int64_t n_out, const float* bias, const float* residual, const float* relu_mask,
                          float* Y, int cout, int flags, void* scratch, scn_stream_t stream);

/* The same convolution for bf16 STORAGE (BASELINE configs 3-5): X, residual, relu_mask and Y are bf16
 * (uint16 bit patterns, row-major; cin % 8 == 0 and cin >= 8: 16-byte row pieces of X; ANY cout); products accumulate in fp32 on
 * v_mfma_f32_16x16x32_bf16 and the result is rounded to bf16 once.  Same tiles, flags and per-row summation order as
 * scn_conv_tiles.  The layer's master weights stay fp32: scn_conv_tiles_bf16_pack rounds them (round-to-nearest-even)
 * into `image` (scn_conv_tiles_bf16_image_bytes bytes, 16-byte aligned), laid out as the kernel's workgroups stage it;
 * SCN_F_W_TRANSPOSED / SCN_F_OFF_REVERSE are properties of the IMAGE (pass them to the pack; the convolution ignores
 * them), so one layer has a forward image and a backward-data image.  An image is valid until the weights change.
 * `arrival`: zeroed counters for the in-launch K reduction, contract as in scn_conv_tiles
 * (scn_conv_tiles_bf16_arrival_counters entries); NULL, or SCN_F_SPLIT_SUM: second launch inside the same call (there is
 * no _finish for bf16).  X and image are 16-byte aligned (SCN_EINVAL otherwise).  Y, residual and relu_mask need only their
 * 2-byte element alignment: the tile kernels' VECTOR epilogue (a lane's NB = 2 or 4 consecutive columns of a row as one 4- or
 * 8-byte access) needs cout % NB == 0 and Y / residual / relu_mask on a 2 NB-byte boundary; otherwise every element is its
 * own 2-byte access -- same results.  bias and scratch need 4 bytes; with an `arrival` array the scratch is 16-byte aligned
 * (the in-launch K reduction stores 16-byte pieces to it).
 * Serves SubmanifoldConvolution / Convolution forward and SubM / Deconvolution backward-data
 * (module_factory.py:232-234,256-258,404-406). */
int64_t scn_conv_tiles_bf16_image_bytes(int cin, int cout, int n_off);
int scn_conv_tiles_bf16_pack(const float* W, int cin, int cout, int n_off, int flags, uint16_t* image, scn_stream_t stream);
/* The same for n images in one launch (all arrays on the HOST; W / image entries are device pointers): a network packs the
 * forward and backward-data images of all its convolutions once per step. */
int scn_conv_tiles_bf16_pack_many(int n, const float* const* W_host, const int32_t* cin_host, const int32_t* cout_host,
                                  const int32_t* n_off_host, const int32_t* flags_host, uint16_t* const* image_host,
                                  scn_stream_t stream);
int64_t scn_conv_tiles_bf16_scratch_bytes(int cin, int64_t n_out, int cout);
int64_t scn_conv_tiles_bf16_arrival_counters(int cin, int64_t n_out, int cout);
int scn_conv_tiles_bf16(const uint16_t* X, int64_t n_in, int cin, const int32_t* tstab, const uint32_t* tile_mask,
                        const int32_t* perm, const int32_t* tile_order, int n_off, int64_t n_out, const uint16_t* image,
                        const float* bias, const uint16_t* residual, const uint16_t* relu_mask, uint16_t* Y, int cout,
                        int flags, void* scratch, int32_t* arrival, scn_stream_t stream);
/* Which path a scn_conv_tiles_bf16 call takes (host only: launches nothing, allocates nothing; tests and tools).  The launcher
 * takes every decision from the function that fills this report, under the developer switches set at the time of the call.
 *   with_arrival: the call passes an `arrival` array.
 *   y_ptr_bits: the low 4 bits of Y | residual | relu_mask;  scratch_ptr_bits: the low 4 bits of scratch | bias.
 *   out[0]  stream: 1 = the offset-outer weight-streaming kernel k_conv_tbs<KS, n_off, NW> takes the call; then
 *   out[1]  KS (K-chunks of 32 a wave contracts per offset)  out[2] NW (waves = tiles per workgroup batch)
 *   out[3]  n_wgb: workgroups per column chunk (a workgroup walks every n_wgb-th batch of NW tiles); 0 without stream
 *   out[4]  NB (16-column blocks per workgroup: 2 or 4)  out[5] KH (32-channel planes per K-chunk: 1 or 2)
 *   out[6]  FUSED (in-launch K reduction)  out[7] PART (Cin no multiple of the K-chunk)       -- k_conv_tb<NB, KH, FUSED, PART>
 *   out[8]  K-chunks  out[9] column chunks
 *   out[10] workgroups per (column chunk, K-chunk) slice of k_conv_tb (0 with stream)  out[11] workgroups of the tile launch
 *   out[12] xbins: groups of XCDs of the XCD-local hand-out (SCN_F_TILE_ORDER_X), 1 = the plain order (0 with stream)
 *   out[13] 1: the tile kernel's epilogue is the vector form, 0: element by element
 *   out[14] 1: the call makes a K-chunk sum launch (k_conv_tb_sum)  out[15] its elements per thread (4 or 1; 0: no sum launch)
 *   out[16] tiles  out[17] dynamic LDS bytes of the tile launch
 * n_out == 0 (the launcher returns without a launch): all zero.  SCN_EINVAL for arguments the launcher rejects (cin % 8,
 * cin < 8, n_off outside 1..27, the row limits) and for pointer bits below the element size (2 bytes for y_ptr_bits, 4 for
 * scratch_ptr_bits). */
int scn_conv_tiles_bf16_plan_describe(int64_t n_in, int cin, int n_off, int64_t n_out, int cout, int flags, int with_arrival,
                                      int y_ptr_bits, int scratch_ptr_bits, int64_t out[18]);

/* Rule-list gather GEMM with row scatter:  Y[out_rows[p]] = bias + in(X[in_rows[p]]) . W[o(p)]
 * where every output row occurs in exactly one pair (Deconvolution fwd, module_factory.py:256-258; backward-data
 * of Convolution).  prefix_host = int64[n_off+1] on the HOST. */
int scn_gemm_rules(const float* X, int cin, const int32_t* in_rows, const int32_t* out_rows,
                   const int64_t* prefix_host, int n_off, const float* W, const float* bias, const float* relu_mask,
                   float* Y, int cout, int flags, scn_stream_t stream);

/* Weight gradient:  dW[o] = sum_{p in R_o} in(X[in_rows[p]])^T . dY[out_rows[p]]     (dW fully overwritten)
 * in_rows == out_rows == NULL means the identity rule list of length prefix_host[1] (NetworkInNetwork).
 * One kernel streams the rules (MFMA operands straight from the gathered rows, no LDS staging) into per-unit partial
 * blocks, a second adds them in a fixed order: bitwise reproducible.  scratch: scn_wgrad_scratch_bytes(...) bytes. */
int64_t scn_wgrad_scratch_bytes(int cin, int cout, const int64_t* prefix_host, int n_off);
int scn_wgrad_rules(const float* X, int cin, const float* dY, int cout, const int32_t* in_rows,
                    const int32_t* out_rows, const int64_t* prefix_host, int n_off, float* dW, void* scratch,
                    int flags, scn_stream_t stream);

/* Weight AND bias gradient in one pass: as scn_wgrad_rules, plus db[c] = sum over the rules of the offsets named in
 * the bit mask db_offsets of dY[out_p][c].  The caller names offsets whose rule lists together contain every output row
 * exactly once (centre offset of a submanifold conv: 1 << (k^3/2); all offsets of a Deconvolution; the identity list),
 * so db equals the column sum of dY.  Any channel count (rows that are not 16-byte aligned take element-wise loads). */
/* Row GEMM over the parts of a JoinTable, A tile staged through LDS (scn_gemm_lt.hip):
 *     [Y0 | Y1][r] = residual[r] + bias + in([X0[r] | X1[r]]) . W        for r < n
 * Two sources (cx1 > 0): NetworkInNetwork(2C -> C) applied to JoinTable([up, skip]) without the concatenated slab
 * (module_factory.py:298-301, 365-367); W is the layer's [cx0 + cx1][cy0] weight.  Two destinations (cy1 > 0) with
 * SCN_F_W_TRANSPOSED: its backward-data, dUp = dY . W[:c0]^T and dSkip = dY . W[c0:]^T from one read of dY; W is the layer's
 * weight unchanged ([cy0 + cy1][cx0] seen from this call).  cx1 == cy1 == 0: the identity-table scn_gemm_table.
 * Channel counts of the sources are multiples of 8, slabs 16-byte aligned; residual / relu_mask only with one destination.
 * bf16_storage != 0: features, residual, relu_mask and outputs are uint16 bf16 bit patterns (W, bias fp32; exact widening,
 * fp32 arithmetic, one rounding of the result). */
int scn_gemm_rows2(const void* X0, int cx0, const void* X1, int cx1, int64_t n, const float* W, const float* bias,
                   const void* residual, const void* relu_mask, void* Y0, int cy0, void* Y1, int cy1, int flags,
                   int bf16_storage, scn_stream_t stream);

/* bf16-storage forms of scn_gemm_table / scn_gemm_rules (features, residual, relu_mask and Y are uint16 bf16 bit
 * patterns; W and bias fp32; rows are widened exactly and the arithmetic is the fp32 kernels'; one rounding of Y). */
int scn_gemm_table_bf16(const uint16_t* X, int64_t n_in, int cin, const int32_t* table, int n_off, int64_t n_out,
                        const float* W, const float* bias, const uint16_t* residual, const uint16_t* relu_mask,
                        uint16_t* Y, int cout, int flags, scn_stream_t stream);
int scn_gemm_rules_bf16(const uint16_t* X, int cin, const int32_t* in_rows, const int32_t* out_rows,
                        const int64_t* prefix_host, int n_off, const float* W, const float* bias,
                        const uint16_t* relu_mask, uint16_t* Y, int cout, int flags, scn_stream_t stream);

/* The same weight gradient for bf16-stored operands (X, dY: uint16 bit patterns; dW fp32): rows are gathered packed
 * and widened to fp32 in registers (exact), arithmetic and summation order are those of scn_wgrad_rules.  Scratch:
 * scn_wgrad_scratch_bytes. */
int scn_wgrad_rules_bf16(const uint16_t* X, int cin, const uint16_t* dY, int cout, const int32_t* in_rows,
                         const int32_t* out_rows, const int64_t* prefix_host, int n_off, float* dW, void* scratch,
                         int flags, scn_stream_t stream);
/* scn_wgrad_bias_rules for bf16-stored operands (dW, db fp32). */
int scn_wgrad_bias_rules_bf16(const uint16_t* X, int cin, const uint16_t* dY, int cout, const int32_t* in_rows,
                              const int32_t* out_rows, const int64_t* prefix_host, int n_off, float* dW, float* db,
                              uint32_t db_offsets, void* scratch, int flags, scn_stream_t stream);
int scn_wgrad_bias_rules(const float* X, int cin, const float* dY, int cout, const int32_t* in_rows,
                         const int32_t* out_rows, const int64_t* prefix_host, int n_off, float* dW, float* db,
                         uint32_t db_offsets, void* scratch, int flags, scn_stream_t stream);

/* The two weight (and bias) gradients of a pre-activation residual unit (module_factory.py:127-183: x + SubM3(ReLU(SubM3(
 * ReLU(x))))) in ONE launch and one sum: both convolutions walk the same rule list with the same channel counts;
 * (X0, dY0) and (X1, dY1) are their operand pairs (fp32).  dW = [2][n_off][cin][cout]; db = [2][cout], or NULL with
 * db_offsets == 0.  Per problem the units, the per-unit arithmetic and the fixed-order sum are those of
 * scn_wgrad_bias_rules under this call's plan; the launch pays its tail and its fixed costs once for twice the work.
 * Scratch: scn_wgrad_scratch_bytes2.  prefix_host[0] must be 0; n_off <= 32. */
/* Deferred unit sums (round 3d).  Between scn_wgrad_defer_begin() and scn_wgrad_defer_flush(stream) ON THE CALLING THREAD the
 * scn_wgrad_* calls launch their unit kernels only and record their sum; the flush adds the recorded sums in batched launches
 * (up to six launches' sums per launch; per layer the arithmetic and its order are unchanged -- same bits).  Every call made
 * in between needs a scratch region of its own that stays untouched until the flush.  Used by scn_exec_run for the weight
 * gradients of a network level (27 sum launches of ~7 us per backbone step become 8). */
int scn_wgrad_defer_begin(void);
int scn_wgrad_defer_flush(scn_stream_t stream);
/* Step scope of the weight gradients (call site: executor.step_weight_gradients, the context SceneStep.forward_backward puts
 * around its backward).  Nothing reads a parameter gradient before the optimizer step, so the weight-gradient launches of
 * ALL backward passes of a step can run after the last pass: one k_wgrad_group grid per kernel variant (~15 rounds of
 * units instead of 3-4 per pass: the ragged end of a grid is paid once) and one launch for all the unit sums.
 *   scn_wgrad_step_begin()      opens the scope on the calling thread; an open scope is restarted and what it recorded is
 *                               dropped (as scn_wgrad_defer_begin after a failed pass).  Holding is off.
 *   scn_wgrad_step_hold(on)     on != 0: from now on a scn_wgrad_defer_flush on this thread launches nothing and hands the
 *                               pass's recorded unit launches and sums to the scope; 0: passes flush as without a scope.
 *                               Returns 1 when holding is in effect, else 0 (no scope open, or the developer switch
 *                               SCN_EXEC_GROUP_STEP=0).  The caller sets it around the passes whose weight gradients it can
 *                               deliver late.
 *   scn_wgrad_step_flush(s)     closes the scope and launches what it holds on stream s: per job the plan, the units, the
 *                               slabs, the instantiation and the fixed-order sum of the standalone launch -- same bits.
 *   scn_wgrad_step_discard()    closes the scope and drops what it holds (a failed step).
 * Until the flush has been queued the caller keeps everything the held launches read or write untouched: the operand slabs,
 * the rule lists, the gradient buffers and a scratch region of its OWN per pass.  The job tables of a flush (any number of
 * jobs; the argument form of a pass's flush carries six) go through a per-device ring of pinned host slots, each guarded by an
 * event, and one hipMemcpyAsync on s: these few buffers are the one thing the library allocates itself.
 * The end of a step in stream order: a flush that holds both grid variants forks -- the table copy runs ahead on a
 * non-blocking side stream the library owns (one per device, created at the first such flush), then k_wgrad_group<4>, the jobs
 * that launch on their own and the held column sums run there behind an event of s, k_wgrad_group<2> runs on s, and s waits
 * for the side stream before the sum launch; HIP events only, no kernel waits for another.  With one variant nothing forks;
 * the developer switch SCN_WGRAD_STEP_OVERLAP=0 keeps everything on s.  Same arguments per job either way: same bits.
 * Held column sums: inside a pass that scn_exec_run runs under a scope that holds, an SCN_OP_COLSUM (fp32) after which the
 * pass has only weight gradients is recorded like them and launched by the flush -- it leaves the backward-data chain; its
 * partial sums stay in the shared region of the pass's own scratch.  SCN_EXEC_HOLD_LEAVES=0: in place. */
int scn_wgrad_step_begin(void);
int scn_wgrad_step_hold(int on);
int scn_wgrad_step_flush(scn_stream_t stream);
int scn_wgrad_step_discard(void);
/* Launch counts since the last reset (process-wide; tests and profiles): out[0] k_wgrad_group<4> launches, out[1]
 * k_wgrad_group<2> launches, out[2] weight-gradient unit launches on their own (k_wgrad_direct, k_wgrad_tb), out[3] unit-sum
 * launches (k_wgradd_sum*).  reset != 0: zero them after reading.  out may be NULL. */
void scn_wgrad_group_counts(int64_t out[4], int reset);
int64_t scn_wgrad_scratch_bytes2(int cin, int cout, const int64_t* prefix_host, int n_off);
int scn_wgrad_bias_rules2(const float* X0, const float* dY0, const float* X1, const float* dY1, int cin, int cout,
                          const int32_t* in_rows, const int32_t* out_rows, const int64_t* prefix_host, int n_off,
                          float* dW, float* db, uint32_t db_offsets, void* scratch, int flags, scn_stream_t stream);

/* The general form: n_prob = 2 ... 4 operand pairs (host arrays of device pointers) on one rule list -- the four
 * convolutions of two stacked residual units (module_factory.py:513-530 `num_units=2`) in one launch.
 * dW = [n_prob][n_off][cin][cout], db = [n_prob][cout] or NULL with db_offsets == 0. */
int64_t scn_wgrad_scratch_bytes_n(int cin, int cout, const int64_t* prefix_host, int n_off, int n_prob);
/* Which path a weight-gradient call takes (host only: launches nothing, allocates nothing; tests and tools).  The launcher
 * and the scratch sizes above take every decision from the function that fills this report.
 *   n_prob 1: the single-problem entry points; 2 ... 4: the _rules2 / _rules_n forms.  bf16_storage: the _bf16 forms.
 *   operand_ptr_bits: the low 4 bits of the OR of every operand pointer (X, dY of all problems); out_ptr_bits: of dW | scratch.
 *   out[0]  kernel: 0 k_wgrad_direct (fp32 MFMA), 1 k_wgrad_tb (bf16 MFMA)
 *   out[1], out[2]  16-channel tiles of a wave along Cin / Cout (TA, TB)
 *   out[3] QUAD  out[4] EDGE  out[5] EDGE with vector row pieces  out[6] bf16 rows on the fp32-MFMA kernel (HB)
 *   out[7]  rules per unit  out[8] units  out[9], out[10] workgroup blocks along Cin / Cout
 *   out[11], out[12]  unit sum: channels per thread (4 or 1), threads per element
 *   out[13]  scratch bytes the call writes without db, out[14] with db (both <= the scn_wgrad_scratch_bytes* of the call)
 *   out[15]  1: no rules at all -- dW and db are cleared by memsets, no kernel runs
 * SCN_EINVAL for arguments the launcher rejects (operand pointers not aligned to their element type among them). */
int scn_wgrad_plan_describe(int cin, int cout, const int64_t* prefix_host, int n_off, int n_prob, int bf16_storage,
                            int operand_ptr_bits, int out_ptr_bits, int64_t out[16]);
int scn_wgrad_bias_rules_n(const float* const* Xs, const float* const* dYs, int n_prob, int cin, int cout,
                          const int32_t* in_rows, const int32_t* out_rows, const int64_t* prefix_host, int n_off,
                          float* dW, float* db, uint32_t db_offsets, void* scratch, int flags, scn_stream_t stream);
int scn_wgrad_bias_rules_n_bf16(const uint16_t* const* Xs, const uint16_t* const* dYs, int n_prob, int cin, int cout,
                               const int32_t* in_rows, const int32_t* out_rows, const int64_t* prefix_host, int n_off,
                               float* dW, float* db, uint32_t db_offsets, void* scratch, int flags, scn_stream_t stream);
/* ... for bf16-stored operand pairs (uint16 bit patterns; dW, db fp32; the bf16-MFMA kernel where it applies). */
int scn_wgrad_bias_rules2_bf16(const uint16_t* X0, const uint16_t* dY0, const uint16_t* X1, const uint16_t* dY1, int cin,
                               int cout, const int32_t* in_rows, const int32_t* out_rows, const int64_t* prefix_host,
                               int n_off, float* dW, float* db, uint32_t db_offsets, void* scratch, int flags,
                               scn_stream_t stream);

/* db[c] = sum_r dY[r][c]   (bias gradient of every conv-type layer).  scratch: SCN_COLSUM_BLOCKS*c floats. */
#define SCN_COLSUM_BLOCKS 512
int scn_colsum(const float* dY, int64_t n, int c, float* db, void* scratch, scn_stream_t stream);
int scn_colsum_bf16(const uint16_t* dY, int64_t n, int c, float* db, void* scratch, scn_stream_t stream);   /* bf16-stored dY */

/* ------------------------------------------------------------------------------------------
 * Elementwise / normalisation / IO
 * ---------------------------------------------------------------------------------------- */

/* scn.ReLU (module_factory.py:88) and scn.AddTable (:52-54,308) */
int scn_relu_fwd(const float* X, int64_t count, float* Y, scn_stream_t stream);
int scn_relu_bwd(const float* X, const float* dY, int64_t count, float* dX, scn_stream_t stream);
int scn_add(const float* A, const float* B, int64_t count, float* Y, scn_stream_t stream);

/* scn.BatchNormReLU / BatchNormLeakyReLU (module_factory.py:92-102): training statistics over all rows. */
int64_t scn_bn_scratch_bytes(int c);
int scn_bn_stats(const float* X, int64_t n, int c, float* mean, float* var_biased,
                 void* scratch /* scn_bn_scratch_bytes(c) */, scn_stream_t stream);
int scn_bn_fwd(const float* X, int64_t n, int c, const float* mean, const float* var, float eps, const float* gamma,
               const float* beta, float leak, float* Y, scn_stream_t stream);
/* dX, dgamma, dbeta for y = lrelu((x-mean)*invstd*gamma+beta); training=1 propagates through the batch statistics */
int scn_bn_bwd(const float* X, const float* dY, int64_t n, int c, const float* mean, const float* var, float eps,
               const float* gamma, const float* beta, float leak, int training, float* dX, float* dgamma, float* dbeta,
               void* scratch /* scn_bn_scratch_bytes(c) */, scn_stream_t stream);

/* The same layer with batch statistics over ALL ranks of a data-parallel step (the reference's BatchNorm sees its whole
 * batch as one feature matrix, module_factory.py:92-102; one scene per GPU splits that matrix): the reductions are
 * exposed as float64 [2][c] sums so that the caller can all-reduce them between the two halves.
 *   forward : scn_bn_sums -> (sum x, sum x^2) -> all-reduce with the row counts -> mean, var -> scn_bn_fwd
 *   backward: scn_bn_bwd_reduce -> local dgamma, dbeta and (sum g, sum g x^) -> all-reduce -> scn_bn_bwd_apply with
 *             n_stat = rows of all ranks. */
int scn_bn_sums(const float* X, int64_t n, int c, double* sums, void* scratch, scn_stream_t stream);
int scn_bn_bwd_reduce(const float* X, const float* dY, int64_t n, int c, const float* mean, const float* var, float eps,
                      const float* gamma, const float* beta, float leak, float* dgamma, float* dbeta, double* sums,
                      void* scratch, scn_stream_t stream);
int scn_bn_bwd_apply(const float* X, const float* dY, int64_t n, int c, const float* mean, const float* var, float eps,
                     const float* gamma, const float* beta, float leak, const double* sums, int64_t n_stat, float* dX,
                     scn_stream_t stream);

/* InputLayerFunction (custom_operations.py:72-80): mode 0 copy, 1 last, 2 first, 3 sum, 4 mean.
 * acc64: scratch of n_rows*c doubles (modes 3,4).  row_last (mode 1): scratch of n_rows int32. */
int scn_input_fwd(const float* feats, const int32_t* item_row, const int32_t* row_count, const int32_t* row_first,
                  int64_t n_items, int64_t n_rows, int c, int mode, float* Y, double* acc64, int32_t* row_last,
                  scn_stream_t stream);
int scn_input_bwd(const float* dY, const int32_t* item_row, const int32_t* row_count, const int32_t* row_first,
                  const int32_t* row_last, int64_t n_items, int c, int mode, float* dfeats, scn_stream_t stream);
/* OutputLayerFunction (custom_operations.py:7-10): Y[i] = X[item_row[i]]; backward = segment sum. */
int scn_gather_rows(const float* X, const int32_t* rows, int64_t m, int c, float* Y, scn_stream_t stream);
int scn_segment_sum(const float* dY, const int32_t* item_row, int64_t n_items, int64_t n_rows, int c, float* dX,
                    double* acc64, scn_stream_t stream);

/* Per-sample pooling of a slab -- the reference's SparseGlobalPool / split_batch (ndsis/modules/custom_operations.py:24-59;
 * sparse class network model.py:507-512, module_factory.py:655-657).  The sample of row r is coords[r][3] (the grid's int32
 * [n][4] rows, x y z b).  op: 0 mean (torch.mean, the reference's default), 1 sum, 2 max (torch.amax).
 *   fwd: Y[b][:] over the rows of sample b; a sample without rows pools to zeros (custom_operations.py:53-54).
 *        cnt[b] = rows of sample b; *unsorted != 0 iff some row has a smaller sample index than the row before it.
 *   bwd: mean dX[r] = dY[b] / cnt[b]; sum dX[r] = dY[b]; max: dY[b][c] split evenly among the rows that hold the maximum.
 * scratch: scn_segment_pool_scratch_bytes(n_samples, c) (fp64 accumulators / tie counts).  No host synchronisation.
 * scn_sample_counts: cnt and *unsorted alone (split_batch: rows grouped by sample are returned as row ranges). */
int64_t scn_segment_pool_scratch_bytes(int n_samples, int c);
int scn_sample_counts(const int32_t* coords, int64_t n, int n_samples, int32_t* cnt, int32_t* unsorted, scn_stream_t stream);
int scn_segment_pool_fwd(const float* X, const int32_t* coords, int64_t n, int c, int n_samples, int op, float* Y,
                         int32_t* cnt, int32_t* unsorted, void* scratch, scn_stream_t stream);
int scn_segment_pool_bwd(const float* X, const float* Y, const float* dY, const int32_t* coords, int64_t n, int c,
                         int n_samples, int op, const int32_t* cnt, float* dX, void* scratch, scn_stream_t stream);

/* scn.SparseToDense (module_factory.py:429-435): out [B][C][X][Y][Z] pre-zeroed by the caller. */
int scn_sparse_to_dense_fwd(const float* X, const int32_t* coords, int64_t n, int c, const int64_t* size3_host,
                            float* out, scn_stream_t stream);
int scn_sparse_to_dense_bwd(const float* dOut, const int32_t* coords, int64_t n, int c, const int64_t* size3_host,
                            float* dX, scn_stream_t stream);

/* scn.MaxPooling / scn.AveragePooling with pool_size = pool_stride = 2 (module_factory.py:315-354), on the child /
 * parent tables of the strided rulebook.  max: Y[c] = max(0, existing children); avg: Y[c] = sum(existing children) / 8. */
int scn_pool_fwd(const float* X, const int32_t* child, int64_t n_coarse, int c, int average, float* Y,
                 scn_stream_t stream);
int scn_pool_bwd(const float* X, const float* Y, const float* dY, const int32_t* parent, int64_t n_fine, int c,
                 int average, float* dX, scn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mask-head epilogue on the device: consumers of the ROI selection in CSR form
 * (rows of the crop are box-major; box_of[r] = box, src_point[r] = point row in the batch).
 * ---------------------------------------------------------------------------------------- */

/* SparseMaskPredictor.forward (model.py:859-882): out (pre-zeroed, the per-sample dense [boxes][points] masks back to
 * back) gets sigmoid(scores[r][class_of_box[box]]) at row_base[box] + src_point[r]; classes < 0, >= num_valid
 * (num_valid > 0) or >= k leave zeros.  row_base[box] = offset of the box's row in out - first point row of its sample. */
int scn_mask_scatter(const float* scores, int64_t m, int k, const int32_t* src_point, const int32_t* box_of,
                     const int64_t* class_of_box, int num_valid, const int64_t* row_base, float* out,
                     scn_stream_t stream);

/* SparseMaskLossSelector gathers (model.py:1157-1227): pred[r] = scores[r][label_of_box[box]],
 * gt[r] = gt_flat[gt_base[box] + src_point[r]] (gt_base[box] = offset of the associated ground-truth mask row in
 * gt_flat - first point row of the sample; < 0 or label < 0: box not kept, rows get 0 and keep_row[r] = 0).
 * keep_row may be NULL.  _bwd: dscores[r][c] = dpred[r] at c = label of a kept box, 0 elsewhere. */
int scn_mask_gather(const float* scores, int64_t m, int k, const int32_t* src_point, const int32_t* box_of,
                    const int64_t* label_of_box, const int64_t* gt_base, const float* gt_flat, float* pred, float* gt,
                    uint8_t* keep_row, scn_stream_t stream);
int scn_mask_gather_bwd(const float* dpred, int64_t m, int k, const int32_t* box_of, const int64_t* label_of_box,
                        const int64_t* gt_base, float* dscores, scn_stream_t stream);

/* Greedy non-maximum suppression of score-sorted 3-D boxes (ndsis/utils/bbox.py:713-759 non_maximum_supression as
 * called by ProposalSelector, proposal_selector.py:60-89): boxes fp32 [batch][n][2][3] = (start xyz, stop xyz), sorted
 * by descending score inside a scene; keep[batch][n] = 1 for boxes that survive.  A box is suppressed by an earlier
 * surviving box whose IoU with it is > overlap_threshold (fp32, the reference's operation order: bit-exact decisions).
 * n <= 8192.  One workgroup per scene, one launch instead of n. */
int scn_nms(const float* boxes, int batch, int n, float overlap_threshold, uint8_t* keep, scn_stream_t stream);
/* The same selection, round 5: the upper triangle of the n x n suppression relation as a bit matrix (one wave per 64 x 64 block,
 * spread over the chip) and ONE serial walk over its rows out of LDS -- keep[] equals scn_nms's bit for bit; 1024 boxes:
 * 12 + 42 us (rocprofv3, one scene) instead of 600 (scn_nms walks the boxes with two workgroup barriers each).  n <= 4096.
 * scratch: scn_nms_scratch_bytes(batch, n) = batch * n * ceil(n / 64) * 8 bytes, need not be initialised. */
int64_t scn_nms_scratch_bytes(int batch, int n);
int scn_nms_bits(const float* boxes, int batch, int n, float overlap_threshold, uint8_t* keep, void* scratch,
                 scn_stream_t stream);

/* Exact top-k of a score field with the boxes gathered along -- what ProposalSelector runs before its NMS
 * (ndsis/modules/proposal_selector.py:60-75: torch.topk(rpn_score, num_keep_pre_nms, sorted) and rpn_bbox[batch, indices]).
 * scores fp32 [batch][n], boxes fp32 [batch][n][6] or NULL; out_scores [batch][k] descending, out_index int64 [batch][k],
 * out_boxes [batch][k][6].  Equal scores come out by ascending index (torch.topk leaves their order open); NaN counts as
 * the largest value, as in torch.  Radix select (two 11-bit histogram passes over an order-preserving key, one compaction,
 * one LDS sort of the candidates): 4 launches instead of torch.topk's 19 on a [1, 524 288] field.  k <= 2048, k <= n.
 * scratch: scn_topk_scratch_bytes(batch) bytes that are ZERO before the first call; every call leaves them zero again
 * (after a failed call: zero them).  One stream at a time per scratch. */
int64_t scn_topk_scratch_bytes(int batch);
int scn_topk_boxes(const float* scores, const float* boxes, int batch, int64_t n, int k, float* out_scores,
                   int64_t* out_index, float* out_boxes, void* scratch, scn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Voxelisation front-end: the deterministic core of augment_coords
 * (ndsis/data/sparse_augmentation.py:81-126) and the batch column of collate_fn (data.py:95-98).
 * The reference's random draws (distortion matrix, sub-pixel offset, cut-out start) are inputs.
 * ---------------------------------------------------------------------------------------- */

/* aug[n][3] = points[n][3] @ rot_and_scale (3x3 row-major, HOST), each element as fma(z, R2j, fma(y, R1j, x*R0j)) -- the
 * association of torch's CPU matmul for K = 3, so the truncation below sees the reference's fp32 values;
 * shift_max[0..2] = -min(aug) + offset (complete_shift, sparse_augmentation.py:95-99), shift_max[3..5] = max(aug).
 * No host synchronisation.  scratch: scn_vox_scratch_bytes(n). */
int64_t scn_vox_scratch_bytes(int64_t n);
int scn_vox_project(const float* points, int64_t n, const float* rot_and_scale_host, const float* offset_host,
                    float* aug, float* shift_max, void* scratch, scn_stream_t stream);

/* discrete[n][3] = trunc(aug + shift)  (`.long()`, :100);  table[i] = i if 0 <= discrete - test_start < size on every axis
 * else -1 (both HOST int32[3]; NULL: no cut-out, every row is kept).  fix_cut_out (:42-47) tests the UNMOVED coordinates
 * (test_start = 0); random_cut_out (:50-78) tests against its start positions.  Feed `table` (one segment) to
 * scn_rules_scan/_fill to obtain the kept rows in ascending order. */
int scn_vox_discretize(const float* aug, int64_t n, const float* shift, const int32_t* test_start_host,
                       const int32_t* size_host, int32_t* discrete, int32_t* table, scn_stream_t stream);

/* out int64 [m][4] = (discrete[rows[j]] - start, batch_index): the rows of one sample of collate_fn's coords_batch. */
int scn_vox_gather(const int32_t* discrete, const int32_t* rows, int64_t m, const int32_t* start_host,
                   int64_t batch_index, int64_t* out, scn_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Channel padding of PARAMETERS, many tensors per launch (scn_elem.hip).  No reference counterpart: the reference's mask
 * network has a 23-channel level (model.py:573-596: 16 U-Net channels ++ 7 raw ones, scannet_config/run.py:741-810); this
 * package runs it on slabs padded to 24 columns and hands its layers zero-padded copies of their logical weights
 * (module_factory.py:383-406 SubmanifoldConvolution, :256-258 Deconvolution, :366-367 NetworkInNetwork keep their logical
 * parameter shapes).  Tensor j is [fv][rows][cols]; desc_host[11 j ..] = fv, src_rows, src_cols, dst_rows, dst_cols, then two
 * row segments (src row, count, dst row): source rows [s, s + count) land on destination rows [d, d + count), every other
 * destination element is zero.  backward = 0: out_host[j] (padded shape) <- in_host[j] (logical shape);
 * backward = 1: out_host[j] (LOGICAL shape) <- the matching elements of in_host[j] (PADDED shape; NULL: zeros).
 * ---------------------------------------------------------------------------------------- */
int scn_pad_params_many(int n, const float* const* in_host, float* const* out_host, const int32_t* desc_host, int backward,
                        scn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * bf16-STORAGE forms of the HBM-bound feature kernels (BASELINE configs 3-5; scn_elem_bf16.hip): slabs are uint16 bf16 bit
 * patterns, values are widened exactly, the arithmetic is that of the fp32 forms above, one round-to-nearest-even per
 * result.  scn.OutputLayer / the ROI feature gather (custom_operations.py:7-10; roi_select_sparse.py:125-133),
 * scn.MaxPooling / AveragePooling (module_factory.py:315-354), scn.SparseToDense (:429-435), scn.AddTable (:308), and
 * the storage casts on either side of a bf16-stored stretch of a network.
 * ---------------------------------------------------------------------------------------- */
int scn_cast_f32_to_bf16(const float* X, int64_t count, uint16_t* Y, scn_stream_t stream);
int scn_cast_bf16_to_f32(const uint16_t* X, int64_t count, float* Y, scn_stream_t stream);
int scn_add_bf16(const uint16_t* A, const uint16_t* B, int64_t count, uint16_t* Y, scn_stream_t stream);
/* scn.ReLU on a bf16-stored slab (module_factory.py:581-611: the dilation stack's last ReLU).  Y[i] is the bf16 whose widening is
 * scn_relu_fwd's result on the widened X[i] (exact: the result is X[i] or a zero); dX[i] = dY[i] bit for bit where the widened
 * X[i] > 0, else +0 -- scn_relu_bwd's test.  count == 0: SCN_OK, no pointer is read. */
int scn_relu_fwd_bf16(const uint16_t* X, int64_t count, uint16_t* Y, scn_stream_t stream);
int scn_relu_bwd_bf16(const uint16_t* X, const uint16_t* dY, int64_t count, uint16_t* dX, scn_stream_t stream);
int scn_gather_rows_bf16(const uint16_t* X, const int32_t* rows, int64_t m, int c, uint16_t* Y, scn_stream_t stream);
int scn_segment_sum_bf16(const uint16_t* dY, const int32_t* item_row, int64_t n_items, int64_t n_rows, int c, uint16_t* dX,
                         double* acc64, scn_stream_t stream);
int scn_pool_fwd_bf16(const uint16_t* X, const int32_t* child, int64_t n_coarse, int c, int average, uint16_t* Y,
                      scn_stream_t stream);
int scn_pool_bwd_bf16(const uint16_t* X, const uint16_t* Y, const uint16_t* dY, const int32_t* parent, int64_t n_fine, int c,
                      int average, uint16_t* dX, scn_stream_t stream);
int scn_sparse_to_dense_fwd_bf16(const uint16_t* X, const int32_t* coords, int64_t n, int c, const int64_t* size3_host,
                                 uint16_t* out, scn_stream_t stream);
int scn_sparse_to_dense_bwd_bf16(const uint16_t* dOut, const int32_t* coords, int64_t n, int c, const int64_t* size3_host,
                                 uint16_t* dX, scn_stream_t stream);

/* Dilation gather (round 5; the first dense same-convolution behind scn.SparseToDense, module_factory.py:581-611 + :396-414: a
 * 3^3 conv3d with padding 1 on a volume whose only non-zero cells are the n active sites of a sparse level).  With
 * P[r][o][:] = X[r] . W[o] from ONE row GEMM over the active rows ([n][27][c]; o = (a*3+b)*3+c' over the kernel taps),
 *   fwd: out[cell][:] = bias + sum_o P[map[cell + (a-1, b-1, c'-1)]][o][:]   (ascending o; map: cell -> active row or -1, [B X Y Z])
 *   bwd: dP[r][o][:]  = dOut[cell(r) - (a-1, b-1, c'-1)][:] or 0 outside the volume   (cell_of_row: int64 [n])
 * out / dOut are the channels-last volume [B X Y Z][c]; bf16 != 0: P, out, dOut, dP are bf16 (fp32 accumulation).  bias may be
 * NULL.  The bias gradient is the column sum of dOut (scn_colsum*). */
int scn_dilate_gather_fwd(const void* P, const int32_t* map, int batch, const int64_t* size3_host, int c, int bf16,
                          const float* bias, void* out, scn_stream_t stream);
int scn_dilate_gather_bwd(const void* dOut, const int64_t* cell_of_row, int64_t n, const int64_t* size3_host, int c, int bf16,
                          void* dP, scn_stream_t stream);
/* The two index vectors of the above from a level's int32 coordinates (x, y, z, sample) [n][4]: cell_of_row[r] =
 * ((sample X + x) Y + y) Z + z and map[cell] = r, -1 on empty cells (map: int32 [batch X Y Z], need not be initialised).
 * *n_outside_dev = rows outside the volume (the caller checks it when it next waits for the device; such rows get cell 0
 * and no map entry). */
int scn_cell_map(const int32_t* coords, int64_t n, int batch, const int64_t* size3_host, int64_t* cell_of_row, int32_t* map,
                 int32_t* n_outside_dev, scn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Step executor (scn_exec.hip): ONE call walks the launch plan of a whole network pass.
 *
 * The reference drives the scn surface layer by layer from Python (module_factory.py builds nested scn.Sequential trees;
 * model.py:414-431 runs them); at ~330 launches per backbone step (~760 with the mask branch) the interpreter, not the
 * GPU, bounds the bf16 steps.  A plan is a flat list of ops over three tables the caller fills per step -- feature slabs
 * (`bufs`), parameters / weight images (`params`) and parameter gradients (`grads`) -- and a table of per-level index
 * structures.  Each op is exactly one of the entry points above with exactly the arguments the layer-by-layer path would
 * pass (same kernels, same bits); the executor adds no arithmetic of its own.
 * ---------------------------------------------------------------------------------------- */
enum {
    SCN_OP_GEMM_IDENT = 1,   /* scn_gemm_table(_bf16), identity table: SubM 1^3 / NetworkInNetwork / Linear; fwd or bwd-data  */
    SCN_OP_CONV_SUBM = 2,    /* scn_conv_tiles(_bf16) over the level's 3^3 tiles (fwd; bwd-data with SCN_F_W_TRANSPOSED|OFF_REVERSE) */
    SCN_OP_CONV_CHILD = 3,   /* scn_conv_tiles(_bf16) over the level's child tiles: Convolution fwd / Deconvolution bwd-data */
    SCN_OP_RULES_CHILD = 4,  /* scn_gemm_rules(_bf16) coarse -> fine: Deconvolution fwd / Convolution bwd-data              */
    SCN_OP_ROWS2 = 5,        /* scn_gemm_rows2: NiN over two joined parts (fwd), or its two-destination bwd-data             */
    SCN_OP_WGRAD_SUBM = 6,   /* scn_wgrad_bias_rules(_bf16) on the level's 3^3 rules; b < 0 (no bias): scn_wgrad_rules(_bf16)    */
    SCN_OP_WGRAD2_SUBM = 7,  /* scn_wgrad_bias_rules2(_bf16): both convolutions of a residual unit                             */
    SCN_OP_WGRAD_DOWN = 8,   /* Convolution: scn_wgrad_rules(_bf16) on the child rules (X fine, dY coarse)                     */
    SCN_OP_WGRAD_UP = 9,     /* Deconvolution: scn_wgrad_bias_rules(_bf16), roles swapped (X coarse, dY fine), db over all 8  */
    SCN_OP_WGRAD_IDENT = 10, /* identity list: NiN / SubM 1^3 / Linear; aux = element offset into grads[w] (joined parts)     */
    SCN_OP_COLSUM = 11,      /* scn_colsum(_bf16): bias gradient alone                                                        */
    SCN_OP_ADD = 12,         /* y = x + x1 (scn_add / scn_add_bf16): the two gradient paths of a skip connection             */
    SCN_OP_CAST = 13,        /* storage cast: SCN_XF_BF16 set = fp32 -> bf16, else bf16 -> fp32                               */
    SCN_OP_RELU = 14,        /* y = max(x, 0) (scn_relu_fwd / _bf16), y may be x: the closing ReLU of a main-path residual unit */
    SCN_OP_RELU_BWD = 15,    /* y = x1 where m > 0, else 0 (scn_relu_bwd / _bf16): m = the slab the ReLU read OR wrote         */
    SCN_OP_ADD_RELU = 16,    /* y = x + max(x1, 0) over rows * cin elements in ONE pass, x1 left as it is, y may be x: the end of a
                              * post-activation residual unit (module_factory.py:163-171, relu_first=False).  The only op that is not
                              * an entry point of its own; scn_relu_fwd's expression, scn_add's operand order and (bf16) one
                              * rounding: bit-equal to SCN_OP_RELU (x1 -> r) followed by SCN_OP_ADD (x, r -> y)                    */
    /* BatchNorm(Leaky)ReLU over the fp32 slab x ([rows][cin]); none of them takes SCN_XF_BF16.  w = params[] id of gamma, beta =
     * params[w + 1].  mean | var: the 2 * cin floats of bufs[x1] (batch statistics), or with x1 < 0 the layer's running buffers
     * params[w + 2], params[w + 3].  aux / c1 = the bits of eps / leakiness as fp32.  Scratch: scn_bn_scratch_bytes(cin) of the
     * pass's shared region (scn_exec_requirements counts it). */
    SCN_OP_BN_STATS = 17,    /* scn_bn_stats: x -> bufs[y] = mean[cin] | biased var[cin]                                       */
    SCN_OP_BN_FWD = 18,      /* scn_bn_fwd: x -> y                                                                             */
    SCN_OP_BN_BWD = 19,      /* scn_bn_bwd: x, m = dY -> y = dX, grads[b] = dgamma[cin] | dbeta[cin]; SCN_XF_BN_TRAINING: the
                              * statistics were the batch's (the gradient passes through them), else constants                 */
    /* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2; scn_clip.hip) over a list of fp32 segments out of
     * the grads[] table; neither op is an entry point of its own or takes SCN_XF_BF16.  T = levels[level].n segments; segment i is
     * grads[w + i] with prefix_host[i + 1] - prefix_host[i] elements (prefix_host: the level's host int64 pointer, here [T + 1]; one
     * flat buffer is T = 1); empty segments are skipped, segments must not overlap.  Checked before anything is launched
     * (SCN_EINVAL, the message names the op): a negative count, a NULL pointer with a positive count, a pointer that is not 4-byte
     * aligned, a record buffer id that is negative or names no buffer.  The table travels in the kernel arguments, at most 80
     * segments per launch; 16-byte accesses after a scalar head of at most 3 elements. */
    SCN_OP_GRAD_NORM = 20,   /* bufs[y] = 4 floats {total_norm, clip_coef, nonfinite, 0}.  S = the sum of squares of every element,
                              * accumulated in double in a fixed order (one partial sum per 4096-element chunk in the pass's shared
                              * scratch -- 8 bytes per chunk, scn_exec_requirements counts them -- then one launch of one workgroup
                              * adds them; no atomics).  total_norm = (float)(sqrt(S) * |gs|), gs = the fp32 whose bits are c1 (the
                              * scale the update applies to the gradient); clip_coef in fp32 as torch computes it: c = max_norm /
                              * (total_norm + 1e-6f), c > 1 ? 1 : c (a NaN stays), max_norm = the fp32 whose bits are aux (+inf:
                              * the coefficient is 1); nonfinite = 1 when S is not finite, else 0                              */
    SCN_OP_GRAD_SCALE = 21   /* every element of every segment: g = g * ((float*)bufs[x1])[1], in place, one fp32 multiply; a
                              * workgroup that reads the coefficient 1.0f returns without touching the gradient (same bits)     */
};
#define SCN_XF_BF16 (1 << 16)        /* op flag: the op's feature slabs are bf16-stored                                      */
#define SCN_XF_BN_TRAINING (1 << 18) /* op flag (BN_BWD; BN_FWD carries it too): batch statistics, see SCN_OP_BN_BWD                    */
#define SCN_XF_COARSE_ROWS (1 << 17) /* op flag (GEMM_IDENT / WGRAD_IDENT / COLSUM / ADD / CAST / RELU / RELU_BWD): rows = n_coarse of `level` */

typedef struct scn_exec_level {
    int64_t n;                       /* rows of this level */
    const int32_t* tstab;            /* SubM 3^3 tiles of this level (scn_tiles_build) */
    const uint32_t* tile_mask;
    const int32_t* perm;
    const int32_t* tile_order;
    const int32_t* in_rows;          /* SubM 3^3 compacted rules */
    const int32_t* out_rows;
    const int64_t* prefix_host;      /* int64[28] on the host */
    int64_t n_coarse;                /* rows of the next (coarser) level; 0: none */
    const int32_t* c_tstab;          /* child tiles [nt_coarse][8][16] */
    const uint32_t* c_tile_mask;
    const int32_t* c_perm;
    const int32_t* c_tile_order;
    const int32_t* c_in_rows;        /* strided rules: in = fine rows, out = coarse rows */
    const int32_t* c_out_rows;
    const int64_t* c_prefix_host;    /* int64[9] on the host */
    int64_t flags;                   /* SCN_XL_* */
} scn_exec_level;
#define SCN_XL_TILE_ORDER_X 1        /* tile_order continues with the XCD-local order (scn_tiles_build_x): bf16 SubM convolutions use it */

typedef struct scn_exec_op {
    int32_t op;                      /* SCN_OP_* */
    int32_t flags;                   /* SCN_F_* of the underlying call | SCN_XF_* */
    int32_t level;
    int32_t cin, cout;               /* of the CALL (backward-data calls swap the layer's) */
    int32_t x, y;                    /* buffer ids: source slab, destination slab (wgrad ops: X operand, dY operand) */
    int32_t r, m;                    /* residual operand, relu-mask operand; -1: none */
    int32_t x1, y1;                  /* ROWS2: second source / second destination; WGRAD2: second operand pair; ADD: x1; RELU_BWD: x1 = dY;
                                      * BN_FWD / BN_BWD: x1 = the mean | var vector, -1: the running buffers */
    int32_t c1;                      /* ROWS2: channels of the second source (fwd) / second destination (bwd); BN_*: leakiness bits */
    int32_t w, b;                    /* params[] ids (weight or bf16 image, bias) -- wgrad / colsum ops: grads[] ids; -1: none;
                                      * BN_*: w = params[] id of gamma (see SCN_OP_BN_STATS), BN_BWD: b = grads[] id */
    int32_t aux;                     /* WGRAD_IDENT: element offset into grads[w]; WGRAD_*: unused; BN_*: eps bits */
    int32_t reserved;
} scn_exec_op;

/* sizeof(scn_exec_op) (which = 0) / sizeof(scn_exec_level) (which = 1): lets a binding check its struct layout. */
int64_t scn_exec_struct_bytes(int which);
/* Scratch bytes and zeroed arrival counters (the scn_conv_tiles contract) the plan needs for these level sizes. */
int scn_exec_requirements(const scn_exec_op* ops, int n_ops, const scn_exec_level* levels, int n_levels,
                          int64_t* scratch_bytes, int64_t* arrival_counters);
/* Walk the plan on `stream`.  Stops at the first failing op (its status is returned, scn_last_error_string names the op). */
int scn_exec_run(const scn_exec_op* ops, int n_ops, const scn_exec_level* levels, int n_levels, void* const* bufs,
                 const void* const* params, void* const* grads, void* scratch, int64_t scratch_bytes, int32_t* arrival,
                 scn_stream_t stream);
/* The same with the parameter-gradient ops (SCN_OP_WGRAD_* / SCN_OP_COLSUM: leaves of a backward pass) on `side_stream`, each
 * behind an event of `stream`; `stream` is ordered behind the last of them before the call returns.  side_scratch: a
 * second scratch buffer of at least scratch_bytes.  side_stream == NULL: scn_exec_run. */
int scn_exec_run_streams(const scn_exec_op* ops, int n_ops, const scn_exec_level* levels, int n_levels, void* const* bufs,
                         const void* const* params, void* const* grads, void* scratch, int64_t scratch_bytes,
                         int32_t* arrival, scn_stream_t stream, scn_stream_t side_stream, void* side_scratch,
                         int64_t side_scratch_bytes);
/* Launch timing inside a pass (round 4; what bench.py's `roofline` samples): while enabled, every scn_exec_run* call brackets
 * its SCN_OP_CONV_SUBM / SCN_OP_CONV_CHILD ops -- one launch of the dominant tile kernel each -- with HIP timing events on
 * `stream`.  Process-wide (a node's backward pass runs on the autograd thread).  scn_exec_timing_collect waits for the
 * recorded events, writes per record the elapsed milliseconds and info[7] = (op, bf16 storage, cin, cout, rows in, rows out,
 * rules of the table), returns the number of records written (at most cap) and forgets THOSE (round 5: a caller whose buffer
 * is smaller than the backlog calls again for the rest; rounds 3-4 dropped what did not fit).
 * on = 2: EVERY op of a pass is bracketed (weight gradients, row GEMMs, casts: tools/exec_launch_table.py); the deferred unit
 * sums of a pass run behind its last op and belong to no record. */
int scn_exec_timing_enable(int on);
int64_t scn_exec_timing_collect(float* ms, int64_t* info, int64_t cap);

/* Round 6 (experiment, opt-in; nothing in the package calls it): the weight gradient of a SubM 3^3 layer with 32 input and 32
 * output channels in TILE-major form -- one row gather per rule: the dY rows of a mask-sorted tile are loaded once into LDS and
 * serve every offset of the tile, the offsets are dealt to the waves of a workgroup (profiles/r6_wgrad_one_gather.txt).  Serves
 * the same call sites as scn_wgrad_rules (the weight gradient of scn.SubmanifoldConvolution: module_factory.py:396-414).
 * X [n_in][32], dY [n_out][32] fp32; tstab / tile_mask / perm from scn_tiles_build over the layer's 27-offset table;
 * prefix_host[28] = the rule prefix (weights of the offset -> wave deal); dW [27][32][32]; scratch >= scn_wgrad_tiles32_scratch_bytes(). */
int64_t scn_wgrad_tiles32_scratch_bytes(void);
int scn_wgrad_tiles32(const float* X, int64_t n_in, const float* dY, int64_t n_out, const int32_t* tstab,
                      const uint32_t* tile_mask, const int32_t* perm, const int64_t* prefix_host, float* dW, void* scratch,
                      int relu_in, scn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Adam / AdamW update (scn_optim.hip): the reference's optimizer, `optim.Adam(learnable_parameter, lr=4e-4)`
 * (scannet_config/run.py:403-416,1449), stepped once per `batches_per_step` micro-batches (training.py:458-460).
 *
 * One call updates a list of fp32 segments.  Per element, in this order, every operation rounded once (correctly rounded
 * division and square root; fma(a, b, c) = a * b + c rounded once, where torch's compiled GPU kernels fuse it, and no
 * other contraction) -- torch.optim.Adam's single-tensor, non-capturable step as torch's GPU kernels compute it:
 *   g  = g_raw * grad_scale;  if (weight_decay != 0) g = fma(weight_decay, p, g)        (coupled decay: Adam)
 *   p  = p * decay                                                                    (decoupled decay: AdamW; 1 = none)
 *   m  = w < 0.5 ? fma(w, g - m, m) : fma(-(g - m), 1 - w, g),   w = 1 - beta1          (torch's lerp)
 *   v  = fma(1 - beta2, g * g, v * beta2)
 *   p  = fma(-step_size, m / (sqrt(v) * inv_bc2_sqrt + eps), p)
 * g is read only.  The per-segment constants are computed by the caller in double and rounded to float:
 * step_size = lr / (1 - beta1^t), inv_bc2_sqrt = 1 / sqrt(1 - beta2^t) (t: the segment's step count AFTER this update;
 * torch divides by a host scalar as a multiplication by its reciprocal),
 * decay = 1 - lr * weight_decay for AdamW (then weight_decay = 0 here).  beta1, beta2, eps and grad_scale are rounded to
 * float in the library, 1 - beta1 and 1 - beta2 in double first.
 * Alignment: every pointer 4-byte aligned; a segment whose four pointers share their address modulo 16 runs 16-byte accesses
 * after a scalar head, any other runs scalar (same results).  Segments must not overlap one another.
 * The segment table is copied into the kernel arguments (at most 80 segments and 4 distinct constant sets per launch,
 * `scn_adam_launches` tells how many launches a table takes): no device table, no host wait, the table may be reused as soon
 * as the call returns.  SCN_EINVAL (nothing launched): segs NULL with n_segs > 0, n < 0, a NULL pointer with n > 0, a pointer
 * not 4-byte aligned, a non-finite beta / eps / grad_scale / step_size / inv_bc2_sqrt / weight_decay / decay,
 * inv_bc2_sqrt <= 0.
 * Segments with n == 0 are skipped. */
typedef struct scn_adam_segment {
    float* p;                        /* parameters [n], updated */
    const float* g;                  /* gradient [n] (scaled by grad_scale) */
    float* m;                        /* first moment [n], updated */
    float* v;                        /* second moment [n], updated */
    int64_t n;
    float step_size;                 /* lr / (1 - beta1^t) */
    float inv_bc2_sqrt;              /* 1 / sqrt(1 - beta2^t) */
    float weight_decay;              /* coupled weight decay; 0: none */
    float decay;                     /* decoupled weight decay factor 1 - lr * weight_decay; 1: none */
} scn_adam_segment;

/* sizeof(scn_adam_segment) (56): lets a binding check its layout. */
int64_t scn_adam_segment_bytes(void);
/* *launches = the number of kernel launches scn_adam_many makes for this table (validates it as scn_adam_many does). */
int scn_adam_launches(const scn_adam_segment* segs, int n_segs, int* launches);
int scn_adam_many(const scn_adam_segment* segs, int n_segs, double grad_scale, double beta1, double beta2, double eps,
                  scn_stream_t stream);

/* ---- RPN loss (ndsis/modules/loss.py RpnLoss with BatchwiseBboxTargetSelector; utils/bbox.py select_bbox, bbox_transform) ----
 * Three steps, every one graph-capturable (no allocation, copy or synchronisation inside; all counts stay on the device):
 *
 * scn_rpn_targets: anchors fp32 [n_anchors][2][3] = (centre, size), shared by every sample; gt_boxes fp32 [total][2][3] =
 * (start, stop), the boxes of sample b at rows box_offsets[b] .. box_offsets[b+1]-1 (box_offsets: HOST array of batch+1
 * non-decreasing values, copied into the kernel arguments).  Per sample b and anchor i: max_overlap[b][i] = the largest IoU
 * with a box of the sample, argmax[b][i] = that box's index within the sample (ties: the lowest), bbox_target[b][i] =
 * bbox_transform(anchor, matched box).  The IoU follows the reference's operation order with every operation rounded once
 * (max_overlap is bit-equal to it); log is within ulps.  A sample with no boxes: overlap 0, argmax -1, the target of a zero
 * box.  Any number of boxes per sample.
 *
 * scn_rpn_sample_batchwise: over all n = batch * anchors overlaps, positive = overlap >= positive_overlap, negative =
 * overlap < negative_overlap; min_count = min(#pos, #neg) members of the larger set (the negatives when the counts are
 * equal) are drawn uniformly without replacement, the smaller set is kept whole.  label = positive; score_weight = (kept or
 * drawn) / max(1, 2 min_count); bbox_weight = label / max(#pos, min_inverse_weight).  counts (may be NULL) = {#pos, #neg}.
 * The draw is a function of (seed, counter) only: key = a keyed bijection of the flat index, the min_count smallest keys
 * of the larger set are drawn (radix select on the device).  workspace: scn_rpn_sample_workspace_bytes(), 8-byte aligned,
 * zero before its first use; every call leaves it zero again (one workspace per stream).  n < 2^31.
 *
 * scn_rpn_loss: score_loss = sum BCE-with-logits(score, label) * score_weight, bbox_loss = sum bbox_weight[i] * smoothL1_sigma
 * (bbox[i] - bbox_target[i]) (over the 6 components); dscore / dbbox = their gradients for an upstream gradient of 1.  n =
 * batch * anchors.  The sums are accumulated in double in a fixed order (per-block partials, one finishing block): bitwise
 * identical from run to run.  scratch: scn_rpn_loss_scratch_bytes(n), 8-byte aligned.
 *
 * scn_rpn_loss_scale: out_dscore = dscore * *grad_score_loss, out_dbbox = dbbox * *grad_bbox_loss (the upstream gradients
 * are read on the device); a NULL output is not written. */
int scn_rpn_targets(const float* anchors, int64_t n_anchors, const float* gt_boxes, const int64_t* box_offsets, int batch,
                    float* max_overlap, int64_t* argmax, float* bbox_target, scn_stream_t stream);
int64_t scn_rpn_sample_workspace_bytes(void);
int scn_rpn_sample_batchwise(const float* overlaps, int64_t n, float positive_overlap, float negative_overlap,
                             float min_inverse_weight, uint64_t seed, uint64_t counter, void* workspace, float* label,
                             float* score_weight, float* bbox_weight, int64_t* counts, scn_stream_t stream);
int64_t scn_rpn_loss_scratch_bytes(int64_t n);
int scn_rpn_loss(const float* score, const float* bbox, const float* label, const float* score_weight, const float* bbox_target,
                 const float* bbox_weight, int64_t n, float sigma, void* scratch, float* score_loss, float* bbox_loss,
                 float* dscore, float* dbbox, scn_stream_t stream);
int scn_rpn_loss_scale(const float* dscore, const float* dbbox, int64_t n, const float* grad_score_loss,
                       const float* grad_bbox_loss, float* out_dscore, float* out_dbbox, scn_stream_t stream);

/* ---- mask loss (ndsis/modules/model.py OverlapCalculator, TrainSelector(0.2, 0, (24, 0, True)), SparseMaskLossSelector;
 * ndsis/modules/loss.py MaskLoss) ----
 * Every call is graph-capturable: the per-sample tables below are HOST arrays copied into the kernel arguments (32 samples
 * per launch), nothing is allocated, copied or waited for.
 *
 * scn_mask_overlap_draw: pred_boxes fp32 [P][2][3] and gt_boxes fp32 [G][2][3] = (start, stop); sample b owns the proposals
 * pred_offsets[b] .. pred_offsets[b+1]-1 (at most 1024 per sample) and the boxes gt_offsets[b] .. gt_offsets[b+1]-1 (both
 * offset arrays: batch+1 non-decreasing values from 0).  overlaps_given = 0: max_overlap[i] = the largest IoU of proposal i
 * with a box of its sample, argmax[i] = that box's index within the sample (ties: the lowest), 0 and 0 without boxes; the IoU
 * follows bbox_overlap_prediction's operation order with every operation rounded once (bit-equal to the reference); either
 * output may be NULL.  overlaps_given = 1: max_overlap / argmax are read instead.  fwd_boxes NULL: nothing else happens.
 * Otherwise the draw: positives = max_overlap >= positive_threshold; n_drawn[b] = min(num_positive, #positives of b) of them
 * are drawn uniformly without replacement.  Forward boxes of sample b start at fwd_offsets[b] (HOST, from 0) and hold
 * cap_b = min(num_positive, P_b) slots, then the G_b boxes of the sample in order:
 *   slot q < n_drawn[b]: the drawn proposal's box, gt_association = its argmax, pred_selection = its index within the sample;
 *   slot q >= n_drawn[b]: start = stop = 0 (a box that selects no point), gt_association = -1, pred_selection = -1;
 *   box cap_b + g: gt_boxes[g] of the sample, gt_association = g.
 * pred_selection (may be NULL) is [sum cap_b] int64, sample b's slots at fwd_offsets[b] - gt_offsets[b]; n_drawn (may be
 * NULL) is [batch] int64.  The drawn slots are in ascending key order, key = a keyed 32-bit bijection of (sample, index)
 * whose round keys derive from (seed, counter): the draw is a function of those only.  batch < 65536.
 *
 * scn_mask_loss: logits fp32 [m][k] over the crop's rows; src_row / box_of int32 [m] (RoiSelection: box-major, the rows of
 * a box contiguous); gt_association int64 [n_boxes], n_boxes = box_offsets[batch], the boxes of sample b at box_offsets[b] ..
 * box_offsets[b+1]-1; labels int64 [gt_offsets[batch]], sample b's at gt_offsets[b]; mask_words: sample b's instances
 * packed as [G_b][ceil(N_b / 32)] uint32 at word_offsets[b] (bit p % 32 of word p / 32 = point row p of the sample, as
 * scn_mask_pack writes them), N_b = point_offsets[b+1] - point_offsets[b] and point row p = src_row - point_offsets[b].
 * All four offset arrays are HOST arrays of batch+1 values.  A box whose association is outside 0 .. G_b-1 or whose label is
 * outside 0 .. k-1 is dropped, and so is a box without rows (the reference's NaN).  loss = sum_b w_b l_b / sum_b w_b over the
 * boxes kept, l_b = the mean BCE-with-logits of the box's label column against the instance's bits, w_b =
 * class_weights[label] (fp32 [k], or NULL: 1); 0 if no box is kept.  Sums in double, fixed order: bitwise identical reruns.
 * scratch: scn_mask_loss_scratch_bytes(n_boxes, m), 8-byte aligned; it keeps what scn_mask_loss_bwd reads.
 *
 * scn_mask_loss_bwd: dlogits fp32 [m][k] = *grad_loss * (sigmoid(x) - t) * w_b / (rows_b * sum w) in the label column of the
 * row's box, 0 elsewhere; scratch as left by scn_mask_loss with the same n_boxes and m.
 *
 * scn_mask_pack: masks[b] = device bool / uint8 [n_gt[b]][n_points[b]] (HOST array of device pointers) -> out_words, the
 * samples back to back in the layout above. */
int scn_mask_overlap_draw(const float* pred_boxes, const int64_t* pred_offsets, const float* gt_boxes, const int64_t* gt_offsets,
                          int batch, float* max_overlap, int64_t* argmax, int overlaps_given, float positive_threshold,
                          int num_positive, uint64_t seed, uint64_t counter, const int64_t* fwd_offsets, float* fwd_boxes,
                          int64_t* gt_association, int64_t* pred_selection, int64_t* n_drawn, scn_stream_t stream);
int64_t scn_mask_loss_scratch_bytes(int64_t n_boxes, int64_t m);
int scn_mask_loss(const float* logits, int64_t m, int k, const int32_t* src_row, const int32_t* box_of,
                  const int64_t* gt_association, const int64_t* box_offsets, const int64_t* labels, const int64_t* gt_offsets,
                  const uint32_t* mask_words, const int64_t* word_offsets, const int64_t* point_offsets, int batch,
                  const float* class_weights, void* scratch, float* loss, scn_stream_t stream);
int scn_mask_loss_bwd(const float* grad_loss, const void* scratch, int64_t n_boxes, int64_t m, int k, const int32_t* box_of,
                      float* dlogits, scn_stream_t stream);
int scn_mask_pack(const uint8_t* const* masks, const int64_t* n_gt, const int64_t* n_points, int batch, uint32_t* out_words,
                  scn_stream_t stream);

/* ---- class and segmentation losses (ndsis/modules/loss.py ClassLoss and the segmentation loss: nn.CrossEntropyLoss(weight,
 * ignore_index=-100, reduction='mean'); ndsis/modules/model.py ClassPredictor, SegmentationPredictor) ----
 * Every call is graph-capturable: nothing is allocated, copied or waited for.  1 <= c <= 256, else SCN_EINVAL.
 *
 * scn_xent_fwd: logits fp32 [n][c] row-major, targets int64 [n], weights fp32 [c] or NULL (all 1).  A row is valid when its
 * target is in 0 .. c-1 and differs from ignore_index.  A row whose target equals ignore_index is dropped, as torch does.  A
 * row whose target is anything else outside 0 .. c-1 is dropped too and counted: *n_bad_targets (device int64, may be NULL) =
 * the number of such rows of this call (torch raises a device assert there).
 *   *loss = sum_valid w[t_i] (logsumexp(x_i) - x_i[t_i]) / sum_valid w[t_i]
 * DEVIATION from torch: when the valid rows' weights sum to 0 -- no valid row at all, or n == 0 -- the loss is 0 and the
 * gradient all zero, where torch returns NaN (0 / 0).  TrainSelector's fixed-capacity slots that drew nothing become ignored
 * rows, so "rows, none valid" is this library's image of the reference's "no box selected", for which ClassLoss returns 0.
 * The sums are in double: one partial per workgroup in a fixed order, then one finishing block (2 launches; 1 for n == 0
 * and for n * lanes-per-row <= 2048, lanes-per-row = 1, 2, 4, 8 for c <= 32, 64, 128, 256: one block finishes itself).
 * Reruns are bitwise identical.  scratch: scn_xent_scratch_bytes(n, c) bytes (-1: bad arguments), 8-byte aligned; it keeps
 * the weight sum that scn_xent_bwd reads.
 *
 * scn_xent_bwd (1 launch): dlogits[i][j] = *grad_loss * w[t_i] * (softmax(x_i)[j] - [j == t_i]) / sum_valid w[t] for a valid
 * row, exactly 0 for every other row.  The softmax is recomputed from the logits (nothing per row is kept); logits, targets,
 * weights, ignore_index, n and c as given to scn_xent_fwd, scratch as it left it.
 *
 * scn_softmax_argmax (1 launch, none for n == 0): indices int64 [n] = the first index of the row's maximum, compared on the
 * logits themselves (exact; rows without NaN); probabilities fp32 [n][c] = softmax of the row, or NULL. */
int64_t scn_xent_scratch_bytes(int64_t n, int c);
int scn_xent_fwd(const float* logits, int64_t n, int c, const int64_t* targets, const float* weights, int64_t ignore_index,
                 void* scratch, float* loss, int64_t* n_bad_targets, scn_stream_t stream);
int scn_xent_bwd(const float* grad_loss, const float* logits, int64_t n, int c, const int64_t* targets, const float* weights,
                 int64_t ignore_index, const void* scratch, float* dlogits, scn_stream_t stream);
int scn_softmax_argmax(const float* logits, int64_t n, int c, float* probabilities, int64_t* indices, scn_stream_t stream);

/* ---- the loss container (ndsis/modules/loss.py Loss.forward :101-191: the criteria's values combined with five log-weights) ----
 * Both calls are one launch of one wave, graph-capturable (nothing is allocated, copied or waited for) and bitwise identical
 * from run to run.  `terms` and `log_weights` are HOST arrays of SCN_LOSS_TERMS DEVICE pointers to 0-dim fp32 values, copied
 * into the kernel arguments:
 *   terms       = (rpn_score, rpn_bbox, class, mask, segmentation); a NULL entry: the term is absent
 *   log_weights = (rpn_class, rpn_bbox, class, mask, segmentation), none NULL: the reference's parameters -log(weight)
 * Term i is scaled by c_i = exp(-w[p(i)]) with the reference's crossing p = (1, 0, 2, 3, 4): the rpn_score term uses the
 * rpn_bbox weight and the rpn_bbox term the rpn_class weight (loss.py:111-114).  Over the present terms, in the order above,
 * each fp32 operation rounded once:
 *   loss = ((0 + t_0 c_0) + t_1 c_1) + ...      extra = ((0 + w[p(0)]) + w[p(1)]) + ...      combined = loss + extra
 * An absent term adds nothing, and neither does its weight.
 *
 * scn_loss_combine: record fp32 [SCN_LOSS_RECORD] = (loss `_total_`, combined `_total_multitask_`, t_0 .. t_4 with 0 where
 * absent, the number of present terms that are NaN).  root_grad fp32 [SCN_LOSS_TERMS] (may be NULL) = scale * c_i, 0 where
 * absent: the gradient of scale * combined at term i.  weight_grad (may be NULL): HOST array of SCN_LOSS_TERMS DEVICE
 * pointers in the order of log_weights, entries may be NULL; for a present term i, *weight_grad[p(i)] += scale * (1 - t_i c_i)
 * (accumulated: micro-batches add up; the caller zeroes); the slot of an absent term's weight is not touched.  Distinct
 * entries must not alias.  running (may be NULL): double [SCN_LOSS_RECORD + 1], the record's entries added to the first
 * SCN_LOSS_RECORD sums and 1 to the last (the caller zeroes it; one running record per stream at a time).  scale: finite.
 * Every pointer 4-byte aligned (running: 8), else SCN_EINVAL.  All stores go to these fixed-size buffers.
 *
 * scn_loss_combine_bwd: the same quantities times an upstream gradient read on the device: term_grad fp32 [SCN_LOSS_TERMS]
 * (may be NULL) = *grad * c_i, weight_grad fp32 [SCN_LOSS_TERMS] in the order of log_weights (may be NULL) [p(i)] =
 * *grad * (1 - t_i c_i); both 0 where the term is absent.  Written, not accumulated. */
#define SCN_LOSS_TERMS 5
#define SCN_LOSS_RECORD 8
int scn_loss_combine(const float* const* terms, const float* const* log_weights, float scale, float* record, float* root_grad,
                     float* const* weight_grad, double* running, scn_stream_t stream);
int scn_loss_combine_bwd(const float* grad, const float* const* terms, const float* const* log_weights, float* term_grad,
                         float* weight_grad, scn_stream_t stream);

/* ---- evaluation (ndsis/training/evaluation.py: MaskOverlapCalculator / BboxOverlapCalculator, PrecisionRecallCurve.
 * calc_tp_indicator, ConfusionCalculator, BinaryMaskConfusionCalculator; ndsis/utils/mask.py:62-148) ----
 * All integer results are exact; every mask IoU is one correctly rounded fp32 division of two exact integers and every box
 * IoU follows bbox_overlap_prediction's operation order, so results are bit-equal to the reference and identical from run to
 * run.  Offsets named *_offsets are HOST arrays of batch + 1 values (pair_offsets[b+1] - pair_offsets[b] = P_b * G_b); every
 * other pointer is device memory.  Packed masks use scn_mask_pack's layout: sample b's [rows_b][ceil(N_b / 32)] uint32
 * words, bit p % 32 of word p / 32 = point row p of the sample, bits beyond N_b zero.
 *
 * scn_eval_mask_bits (1 memset + 1 launch): logits fp32 [m][k], src_row / box_of int32 [m] (RoiSelection), class_of_box int64
 * [n_boxes], bit_base int64 [n_boxes] = 32 * (first word of the box's mask row in out_words) - (first point row of the box's
 * sample).  Bit = sigmoid(logits[r][class]) > mask_threshold with scn_mask_scatter's sigmoid and class validity rule; all
 * n_words words are written.
 * scn_eval_pack_threshold (1 launch): masks fp32 [p][n] > mask_threshold -> out_words [p][ceil(n / 32)].
 * scn_eval_mask_iou (per 32 samples: row counts, tiles, finish): inter int32 [pairs] = popcount(pred & gt), pred_count int32
 * [sum P], gt_count int32 [sum G], iou fp32 [pairs] (may be NULL) = float(inter) / float(|pred| + |gt| - inter), NaN for
 * 0 / 0; pair_confusion (may be NULL; needs P_b == G_b) int64 [sum P][2][2] = [[tp, fp], [fn, tn]] of prediction i against
 * ground truth i.  N_b < 2^31; the counts are exact for every such N_b, the quotient is the division of two exact integers
 * for N_b <= 2^24 (beyond that the int -> fp32 conversions round first; the reference's fp32 sums stop being exact there too).
 * scn_eval_bbox_iou (1 launch per 32 samples): boxes fp32 [n][2][3] (start, stop) -> iou fp32 [pairs].
 * scn_eval_match (1 launch, one wave per problem): problem q = (problem_sample[q], problem_class[q] or -1 for all classes,
 * problem_threshold[q]); pred_offsets / gt_offsets / pair_offsets are DEVICE int64 [batch + 1] here.  Its predictions are
 * those of the sample with keep != 0 (keep uint8 [sum P], NULL: all) and pred_class == class, in their given order, its
 * ground truths those with gt_class == class.  flags int8 at problem_out[q], P_b values: -1 not part of the problem, 1 true
 * positive (the maximum IoU over the ground truths not yet matched, first index on a tie, is >= threshold; that ground truth
 * is retired), 0 false positive (also when a NaN is among the remaining ground truths).  num_gt int32 [n_problems].
 * max_gt = the largest G_b, at most 4096.
 * scn_eval_confusion (2 memsets + 1 launch): confusion int64 [c][c] = counts of pred * c + gt over the rows with 0 <= gt < c;
 * *n_bad_pred (may be NULL) = such rows whose pred is outside 0 .. c-1 (not counted in the matrix).  c <= 64. */
int scn_eval_mask_bits(const float* logits, int64_t m, int k, const int32_t* src_row, const int32_t* box_of,
                       const int64_t* class_of_box, int num_valid, float mask_threshold, const int64_t* bit_base,
                       int64_t n_boxes, int64_t n_words, uint32_t* out_words, scn_stream_t stream);
int scn_eval_pack_threshold(const float* masks, int64_t p, int64_t n, float mask_threshold, uint32_t* out_words,
                            scn_stream_t stream);
int scn_eval_mask_iou(const uint32_t* pred_words, const int64_t* pred_word_offsets, const uint32_t* gt_words,
                      const int64_t* gt_word_offsets, const int64_t* pred_offsets, const int64_t* gt_offsets,
                      const int64_t* pair_offsets, const int64_t* n_points, int batch, int32_t* inter, int32_t* pred_count,
                      int32_t* gt_count, float* iou, int64_t* pair_confusion, scn_stream_t stream);
int scn_eval_bbox_iou(const float* pred_boxes, const int64_t* pred_offsets, const float* gt_boxes, const int64_t* gt_offsets,
                      const int64_t* pair_offsets, int batch, float* iou, scn_stream_t stream);
int scn_eval_match(const float* iou, const int64_t* pred_offsets, const int64_t* gt_offsets, const int64_t* pair_offsets,
                   int batch, int64_t max_gt, const uint8_t* keep, const int64_t* pred_class, const int64_t* gt_class,
                   const int32_t* problem_sample, const int64_t* problem_class, const float* problem_threshold,
                   const int64_t* problem_out, int n_problems, int any_class_problem, int8_t* flags, int32_t* num_gt,
                   scn_stream_t stream);
int scn_eval_confusion(const int64_t* pred, const int64_t* gt, int64_t n, int num_classes, int64_t* confusion,
                       int64_t* n_bad_pred, scn_stream_t stream);

/* ---- training-sample conversion (ndsis/data/sparse_augmentation.py convert_sample :250-313 after augment_coords: get_masks
 * :208-234, get_bbox :188-205, get_semantic_segmentation_labels :237-247, augment_features :152-185) ----
 * A stored sample has N points with an instance id each, 0 .. I-1 or I = "no instance" (I = n_instances).  Neither call
 * waits for the host; both are integer-exact or elementwise, so reruns give identical bits.
 *
 * scn_sample_stats (2 launches): discrete / table as scn_vox_discretize left them, start_host = the cut-out's start (what
 * scn_vox_gather subtracts).  stats int32 [I + 1][8] per instance slot = (points, points with table >= 0, min x y z, max
 * x y z of discrete - start over those kept points; INT32_MAX / INT32_MIN where there is none).  *n_bad_ids (device int32) =
 * the points whose id is outside 0 .. I; they are in no slot.  Each workgroup collects in an LDS table of (I + 1) * 32 bytes
 * and merges it with integer atomics.  I > SCN_SAMPLE_MAX_INSTANCES: SCN_ESIZE, nothing launched.  n < 1: SCN_EINVAL.
 *
 * scn_sample_pack (1 memset + 1 launch; nothing for m == 0), over the m kept rows `rows` (ascending, int32) in that order:
 *   features fp32 [m][C], C = 3 use_color + use_ones + 3 use_normal = (colors[row] + color_noise, 1, normals[row] @ rotation
 *     + normal_noise); rotation_host = the 3x3 almost_orthonormal (HOST, row-major), each product as fma(z, R2j, fma(y, R1j,
 *     x * R0j)) like scn_vox_project; a noise pointer is device fp32 [3] or, with *_per_point != 0, [m][3] in kept-row order;
 *     NULL = none.  The noise is added after the rotation, as the reference does.
 *   seg_labels int64 [m] = seg_table[id of the row], seg_table device int64 [I + 1] (the mapped labels, then the background
 *     label); both NULL: not wanted.  An id outside 0 .. I reads slot I.
 *   mask_words uint32 [n_kept][ceil(m / 32)] = loss.PackedMasks' / scn_mask_pack's layout: bit p % 32 of word p / 32 of row
 *     slot_of_instance[id] (device int32 [I + 1], -1 = instance not kept) is set for kept row p; every other bit, the bits
 *     beyond m included, is zero.  n_kept == 0: slot_of_instance and mask_words may be NULL. */
#define SCN_SAMPLE_MAX_INSTANCES 1023
int scn_sample_stats(const int32_t* discrete, const int32_t* table, const int64_t* instance_ids, int64_t n, int n_instances,
                     const int32_t* start_host, int32_t* stats, int32_t* n_bad_ids, scn_stream_t stream);
int scn_sample_pack(const int32_t* rows, int64_t m, const float* colors, const float* normals, const int64_t* instance_ids,
                    int n_instances, const float* rotation_host, const float* color_noise, int color_noise_per_point,
                    const float* normal_noise, int normal_noise_per_point, int use_color, int use_ones, int use_normal,
                    float* features, const int64_t* seg_table, int64_t* seg_labels, const int32_t* slot_of_instance,
                    int64_t n_kept, uint32_t* mask_words, scn_stream_t stream);

/* ---- the sample conversion's random numbers, drawn on the device -- csrc/scn_rng.h, scn_draws.hip, scn_sample.hip ----
 * Generator: Philox4x32-10 (Random123: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with
 *   key = (seed lo32, seed hi32), counter = (index, stream, sample counter lo32, sample counter hi32),
 * so every value is a function of (seed, sample counter, stream, index) alone: no state, no dependence on the launch shape or
 * the order of calls.  Streams: SCN_RNG_* below.  A uniform of a word w is u(w) = ((w >> 9) + 0.5) * 2^-23 (exact in fp32, inside
 * (0, 1)); the three normals of a draw (w0 .. w3) are z0 = r0 cospi(2 u(w1)), z1 = r0 sinpi(2 u(w1)), z2 = r1 cospi(2 u(w3)) with
 * r0 = sqrt(-2 log u(w0)), r1 = sqrt(-2 log u(w2)), in fp32 with the accurate logf / sqrtf / sincospif.  A noise value is
 * sigma * z rounded once; it is added to the feature with one more rounding.
 *
 * scn_philox_words_host: the four words of one draw, computed on the HOST (no GPU is touched).
 * scn_philox_fill (1 launch, none for n == 0): the draws of indices first_index .. first_index + n - 1 of one stream; mode 0:
 *   out uint32 [n][4] = the words; mode 1: out fp32 [n][3] = sigma * (z0, z1, z2).  Indices beyond 2^32: SCN_ESIZE.
 * scn_sample_pack_drawn: scn_sample_pack with the noise drawn in the kernel instead of read -- kept row p of a per-point noise
 *   is index p of stream SCN_RNG_COLOR / SCN_RNG_NORMAL, a common noise (*_common != 0) is index 0 of SCN_RNG_COLOR_COMMON /
 *   SCN_RNG_NORMAL_COMMON.  A sigma of 0: no noise, no generator call.  Every output is bit-equal to scn_sample_pack fed the
 *   tensors scn_philox_fill (mode 1) writes for the same seed, counter and sigma.  Launches and error codes as scn_sample_pack.
 * scn_sample_cut_start (1 launch of one workgroup): the start positions of the reference's random_cut_out
 *   (sparse_augmentation.py:50-78) over discrete int32 [n][3] (scn_vox_discretize's voxels before a cut-out); size_host /
 *   border_host int32 [3] on the HOST (border = the largest empty border per dimension, 0 <= border <= size).  With (w0, w1, ..) the draw of
 *   (SCN_RNG_CUT, index 0): i = (w0 * 3) >> 32, j = (w1 * 2) >> 32, the dimension order is [0, 1, 2] with element i, then
 *   element j of the rest, taken out.  For the k-th dimension d of that order: lo / hi / count over the voxels the dimensions
 *   before left alive; count == 0 ends the loop (later starts stay 0); min_start = lo - border, max_start = hi + 1 - size +
 *   border; max_start <= min_start: start[d] = min_start and nothing is cut along d; else start[d] = min_start + ((w_k of
 *   (SCN_RNG_CUT, index 1) * (uint64)(max_start - min_start)) >> 32) and only voxels with 0 <= x[d] - start[d] < size[d] stay
 *   alive.  out8 (DEVICE int32 [8]) = start[3], order[3], voxels alive after the last processed dimension, dimensions
 *   processed.  n < 1, a size < 1 or a border outside 0 .. size: SCN_EINVAL.  Starts are formed in 64 bits and
 *   saturate at the int32 range.  Integers only: reruns give identical values.  Does not wait for the host. */
#define SCN_RNG_HOST 0           /* distortion matrix, mirror, angle, sub-pixel offset: drawn on the host */
#define SCN_RNG_CUT 1
#define SCN_RNG_COLOR 2
#define SCN_RNG_NORMAL 3
#define SCN_RNG_COLOR_COMMON 4
#define SCN_RNG_NORMAL_COMMON 5
int scn_philox_words_host(uint64_t seed, uint64_t counter, uint32_t stream, uint32_t index, uint32_t* out4);
int scn_philox_fill(uint64_t seed, uint64_t counter, uint32_t stream, int64_t first_index, int64_t n, int mode, float sigma,
                    void* out, scn_stream_t stream_handle);
int scn_sample_pack_drawn(const int32_t* rows, int64_t m, const float* colors, const float* normals, const int64_t* instance_ids,
                          int n_instances, const float* rotation_host, uint64_t seed, uint64_t counter, float color_sigma,
                          int color_common, float normal_sigma, int normal_common, int use_color, int use_ones, int use_normal,
                          float* features, const int64_t* seg_table, int64_t* seg_labels, const int32_t* slot_of_instance,
                          int64_t n_kept, uint32_t* mask_words, scn_stream_t stream);
int scn_sample_cut_start(const int32_t* discrete, int64_t n, const int32_t* size_host, const int32_t* border_host, uint64_t seed,
                         uint64_t counter, int32_t* out8, scn_stream_t stream);

/* ---- dense RoiAlign and the unclamped dense max pool of the reference's dense class branch (ndsis/modules/
 * roi_select_dense.py:28-141 RoiAlign with clip_boxes=True; nn.MaxPool3d(2)) -- csrc/scn_roialign.hip, fp32 (the bf16
 * forms follow) ----
 * F fp32 [batch X Y Z][c], channels-last, row ((b X + x) Y + y) Z + z; size_host = (X, Y, Z) and extract_host = (ex, ey, ez),
 * each >= 2, int64 [3] on the HOST.  boxes fp32 [n_boxes][2][3] = (start, stop) in cells, already transformed and clipped to
 * [0, size - 1]; sample_of_box int32 [n_boxes], ascending, in 0 .. batch - 1.  Out fp32 [n_boxes ex ey ez][c], row
 * ((r ex + i) ey + j) ez + k.  Per axis sample i sits at c_i = min(i * ((stop - start) / (e - 1)) + start, stop), every
 * operation rounded once; it reads cells floor(c_i) and ceil(c_i) with weights 1 - w and w, w = c_i - floor(c_i); a corner's
 * weight is (wx * wy) * wz.  `table` is DEVICE memory of 4 * n_boxes * (3 * (ex + ey + ez) + 2 * (X + Y + Z)) bytes that the
 * forward fills (the cells, clamped to the volume, and the weights of every (box, axis, sample); per (box, axis, cell) the
 * first sample that touches the cell and how many consecutive ones do) and the backward reads.  Extents <= 1024, sizes <= 65536.
 * scn_roialign_fwd: 3 launches, none for n_boxes == 0.
 * scn_roialign_bwd: 1 launch (n_boxes == 0: one memset).  dF fp32 [batch X Y Z][c], EVERY row written, 0 where no sample
 * reads the cell.  A gather per (cell, channel) in a fixed order -- the boxes of the cell's sample ascending, within a box the
 * touching samples i, j, k ascending, nested (sum over k, times the y weight, sum over j, times the x weight, sum over i) --
 * without atomics: reruns give identical bits.
 * scn_dense_maxpool_fwd / _bwd (1 launch each, none for n_boxes == 0): X fp32 [n_boxes ex ey ez][c] -> Y fp32
 * [n_boxes ex/2 ey/2 ez/2][c], extent_host = (ex, ey, ez) int64 [3] on the HOST, every extent even.  Y = the maximum of the 8
 * children, NOT clamped at 0 (scn_pool_fwd is); argmax uint8, one per element of Y = the child (dx * 2 + dy) * 2 + dz that
 * gave it, the first one on a tie, a NaN child wins.  The backward writes every element of dX: dY at that child, 0 at the
 * other seven.  Neither call waits for the host. */
int scn_roialign_fwd(const float* F, int batch, const int64_t* size_host, int c, const float* boxes,
                     const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table, float* Out,
                     scn_stream_t stream);
int scn_roialign_bwd(const float* dOut, const void* table, const int32_t* sample_of_box, int64_t n_boxes, int batch,
                     const int64_t* size_host, int c, const int64_t* extract_host, float* dF, scn_stream_t stream);
int scn_dense_maxpool_fwd(const float* X, int64_t n_boxes, const int64_t* extent_host, int c, float* Y, uint8_t* argmax,
                          scn_stream_t stream);
int scn_dense_maxpool_bwd(const float* dY, const uint8_t* argmax, int64_t n_boxes, const int64_t* extent_host, int c,
                          float* dX, scn_stream_t stream);

/* ---- the same four calls on bf16-STORED slabs (the dense class branch under bf16 storage) -- csrc/scn_roialign.hip ----
 * Arguments, layouts, range checks, launch counts and the n_boxes == 0 paths are those of the fp32 forms above; F, Out, dOut,
 * dF, X, Y, dY, dX hold bf16 bit patterns (uint16_t).  boxes stay fp32, sample_of_box int32, and `table` is the same buffer,
 * filled by the same kernels: the sample cells and weights are bit-identical to the fp32 call's, and a table written by
 * either forward serves either backward.
 * Arithmetic: every element is widened exactly when it is read; the products and sums are the fp32 kernels', in the same
 * order (corner order and (wx * wy) * wz forward; the nested ordered gather over boxes, i, j, k backward; no atomics); the
 * result is rounded to bf16 ONCE, at the store, to nearest even.  So each call's output equals the fp32 call's output on the
 * widened inputs, rounded once, bit for bit.  scn_roialign_bwd_bf16 writes every cell of dF, +0 where no sample reads it
 * (n_boxes == 0: one memset); reruns give identical bits.
 * scn_dense_maxpool_fwd_bf16: the maximum of 8 bf16 children is one of them -- exact; the first child wins a tie, a NaN child
 * wins, argmax is a uint8 per element.  scn_dense_maxpool_bwd_bf16: dY at that child, +0 at the other seven.
 * Lanes are 16 bytes = 8 channels: c % 8 == 0 and 16-byte aligned feature pointers are REQUIRED (the storage rule of the Python
 * side: a slab is bf16-stored only when its width is a multiple of 8); anything else returns SCN_EINVAL with a message before
 * anything is launched.  Neither call waits for the host. */
int scn_roialign_fwd_bf16(const uint16_t* F, int batch, const int64_t* size_host, int c, const float* boxes,
                          const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table, uint16_t* Out,
                          scn_stream_t stream);
int scn_roialign_bwd_bf16(const uint16_t* dOut, const void* table, const int32_t* sample_of_box, int64_t n_boxes, int batch,
                          const int64_t* size_host, int c, const int64_t* extract_host, uint16_t* dF, scn_stream_t stream);
int scn_dense_maxpool_fwd_bf16(const uint16_t* X, int64_t n_boxes, const int64_t* extent_host, int c, uint16_t* Y,
                               uint8_t* argmax, scn_stream_t stream);
int scn_dense_maxpool_bwd_bf16(const uint16_t* dY, const uint8_t* argmax, int64_t n_boxes, const int64_t* extent_host, int c,
                               uint16_t* dX, scn_stream_t stream);

/* ---- RoiAlign and the 2^3 max pool in ONE pass (the reference's class head without an input convolution cuts 8^3 boxes out of
 * the RPN stack's volume at its full width: the un-pooled samples are never written) -- csrc/scn_roialign.hip ----
 * Arguments, layouts, range checks and `table` (the same buffer, filled by the same two kernels) are those of scn_roialign_fwd /
 * _bwd, except: Y [n_boxes ex/2 ey/2 ez/2][c] takes the place of Out, dY that of dOut, and argmax uint8, one byte per element of
 * Y, is written by the forward and read by the backward.  Every extent must be even (and >= 2): else SCN_EINVAL before any
 * launch.  The _bf16 forms take bf16 bit patterns and refuse c % 8 != 0 as the calls above do.
 * scn_roialign_pool_fwd (3 launches, none for n_boxes == 0) = scn_roialign_fwd then scn_dense_maxpool_fwd, BIT FOR BIT, Y and
 * argmax: each of the 8 children is the RoiAlign sample (the same corner order, (wx * wy) * wz weights; one device function
 * serves both kernels), in the bf16 form rounded to bf16 once before the comparison; the first child wins a tie, a NaN child
 * wins.
 * scn_roialign_pool_bwd (1 launch; n_boxes == 0: one memset) = scn_dense_maxpool_bwd then scn_roialign_bwd, equal as numbers
 * (a -0 of the pair may be a +0 here): scn_roialign_bwd's ordered gather with dOut[r, i, j, k] = dY[r, i/2, j/2, k/2] where
 * argmax names child (i & 1, j & 1, k & 1) and 0 elsewhere; terms that are zero by that rule are skipped.  No atomics, reruns
 * give identical bits, every cell of dF is written.  No call waits for the host. */
int scn_roialign_pool_fwd(const float* F, int batch, const int64_t* size_host, int c, const float* boxes,
                          const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table, float* Y,
                          uint8_t* argmax, scn_stream_t stream);
int scn_roialign_pool_bwd(const float* dY, const uint8_t* argmax, const void* table, const int32_t* sample_of_box,
                          int64_t n_boxes, int batch, const int64_t* size_host, int c, const int64_t* extract_host, float* dF,
                          scn_stream_t stream);
int scn_roialign_pool_fwd_bf16(const uint16_t* F, int batch, const int64_t* size_host, int c, const float* boxes,
                               const int32_t* sample_of_box, int64_t n_boxes, const int64_t* extract_host, void* table,
                               uint16_t* Y, uint8_t* argmax, scn_stream_t stream);
int scn_roialign_pool_bwd_bf16(const uint16_t* dY, const uint8_t* argmax, const void* table, const int32_t* sample_of_box,
                               int64_t n_boxes, int batch, const int64_t* size_host, int c, const int64_t* extract_host,
                               uint16_t* dF, scn_stream_t stream);

/* ---- the reference's Reshaper (`x.view(R, -1)` of [R, C, x, y, z]) on box grids, with the ReLU behind it -- fp32 ----
 * X fp32 [n_boxes v][c] (v sites per box, row r v + s) <-> Y fp32 [n_boxes][c v], channel-major: Y[r][ch v + s] =
 * relu ? max(X[r v + s][ch], 0) : X[r v + s][ch]; a NaN stays a NaN.  scn_box_flatten_bwd writes EVERY element of dX:
 * dY[r][ch v + s] where !relu or X > 0, else 0 (X may be NULL when !relu).  1 launch each, none for n_boxes == 0; v c < 2^31.
 * Neither call waits for the host. */
int scn_box_flatten_fwd(const float* X, int64_t n_boxes, int64_t v, int c, int relu, float* Y, scn_stream_t stream);
int scn_box_flatten_bwd(const float* X, const float* dY, int64_t n_boxes, int64_t v, int c, int relu, float* dX,
                        scn_stream_t stream);

/* ---- the permutation half of the reference's up-sampling RPN heads (ndsis/modules/anchor_network.py:127-219
 * AnchorNetworkUpsample; anchor.py:167-192 rpn_permuter + rpn_bbox_score_splitter) -- csrc/scn_anchor_up.hip, fp32 ----
 * One call per anchor level.  P fp32 [batch X Y Z][ncol]: the level's channels-last slab times the packed head weights, row
 * ((b X + x) Y + y) Z + z; size_host = (X, Y, Z), int64 [3] on the HOST.  groups_host int64 [n_groups][6] on the HOST, per
 * group (s0, s1, s2, A_g, first column, first index in the all-anchor order): the group's transposed convolution has kernel =
 * stride = (s0, s1, s2) and A_g anchors; its s0 s1 s2 A_g 7 columns start at `first column` -- the groups' columns tile
 * [0, ncol) in group order -- and column first + ((a s1 + b) s2 + c) (A_g 7) + anchor 7 + k holds component k (0..5 box
 * deltas, 6 the score) of `anchor` at the fine cell (x s0 + a, y s1 + b, z s2 + c).  The group's anchors take the
 * all-anchor indices first index + fine cell * A_g + anchor, fine cells row-major over (X s0, Y s1, Z s2), z fastest.
 * dest int32 [n_all] on the device, shared by every sample and every level: the anchor's rank among the n_inside anchors
 * inside the scene, -1 outside (any other value outside [0, n_inside) counts as -1).
 * scn_anchor_up_fwd: rpn_bbox fp32 [batch][n_inside][2][3] and rpn_score fp32 [batch][n_inside]; the level writes the
 * records of its own inside anchors and leaves every other byte alone.  1 launch (none for batch == 0 or n_inside == 0).
 * scn_anchor_up_bwd: dP fp32 [batch X Y Z][ncol], EVERY element written exactly once: the incoming value where dest >= 0, 0
 * where it is -1; d_bbox / d_score may be NULL (= zeros).  A gather without atomics: reruns give identical bits.  1 launch.
 * Both only copy.  A bad group table, size or count returns SCN_EINVAL before anything is launched.  Neither waits for the host. */
#define SCN_ANCHOR_UP_MAX_GROUPS 16
int scn_anchor_up_fwd(const float* P, int batch, const int64_t* size_host, int ncol, const int64_t* groups_host, int n_groups,
                      const int32_t* dest, int64_t n_all, int64_t n_inside, float* rpn_bbox, float* rpn_score,
                      scn_stream_t stream);
int scn_anchor_up_bwd(const float* d_bbox, const float* d_score, int batch, const int64_t* size_host, int ncol,
                      const int64_t* groups_host, int n_groups, const int32_t* dest, int64_t n_all, int64_t n_inside,
                      float* dP, scn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCN_MI355X_H */
