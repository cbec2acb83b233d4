// The data format of the launch-list executor: the ONE declaration of what every int64 word of an operator row and of a
// kernel-map descriptor means.  csrc/exec.hip includes it; fcaf3d_amd/executor.py and sparse.py read the same text
// (_lib.parse_enums: plain enums, `NAME`, `NAME = integer` or `NAME = earlier names + integers`, // comments) — nothing
// else states a word number.
//
// An operator row is OPW words: word 0 = the opcode, word 1 = the stream (0 main, 1 head branch, 2 weight gradients), the
// operator's fields from word 2 on, unused words 0.  Per operator OP_X the fields are X_<FIELD>, closed by X_END.
// Field values: (dim) an index into the row-count table, (map) an index into the descriptor table, (f64) the bit pattern
// of a double, a plain integer, or — everything else — an index into the address table.  Two encodings of "absent":
//   * a field named ..._P1 holds index + 1, 0 = none (exec.hip P1<>, executor.py emit adds the 1);
//   * every other optional address holds -1 = none (exec.hip P<>).
#ifndef FCAF3D_EXEC_OPS_H
#define FCAF3D_EXEC_OPS_H

enum {
  OPW = 24,      // int64 words per operator
  MAPW = 20,     // int64 words per kernel-map descriptor
  NSTREAM = 3
};
enum { ROW_OP, ROW_STREAM };     // the two words every row starts with

// ---- opcodes.  OP_NORM_FWD, OP_MAXPOOL_FWD, OP_UNION_FWD, OP_NORM_BWD, OP_MAXPOOL_BWD are retired: never emitted, no fields, no
// case in exec.hip (the stem's tail runs as OP_NORM_POOL_FWD / OP_POOL_NORM_BWD, the unions inside OP_BN_FWD); the numbers stay
enum {
  OP_STEM_FWD = 1, OP_COL_STATS, OP_NORM_FWD, OP_MAXPOOL_FWD, OP_CONV, OP_BN_FWD, OP_UNION_FWD, OP_HEAD_FWD, OP_RECORD, OP_WAIT,
  OP_HEAD_BWD, OP_WGRAD, OP_BN_BWD, OP_NORM_BWD, OP_MAXPOOL_BWD, OP_STEM_WGRAD, OP_GATHER, OP_ADD, OP_SMALL_GRADS,
  OP_PERMUTE_GENT, OP_HEAD_WFIN, OP_COPY, OP_COL_SUM, OP_ROW_SUM, OP_AMAX, OP_CLEAR, OP_NORM_POOL_FWD, OP_POOL_NORM_BWD, OP_INV_ROWS,
  OP_BN_EVAL_BWD
};

// ---- operator fields
enum {  // the stem convolution (3 input channels)
  STEM_FWD_X = 2,
  STEM_FWD_W,
  STEM_FWD_MAP,        // (map)
  STEM_FWD_OUT,
  STEM_FWD_COL,        // the gathered column matrix, kept for the weight gradient | -1
  STEM_FWD_END
};
enum {  // per-segment column statistics (instance norm)
  COL_STATS_X = 2,
  COL_STATS_SEG,       // segment of every row | -1
  COL_STATS_N,         // (dim)
  COL_STATS_C,
  COL_STATS_NSEG,      // (dim)
  COL_STATS_MEAN,
  COL_STATS_VAR,
  COL_STATS_CNT,
  COL_STATS_END
};
enum {  // convolution on a kernel map, forward or backward-data, or a dense GEMM over n rows
  CONV_X = 2,
  CONV_IMG,            // the pre-split weight image (of the transposed kernel for DIR = 1)
  CONV_MAP,            // (map) | -1: dense GEMM
  CONV_DIR,            // 0 forward, 1 backward-data
  CONV_OUT,
  CONV_N,              // (dim) rows, dense only | -1
  CONV_CIN,
  CONV_COUT,
  CONV_STATS_P1,       // the statistics table the epilogue leaves (column sums per row block)
  CONV_BN_X_P1,        // BatchNorm-backward form of the table (the layer's two reductions): the layer's input ...
  CONV_BN_MEAN,
  CONV_BN_VAR,
  CONV_BN_GAMMA,
  CONV_BN_BETA,
  CONV_BN_EPS,         // (f64)
  CONV_BN_ACT,
  CONV_BN_ADD_P1,      // ... an earlier gradient contribution added to OUT on the fly
  CONV_BN_Y_P1,        // ... the layer's output where act' needs it (a residual layer)
  CONV_AMAX_X_P1,      // the amax word of X (h3 split; none: the entry point makes its own pass)
  CONV_END
};
enum {  // BatchNorm (+ residual) + activation (+ the neck's sparse sum)
  BN_FWD_X = 2,
  BN_FWD_N,            // (dim)
  BN_FWD_C,
  BN_FWD_EPS,          // (f64)
  BN_FWD_GAMMA,
  BN_FWD_BETA,
  BN_FWD_RES,          // residual | -1
  BN_FWD_ACT,
  BN_FWD_MOMENTUM,     // (f64)
  BN_FWD_Y,
  BN_FWD_MEAN,         // saved batch statistics | -1 (eval)
  BN_FWD_VAR,
  BN_FWD_CNT,
  BN_FWD_RMEAN,
  BN_FWD_RVAR,
  BN_FWD_NBT,          // num_batches_tracked
  BN_FWD_TRAIN,        // 0: eval mode, the running statistics are the statistics
  BN_FWD_PRODUCER_P1,  // row index (this list) of the OP_CONV that wrote X and left its statistics table
  BN_FWD_GROUPS,       // column groups of that table per channel (1 | 8)
  BN_FWD_AMAX_Y_P1,    // the amax word the apply kernel folds max |y| into (y feeds a convolution)
  BN_FWD_ADD_INV_P1,   // inverse row map and ...
  BN_FWD_ADD_SRC_P1,   // ... tensor whose rows are added behind the activation: Y is the union then
  BN_FWD_END
};
enum {  // the packed head GEMM's output -> centerness, bbox, class scores, class maximum
  HEAD_FWD_Y = 2,
  HEAD_FWD_LD,
  HEAD_FWD_BIAS,
  HEAD_FWD_SCALE,
  HEAD_FWD_N,          // (dim)
  HEAD_FWD_N_REG,
  HEAD_FWD_N_CLS,
  HEAD_FWD_CENT,
  HEAD_FWD_BBOX,
  HEAD_FWD_CLS,
  HEAD_FWD_CMAX,
  HEAD_FWD_END
};
enum { RECORD_EVENT = 2, RECORD_END };   // event number, recorded on the row's stream
enum { WAIT_EVENT = 2, WAIT_END };       // event number, the row's stream waits for it
enum {
  HEAD_BWD_Y = 2,
  HEAD_BWD_LD,
  HEAD_BWD_SCALE,
  HEAD_BWD_BBOX,
  HEAD_BWD_G_CENT,
  HEAD_BWD_G_BBOX,
  HEAD_BWD_G_CLS,
  HEAD_BWD_N,          // (dim)
  HEAD_BWD_N_REG,
  HEAD_BWD_N_CLS,
  HEAD_BWD_GY,
  HEAD_BWD_GS_ROW,     // per-row d scale | -1: the scale / class-bias reductions of this level come out of the same pass
  HEAD_BWD_G_SCALE,
  HEAD_BWD_BIAS_PART,  // this level's column sums of d loss / d cls_score
  HEAD_BWD_AMAX_GY_P1,
  HEAD_BWD_END
};
enum {  // weight gradient on a kernel map or dense
  WGRAD_X = 2,
  WGRAD_GOUT,
  WGRAD_MAP,           // (map) | -1: dense
  WGRAD_GW,
  WGRAD_N,             // (dim) rows, dense only | -1
  WGRAD_CIN,
  WGRAD_COUT,
  WGRAD_AMAX_X_P1,
  WGRAD_AMAX_GOUT_P1,
  WGRAD_END
};
enum {
  BN_BWD_X = 2,
  BN_BWD_Y,            // the layer's output | -1 (no residual: act' is recomputed from X)
  BN_BWD_GY,
  BN_BWD_N,            // (dim)
  BN_BWD_C,
  BN_BWD_MEAN,
  BN_BWD_VAR,
  BN_BWD_CNT,
  BN_BWD_EPS,          // (f64)
  BN_BWD_GAMMA,
  BN_BWD_BETA,
  BN_BWD_ACT,
  BN_BWD_GX,
  BN_BWD_GRES,         // | -1
  BN_BWD_SUMS,         // d beta, d gamma (2, C)
  BN_BWD_GY2_P1,       // a second gradient contribution, added on the fly
  BN_BWD_PRODUCER_P1,  // row index (this list) of the backward-data OP_CONV that left this layer's two reductions
  BN_BWD_AMAX_GX_P1,
  BN_BWD_END
};
enum {
  STEM_WGRAD_COL = 2,
  STEM_WGRAD_GOUT,
  STEM_WGRAD_MAP,      // (map)
  STEM_WGRAD_GW,
  STEM_WGRAD_END
};
enum {  // dst[i] = src[idx[i]]
  GATHER_SRC = 2,
  GATHER_IDX,
  GATHER_N,            // (dim)
  GATHER_C,
  GATHER_DST,
  GATHER_END
};
enum {  // dst += src over n * C floats (C % 4 == 0)
  ADD_DST = 2,
  ADD_SRC,
  ADD_N,               // (dim)
  ADD_C,
  ADD_END
};
enum {  // the d gamma / d beta sums of the normalisation layers -> their gradient slices
  SMALL_GRADS_DESC = 2,  // descriptor array (device)
  SMALL_GRADS_FIRST,     // first entry
  SMALL_GRADS_COUNT,     // entries
  SMALL_GRADS_END
};
enum {  // (Cin, 8 Cout) -> (8, Cin, Cout)
  PERMUTE_GENT_SRC = 2,
  PERMUTE_GENT_DST,
  PERMUTE_GENT_CIN,
  PERMUTE_GENT_COUT,
  PERMUTE_GENT_END
};
enum {  // the packed head kernel's gradient: sum of the per-level partials, split into the three kernels (+ the class bias)
  HEAD_WFIN_PART = 2,
  HEAD_WFIN_NL,
  HEAD_WFIN_R,
  HEAD_WFIN_LD,
  HEAD_WFIN_N_REG,
  HEAD_WFIN_N_CLS,
  HEAD_WFIN_G_CENT,
  HEAD_WFIN_G_REG,
  HEAD_WFIN_G_CLS,
  HEAD_WFIN_BIAS_PART,  // | -1
  HEAD_WFIN_G_BIAS,     // | -1
  HEAD_WFIN_END
};
enum {
  COPY_DST = 2,
  COPY_SRC,
  COPY_N,              // (dim)
  COPY_C,
  COPY_END
};
enum {  // dst[c] = sum over rows of x[r][c]
  COL_SUM_X = 2,
  COL_SUM_N,           // (dim)
  COL_SUM_C,
  COL_SUM_DST,
  COL_SUM_END
};
enum {
  ROW_SUM_X = 2,
  ROW_SUM_N,           // (dim)
  ROW_SUM_DST,
  ROW_SUM_END
};
enum {  // max |x| over n * C floats -> slot word 0
  AMAX_X = 2,
  AMAX_N,              // (dim)
  AMAX_C,
  AMAX_SLOT,
  AMAX_END
};
enum {  // zero-fill (the amax words a pass's producers fold into)
  CLEAR_DST = 2,
  CLEAR_BYTES,
  CLEAR_END
};
enum {  // the stem's instance norm + activation + 2x2x2 max pool in one pass
  NORM_POOL_FWD_X = 2,
  NORM_POOL_FWD_SEG,   // | -1
  NORM_POOL_FWD_C,
  NORM_POOL_FWD_MEAN,
  NORM_POOL_FWD_VAR,
  NORM_POOL_FWD_EPS,   // (f64)
  NORM_POOL_FWD_GAMMA,
  NORM_POOL_FWD_BETA,
  NORM_POOL_FWD_ACT,
  NORM_POOL_FWD_MAP,   // (map) K = 8
  NORM_POOL_FWD_OUT,
  NORM_POOL_FWD_ARG,   // arg-max rows | -1 (with MASK_P1 only)
  NORM_POOL_FWD_Y,     // the normalised tensor, stored for `decisions` only | -1
  NORM_POOL_FWD_AMAX_OUT_P1,
  NORM_POOL_FWD_PARENT,  // child row -> pooled row, for the backward pass | -1
  NORM_POOL_FWD_MASK_P1, // per-child arg-max mask (8 bytes per input row), for the backward pass: ARG may then be -1 (fc_norm_act_maxpool8_mask_fwd)
  NORM_POOL_FWD_END
};
enum {  // ... and its backward: pool backward + instance-norm backward without the scattered gradient in between
  POOL_NORM_BWD_X = 2,
  POOL_NORM_BWD_G_POOL,
  POOL_NORM_BWD_ARG,   // | -1 (with MASK_P1 only)
  POOL_NORM_BWD_PARENT,
  POOL_NORM_BWD_SEG,   // | -1
  POOL_NORM_BWD_N,     // (dim)
  POOL_NORM_BWD_C,
  POOL_NORM_BWD_NSEG,  // (dim)
  POOL_NORM_BWD_MEAN,
  POOL_NORM_BWD_VAR,
  POOL_NORM_BWD_CNT,
  POOL_NORM_BWD_EPS,   // (f64)
  POOL_NORM_BWD_GAMMA,
  POOL_NORM_BWD_BETA,
  POOL_NORM_BWD_ACT,
  POOL_NORM_BWD_GX,
  POOL_NORM_BWD_SUMS,
  POOL_NORM_BWD_MASK_P1, // the forward's mask: read instead of ARG (fc_maxpool8_mask_norm_act_bwd)
  POOL_NORM_BWD_END
};
enum {  // inv = -1, inv[rows[i]] = i
  INV_ROWS_ROWS = 2,
  INV_ROWS_N,          // (dim)
  INV_ROWS_N_INV,      // (dim)
  INV_ROWS_INV,
  INV_ROWS_END
};
enum {  // the backward through a BatchNorm that reads its running statistics (fc_bn_eval_bwd): one pass, no producer table
  BN_EVAL_BWD_X = 2,
  BN_EVAL_BWD_Y,            // the layer's output | -1 (no residual: act' is recomputed from X)
  BN_EVAL_BWD_GY,
  BN_EVAL_BWD_N,            // (dim)
  BN_EVAL_BWD_C,
  BN_EVAL_BWD_RMEAN,
  BN_EVAL_BWD_RVAR,
  BN_EVAL_BWD_EPS,          // (f64)
  BN_EVAL_BWD_GAMMA,
  BN_EVAL_BWD_BETA,
  BN_EVAL_BWD_ACT,
  BN_EVAL_BWD_GX,
  BN_EVAL_BWD_GRES,         // | -1
  BN_EVAL_BWD_SUMS,         // d beta, d gamma (2, C) | -1 (gamma and beta frozen: no sums, no workspace)
  BN_EVAL_BWD_GY2_P1,       // a second gradient contribution, added on the fly
  BN_EVAL_BWD_AMAX_GX_P1,
  BN_EVAL_BWD_END
};

static_assert(STEM_FWD_END <= OPW && COL_STATS_END <= OPW && CONV_END <= OPW && BN_FWD_END <= OPW && HEAD_FWD_END <= OPW, "operator row");
static_assert(RECORD_END <= OPW && WAIT_END <= OPW && HEAD_BWD_END <= OPW && WGRAD_END <= OPW && BN_BWD_END <= OPW, "operator row");
static_assert(STEM_WGRAD_END <= OPW && GATHER_END <= OPW && ADD_END <= OPW && SMALL_GRADS_END <= OPW && PERMUTE_GENT_END <= OPW, "operator row");
static_assert(HEAD_WFIN_END <= OPW && COPY_END <= OPW && COL_SUM_END <= OPW && ROW_SUM_END <= OPW && AMAX_END <= OPW, "operator row");
static_assert(CLEAR_END <= OPW && NORM_POOL_FWD_END <= OPW && POOL_NORM_BWD_END <= OPW && INV_ROWS_END <= OPW, "operator row");
static_assert(BN_EVAL_BWD_END <= OPW && OP_BN_EVAL_BWD == OP_INV_ROWS + 1, "operator row; existing opcodes keep their numbers");

// ---- kernel-map descriptor (sparse.KernelMap.desc): device addresses as plain integers, 0 where a table is not built
enum {  // one group of exact pair lists, relative to MAP_PAIRS / MAP_PAIRS_T
  PAIR_IN,             // input row of every pair
  PAIR_OUT,            // output row
  PAIR_POS,            // start of every kernel offset's run
  PAIR_CNT,            // pairs per kernel offset
  PAIR_TILES,          // a plain integer: tiles of the per-offset launch (sparse.KernelMap.pair_tiles)
  PAIR_END
};
enum {
  MAP_N_IN,
  MAP_N_OUT,
  MAP_K,               // kernel offsets
  MAP_NBR,             // (n_out, K) input row per output row and offset
  MAP_NBR_T,           // the transposed table (backward-data)
  MAP_FWD_TAB,         // forward table in mask order and ...
  MAP_FWD_IDX,         // ... its row order | 0: MAP_FWD_TAB is the plain table
  MAP_BWD_TAB,         // the same for backward-data
  MAP_BWD_IDX,
  MAP_PAIRS,           // PAIR_* of the map (forward, weight gradient)
  MAP_PAIRS_T = MAP_PAIRS + PAIR_END,     // PAIR_* of the transposed map (backward-data)
  MAP_FLAGS = MAP_PAIRS_T + PAIR_END,     // MAP_ROUTE_* bits
  MAP_END
};
enum {  // which launches take the per-offset route over the pair lists
  MAP_ROUTE_FWD_PAIRS = 1,
  MAP_ROUTE_BWD_PAIRS = 2,
  MAP_ROUTE_WGRAD_PAIRS = 4
};
static_assert(MAP_END <= MAPW, "kernel-map descriptor");

#endif
