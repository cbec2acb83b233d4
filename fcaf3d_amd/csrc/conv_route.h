// Which launch a convolution call becomes — decided once, as plain data, before anything is launched.  Host code only: the route
// functions are pure (no HIP call, no pointer, no global; the process-global switches arrive in a RouteEnv filled once per entry
// point).  conv.hip computes a route per call, launch_conv / launch_wgrad map it to a template instantiation, the size queries read
// S / the tile / the epilogue from it, and fc_conv_fwd_route / fc_conv_wgrad_route hand it out (include/fcaf3d_hip.h, FC_ROUTE_*).
// The measurements behind each rule stand beside the rule.
#ifndef FC_CONV_ROUTE_H
#define FC_CONV_ROUTE_H
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"

struct RouteEnv { int split_mode, bf16_fast, h3r; };      // fc_get_split_mode (0 while bf16_fast), fc_set_bf16_fast, fc_debug_set_h3r
struct ConvShape { int64_t n_in, n_out; int K, Cin, Cout; };

struct ConvRoute {           // forward / backward-data; field by field the out[] of fc_conv_fwd_route
  int family;                // FC_FAM_*, FC_FAM_INVALID: the call returns FC_EINVAL
  int bm, bn, wm;            // tile rows x columns, waves along the rows
  int S;                     // partial sums in the workspace: offset split of a table launch, K for pair lists; 1 = written in place
  int wsrc, mode, buf, epi;  // FC_WSRC_*, FC_MODE_*, buffer (1) or flat (0) addressing, FC_EPI_*: where a statistics epilogue runs
  unsigned grid[3];
};
struct WgradRoute {          // weight gradient; the out[] of fc_conv_wgrad_route
  int family;                // FC_WFAM_*
  int bm, bn, ko, bkr;       // Cin x Cout tile, offsets per workgroup, rows per chunk
  int table, mode, S;        // FC_TABLE_*, FC_MODE_*, row ranges = partial gradients (1: written in place)
  int64_t rps;               // rows per range
  int wbuf;                  // k_wgrad_x6t: both operands through buffer descriptors
  unsigned grid_y;
};

static inline int flag_bm(int flags) { return (flags >> FC_CONV_BM_SHIFT) & FC_CONV_TILE_MASK; }      // tuning overrides, 0 = the route's choice
static inline int flag_bn(int flags) { return (flags >> FC_CONV_BN_SHIFT) & FC_CONV_TILE_MASK; }
static inline int flag_s(int flags) { return (flags >> FC_CONV_S_SHIFT) & FC_CONV_S_MASK; }
static inline bool below_2gb(uint64_t bytes) { return bytes < (1ull << 31) - 4096u; }        // what one buffer descriptor spans

// the stem convolution's shape (k_stem_fwd / k_stem_wgrad: 3 -> 64 channels, up to 27 offsets), both directions
static inline bool stem_shape(int K, int Cin, int Cout, int flags) { return !(flags & FC_CONV_FMA) && Cin == 3 && Cout == 64 && K <= 27; }

// split over kernel offsets: the LARGEST split that still fits one resident round (1024 workgroup slots) — one workgroup
// over (r1 rounded up) starts a second, nearly empty round (r2 sweep: 256->256 on 6.9k rows 275 us at S = 10 -> 238 at
// S = 9); from ~400 tiles on the unsplit launch wins (64->64 on 64k rows: 159 us at S = 2 -> 144 at S = 1, and no
// partial tiles to write and sum)
static inline int offset_split(int64_t tiles, int K) {
  if (K <= 1 || tiles >= 384) return 1;          // (r5 sweep with the split-bf16 kernels: 256 / 512 / 768 change nothing, 368.1-368.5 scenes/s)
  return (int)(1024 / tiles < K ? 1024 / tiles : K);
}

// table: FC_TABLE_* (| FC_TABLE_STATS: the caller wants the statistics epilogue); live_tiles > 0: the linear pair-list launch
static inline ConvRoute conv_route(const ConvShape& s, int flags, int table, int64_t live_tiles, const RouteEnv& env) {
  const bool stats = (table & FC_TABLE_STATS) != 0;
  table &= ~FC_TABLE_STATS;
  const bool pairs = table == FC_TABLE_PAIRS, gather = table != FC_TABLE_NONE, split = (flags & FC_CONV_SPLIT) != 0;
  const bool image = split && (flags & FC_CONV_IMAGE);       // W is a pre-split image: already the operator of its direction, FC_CONV_WT or not
  const bool wt = (flags & FC_CONV_WT) && !image;            // W[k] given as (Cout, Cin): the backward-data pass on the layer's own kernel
  const int64_t n = s.n_out > 0 ? s.n_out : 1;
  const int K = s.K, Cin = s.Cin, Cout = s.Cout;
  ConvRoute r = {};
  r.family = FC_FAM_INVALID;
  r.wsrc = image ? FC_WSRC_IMAGE : wt ? FC_WSRC_FP32_T : FC_WSRC_FP32;
  if (!gather && (K != 1 || s.n_in != s.n_out)) return r;
  if ((flags & FC_CONV_WT) && !gather) return r;             // transposed weights: neighbour-table / pair-list launches only
  // the MFMA kernels' shapes (32-deep slabs, 64-column tiles); a table launch keeps all offsets of a tile in one workgroup
  const bool mfma = Cin % 32 == 0 && Cout % 64 == 0 && (pairs || (!(flags & FC_CONV_FMA) && K <= 32));
  if (pairs && !mfma) return r;                              // MFMA shapes only; callers use fc_conv_fwd otherwise
  if (stats && !(mfma && split)) return r;                   // the statistics epilogue lives in the split-bf16 route
  // ---- tile and offset split
  r.bn = (Cout % 128 == 0) ? 128 : 64;
  if (pairs) {
    // (r5, measured null: 64-column tiles for the few-thousand-row pair-list launches — 4 workgroups per CU, finer rounds — 373.6 /
    // 372.5 / 372.2 scenes/s at <= 1k / 4k / 16k rows against 375.4: profiles/r5_notes.md)
    if (flag_bn(flags) == 1) r.bn = 64;
    r.bm = 128;
    r.S = K;                                                  // per offset a compacted gather-GEMM into the workspace, then a gather-sum
  } else {
    // measured on the benchmark's layers (tools/convbench.py): 128-row tiles win at every size once the grid
    // is topped up to ~1024 workgroups by splitting over kernel offsets
    r.bm = (n > 64 && fc_cdiv(n, 128) * (Cout / r.bn) >= 4) ? 128 : 64;
    // 64-wide outputs on big maps: 256 x 64 tiles, 4 waves along the rows (r2: +6 % on the 441k-row level, 88 / 95 TF)
    if (Cout == 64 && fc_cdiv(n, 256) >= 1024 && !split) r.bm = 256;      // (split-bf16: 128 x 64 at 4 waves / SIMD is ahead, 613 vs 628 us)
    const int fbm = flag_bm(flags), fbn = flag_bn(flags);     // tuning overrides: BM (1=64, 2=128, 3=256), BN (1=64, 2=128), S
    if (fbm) r.bm = fbm == 1 ? 64 : (fbm == 2 ? 128 : 256);
    if (fbn && (Cout % (fbn == 1 ? 64 : 128) == 0)) r.bn = fbn == 1 ? 64 : 128;
    if (r.bm == 256) r.bn = 64;                               // the 4 x 1 wave arrangement: 256 x 64 tiles
    if (split && mfma && r.bm == 64) r.bm = 128;              // the split-bf16 kernel has 128- and 256-row tiles only
    r.S = mfma ? offset_split(fc_cdiv(n, r.bm) * (Cout / r.bn), K) : 1;
    if (flag_s(flags)) r.S = flag_s(flags) > K ? K : flag_s(flags);
  }
  r.wm = r.bm == 256 ? 4 : 2;
  if (stem_shape(K, Cin, Cout, flags) && !(flags & FC_CONV_WT) && table == FC_TABLE_DENSE) { r.family = FC_FAM_STEM; return r; }
  if (!mfma && table != FC_TABLE_SORTED && !(flags & FC_CONV_IMAGE)) r.family = FC_FAM_FMA;      // sorted-row tables and weight images are MFMA-path features
  if (!mfma) return r;
  r.grid[0] = (unsigned)fc_cdiv(n, r.bm), r.grid[1] = (unsigned)(Cout / r.bn), r.grid[2] = (unsigned)r.S;
  if (pairs && live_tiles > 0) r.grid[0] = (unsigned)live_tiles, r.grid[2] = 1;      // linear list of the live (offset, tile) pairs
  // ---- kernel family
  if (split) {
    // split-bf16 kernel (conv_x6.h); the arithmetic follows the image: bf16-fast reads plane 0 of a six-product image (128-row tiles)
    r.family = FC_FAM_X6;
    r.mode = !image ? FC_MODE_SIX : (env.bf16_fast && r.bm == 128) ? FC_MODE_BF16 : env.split_mode == 2 ? FC_MODE_H3 : FC_MODE_SIX;
    // r6: h3 launches on 128 x 128 tiles take the register-operand kernel (conv_h3r.h): +1...11 % per launch there (tools/nbench, same
    // box), while the 64-column tiles LOSE 7-14 % on the 441k-row maps — a lane-per-row load touches 32 cache lines per instruction
    // where the LDS staging touches 8, and those launches are bound by the gather.  fc_debug_set_h3r: 0 never, 1 (default)
    // 128-column tiles, 2 every 128-row tile.
    if (r.mode == FC_MODE_H3 && r.bm == 128 && (env.h3r == 2 || (env.h3r == 1 && r.bn == 128))) r.family = FC_FAM_H3R;
    // buffer addressing (k_conv_x6 BUF, k_conv_h3r; gathering launches on a weight image, 128-row tiles): the gathered operand must end
    // below the 2 GB its descriptor spans (r6: the neighbour table goes through a descriptor too); FC_CONV_FLAT: flat addresses
    r.buf = image && gather && r.bm == 128 && r.mode != FC_MODE_BF16 && !(flags & FC_CONV_FLAT) &&
            below_2gb((uint64_t)s.n_in * (uint64_t)Cin * 4u) && below_2gb((uint64_t)K * (uint64_t)s.n_out * 4u);
    r.epi = (pairs || r.S > 1) ? FC_EPI_SUM : FC_EPI_KERNEL;
    return r;
  }
  // The deeper-pipelined LDS kernel (k_conv_mfma_p) holds 3 workgroups per CU (768 slots) where k_conv_mfma holds 4 (1024): it
  // wins on launches of many rounds and on launches that fit 768 slots anyway, and loses a round in between (r2: +5.5 / +7 %
  // on the 441k / 55k-row levels, +5 % on the 862-row pair mode, -12 % on the 3.5k-row pair mode with its 972 workgroups).
  // FC_CONV_PIPE_ON forces it on, FC_CONV_PIPE_OFF off.  FC_CONV_GLDS: the LDS-DMA kernel (k_conv_glds, 2 workgroups per CU) instead.
  const int64_t wgs = (int64_t)r.grid[0] * r.grid[1] * r.grid[2];
  r.mode = FC_MODE_FP32;
  if (flags & FC_CONV_GLDS) r.family = FC_FAM_GLDS;
  else if (flags & FC_CONV_PIPE_ON) r.family = FC_FAM_MFMA_P;
  else if ((flags & FC_CONV_PIPE_OFF) || (pairs && live_tiles <= 0)) r.family = FC_FAM_MFMA;      // (the per-offset pair grid: flags only)
  else if (wgs >= 1536 || wgs <= 768) r.family = FC_FAM_MFMA_P;
  // in between: offset-split launches of a dense table go to the LDS-DMA kernel (r2 nbench, same box: 6.9k rows 256->256
  // 251 -> 232 us, 256->128 139 -> 128 us, 14.9k rows 128->128 163 -> 146 us; unsplit and pair-list launches: neutral)
  else r.family = (r.grid[2] > 1 && !(flags & FC_CONV_GLDS_OFF)) ? FC_FAM_GLDS : FC_FAM_MFMA;
  if (r.family == FC_FAM_GLDS && wt) r.family = FC_FAM_MFMA;        // the LDS-DMA image cannot be transposed in flight
  if (r.bm == 64) r.family = FC_FAM_MFMA;                           // 64-row tiles: k_conv_mfma only
  return r;
}

// several offsets per workgroup (k_wgrad_multi): every dense table with >= 4096 rows (r2 nbench, one-offset kernel -> multi:
// 55k rows 128->128 504 -> 446 us, 6.9k rows 256->256 278 -> 247, 256->128 148 -> 135, 441k rows 128->64 2121 -> 2003, 64->64
// 1086 -> 1051); FC_CONV_WGRAD_MULTI_OFF disables it, FC_CONV_WGRAD_MULTI_FIRST restricts it to its first rule (Cin = 64, >= 32768 rows)
#define WGRAD_KO 3

static inline WgradRoute wgrad_route(const ConvShape& s, int flags, int table, const RouteEnv& env) {
  const int64_t n = s.n_out > 0 ? s.n_out : 1;
  const int K = s.K, Cin = s.Cin, Cout = s.Cout, fbm = flag_bm(flags), fbn = flag_bn(flags);
  const bool dense = table == FC_TABLE_DENSE, pairs = table == FC_TABLE_PAIRS, split = (flags & FC_CONV_SPLIT) != 0;
  if (pairs) flags &= ~FC_CONV_WGRAD_DEEP;                   // (a table option)
  WgradRoute r = {};
  r.family = FC_WFAM_INVALID;
  r.table = table, r.ko = 1, r.bkr = 32, r.mode = FC_MODE_FP32;
  if (table == FC_TABLE_SORTED || (table == FC_TABLE_NONE && (K != 1 || s.n_in != s.n_out))) return r;
  const bool mfma = !(flags & FC_CONV_FMA) && Cin % 64 == 0 && Cout % 64 == 0;
  if (pairs && !mfma) return r;                              // pair lists are an MFMA-path feature
  if (stem_shape(K, Cin, Cout, flags)) {                     // stem: 1024 rows per block (r2: 512 rows per block is slower — more partial tiles to write and reduce)
    r.family = dense ? FC_WFAM_STEM : FC_WFAM_FMA;
    r.rps = 1024, r.S = (int)fc_cdiv(n, 1024), r.grid_y = dense ? 1 : (unsigned)K;
    return r;
  }
  const bool multi = dense && mfma && !(flags & FC_CONV_WGRAD_MULTI_OFF) && K % WGRAD_KO == 0 && n >= 4096 &&
                     (!(flags & FC_CONV_WGRAD_MULTI_FIRST) || (Cin == 64 && n >= 32768));
  // split-bf16 weight gradients: rows loaded 16 B per lane and transposed by ds_read_b64_tr_b16 (k_wgrad_x6t, r4; the register
  // transposition of r3, k_wgrad_x6, is gone since r5), every pair-list and table-free dense shape included; the dense tables that
  // do not qualify for several offsets per workgroup stay on the fp32 kernels
  const bool x6t = mfma && split && (multi || !dense);
  const int wide = (Cout % 128 == 0) ? 128 : 64;
  // ---- tile the row split is sized on
  r.bm = 64;                                                 // measured: 64-channel Cin tiles beat 128 on every benchmark layer
  r.bn = wide;
  if (fbm == 2 && Cin % 128 == 0) r.bm = 128;                // tuning overrides
  if (fbn == 1) r.bn = 64;
  if (fbn == 2 && Cout % 128 == 0) r.bn = 128;
  if (split && !dense && Cin % 128 == 0) r.bm = 128;         // split-bf16 pair-list / table-free kernel: 128-channel tiles
  // aim for ~1728 workgroups (r2 sweep: 2048 rounded UP left a nearly empty last round on most layers — 128->128 on 55k
  // rows 559 us at 38 splits, 448 at 32), at least 512 rows per split, at most 256 splits
  int64_t sp = 1728 / (mfma ? (int64_t)K * (Cin / r.bm) * (Cout / r.bn) : (int64_t)K);      // (same-box A/B in the full step: neutral, 230.3 vs 230.9 scenes/s; kept: fewer partial tiles)
  if (multi) {
    // uniform long workgroups: exactly one resident round (3 per CU), fewer partial gradients to write and re-read.
    // r4 A/B in the full step (weight gradients beside the dependent chain): 3/4 of a resident round 22.91 ms, a full round
    // (r3) 23.34, half 23.70, a quarter 28.63, two rounds 23.25 — the main stream's kernels find a slot sooner.  With the
    // transposing-read kernel (k_wgrad_x6t, 1.4x faster per launch) half a round of the wide variant is ahead: 256 / 512
    // 22.26-22.35 ms, 192 / 512 22.41, 384 / 512 22.65, 128 / 512 23.36 (same box)
    constexpr int round_wide = 256, round_narrow = 512;      // the 128-column variant holds 2 workgroups per CU (registers)
    sp = (wide == 128 ? round_wide : round_narrow) / ((int64_t)(K / WGRAD_KO) * (Cin / 64) * (Cout / wide));
  }
  const int64_t max_by_rows = fc_cdiv(n, mfma ? 512 : 2048);
  sp = sp > max_by_rows ? max_by_rows : sp;
  sp = sp > 256 ? 256 : sp < 1 ? 1 : sp;
  if (flag_s(flags)) sp = flag_s(flags);                     // tuning override
  r.rps = fc_align(fc_cdiv(n, sp), 64);
  r.S = (int)fc_cdiv(n, r.rps);
  // ---- kernel family and the tile it launches
  if (!mfma) { r.family = FC_WFAM_FMA, r.grid_y = (unsigned)K; return r; }
  if (x6t) {
    r.family = FC_WFAM_X6T;
    // h3 (conv_x6.h): both operands split into two fp16 pieces, scaled by their amax words
    r.mode = env.bf16_fast ? FC_MODE_BF16 : env.split_mode == 2 ? FC_MODE_H3 : FC_MODE_SIX;
    r.bn = wide;                                             // (no column override on the split kernels)
    if (multi) r.bm = 64, r.ko = WGRAD_KO;
    // split-bf16 over the pair lists (r3 nbench: 128 x 128 tiles 119 -> 95 us on 15k rows 128->128, 111 -> 89 / 109 -> 87 on
    // the 256- and 512-channel levels; 64 x 64 tiles — one accumulator per wave, a dependent MFMA chain — lost to the fp32
    // kernel with the r3 kernel and win with k_wgrad_x6t).  128-channel Cin tiles only while they still fill the
    // chip (862 rows, 512->128: 216 workgroups of 128 x 128 tiles 49 us, fp32 36 us); the table-free dense GEMM gW = in^T gout
    // over the rows (K = 1) is the same kernel with the row itself as the index
    else if (r.bm == 128 && r.bn == 128 && (int64_t)r.S * K * (Cin / 128) * (Cout / 128) < 512) r.bm = 64;
    // buffer addressing of both operands (wgrad_x6.h): below 2 GB each, row indices below 2^24; FC_CONV_FLAT: flat addresses (A/B, tests)
    r.wbuf = !(flags & FC_CONV_FLAT) && below_2gb((uint64_t)s.n_in * (uint64_t)Cin * 4u) && below_2gb((uint64_t)s.n_out * (uint64_t)Cout * 4u) &&
             s.n_in < (1 << 24) && s.n_out < (1 << 24) && below_2gb((uint64_t)K * (uint64_t)s.n_out * 4u);
  } else if (multi) {
    r.family = FC_WFAM_MULTI, r.bm = 64, r.bn = wide, r.ko = WGRAD_KO;
  } else {
    if (pairs) r.bm = 64;
    // k_wgrad_mfma_p where it measured ahead (r2 nbench, same box: pair lists with 128-wide gout tiles +3..7 %; 64-wide
    // tiles -5 %, dense tables -7..13 %).  FC_CONV_WGRAD_PIPE_OFF: never, _ON: wherever it applies (tests / A-B).
    const bool wpipe = r.bm == 64 && !(flags & FC_CONV_WGRAD_DEEP) && !(flags & FC_CONV_WGRAD_PIPE_OFF) &&
                       ((flags & FC_CONV_WGRAD_PIPE_ON) || (pairs && r.bn == 128));
    r.family = wpipe ? FC_WFAM_MFMA_P : FC_WFAM_MFMA;
    if (!wpipe && dense && (flags & FC_CONV_WGRAD_DEEP) && r.bm == 64) r.bkr = 64;      // 64-row chunks (tuning flag)
  }
  r.grid_y = (unsigned)((K / r.ko) * (Cin / r.bm) * (Cout / r.bn));
  return r;
}
#endif
