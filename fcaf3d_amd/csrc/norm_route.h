// Which launches a normalisation call becomes — decided once, as plain data, before anything is launched.  Host code only: the route functions are
// pure (no HIP call, no pointer, no global).  norm.hip computes a route per call, bn_fwd / norm_bwd map it to its kernels, the size queries return the same
// byte counts, fc_bn_train_fwd_route / fc_bn_train_bwd_route hand it out (include/fcaf3d_hip.h, FC_NROUTE_*).  Each rule stands beside its measurement.
#ifndef FC_NORM_ROUTE_H
#define FC_NORM_ROUTE_H
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"

#define MAXSEG 64
// row-block caps of the two-level reductions and of the kernels that re-reduce a table in their prologue
#define MAXBLOCKS 1024       // partial-sum blocks of a reduction whose table a finalize kernel adds
#define BN1_MAXB 64          // partial blocks an apply kernel re-reduces in its prologue (a few hundred KB out of L2): ONE launch less
#define AP_MAXB 256          // apply grid of the prologue-reducing kernels behind a producer's table
// finalize kernels (k_stats_final, k_bn2_finalize, k_seg_meanvar_final): a block is FIN_CB channels x FIN_SL slices of the table.
// r5: 4 channels x 64 slices = 256 threads per block (r1-r4: 64 channels x 16 slices = 1 024 threads).  These launches are pure
// latency, and a 1 024-thread workgroup needs four free wave slots on every SIMD of ONE compute unit: beside the weight-gradient
// stream (two resident 250-register workgroups per CU) it waited for a whole CU to drain — up to 1.8 ms for a 10 us kernel
// (rocprofv3, r5).  256-thread workgroups fit next to anything; 64 slices keep the chain per thread at nb / 256 loads.
#define FIN_CB 4
#define FIN_SL 64
struct RowBlocks { int64_t nb, rpb; };      // blocks, rows per block
// rows of a matrix over at most `cap` blocks of at least 64 rows; every block but the last gets rpb rows, none is empty
static inline RowBlocks row_blocks(int64_t n, int64_t cap) {
  const int64_t m = n > 0 ? n : 1;
  int64_t g = fc_cdiv(m, 64);
  if (g > cap) g = cap;
  const int64_t rpb = fc_cdiv(m, g);
  return {fc_cdiv(m, rpb), rpb};
}
// block of the row-blocked kernels: a thread per four channels, up to 16 row lanes, at most 256 threads; false: C is refused
struct StatsGeometry { int threads; size_t lds_fwd, lds_bwd; };
static inline bool stats_geometry(int C, StatsGeometry* g) {
  if (C < 4 || C % 4 || C > 1024) return false;
  const int c4n = C / 4;
  int nrl = 256 / c4n;
  if (nrl < 1) nrl = 1;
  if (nrl > 16) nrl = 16;
  g->threads = nrl * c4n;
  g->lds_fwd = (size_t)(nrl * C + nrl) * sizeof(float);
  g->lds_bwd = (size_t)(nrl * 2 * C) * sizeof(float);
  return true;
}
// channel window of the prologue-reducing apply kernels: with few row blocks (the deep levels: 872 x 512, 3.5k x 256) a block owns 64
// channels and the grid's y dimension walks the windows — 8x the blocks, 16 row lanes each, the SAME total table traffic; else all of C
// (r6: 872 x 512 used to be 14 blocks of 2 row lanes, 49 us)
static inline int ap_window(int64_t n, int C) {
  const int64_t g = fc_cdiv(n > 0 ? n : 1, 64);
  return (C >= 128 && C % 64 == 0 && g * (C / 64) <= 1024 && g < 128) ? 64 : C;
}
// partial sums in the workspace: [blocks][nseg][2][C] floats (sums of x and x^2, or of g' and g' xhat)
static inline int64_t part_bytes(int64_t blocks, int C, int nseg) { return blocks * nseg * 2 * (int64_t)C * (int64_t)sizeof(float); }
static inline int64_t small_ws_bytes(int C) { return part_bytes(BN1_MAXB, C, 1); }      // the two-launch routes: room for the cap, whatever n
static inline int64_t reduce_ws_bytes(int64_t n, int C, int nseg) { return part_bytes(row_blocks(n, MAXBLOCKS).nb, C, nseg); }
struct NormLaunch { unsigned grid_x, grid_y; int threads; size_t lds; };      // threads 0: not launched
// k_norm_act_fwd / k_norm_bwd_apply: a thread per four channels of a row
static inline NormLaunch rows_launch(int64_t n, int C) { return {(unsigned)fc_cdiv(n * (C / 4), 256), 1, 256, 0}; }
static inline NormLaunch final_launch(int nseg, int cols) { return {(unsigned)(nseg * ((cols + FIN_CB - 1) / FIN_CB)), 1, FIN_CB * FIN_SL, 0}; }

struct NormRoute {             // field by field the out[] of fc_bn_train_fwd_route / fc_bn_train_bwd_route
  int sums;                    // who makes the per-block sums: forward FC_NSTATS_*, backward FC_NRED_*; 0 (INVALID): the call returns FC_EINVAL
  int apply;                   // forward FC_NAPPLY_*, backward FC_NBAPPLY_*: the kernel(s) behind the sums
  int amax;                    // FC_NAMAX_*: where max |y| / max |gx| is taken when the caller left a word
  int64_t np, red_rpb;         // blocks of the table of sums (the producer's, or those of k_bn1_partial / k_norm_bwd_partial with its rows per block)
  int64_t nb, rpb;             // row blocks and rows per block of the prologue-reducing apply kernel (k_bn1_apply, k_bn2_apply, k_bn1_bwd_apply)
  int cg;                      // channels a block of that kernel owns (ap_window)
  NormLaunch red, fin, ap;     // the partial-sum kernel; the finalize kernel; the apply kernel
  int64_t ws_bytes;
};
// what an entry point answers before it launches: FC_EINVAL for a refused call, FC_EWS for a short workspace (no partial sums: none is looked at)
static inline int route_check(const NormRoute& r, int64_t ws_bytes) { return !r.sums ? FC_EINVAL : (r.ws_bytes && ws_bytes < r.ws_bytes) ? FC_EWS : FC_OK; }

// fc_bn_train_fwd / fc_bn_train_add_fwd.  has_part: nb_part row blocks of producer-written column sums; else the statistics are computed
// from x: up to small_elems elements (the callers' BN_SMALL_ELEMS = 1 M) by the two-launch route (measured r1: equal speed up to 1 M
// elements, fewer host launches; at 4 M the <= 64-block grid is slower than the general path).  fc_bn_act_train_fwd is this route with
// small_elems = INT64_MAX, fc_bn_stats_train the statistics step of small_elems = -1.
static inline NormRoute norm_fwd_route(int64_t n, int C, bool has_part, int64_t nb_part, int groups, int64_t small_elems) {
  NormRoute r = {};
  StatsGeometry g;
  if (n < 1 || !stats_geometry(C, &g)) return r;
  r.cg = C, r.amax = FC_NAMAX_FOLDED;
  if (has_part) {
    if (nb_part < 1 || nb_part > 0x7fffffff / 64 || groups < 1 || groups > 64) return r;
    r.np = nb_part;
    if (nb_part > BN1_MAXB) {      // a table too long for a prologue: k_bn2_finalize adds it once
      r.sums = FC_NSTATS_TABLE, r.fin = final_launch(1, C);
      r.apply = FC_NAPPLY_ROWS, r.ap = rows_launch(n, C);
      return r;
    }
    // ONE launch: every block of k_bn2_apply re-reduces the table (fp64) and applies to its rows
    const RowBlocks b = row_blocks(n, AP_MAXB);
    r.sums = FC_NSTATS_PROLOGUE, r.apply = FC_NAPPLY_BN2, r.nb = b.nb, r.rpb = b.rpb, r.cg = ap_window(n, C);
    stats_geometry(r.cg, &g);
    r.ap = {(unsigned)b.nb, (unsigned)(C / r.cg), g.threads, (size_t)(g.threads / (r.cg / 4)) * 2 * r.cg * sizeof(double)};
    return r;
  }
  const bool small = n * C <= small_elems;
  const RowBlocks b = row_blocks(n, small ? BN1_MAXB : MAXBLOCKS);
  r.np = b.nb, r.red_rpb = b.rpb;
  r.red = {(unsigned)b.nb, 1, g.threads, g.lds_bwd};
  if (small) {      // k_bn1_apply does not fold the amax: a pass of its own
    r.sums = FC_NSTATS_PARTIAL_SMALL, r.apply = FC_NAPPLY_BN1, r.amax = FC_NAMAX_PASS, r.nb = b.nb, r.rpb = b.rpb, r.ap = r.red;
    r.ws_bytes = small_ws_bytes(C);
    return r;
  }
  r.sums = FC_NSTATS_PARTIAL, r.fin = {(unsigned)((C + 63) / 64), 1, 1024, 0};      // k_bn_finalize: 64 channels x 16 slices
  r.apply = FC_NAPPLY_ROWS, r.ap = rows_launch(n, C);
  r.ws_bytes = reduce_ws_bytes(n, C, 1);
  return r;
}

// form (FC_NFORM_*): TRAIN fc_bn_train_bwd; SMALL fc_bn_act_train_bwd, the two-launch route whatever the size, every block all of C; SEG
// fc_norm_act_bwd and, over its n_in rows, fc_maxpool8_norm_act_bwd: nseg segments, always through k_stats_final (n == 0: the sums are
// zero-filled).  has_part (TRAIN): nb_part blocks [2][C] from gy's producer.
static inline NormRoute norm_bwd_route(int64_t n, int C, int nseg, bool has_part, int64_t nb_part, int64_t small_elems, int form) {
  NormRoute r = {};
  const bool seg = form == FC_NFORM_SEG;
  StatsGeometry g;
  if (n < (seg ? 0 : 1) || nseg < 1 || nseg > (seg ? MAXSEG : 1) || !stats_geometry(C, &g)) return r;
  r.cg = C, r.amax = FC_NAMAX_FOLDED;
  if (form == FC_NFORM_TRAIN && has_part) {
    if (nb_part < 1) return r;
    r.sums = FC_NRED_TABLE, r.np = nb_part;
  } else {
    const bool small = form == FC_NFORM_SMALL || (form == FC_NFORM_TRAIN && n * C <= small_elems);
    const RowBlocks b = row_blocks(n, small ? BN1_MAXB : MAXBLOCKS);
    r.sums = FC_NRED_PARTIAL, r.np = b.nb, r.red_rpb = b.rpb;
    r.ws_bytes = small ? small_ws_bytes(C) : reduce_ws_bytes(n, C, nseg);
    if (n == 0) return r;      // (apply FC_NBAPPLY_NONE)
    r.red = {(unsigned)b.nb, 1, g.threads, g.lds_bwd};
  }
  if (!seg && r.np <= BN1_MAXB) {
    // every block of k_bn1_bwd_apply re-reduces the table and applies: behind a producer's table up to AP_MAXB blocks, behind our
    // own partial launch its blocks
    const RowBlocks b = row_blocks(n, r.sums == FC_NRED_TABLE ? AP_MAXB : BN1_MAXB);
    r.apply = FC_NBAPPLY_PROLOGUE, r.nb = b.nb, r.rpb = b.rpb;
    if (form == FC_NFORM_TRAIN) r.cg = ap_window(n, C);
    stats_geometry(r.cg, &g);
    r.ap = {(unsigned)b.nb, (unsigned)(C / r.cg), g.threads, g.lds_bwd};
    return r;
  }
  r.apply = FC_NBAPPLY_FINAL, r.fin = final_launch(nseg, 2 * C), r.ap = rows_launch(n, C);
  return r;
}

// fc_bn_eval_bwd: the backward through a BatchNorm that reads its running statistics (norm_eval.h).  gx needs no sum, so there is one pass over the
// rows whatever the size.  want_sums false (gamma and beta frozen): k_bn_eval_bwd on the geometry of k_norm_act_fwd, no workspace.  want_sums: the
// same kernel row-blocked as k_norm_bwd_partial (over channel windows where the row blocks are few, ap_window), leaving [nb][1][2][C] partial sums
// that k_stats_final adds in a fixed order.  n == 0: nothing
// but the zero fill of the sums.
static inline NormRoute norm_eval_bwd_route(int64_t n, int C, bool want_sums) {
  NormRoute r = {};
  StatsGeometry g;
  if (n < 0 || !stats_geometry(C, &g)) return r;
  r.cg = C, r.amax = FC_NAMAX_FOLDED;
  r.sums = want_sums ? FC_NRED_PARTIAL : FC_NRED_NONE;
  if (n == 0) return r;      // (apply FC_NBAPPLY_NONE)
  r.apply = FC_NBAPPLY_ROWS;
  if (!want_sums) {
    r.ap = rows_launch(n, C);
    return r;
  }
  const RowBlocks b = row_blocks(n, MAXBLOCKS);
  r.np = r.nb = b.nb, r.red_rpb = r.rpb = b.rpb;
  r.cg = ap_window(n, C);      // few row blocks: a block owns 64 channels, grid.y walks the windows
  stats_geometry(r.cg, &g);
  r.ap = {(unsigned)b.nb, (unsigned)(C / r.cg), g.threads, g.lds_bwd};
  r.fin = final_launch(1, 2 * C);
  r.ws_bytes = reduce_ws_bytes(n, C, 1);
  return r;
}
#endif
