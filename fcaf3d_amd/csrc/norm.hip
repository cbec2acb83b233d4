// Bandwidth-bound feature-matrix ops on gfx950: segmented column statistics (BatchNorm over all
// voxels / InstanceNorm per scene), fused normalise + affine + residual + ReLU/ELU forward and
// backward, max pooling over the k2s2 kernel map, row gather / scatter.
// All reductions are two-level with a fixed summation order (deterministic, no float atomics).
//
// Replaces MinkowskiBatchNorm / MinkowskiInstanceNorm / MinkowskiReLU / MinkowskiELU /
// MinkowskiMaxPooling / MinkowskiPruning feature paths used at me_resnet.py:22-24,63,
// BasicBlock (MinkowskiEngine.modules.resnet_block), fcaf3d_neck_with_head.py:53-54,67-71,76,125.
// This file is the host side: a route (norm_route.h) to its launches, and the entry points.  The kernels live in headers by family.
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "norm_route.h"      // every launch's geometry, the row-block caps, FIN_CB x FIN_SL
#include "norm_elem.h"       // segment of a row, activations, pre-activation, the blocks the kernels share
#include "norm_stats.h"      // k_stats_partial, k_seg_meanvar_final, k_stats_final
#include "norm_rows.h"       // k_norm_act_fwd, k_norm_bwd_partial, k_norm_bwd_apply
#include "norm_bn.h"         // k_bn1_partial / _apply / _bwd_apply, k_bn_finalize, k_bn2_apply / _finalize, k_bn_running
#include "norm_eval.h"     // k_bn_eval_bwd
#include "pool_rows.h"       // k_maxpool_fwd / 8_fwd / _bwd, k_norm_act_maxpool8_fwd, k_inverse_rows, k_gather_rows, k_scatter_rows_add

// ---- r6: max |.| of what a kernel writes, for the convolution that will gather it (csrc/conv_x6.h h3: the operand's scale) ----------
// A producer that is told where (fc_amax_out_hint -> amax_out, a ZEROED slot of FC_AMAX_SUB sub-words) folds the finite elements it
// stores into one integer atomicMax per block on its block's sub-word — skipped when that already holds a larger value — instead of
// the consumer reading the tensor once more (fc_amax).  Integer max: order-independent, bit-reproducible.  EVERY lane of the wave must reach amax_commit.
thread_local unsigned* t_fc_amax_out = nullptr;          // fc_amax_out_hint: consumed by the next producer entry point of this thread (fc_common.h)

// ---- a route (norm_route.h) to its launches ------------------------------------------------------------------------------------------
#define FC_GRID(l, stream) dim3((l).grid_x, (l).grid_y), (l).threads, (l).lds, stream

// fc_bn_train_fwd / fc_bn_train_add_fwd / fc_bn_act_train_fwd, and with apply == false fc_bn_stats_train: the argument checks, the route, its
// workspace, its launches.  table: the producer's [nb_part][2][groups * C]; amax (nullable): max |y| into the caller's (zeroed) word
static int bn_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta, const float* residual, int act, float momentum,
                  float* y, float* mean, float* var, float* cnt, float* rmean, float* rvar, long long* nbt, const float* table, int64_t nb_part, int groups,
                  int64_t small_elems, const int* add_inv, const float* add_src, void* ws, int64_t ws_bytes, hipStream_t stream, unsigned* amax,
                  bool apply = true) {
  if (act < 0 || act > 2 || (add_inv == nullptr) != (add_src == nullptr)) return FC_EINVAL;
  const NormRoute r = norm_fwd_route(n, C, table != nullptr, nb_part, groups, small_elems);
  if (int rc = route_check(r, ws_bytes)) return rc;
  float* part = (float*)ws;
  if (r.red.threads) { k_bn1_partial<<<FC_GRID(r.red, stream)>>>(x, n, C, r.red_rpb, part); FC_CHECK_LAUNCH(); }
  if (r.fin.threads) {
    if (r.sums == FC_NSTATS_PARTIAL) k_bn_finalize<<<FC_GRID(r.fin, stream)>>>(part, (int)r.np, C, n, x, momentum, mean, var, cnt, rmean, rvar, nbt);
    else k_bn2_finalize<<<FC_GRID(r.fin, stream)>>>(table, (int)r.np, C, groups, n, momentum, mean, var, cnt, rmean, rvar, nbt);
    FC_CHECK_LAUNCH();
  }
  if (!apply) return FC_OK;
  if (r.apply == FC_NAPPLY_BN1)
    k_bn1_apply<<<FC_GRID(r.ap, stream)>>>(x, n, C, r.rpb, part, (int)r.np, eps, gamma, beta, residual, act, momentum, y, mean, var, cnt, rmean, rvar, nbt, add_inv, add_src);
  else if (r.apply == FC_NAPPLY_BN2)
    k_bn2_apply<<<FC_GRID(r.ap, stream)>>>(x, n, C, r.rpb, table, (int)r.np, groups, eps, gamma, beta, residual, act, momentum, y, mean, var, cnt, rmean, rvar, nbt, r.cg,
                                   add_inv, add_src, amax);
  else
    k_norm_act_fwd<<<FC_GRID(r.ap, stream)>>>(x, nullptr, 0, n, C, mean, var, eps, gamma, beta, residual, act, add_inv, add_src, y, amax);
  FC_CHECK_LAUNCH();
  if (r.amax == FC_NAMAX_PASS && amax) return fc_amax(y, n * (int64_t)C, amax, stream);      // (k_bn1_apply does not fold)
  return FC_OK;
}

// every backward entry point: the argument checks, the route, its workspace, its launches.  gy2 (nullable): a second contribution to the
// incoming gradient; table: gy's producer's [nb_part][2][C]; POOL (norm_rows.h POOL_*): gy is the pooled gradient, read through parent and argrow (POOL_ARG: the arg-max rows; POOL_MASK: the per-child mask); amax (nullable):
// max |gx| into the caller's (zeroed) word — late_hint: the word of fc_amax_out_hint, consumed once the checks have passed
template <int POOL>
static int norm_bwd(int form, const float* x, const float* y, const float* gy, const float* gy2, const int* parent, const int* argrow, const int* seg,
                    int seg_stride, int64_t n, int C, int nseg, const float* mean, const float* var, const float* cnt, float eps, const float* gamma,
                    const float* beta, int act, float* gx, float* gres, float* sums, const float* table, int64_t nb_part, int64_t small_elems, void* ws,
                    int64_t ws_bytes, hipStream_t stream, unsigned* amax, bool late_hint = false) {
  if (act < 0 || act > 2) return FC_EINVAL;
  const NormRoute r = norm_bwd_route(n, C, nseg, table != nullptr, nb_part, small_elems, form);
  if (int rc = route_check(r, ws_bytes)) return rc;
  if (late_hint) amax = take_amax_out();
  if (r.apply == FC_NBAPPLY_NONE) {      // no rows
    FC_HIP(hipMemsetAsync(sums, 0, sizeof(float) * nseg * 2 * C, stream));
    return FC_OK;
  }
  if (r.sums == FC_NRED_PARTIAL) {
    // the instantiation that reads the operands this call has (norm_rows.h): y only where the activation's derivative is taken from it
    const bool from_y = act && y;
#define FC_PARTIAL(P, Y, G2) \
  k_norm_bwd_partial<P, Y, G2><<<FC_GRID(r.red, stream)>>>(x, y, gy, gy2, parent, argrow, seg, seg_stride, n, C, nseg, mean, var, eps, act, gamma, beta, r.red_rpb, (float*)ws)
    if constexpr (POOL != POOL_NONE) {
      if (from_y || gy2) return FC_EINVAL;      // (the pooled entry point passes neither)
      FC_PARTIAL(POOL, false, false);
    } else if (from_y) {
      if (gy2) FC_PARTIAL(POOL_NONE, true, true); else FC_PARTIAL(POOL_NONE, true, false);
    } else {
      if (gy2) FC_PARTIAL(POOL_NONE, false, true); else FC_PARTIAL(POOL_NONE, false, false);
    }
#undef FC_PARTIAL
    FC_CHECK_LAUNCH();
    table = (const float*)ws;
  }
  if (r.apply == FC_NBAPPLY_PROLOGUE) {
    k_bn1_bwd_apply<<<FC_GRID(r.ap, stream)>>>(x, y, gy, gy2, n, C, r.rpb, table, (int)r.np, mean, var, eps, gamma, beta, act, gx, gres, sums, r.cg, amax);
  } else {
    k_stats_final<<<FC_GRID(r.fin, stream)>>>(table, r.np, nseg, 2 * C, sums);
    FC_CHECK_LAUNCH();
    k_norm_bwd_apply<POOL><<<FC_GRID(r.ap, stream)>>>(x, y, gy, gy2, parent, argrow, seg, seg_stride, n, C, mean, var, eps, gamma, beta, sums, cnt, act, gx, gres, amax);
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}

constexpr int ROUTE_OUT_INTS = 16;      // out[] of the route queries: include/fcaf3d_hip.h promises 16 ints, the FC_NROUTE_* fields first, the rest 0
static_assert(FC_NROUTE_LAUNCHES < ROUTE_OUT_INTS, "every FC_NROUTE_* field lies inside out[]");
static int route_out(const NormRoute& r, int* out) {
  const int f[ROUTE_OUT_INTS] = {r.sums, r.apply, r.amax, (int)r.np, (int)r.nb, (int)r.rpb, r.cg, r.ap.threads, (int)r.ap.lds, (int)r.ap.grid_x, (int)r.ap.grid_y,
                                 (int)r.ws_bytes, (r.red.threads != 0) + (r.fin.threads != 0) + (r.ap.threads != 0)};
  for (int i = 0; i < ROUTE_OUT_INTS; ++i) out[i] = f[i];
  return r.sums ? FC_OK : FC_EINVAL;
}

// fc_col_stats (stats: out = mean, with var and cnt) and fc_seg_col_sums (out = the column sums of x per segment): the argument checks, pass 1 over
// the row blocks into the workspace, its finalize kernel.  The statistics take ONE pass over x (r5: sums of x and of x^2 per block and segment with
// the counts behind them, combined in fp64 — r1-r4 read x twice, mean, then the centred squares: four launches)
static int col_stats(bool stats, const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* out, float* var, float* cnt, void* ws,
                     int64_t ws_bytes, hipStream_t stream) {
  if (n < 0 || nseg < 1 || nseg > MAXSEG) return FC_EINVAL;
  StatsGeometry g;
  if (!stats_geometry(C, &g)) return FC_EINVAL;
  if (ws_bytes < fc_col_stats_ws_bytes(n, C, nseg)) return FC_EWS;
  if (n == 0) {
    FC_HIP(hipMemsetAsync(out, 0, sizeof(float) * nseg * C, stream));
    if (stats) FC_HIP(hipMemsetAsync(var, 0, sizeof(float) * nseg * C, stream));
    if (stats) FC_HIP(hipMemsetAsync(cnt, 0, sizeof(float) * nseg, stream));
    return FC_OK;
  }
  const RowBlocks b = row_blocks(n, MAXBLOCKS);
  float* part = (float*)ws;
  float* part_cnt = stats ? part + b.nb * nseg * 2 * C : nullptr;
  k_stats_partial<<<(unsigned)b.nb, g.threads, g.lds_fwd, stream>>>(x, seg, seg_stride, n, C, nseg, stats, b.rpb, part, part_cnt);
  FC_CHECK_LAUNCH();
  if (stats) k_seg_meanvar_final<<<FC_GRID(final_launch(nseg, C), stream)>>>(part, part_cnt, b.nb, nseg, C, out, var, cnt);
  else k_stats_final<<<FC_GRID(final_launch(nseg, C), stream)>>>(part, b.nb, nseg, C, out);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

extern "C" {

int64_t fc_col_stats_ws_bytes(int64_t n, int C, int nseg) {
  return row_blocks(n, MAXBLOCKS).nb * nseg * (2 * (int64_t)C + 1) * (int64_t)sizeof(float);
}

// mean (nseg,C), var (nseg,C) biased, cnt (nseg) ; seg = per-row segment id pointer (NULL -> one segment)
int fc_col_stats(const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* mean, float* var,
                 float* cnt, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return col_stats(true, x, seg, seg_stride, n, C, nseg, mean, var, cnt, ws, ws_bytes, stream);
}

// out (nseg,C) = per-segment column sums of x (N,C) — deterministic two-level reduction
int fc_seg_col_sums(const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* out, void* ws,
                    int64_t ws_bytes, hipStream_t stream) {
  return col_stats(false, x, seg, seg_stride, n, C, nseg, out, nullptr, nullptr, ws, ws_bytes, stream);
}

int fc_bn_running_update(const float* mean, const float* var, const float* cnt, float momentum, int C, float* running_mean,
                         float* running_var, long long* num_batches_tracked, hipStream_t stream) {
  if (C < 1) return FC_EINVAL;
  k_bn_running<<<(unsigned)fc_cdiv(C, 256), 256, 0, stream>>>(mean, var, cnt, momentum, C, running_mean, running_var,
                                                             num_batches_tracked);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// ---- the normalisation entry points -------------------------------------------------------------------------------------------------
int fc_bn_train_fwd_route(int64_t n, int C, int has_part, int64_t nb_part, int groups, int64_t small_elems, int* out) {
  return out ? route_out(norm_fwd_route(n, C, has_part != 0, nb_part, groups, small_elems), out) : FC_EINVAL;
}
int fc_bn_train_bwd_route(int64_t n, int C, int nseg, int has_part, int64_t nb_part, int64_t small_elems, int form, int* out) {
  if (!out || form < FC_NFORM_TRAIN || form > FC_NFORM_SEG) return FC_EINVAL;
  return route_out(norm_bwd_route(n, C, nseg, has_part != 0, nb_part, small_elems, form), out);
}

// the byte counts the routes check (norm_route.h)
int64_t fc_bn_small_ws_bytes(int C) { return small_ws_bytes(C); }
int64_t fc_bn_stats_ws_bytes(int64_t n, int C) { return reduce_ws_bytes(n, C, 1); }
int64_t fc_norm_act_bwd_ws_bytes(int64_t n, int C, int nseg) { return reduce_ws_bytes(n, C, nseg); }
int64_t fc_maxpool8_norm_act_bwd_ws_bytes(int64_t n_in, int C, int nseg) { return reduce_ws_bytes(n_in, C, nseg); }
// whichever route fc_bn_train_fwd / fc_bn_train_bwd take of (n, C): small or general without a table, none behind a table
int64_t fc_bn_train_ws_bytes(int64_t n, int C) { return reduce_ws_bytes(n, C, 1) > small_ws_bytes(C) ? reduce_ws_bytes(n, C, 1) : small_ws_bytes(C); }

// training-mode BatchNorm statistics of a feature matrix of any size in one pass over x (+ buffer update):
// mean (C), biased var (C), cnt (1).  Follow with fc_norm_act_fwd.
int fc_bn_stats_train(const float* x, int64_t n, int C, float momentum, float* mean, float* var, float* cnt,
                      float* running_mean, float* running_var, long long* num_batches_tracked, void* ws,
                      int64_t ws_bytes, hipStream_t stream) {
  return bn_fwd(x, n, C, 0.f, nullptr, nullptr, nullptr, 0, momentum, nullptr, mean, var, cnt, running_mean, running_var, num_batches_tracked, nullptr, 0, 1,
                -1, nullptr, nullptr, ws, ws_bytes, stream, nullptr, false);      // the statistics step of the general route (no n * C is <= -1)
}

// training-mode BatchNorm forward for one segment: statistics + running-buffer update + normalise/affine/residual/act.
// mean/var (C) and cnt (1) are written for the backward pass; running_* / num_batches_tracked may be NULL.
int fc_bn_act_train_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta,
                        const float* residual, int act, float momentum, float* y, float* mean, float* var, float* cnt,
                        float* running_mean, float* running_var, long long* num_batches_tracked, void* ws,
                        int64_t ws_bytes, hipStream_t stream) {
  return bn_fwd(x, n, C, eps, gamma, beta, residual, act, momentum, y, mean, var, cnt, running_mean, running_var, num_batches_tracked, nullptr, 0, 1,
                INT64_MAX, nullptr, nullptr, ws, ws_bytes, stream, nullptr);      // the two-launch route whatever the size; the hint is not consumed
}

// its backward: sums (2,C) = [d beta, d gamma]; max |gx| into the word of fc_amax_out_hint
int fc_bn_act_train_bwd(const float* x, const float* y, const float* gy, int64_t n, int C, const float* mean,
                        const float* var, float eps, const float* gamma, const float* beta, int act, float* gx, float* gres,
                        float* sums, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return norm_bwd<POOL_NONE>(FC_NFORM_SMALL, x, y, gy, nullptr, nullptr, nullptr, nullptr, 0, n, C, 1, mean, var, nullptr, eps, gamma, beta, act, gx, gres, sums,
                         nullptr, 0, 0, ws, ws_bytes, stream, nullptr, true);
}

// add_inv / add_src (both or neither): y[r] += add_src[add_inv[r]] where add_inv[r] >= 0, behind the activation
int fc_norm_act_add_fwd(const float* x, const int* seg, int seg_stride, int64_t n, int C, const float* mean, const float* var,
                        float eps, const float* gamma, const float* beta, const float* residual, int act, const int* add_inv,
                        const float* add_src, float* y, hipStream_t stream) {
  unsigned* ao = take_amax_out();                // fc_amax_out_hint: max |y| into the caller's (zeroed) word
  if (n < 0 || C < 4 || C % 4 || act < 0 || act > 2 || (add_inv == nullptr) != (add_src == nullptr)) return FC_EINVAL;
  if (n == 0) return FC_OK;
  k_norm_act_fwd<<<FC_GRID(rows_launch(n, C), stream)>>>(x, seg, seg_stride, n, C, mean, var, eps, gamma, beta, residual, act, add_inv, add_src, y, ao);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int fc_norm_act_fwd(const float* x, const int* seg, int seg_stride, int64_t n, int C, const float* mean, const float* var,
                    float eps, const float* gamma, const float* beta, const float* residual, int act, float* y,
                    hipStream_t stream) {
  return fc_norm_act_add_fwd(x, seg, seg_stride, n, C, mean, var, eps, gamma, beta, residual, act, nullptr, nullptr, y, stream);
}

// sums (nseg,2,C): [.,0,.] = sum g' (= d beta per segment), [.,1,.] = sum g'*xhat (= d gamma per segment); max |gx| into the hint's word
int fc_norm_act_bwd(const float* x, const float* y, const float* gy, const int* seg, int seg_stride, int64_t n, int C,
                    int nseg, const float* mean, const float* var, const float* cnt, float eps, const float* gamma,
                    const float* beta, int act, float* gx, float* gres, float* sums, void* ws, int64_t ws_bytes,
                    hipStream_t stream) {
  unsigned* ao = take_amax_out();
  return norm_bwd<POOL_NONE>(FC_NFORM_SEG, x, y, gy, nullptr, nullptr, nullptr, seg, seg_stride, n, C, nseg, mean, var, cnt, eps, gamma, beta, act, gx, gres, sums,
                         nullptr, 0, 0, ws, ws_bytes, stream, ao);
}

// ---- r5: training-mode BatchNorm, one entry point per direction for every size ------------------------------------------------
// Forward.  part == NULL: the statistics are computed here from x (n * C <= small_elems: the two launches of fc_bn_act_train_fwd, else
// those of fc_bn_stats_train + fc_norm_act_fwd — the r1-r4 routes).  part != NULL: nb_part row blocks of producer-written column sums
// [nb_part][2][groups * C] (see k_bn2_apply); x is then (groups * n_rows_of_the_producer, C) = n rows.
// add_inv / add_src (both or neither, r7): the sparse sum behind the layer, y[r] += add_src[add_inv[r]] where add_inv[r] >= 0,
// written (and folded into the amax word of fc_amax_out_hint) by whichever apply kernel the size routes to
int fc_bn_train_add_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta, const float* residual,
                        int act, float momentum, float* y, float* mean, float* var, float* cnt, float* running_mean,
                        float* running_var, long long* num_batches_tracked, const float* part, int64_t nb_part, int groups,
                        int64_t small_elems, const int* add_inv, const float* add_src, void* ws, int64_t ws_bytes,
                        hipStream_t stream) {
  unsigned* ao = take_amax_out();
  return bn_fwd(x, n, C, eps, gamma, beta, residual, act, momentum, y, mean, var, cnt, running_mean, running_var, num_batches_tracked, part, nb_part, groups,
                small_elems, add_inv, add_src, ws, ws_bytes, stream, ao);
}

int fc_bn_train_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta, const float* residual,
                    int act, float momentum, float* y, float* mean, float* var, float* cnt, float* running_mean,
                    float* running_var, long long* num_batches_tracked, const float* part, int64_t nb_part, int groups,
                    int64_t small_elems, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return fc_bn_train_add_fwd(x, n, C, eps, gamma, beta, residual, act, momentum, y, mean, var, cnt, running_mean, running_var, num_batches_tracked, part, nb_part,
                             groups, small_elems, nullptr, nullptr, ws, ws_bytes, stream);
}

// Backward.  gy2 (nullable): a second contribution to the incoming gradient, added on the fly.  part == NULL: the sums of g' and
// g' xhat are reduced here (two or three launches by size); part != NULL: nb_part blocks [nb_part][2][C] written by the producer of gy.
int fc_bn_train_bwd(const float* x, const float* y, const float* gy, const float* gy2, int64_t n, int C, const float* mean,
                    const float* var, const float* cnt, float eps, const float* gamma, const float* beta, int act, float* gx,
                    float* gres, float* sums, const float* part, int64_t nb_part, int64_t small_elems, void* ws, int64_t ws_bytes,
                    hipStream_t stream) {
  unsigned* ao = take_amax_out();
  return norm_bwd<POOL_NONE>(FC_NFORM_TRAIN, x, y, gy, gy2, nullptr, nullptr, nullptr, 0, n, C, 1, mean, var, cnt, eps, gamma, beta, act, gx, gres, sums, part, nb_part,
                         small_elems, ws, ws_bytes, stream, ao);
}

// ---- eval-mode BatchNorm in a layer that trains: the backward with constant statistics (norm_eval.h) ----------------------------------
int fc_bn_eval_bwd_route(int64_t n, int C, int want_sums, int* out) {
  return out ? route_out(norm_eval_bwd_route(n, C, want_sums != 0), out) : FC_EINVAL;
}
int64_t fc_bn_eval_bwd_ws_bytes(int64_t n, int C, int want_sums) { return norm_eval_bwd_route(n, C, want_sums != 0).ws_bytes; }

// sums (2, C) = [d beta, d gamma], NULL where gamma and beta are frozen; amax_gx (nullable): max |gx| into the caller's (zeroed) word
int fc_bn_eval_bwd(const float* x, const float* y, const float* gy, const float* gy2, int64_t n, int C, const float* running_mean,
                   const float* running_var, float eps, const float* gamma, const float* beta, int act, float* gx, float* gres,
                   float* sums, unsigned* amax_gx, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (act < 0 || act > 2) return FC_EINVAL;
  const NormRoute r = norm_eval_bwd_route(n, C, sums != nullptr);
  if (int rc = route_check(r, ws_bytes)) return rc;
  if (r.apply == FC_NBAPPLY_NONE) {      // no rows
    if (sums) FC_HIP(hipMemsetAsync(sums, 0, sizeof(float) * 2 * C, stream));
    return FC_OK;
  }
  const bool from_y = act && y;
#define FC_EVAL(Y, G2, S) \
  k_bn_eval_bwd<Y, G2, S><<<FC_GRID(r.ap, stream)>>>(x, y, gy, gy2, n, C, running_mean, running_var, eps, gamma, beta, act, r.rpb, r.cg, gx, gres, (float*)ws, amax_gx)
#define FC_EVAL_S(Y, G2) do { if (sums) FC_EVAL(Y, G2, true); else FC_EVAL(Y, G2, false); } while (0)
  if (from_y) { if (gy2) FC_EVAL_S(true, true); else FC_EVAL_S(true, false); }
  else { if (gy2) FC_EVAL_S(false, true); else FC_EVAL_S(false, false); }
#undef FC_EVAL_S
#undef FC_EVAL
  FC_CHECK_LAUNCH();
  if (sums) {
    k_stats_final<<<FC_GRID(r.fin, stream)>>>((const float*)ws, r.np, 1, 2 * C, sums);
    FC_CHECK_LAUNCH();
  }
  return FC_OK;
}

int fc_amax_out_hint(unsigned* amax_word) {
  t_fc_amax_out = amax_word;
  return FC_OK;
}

int fc_maxpool_fwd(const float* in, const int* nbr, int64_t n_out, int K, int C, float* out, int* argrow,
                   hipStream_t stream) {
  unsigned* ao = take_amax_out();                // fc_amax_out_hint: max |out| into the caller's (zeroed) word
  if (n_out < 0 || K < 1 || C < 1) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  if (K == 8 && C % 4 == 0) k_maxpool8_fwd<<<FC_GRID(rows_launch(n_out, C), stream)>>>(in, nbr, n_out, C, out, argrow, ao);
  else k_maxpool_fwd<<<(unsigned)fc_cdiv(n_out * C, 256), 256, 0, stream>>>(in, nbr, n_out, K, C, out, argrow);
  FC_CHECK_LAUNCH();
  if (ao && !(K == 8 && C % 4 == 0)) return fc_amax(out, n_out * (int64_t)C, ao, stream);
  return FC_OK;
}

// gin must be zero-filled by the caller (n_in rows)
int fc_maxpool_bwd(const float* gout, const int* argrow, int64_t n_out, int C, float* gin, hipStream_t stream) {
  if (n_out < 0 || C < 1) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  k_maxpool_bwd<<<(unsigned)fc_cdiv(n_out * C, 256), 256, 0, stream>>>(gout, argrow, n_out, C, gin);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int fc_gather_rows(const float* src, const int* idx, int64_t n, int C, float* dst, hipStream_t stream) {
  if (n < 0 || C < 1) return FC_EINVAL;
  if (n == 0) return FC_OK;
  k_gather_rows<<<(unsigned)fc_cdiv(n * C, 256), 256, 0, stream>>>(src, idx, n, C, dst);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int fc_scatter_rows_add(const float* src, const int* idx, int64_t n, int C, float* dst, hipStream_t stream) {
  if (n < 0 || C < 1) return FC_EINVAL;
  if (n == 0) return FC_OK;
  k_scatter_rows_add<<<(unsigned)fc_cdiv(n * C, 256), 256, 0, stream>>>(src, idx, n, C, dst);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// ---- r7: the stem's tail fused (pool_rows.h) ---------------------------------------------------------------------------------------
int fc_norm_act_maxpool8_fwd(const float* x, const int* seg, int seg_stride, int C, const float* mean, const float* var, float eps,
                             const float* gamma, const float* beta, int act, const int* nbr, int64_t n_out, float* out,
                             int* argrow, float* y, int* parent, hipStream_t stream) {
  unsigned* ao = take_amax_out();                // fc_amax_out_hint: max |out| into the caller's (zeroed) word
  if (n_out < 0 || C < 4 || C % 4 || act < 0 || act > 2) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  k_norm_act_maxpool8_fwd<false><<<FC_GRID(rows_launch(n_out, C), stream)>>>(x, seg, seg_stride, C, mean, var, eps, gamma, beta, act, nbr, n_out, out, argrow,
                                                                            y, parent, nullptr, ao);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// the same pass writing the per-child arg-max mask (8 bytes per input row) for fc_maxpool8_mask_norm_act_bwd; argrow (nullable) only for a caller
// that reads the arg-max rows itself.  C == 64: the mask word is 64 channels wide
int fc_norm_act_maxpool8_mask_fwd(const float* x, const int* seg, int seg_stride, int C, const float* mean, const float* var, float eps,
                                  const float* gamma, const float* beta, int act, const int* nbr, int64_t n_out, float* out,
                                  int* argrow, float* y, int* parent, unsigned long long* mask, hipStream_t stream) {
  unsigned* ao = take_amax_out();                // fc_amax_out_hint: max |out| into the caller's (zeroed) word
  if (n_out < 0 || C != 64 || act < 0 || act > 2 || !parent || !mask) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  k_norm_act_maxpool8_fwd<true><<<FC_GRID(rows_launch(n_out, C), stream)>>>(x, seg, seg_stride, C, mean, var, eps, gamma, beta, act, nbr, n_out, out, argrow,
                                                                           y, parent, mask, ao);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// fc_norm_act_bwd (y == NULL, no residual) whose incoming gradient is read through the pool: the launches, the geometry and the order of
// every sum are those of fc_norm_act_bwd over the n_in rows — gx and sums are bit for bit what zero fill + fc_maxpool_bwd + fc_norm_act_bwd give
int fc_maxpool8_norm_act_bwd(const float* x, const float* gout, const int* argrow, const int* parent, const int* seg, int seg_stride,
                             int64_t n_in, int C, int nseg, const float* mean, const float* var, const float* cnt, float eps,
                             const float* gamma, const float* beta, int act, float* gx, float* sums, void* ws, int64_t ws_bytes,
                             hipStream_t stream) {
  if (!parent || !argrow) return FC_EINVAL;
  return norm_bwd<POOL_ARG>(FC_NFORM_SEG, x, nullptr, gout, nullptr, parent, argrow, seg, seg_stride, n_in, C, nseg, mean, var, cnt, eps, gamma, beta, act, gx, nullptr,
                        sums, nullptr, 0, 0, ws, ws_bytes, stream, nullptr);      // (the hint is not consumed)
}

// fc_maxpool8_norm_act_bwd reading the mask of fc_norm_act_maxpool8_mask_fwd where that reads the arg-max rows: the same route, launches and order of
// every sum; the select has the same values, so gx and sums are its bits
int fc_maxpool8_mask_norm_act_bwd(const float* x, const float* gout, const unsigned long long* mask, const int* parent, const int* seg,
                                  int seg_stride, int64_t n_in, int C, int nseg, const float* mean, const float* var, const float* cnt, float eps,
                                  const float* gamma, const float* beta, int act, float* gx, float* sums, void* ws, int64_t ws_bytes,
                                  hipStream_t stream) {
  if (!parent || !mask || C != 64) return FC_EINVAL;
  return norm_bwd<POOL_MASK>(FC_NFORM_SEG, x, nullptr, gout, nullptr, parent, reinterpret_cast<const int*>(mask), seg, seg_stride, n_in, C, nseg, mean, var, cnt,
                             eps, gamma, beta, act, gx, nullptr, sums, nullptr, 0, 0, ws, ws_bytes, stream, nullptr);      // (the hint is not consumed)
}

int fc_inverse_rows(const int* rows, int64_t n, int64_t n_inv, int* inv, hipStream_t stream) {
  if (n < 0 || n_inv < 0) return FC_EINVAL;
  if (n_inv > 0) FC_HIP(hipMemsetAsync(inv, 0xff, sizeof(int) * n_inv, stream));
  if (n == 0) return FC_OK;
  k_inverse_rows<<<(unsigned)fc_cdiv(n, 256), 256, 0, stream>>>(rows, n, n_inv, inv);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
