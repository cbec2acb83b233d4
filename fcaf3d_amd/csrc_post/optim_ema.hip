// AdamW over the flat buffers WITH an exponential moving average of the parameters in the same launch, and the exchange of two
// flat buffers — what mmcv's EMAHook (custom_hooks = [dict(type='EMAHook', momentum=0.0002, interval=1, warm_up=100)]; mmcv 1.3.x,
// third party: no file of the reference tree) does with two tensor ops per parameter after every optimizer step, and with one
// copy pair per parameter at every epoch edge.
//
// k_adamw_ema is k_adamw_groups' pass (csrc_post/optim_groups.hip: 28 B per parameter, HBM-bound, the run table staged in LDS
// behind the workgroup's own loads) plus one more 16-byte read and write per thread: the thread that has just computed the new
// parameter vector updates the average of the same vector (ema_elem.h) — 36 B per parameter, no extra launch.  R == 0 means no
// multipliers: decay and step_size are then the operands fc_adamw_step (csrc/optim.hip) gives adamw_elem, step_size among them as
// the host's own quotient.  The AdamW element update is csrc/adamw_elem.h, untouched; the run search restates optim_groups.hip's
// (that file's text is cut for its own host emulator and stays as it is).
//
// Kept apart from csrc/ as optim_groups.hip is: not part of the profiled step, so source_hash() does not cover it.
//
// tools/ema_host_emu.cpp compiles this file's text from EMA_THREADS to the end of the anonymous namespace for the host
// (tests/test_ema_cpu.py) and includes adamw_elem.h and ema_elem.h itself: keep that stretch free of #include lines and of
// anything but the constants, the search and the two kernels.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "../csrc/adamw_elem.h"
#include "ema_elem.h"

#include <cmath>
#include <cstdint>

#define EMA_THREADS 256
#define EMA_MAX_RUNS 1024           // include/fcaf3d_hip.h FC_ADAMW_MAX_RUNS: three 4 KB columns of LDS per workgroup
#define EMA_SLICE_VECS 16           // 16-byte vectors per 64-float slice (flat.ALIGN)

typedef float oe4 __attribute__((ext_vector_type(4)));

namespace {

// the packed table of fc_adamw_groups_pack: R first slices (ascending, [0] == 0), R learning-rate multipliers, R weight-decay multipliers
struct EmaRuns {
  unsigned begin[EMA_MAX_RUNS];
  float lr_mult[EMA_MAX_RUNS];
  float decay_mult[EMA_MAX_RUNS];
};

// the last run whose first slice is <= slice (begin[0] == 0: there is one); never reads outside [0, R), R >= 1
__device__ inline int ema_run_of(const unsigned* begin, int R, unsigned slice) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= slice) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// k_adamw_groups' update of (p, m, v), then  e <- e * keep + mu * p_new  (ema_elem.h: three roundings) on the vector just computed.
// R == 0: table is not read, decay = 1 - lr * wd and step_size = step_plain (= lr / bc1, the host's quotient) as in k_adamw.
__global__ __launch_bounds__(EMA_THREADS) void k_adamw_ema(oe4* __restrict__ p, const oe4* __restrict__ g, oe4* __restrict__ m,
                                                           oe4* __restrict__ v, oe4* __restrict__ ema, int64_t n4, float lr, float b1,
                                                           float b2, float eps, float wd, float bc1, float step_plain, float bc2_sqrt,
                                                           const float* __restrict__ clip, const unsigned* __restrict__ table, int R,
                                                           float mu, float keep) {
  __shared__ EmaRuns runs;
  const int64_t i = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x;
  const bool live = i < n4;
  oe4 pv = {0.f, 0.f, 0.f, 0.f}, gv = pv, mv = pv, vv = pv, ev = pv;
  if (live) { pv = p[i]; gv = g[i]; mv = m[i]; vv = v[i]; ev = ema[i]; }      // all five in flight while the table is staged
  for (int k = threadIdx.x; k < R; k += EMA_THREADS) {
    runs.begin[k] = table[k];
    runs.lr_mult[k] = __uint_as_float(table[R + k]);
    runs.decay_mult[k] = __uint_as_float(table[2 * R + k]);
  }
  __syncthreads();
  if (!live) return;
  const float c = clip ? fc_ld(&clip[1]) : 1.f;      // written by k_sqsum_final one launch ago, same address every step
  float decay, step_size;
  if (R > 0) {
    const int r = ema_run_of(runs.begin, R, (unsigned)(i / EMA_SLICE_VECS));
    const float lr_r = lr * runs.lr_mult[r];
    const float wd_r = wd * runs.decay_mult[r];
    decay = 1.f - lr_r * wd_r;
    step_size = lr_r / bc1;
  } else {
    decay = 1.f - lr * wd;
    step_size = step_plain;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const AdamwElem e = adamw_elem(pv[j], gv[j], mv[j], vv[j], c, decay, step_size, b1, b2, eps, bc2_sqrt);
    pv[j] = e.p; mv[j] = e.m; vv[j] = e.v;
    ev[j] = ema_elem(ev[j], e.p, mu, keep);
  }
  p[i] = pv; m[i] = mv; v[i] = vv; ema[i] = ev;
}

// a <-> b, one 16-byte vector of each per thread (the ranges do not overlap: fc_swap_f32 refuses those)
__global__ __launch_bounds__(EMA_THREADS) void k_swap_f32(oe4* __restrict__ a, oe4* __restrict__ b, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x;
  if (i >= n4) return;
  const oe4 av = a[i], bv = b[i];
  a[i] = bv; b[i] = av;
}

}  // namespace

static_assert(EMA_MAX_RUNS == FC_ADAMW_MAX_RUNS, "run cap of the header");

extern "C" {

int fc_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float bias_correction1, float bias_correction2, const float* norm_and_clip,
                      const void* table_dev, int R, float ema_mu, float ema_keep, hipStream_t stream) {
  if (n < 0 || n % 4 || bias_correction1 <= 0.f || bias_correction2 <= 0.f) return FC_EINVAL;
  if (table_dev ? (R < 1 || R > EMA_MAX_RUNS) : R != 0) return FC_EINVAL;      // no table with R == 0, or a table of 1 .. cap runs
  if (n / 64 > (int64_t)0xffffffffu) return FC_EINVAL;
  if (!ema && n > 0) return FC_EINVAL;
  if (!std::isfinite(ema_mu) || !std::isfinite(ema_keep) || ema_mu < 0.f || ema_mu > 1.f || ema_keep < 0.f || ema_keep > 1.f)
    return FC_EINVAL;
  if (n == 0) return FC_OK;
  const int64_t n4 = n / 4;
  k_adamw_ema<<<(unsigned)fc_cdiv(n4, EMA_THREADS), EMA_THREADS, 0, stream>>>(
      (oe4*)p, (const oe4*)g, (oe4*)m, (oe4*)v, (oe4*)ema, n4, lr, beta1, beta2, eps, weight_decay, bias_correction1,
      lr / bias_correction1, sqrtf(bias_correction2), norm_and_clip, (const unsigned*)table_dev, R, ema_mu, ema_keep);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int fc_swap_f32(float* a, float* b, int64_t n, hipStream_t stream) {
  if (n < 0 || n % 4 || a == b) return FC_EINVAL;
  if (n == 0) return FC_OK;
  if (!a || !b) return FC_EINVAL;
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  if (ua < ub + bytes && ub < ua + bytes) return FC_EINVAL;      // overlapping ranges
  const int64_t n4 = n / 4;
  k_swap_f32<<<(unsigned)fc_cdiv(n4, EMA_THREADS), EMA_THREADS, 0, stream>>>((oe4*)a, (oe4*)b, n4);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
