// AdamW over the flat buffers with a learning-rate and a weight-decay MULTIPLIER per parameter (fine-tuning: a lower rate on the
// backbone than on a new head, no decay on normalisation layers) — what mmcv's DefaultOptimizerConstructor expresses as one
// torch param group per parameter (paramwise_cfg) on top of optimizer = dict(type='AdamW', lr=0.001, weight_decay=0.0001)
// (configs/fcaf3d/fcaf3d.py:30).  The reference tree holds no such constructor call; the rule is mmcv's.
//
// The flat layout (fcaf3d_amd/flat.py) starts every parameter on a 64-float boundary, so a RUN — a maximal stretch of consecutive
// parameters with the same pair of multipliers — starts on a 64-float "slice" and a thread's 16-byte vector never straddles two.
// One launch does k_adamw's pass (csrc/optim.hip; 28 B per parameter, HBM-bound) with lr * lr_mult[r], weight_decay * decay_mult[r]
// of the run r its vector lies in: the run table (at most ADAMW_MAX_RUNS entries, 12 bytes each) is staged in LDS once per
// workgroup, behind the workgroup's own loads, and every thread finds its run by binary search over the runs' first slices.
//
// Kept apart from csrc/ as batch.hip, eval.hip, eiou.hip and merge.hip are: the kernel is not part of the profiled step, so
// source_hash() does not cover it.  The element update is k_adamw's own (csrc/adamw_elem.h, shared with csrc/optim.hip); with all
// multipliers 1 the two kernels give it the same operands (lr * 1, weight_decay * 1, (lr * 1) / bias_correction1).  The host never
// routes that case here (runner.FlatAdamW).
//
// tools/optim_host_emu.cpp compiles this file's text from ADAMW_THREADS to the end of the anonymous namespace for the host
// (tests/test_finetune_cpu.py) and includes adamw_elem.h itself: keep that stretch free of #include lines and of anything but the
// constants, the search and the kernel.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "../csrc/adamw_elem.h"

#include <cmath>
#include <cstring>

#define ADAMW_THREADS 256
#define ADAMW_MAX_RUNS 1024         // include/fcaf3d_hip.h FC_ADAMW_MAX_RUNS: three 4 KB columns of LDS per workgroup
#define ADAMW_SLICE_VECS 16         // 16-byte vectors per 64-float slice (flat.ALIGN)

typedef float og4 __attribute__((ext_vector_type(4)));

namespace {

// the packed table: R first slices (ascending, [0] == 0), then R learning-rate multipliers, then R weight-decay multipliers
struct AdamwRuns {
  unsigned begin[ADAMW_MAX_RUNS];
  float lr_mult[ADAMW_MAX_RUNS];
  float decay_mult[ADAMW_MAX_RUNS];
};

// the last run whose first slice is <= slice (begin[0] == 0: there is one); never reads outside [0, R)
__device__ inline int adamw_run_of(const unsigned* begin, int R, unsigned slice) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= slice) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// torch.optim.AdamW (decoupled weight decay, no amsgrad) as k_adamw states it, with the run's rates:
//   p *= 1 - lr_r * wd_r ; m += (g - m) * (1 - b1) ; v = b2 * v + (1 - b2) * g * g ;
//   p -= (lr_r / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)          with g already scaled by the clip coefficient
// lr_mult == 0: decay = 1 and step_size = 0, p * 1 - 0 * finite leaves p's bits alone while m and v advance
__global__ __launch_bounds__(ADAMW_THREADS) void k_adamw_groups(og4* __restrict__ p, const og4* __restrict__ g, og4* __restrict__ m,
                                                                og4* __restrict__ v, int64_t n4, float lr, float b1, float b2, float eps,
                                                                float wd, float bc1, float bc2_sqrt, const float* __restrict__ clip,
                                                                const unsigned* __restrict__ table, int R) {
  __shared__ AdamwRuns runs;
  const int64_t i = (int64_t)blockIdx.x * ADAMW_THREADS + threadIdx.x;
  const bool live = i < n4;
  og4 pv = {0.f, 0.f, 0.f, 0.f}, gv = pv, mv = pv, vv = pv;
  if (live) { pv = p[i]; gv = g[i]; mv = m[i]; vv = v[i]; }      // in flight while the table is staged
  for (int k = threadIdx.x; k < R; k += ADAMW_THREADS) {
    runs.begin[k] = table[k];
    runs.lr_mult[k] = __uint_as_float(table[R + k]);
    runs.decay_mult[k] = __uint_as_float(table[2 * R + k]);
  }
  __syncthreads();
  if (!live) return;
  const float c = clip ? fc_ld(&clip[1]) : 1.f;      // written by k_sqsum_final one launch ago, same address every step
  const int r = adamw_run_of(runs.begin, R, (unsigned)(i / ADAMW_SLICE_VECS));
  const float lr_r = lr * runs.lr_mult[r];
  const float wd_r = wd * runs.decay_mult[r];
  const float decay = 1.f - lr_r * wd_r;
  const float step_size = lr_r / bc1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const AdamwElem e = adamw_elem(pv[j], gv[j], mv[j], vv[j], c, decay, step_size, b1, b2, eps, bc2_sqrt);
    pv[j] = e.p; mv[j] = e.m; vv[j] = e.v;
  }
  p[i] = pv; m[i] = mv; v[i] = vv;
}

}  // namespace

static_assert(ADAMW_MAX_RUNS == FC_ADAMW_MAX_RUNS, "run cap of the header");

extern "C" {

int64_t fc_adamw_groups_table_bytes(int R) { return R < 1 || R > ADAMW_MAX_RUNS ? 0 : (int64_t)R * 12; }

int fc_adamw_groups_pack(const int64_t* begin, const float* lr_mult, const float* decay_mult, int R, int64_t n, void* out,
                         int64_t out_bytes) {
  if (!begin || !lr_mult || !decay_mult || !out || R < 1 || R > ADAMW_MAX_RUNS || n < 0 || n % 4) return FC_EINVAL;
  if (n / 64 > (int64_t)0xffffffffu) return FC_EINVAL;      // a slice index is 32 bits wide
  if (out_bytes < fc_adamw_groups_table_bytes(R)) return FC_EWS;
  if (begin[0] != 0) return FC_EINVAL;
  for (int r = 0; r < R; ++r) {
    if (begin[r] % 64 || begin[r] >= n) return FC_EINVAL;
    if (r && begin[r] <= begin[r - 1]) return FC_EINVAL;
    if (!std::isfinite(lr_mult[r]) || !std::isfinite(decay_mult[r]) || lr_mult[r] < 0.f || decay_mult[r] < 0.f) return FC_EINVAL;
  }
  unsigned* o = (unsigned*)out;
  for (int r = 0; r < R; ++r) o[r] = (unsigned)(begin[r] / 64);
  std::memcpy(o + R, lr_mult, (size_t)R * 4);
  std::memcpy(o + 2 * R, decay_mult, (size_t)R * 4);
  return FC_OK;
}

int fc_adamw_step_groups(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float bias_correction1, float bias_correction2, const float* norm_and_clip,
                         const void* table_dev, int R, hipStream_t stream) {
  if (n < 0 || n % 4 || bias_correction1 <= 0.f || bias_correction2 <= 0.f || R < 1 || R > ADAMW_MAX_RUNS || !table_dev) return FC_EINVAL;
  if (n / 64 > (int64_t)0xffffffffu) return FC_EINVAL;
  if (n == 0) return FC_OK;
  const int64_t n4 = n / 4;
  k_adamw_groups<<<(unsigned)fc_cdiv(n4, ADAMW_THREADS), ADAMW_THREADS, 0, stream>>>(
      (og4*)p, (const og4*)g, (og4*)m, (og4*)v, n4, lr, beta1, beta2, eps, weight_decay, bias_correction1, sqrtf(bias_correction2),
      norm_and_clip, (const unsigned*)table_dev, R);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
