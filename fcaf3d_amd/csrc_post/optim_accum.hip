// Gradient accumulation over the flat buffers — what mmcv's GradientCumulativeOptimizerHook (optimizer_config = dict(type=
// 'GradientCumulativeOptimizerHook', cumulative_iters=k, grad_clip=...); mmcv 1.3.x, third party: no file of the reference tree) gets
// from `loss / k` and autograd's accumulation into `.grad`.  Here every backward pass OVERWRITES the flat gradient buffer g, so the
// group's sum lives in one more flat buffer acc, and the factor is applied after the pass (accum_elem.h: two roundings).
//
//   k_grad_accum<first, ema>    a micro-iteration that does not step:  acc = g * s (first of the group: acc is not read, 8 B per
//                               parameter) or acc = acc + g * s (12 B).  With the average operands the thread also moves the
//                               weight average towards the UNCHANGED parameter (ema_elem.h: EMAHook's update is due whether or not
//                               the optimizer stepped): + 12 B, no extra launch.
//   k_accum_sqsum_partial       the stepping iteration of a group: G = acc + g * s is written over g and its squares are summed in
//   + k_accum_sqsum_final       the same pass, in fc_grad_norm's block assignment and order (sqsum_order.h) — the pair replaces
//                               fc_grad_norm at 12 B per parameter instead of 4 and G is never re-read for the norm; out2 is, bit
//                               for bit, fc_grad_norm run on G.  fc_adamw_step / _groups / _ema_step follows unchanged.
//   k_grad_accum_sum            the same G without a norm (no clip configured).
//
// Pure streaming kernels, float4 per lane, 256-thread groups, as optim.hip's and optim_ema.hip's.  Kept apart from csrc/ as those
// of optim_groups.hip and optim_ema.hip are: a config without the hook never launches them, so source_hash() does not cover them.
//
// tools/accum_host_emu.cpp compiles this file's text from ACC_THREADS to the end of the anonymous namespace for the host
// (tests/test_accum_cpu.py) and includes accum_elem.h, ema_elem.h and sqsum_order.h itself: keep that stretch free of #include lines
// and of anything but the constant and the kernels.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "accum_elem.h"
#include "ema_elem.h"
#include "sqsum_order.h"

#include <cmath>
#include <cstdint>

#define ACC_THREADS 256

typedef float oa4 __attribute__((ext_vector_type(4)));

namespace {

// one 16-byte vector of each buffer per thread.  FIRST: acc is written, not read.  EMA: e <- e * keep + mu * p on the same vector
template <bool FIRST, bool EMA>
__global__ __launch_bounds__(ACC_THREADS) void k_grad_accum(oa4* __restrict__ acc, const oa4* __restrict__ g, int64_t n4, float s,
                                                            oa4* __restrict__ ema, const oa4* __restrict__ p, float mu, float keep) {
  const int64_t i = (int64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n4) return;
  oa4 av = {0.f, 0.f, 0.f, 0.f}, ev = av, pv = av;
  const oa4 gv = g[i];
  if (!FIRST) av = acc[i];
  if (EMA) { ev = ema[i]; pv = p[i]; }           // every load in flight before the first store
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    av[j] = FIRST ? accum_first_elem(gv[j], s) : accum_elem(av[j], gv[j], s);
    if (EMA) ev[j] = ema_elem(ev[j], pv[j], mu, keep);
  }
  acc[i] = av;
  if (EMA) ema[i] = ev;
}

// g <- G = acc + g * s, one 16-byte vector per thread
__global__ __launch_bounds__(ACC_THREADS) void k_grad_accum_sum(oa4* __restrict__ g, const oa4* __restrict__ acc, int64_t n4, float s) {
  const int64_t i = (int64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
  if (i >= n4) return;
  oa4 gv = g[i];
  const oa4 av = acc[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) gv[j] = accum_elem(av[j], gv[j], s);
  g[i] = gv;
}

// g <- G and part[b] = the sum of G^2 over block b's float4 slices: k_sqsum_partial's sweep (csrc/optim.hip; grid-stride, fixed
// assignment, four vectors of either buffer in flight), the masked lanes contributing 0 + 0 * s = 0 as its zero vectors do
__global__ __launch_bounds__(SQO_THREADS) void k_accum_sqsum_partial(oa4* __restrict__ g, const oa4* __restrict__ acc, int64_t n4, float s,
                                                                    double* __restrict__ part) {
  __shared__ double red[4];
  double sum = 0.0;
  const int64_t stride = (int64_t)gridDim.x * SQO_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * SQO_THREADS + threadIdx.x; i < n4; i += 4 * stride) {
    oa4 a[4], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = i + u * stride;
      a[u] = j < n4 ? acc[j] : oa4{0.f, 0.f, 0.f, 0.f};
      v[u] = j < n4 ? g[j] : oa4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = i + u * stride;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[u][c] = accum_elem(a[u][c], v[u][c], s);
      if (j < n4) g[j] = v[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) sum += (double)sqo_vec(v[u]);
  }
  sqo_block_store(sum, red, part);
}

__global__ __launch_bounds__(SQO_FINAL_THREADS) void k_accum_sqsum_final(const double* __restrict__ part, int nb, float max_norm,
                                                                        float* __restrict__ out) {
  __shared__ double red[16];
  sqo_final(part, nb, max_norm, out, red);
}

}  // namespace

namespace {

bool overlap(const void* a, const void* b, int64_t n) {
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  return ua < ub + bytes && ub < ua + bytes;
}

bool unit(float x) { return std::isfinite(x) && x >= 0.f && x <= 1.f; }

}  // host helpers

extern "C" {

int fc_grad_accum(float* acc, const float* g, int64_t n, float scale, int first, float* ema, const float* p, float ema_mu,
                  float ema_keep, hipStream_t stream) {
  if (n < 0 || n % 4 || !std::isfinite(scale) || scale <= 0.f || !unit(ema_mu) || !unit(ema_keep)) return FC_EINVAL;
  if (ema && !p) return FC_EINVAL;
  if (n == 0) return FC_OK;
  if (!acc || !g || overlap(acc, g, n)) return FC_EINVAL;
  if (ema && (overlap(ema, acc, n) || overlap(ema, g, n) || overlap(ema, p, n))) return FC_EINVAL;
  const int64_t n4 = n / 4;
  const unsigned grid = (unsigned)fc_cdiv(n4, ACC_THREADS);
  oa4* a = (oa4*)acc;
  const oa4* gg = (const oa4*)g;
  if (ema) {
    if (first) k_grad_accum<true, true><<<grid, ACC_THREADS, 0, stream>>>(a, gg, n4, scale, (oa4*)ema, (const oa4*)p, ema_mu, ema_keep);
    else k_grad_accum<false, true><<<grid, ACC_THREADS, 0, stream>>>(a, gg, n4, scale, (oa4*)ema, (const oa4*)p, ema_mu, ema_keep);
  } else {
    if (first) k_grad_accum<true, false><<<grid, ACC_THREADS, 0, stream>>>(a, gg, n4, scale, nullptr, nullptr, 0.f, 0.f);
    else k_grad_accum<false, false><<<grid, ACC_THREADS, 0, stream>>>(a, gg, n4, scale, nullptr, nullptr, 0.f, 0.f);
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int64_t fc_grad_accum_norm_ws_bytes(int64_t n) { return (int64_t)SQO_BLOCKS * (int64_t)sizeof(double); }

int fc_grad_accum_norm(float* g_inout, const float* acc, int64_t n, float scale, float max_norm, float* out2, void* ws, int64_t ws_bytes,
                       hipStream_t stream) {
  if (n < 0 || n % 4 || !std::isfinite(scale) || scale <= 0.f) return FC_EINVAL;
  if (n == 0) return FC_OK;
  if (!g_inout || !acc || overlap(acc, g_inout, n)) return FC_EINVAL;
  const int64_t n4 = n / 4;
  if (!out2) {
    k_grad_accum_sum<<<(unsigned)fc_cdiv(n4, ACC_THREADS), ACC_THREADS, 0, stream>>>((oa4*)g_inout, (const oa4*)acc, n4, scale);
    FC_CHECK_LAUNCH();
    return FC_OK;
  }
  if (!ws || ws_bytes < fc_grad_accum_norm_ws_bytes(n)) return FC_EWS;
  const int nb = sqo_blocks(n4);
  k_accum_sqsum_partial<<<nb, SQO_THREADS, 0, stream>>>((oa4*)g_inout, (const oa4*)acc, n4, scale, (double*)ws);
  FC_CHECK_LAUNCH();
  k_accum_sqsum_final<<<1, SQO_FINAL_THREADS, 0, stream>>>((const double*)ws, nb, max_norm, out2);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
