// The backward through a BatchNorm that reads its running statistics (included by norm.hip): mean and variance are constants, so
//   g' = (gy (+ gy2)) act'(pre)     gx = g' gamma rstd     gres = g'     d beta = sum_rows g'     d gamma = sum_rows g' xhat
// and gx needs neither sum: ONE pass over the rows, no reduce-then-apply, no table from the convolution that produced gy.
#pragma once

// ELU below zero has act' = exp(pre), and exp turns the ABSOLUTE error of pre — about 4.5 x 2^-24 |xhat gamma| when bn_pre forms it in fp32 — into a
// RELATIVE error of act': up to 14 x 2^-24 measured, over the 8 x 2^-24 the entry point promises for gx.  So the VALUE of that derivative is taken from a
// pre-activation formed in fp64 (rstd by one Newton step from the fp32 value: relative error ~1e-14), split into an fp32 head and tail:
// exp(p) = expf(head) (1 + tail).  The DECISION pre > 0 stays the fp32 bn_pre's, the forward kernels' bit for bit.  Three fp64 operations per
// element under a pass that waits for HBM; only ELU without a residual (the neck's layers) takes the path.
__device__ __forceinline__ double bn_eval_rstd64(float va, float eps, float is) {
  const double v = (double)va + (double)eps, r = (double)is;
  return r * (1.5 - 0.5 * v * r * r);
}
__device__ __forceinline__ float elu_bwd_from_pre64(float x, float mu, double isd, float g, float b) {
  const double p = fma(((double)x - (double)mu) * isd, (double)g, (double)b);
  const float ph = (float)p, pl = (float)(p - (double)ph);
  const float e = expf(ph);
  return fmaf(e, pl, e);
}

// One element group (four channels of a row): g' into gr, gx into o.  act' is taken from y where the forward had a residual (FROM_Y), else
// recomputed from x with bn_pre — the decisions of k_norm_bwd_partial / k_norm_bwd_apply, from the same helpers (norm_elem.h).
template <bool FROM_Y>
__device__ __forceinline__ void bn_eval_bwd_elem(const float (&xv)[4], const float (&yv)[4], const float (&gv)[4], const float (&mu)[4], const float (&is)[4],
                                                 const float (&gm)[4], const float (&bt)[4], const float (&gis)[4], const double (&isd)[4], int act, float (&gr)[4],
                                                 float (&o)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float g = gv[j];
    if (FROM_Y) g *= act_bwd_from_y(yv[j], act);
    else if (act) {
      const float pf = bn_pre(xv[j], mu[j], is[j], gm[j], bt[j]);
      g *= (act == 2 && !(pf > 0.f)) ? elu_bwd_from_pre64(xv[j], mu[j], isd[j], gm[j], bt[j]) : act_bwd_from_pre(pf, act);
    }
    gr[j] = g;
    o[j] = g * gis[j];
  }
}

// FROM_Y (act && y) / GY2 (gy2 != NULL) / SUMS (gamma or beta trains): compile-time, so that an instantiation holds the row registers it loads
// and no others (see k_norm_bwd_partial).
// SUMS == false: the geometry of k_norm_act_fwd (rows_launch) — a thread per four channels of a row, pure elementwise; rpb, part unused.
// SUMS == true: the geometry of k_norm_bwd_partial (stats_geometry, row_blocks(n, MAXBLOCKS)) — block b owns rows [b rpb, (b + 1) rpb), four rows
// in flight per thread, and leaves its sums of g' and g' xhat in part[b][1][2][C] for k_stats_final to add in a fixed order (no float atomics).
// With few row blocks (the deep levels) a block owns a window of CG = 64 channels and grid.y walks the windows, as k_bn1_bwd_apply (ap_window):
// 853 x 512 is 112 blocks of 16 row lanes instead of 14 blocks of 2.
// amax_out (nullable): max |gx| by one integer atomicMax per block into the block's sub-word, as k_norm_bwd_apply.
template <bool FROM_Y, bool GY2, bool SUMS>
__global__ __launch_bounds__(256) void k_bn_eval_bwd(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                                     const float* __restrict__ gy2, int64_t n, int C, const float* __restrict__ rmean,
                                                     const float* __restrict__ rvar, float eps, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int act, int64_t rpb, int CG, float* __restrict__ gx,
                                                     float* __restrict__ gres, float* __restrict__ part, unsigned* __restrict__ amax_out) {
  unsigned am = 0u;
  if constexpr (!SUMS) {
    const int c4n = C / 4;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * c4n) {
      const int64_t r = t / c4n;
      const int c = (int)(t % c4n) * 4;
      float xv[4], gv[4], yv[4] = {0.f, 0.f, 0.f, 0.f}, mu[4], is[4], gm[4], bt[4], gis[4], gr[4], o[4];
      double isd[4] = {0., 0., 0., 0.};
      *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + r * C + c);
      *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(gy + r * C + c);
      if (GY2) {
        const float4 t2 = *reinterpret_cast<const float4*>(gy2 + r * C + c);
        gv[0] += t2.x; gv[1] += t2.y; gv[2] += t2.z; gv[3] += t2.w;
      }
      if (FROM_Y) *reinterpret_cast<float4*>(yv) = *reinterpret_cast<const float4*>(y + r * C + c);
      *reinterpret_cast<float4*>(mu) = *reinterpret_cast<const float4*>(rmean + c);
      *reinterpret_cast<float4*>(is) = *reinterpret_cast<const float4*>(rvar + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float va = is[j];
        is[j] = 1.f / sqrtf(va + eps);
        if (!FROM_Y && act == 2) isd[j] = bn_eval_rstd64(va, eps, is[j]);
        gm[j] = gamma ? gamma[c + j] : 1.f;
        bt[j] = beta ? beta[c + j] : 0.f;
        gis[j] = gm[j] * is[j];
      }
      bn_eval_bwd_elem<FROM_Y>(xv, yv, gv, mu, is, gm, bt, gis, isd, act, gr, o);
      *reinterpret_cast<float4*>(gx + r * C + c) = *reinterpret_cast<float4*>(o);
      if (gres) *reinterpret_cast<float4*>(gres + r * C + c) = *reinterpret_cast<float4*>(gr);
#pragma unroll
      for (int j = 0; j < 4; ++j) amax_fold(am, o[j]);
    }
  } else {
    extern __shared__ float sm[];               // [rl][2][CG]
    const int c0 = blockIdx.y * CG;             // this block's channel window: the row stride stays C
    x += c0; gy += c0; gx += c0; rmean += c0; rvar += c0; part += c0;
    if (FROM_Y) y += c0;
    if (GY2) gy2 += c0;
    if (gres) gres += c0;
    if (gamma) gamma += c0;
    if (beta) beta += c0;
    const auto [cl, rl, nrl] = lane_coord(CG / 4);
    const auto [r0, r1] = row_span(rpb, n);
    float mu[4], is[4], gm[4], bt[4], gis[4];
    double isd[4] = {0., 0., 0., 0.};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mu[j] = rmean[cl * 4 + j];
      is[j] = 1.f / sqrtf(rvar[cl * 4 + j] + eps);
      if (!FROM_Y && act == 2) isd[j] = bn_eval_rstd64(rvar[cl * 4 + j], eps, is[j]);
      gm[j] = gamma ? gamma[cl * 4 + j] : 1.f;
      bt[j] = beta ? beta[cl * 4 + j] : 0.f;
      gis[j] = gm[j] * is[j];
    }
    float a1[4][4], a2[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) a1[u][j] = a2[u][j] = 0.f;
    for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (int64_t)nrl) {      // four rows of every operand in flight per thread (rows past the range re-read r0)
      float xv[4][4], gv[4][4], yv[4][4], g2[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t r = rb + (int64_t)u * nrl;
        const int64_t rc = r < r1 ? r : r0;
        *reinterpret_cast<float4*>(xv[u]) = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
        *reinterpret_cast<float4*>(gv[u]) = *reinterpret_cast<const float4*>(gy + rc * C + cl * 4);
        if (GY2) *reinterpret_cast<float4*>(g2[u]) = *reinterpret_cast<const float4*>(gy2 + rc * C + cl * 4);
        if (FROM_Y) *reinterpret_cast<float4*>(yv[u]) = *reinterpret_cast<const float4*>(y + rc * C + cl * 4);
        else yv[u][0] = yv[u][1] = yv[u][2] = yv[u][3] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t r = rb + (int64_t)u * nrl;
        if (r >= r1) continue;
        float gr[4], o[4];
        if (GY2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) gv[u][j] += g2[u][j];
        }
        bn_eval_bwd_elem<FROM_Y>(xv[u], yv[u], gv[u], mu, is, gm, bt, gis, isd, act, gr, o);
        *reinterpret_cast<float4*>(gx + r * C + cl * 4) = *reinterpret_cast<float4*>(o);
        if (gres) *reinterpret_cast<float4*>(gres + r * C + cl * 4) = *reinterpret_cast<float4*>(gr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          amax_fold(am, o[j]);
          a1[u][j] += gr[j];
          a2[u][j] += gr[j] * ((xv[u][j] - mu[j]) * is[j]);
        }
      }
    }
    float b1[4], b2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b1[j] = (a1[0][j] + a1[1][j]) + (a1[2][j] + a1[3][j]);
      b2[j] = (a2[0][j] + a2[1][j]) + (a2[2][j] + a2[3][j]);
    }
    *reinterpret_cast<float4*>(&sm[(rl * 2 + 0) * CG + cl * 4]) = *reinterpret_cast<float4*>(b1);
    *reinterpret_cast<float4*>(&sm[(rl * 2 + 1) * CG + cl * 4]) = *reinterpret_cast<float4*>(b2);
    __syncthreads();
    if (rl == 0) {
      float4 t1 = make_float4(0.f, 0.f, 0.f, 0.f), t2 = t1;
      for (int j = 0; j < nrl; ++j) {
        const float4 u = *reinterpret_cast<const float4*>(&sm[(j * 2 + 0) * CG + cl * 4]);
        const float4 w = *reinterpret_cast<const float4*>(&sm[(j * 2 + 1) * CG + cl * 4]);
        t1.x += u.x; t1.y += u.y; t1.z += u.z; t1.w += u.w;
        t2.x += w.x; t2.y += w.y; t2.z += w.z; t2.w += w.w;
      }
      float* dst = part + (int64_t)blockIdx.x * 2 * C;
      *reinterpret_cast<float4*>(dst + cl * 4) = t1;
      *reinterpret_cast<float4*>(dst + C + cl * 4) = t2;
    }
  }
  if (amax_out) amax_commit(am, amax_out);
}
