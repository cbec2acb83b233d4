// The one-segment BatchNorm kernels (included by norm.hip): row-blocked partial sums, the apply kernels that re-reduce a small table of partials in
// their prologue (bn1: our own fp32 sums; bn2: a producer's table, fp64), the finalize kernels for longer tables, the running-buffer update alone.
#pragma once

// ================================================================================================
// Small-tensor BatchNorm (n*C <= 4 M elements: backbone levels 2-4, coarse neck levels): TWO launches per
// direction instead of six / three.  Launch 1 writes per-block partial sums; launch 2 lets every block
// re-reduce the (<= 64) partials in its prologue (a few hundred KB out of L2) and apply straight away.
// Forward statistics in one pass: sums of (x - s) and (x - s)^2 with the shift s = x[0][c] (a sample of the
// column, so |mean - s| ~ sigma and E[(x-s)^2] - E[x-s]^2 loses no digits).

// part [nb][2][C]
__global__ void k_bn1_partial(const float* __restrict__ x, int64_t n, int C, int64_t rpb, float* __restrict__ part) {
  extern __shared__ float sm[];               // [rl][2][C]
  const auto [cl, rl, nrl] = lane_coord(C / 4);
  const auto [r0, r1] = row_span(rpb, n);
  const float4 sh = *reinterpret_cast<const float4*>(x + cl * 4);
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
  for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (int64_t)nrl) {      // four rows in flight per thread (padding rows read the shift: 0)
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      // (a padding row re-reads row 0, which IS the shift: as `r < r1 ? load : sh` the compiler selects between two ADDRESSES and keeps sh on the stack)
      v[u] = *reinterpret_cast<const float4*>(x + (r < r1 ? r : 0) * C + cl * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u].x -= sh.x; v[u].y -= sh.y; v[u].z -= sh.z; v[u].w -= sh.w;
      a1.x += v[u].x; a1.y += v[u].y; a1.z += v[u].z; a1.w += v[u].w;
      a2.x += v[u].x * v[u].x; a2.y += v[u].y * v[u].y; a2.z += v[u].z * v[u].z; a2.w += v[u].w * v[u].w;
    }
  }
  *reinterpret_cast<float4*>(&sm[(rl * 2 + 0) * C + cl * 4]) = a1;
  *reinterpret_cast<float4*>(&sm[(rl * 2 + 1) * C + cl * 4]) = a2;
  __syncthreads();
  if (rl == 0) {
    float4 t1 = make_float4(0.f, 0.f, 0.f, 0.f), t2 = t1;
    for (int j = 0; j < nrl; ++j) {
      float4 u = *reinterpret_cast<const float4*>(&sm[(j * 2 + 0) * C + cl * 4]);
      float4 w = *reinterpret_cast<const float4*>(&sm[(j * 2 + 1) * C + cl * 4]);
      t1.x += u.x; t1.y += u.y; t1.z += u.z; t1.w += u.w;
      t2.x += w.x; t2.y += w.y; t2.z += w.z; t2.w += w.w;
    }
    float* dst = part + ((int64_t)blockIdx.x * 2) * C;
    *reinterpret_cast<float4*>(dst + cl * 4) = t1;
    *reinterpret_cast<float4*>(dst + C + cl * 4) = t2;
  }
}

// every block: reduce part[nb][2][C] -> (S1,S2) per channel (fixed order), then apply to its rows
// (CG channels from c0 on: a block may own a channel window of the table, k_bn1_bwd_apply's grid.y; CG == C, c0 == 0: all of them)
__device__ static inline void bn1_reduce_parts(const float* __restrict__ part, int nb, int C, int cl, int rl, int nrl,
                                               float* sm /*[nrl][2][CG]*/, float4* s1, float4* s2, int CG, int c0) {
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
  // a SMALL table (the deep levels: a few KB at the same workspace address layer after layer) can survive in a CU's L1
  // from the previous layer: read it past the L1 (fc_common.h: fc_ld4); a big one streams through the L1 anyway
  const bool past_l1 = (int64_t)nb * C * 8 <= 32768;
  for (int b = rl; b < nb; b += nrl) {
    const float* src = part + ((int64_t)b * 2) * C + c0;
    float4 u = past_l1 ? fc_ld4(src + cl * 4) : *reinterpret_cast<const float4*>(src + cl * 4);
    float4 w = past_l1 ? fc_ld4(src + C + cl * 4) : *reinterpret_cast<const float4*>(src + C + cl * 4);
    a1.x += u.x; a1.y += u.y; a1.z += u.z; a1.w += u.w;
    a2.x += w.x; a2.y += w.y; a2.z += w.z; a2.w += w.w;
  }
  *reinterpret_cast<float4*>(&sm[(rl * 2 + 0) * CG + cl * 4]) = a1;
  *reinterpret_cast<float4*>(&sm[(rl * 2 + 1) * CG + cl * 4]) = a2;
  __syncthreads();
  float4 t1 = make_float4(0.f, 0.f, 0.f, 0.f), t2 = t1;
  for (int j = 0; j < nrl; ++j) {
    float4 u = *reinterpret_cast<const float4*>(&sm[(j * 2 + 0) * CG + cl * 4]);
    float4 w = *reinterpret_cast<const float4*>(&sm[(j * 2 + 1) * CG + cl * 4]);
    t1.x += u.x; t1.y += u.y; t1.z += u.z; t1.w += u.w;
    t2.x += w.x; t2.y += w.y; t2.z += w.z; t2.w += w.w;
  }
  *s1 = t1; *s2 = t2;
}

__global__ void k_bn1_apply(const float* __restrict__ x, int64_t n, int C, int64_t rpb, const float* __restrict__ part, int nb,
                            float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                            const float* __restrict__ residual, int act, float momentum, float* __restrict__ y,
                            float* __restrict__ mean_out, float* __restrict__ var_out, float* __restrict__ cnt_out,
                            float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ nbt,
                            const int* __restrict__ add_inv, const float* __restrict__ add_src) {
  extern __shared__ float sm[];
  const int c4n = C / 4;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;      // (a copy of lane_coord: the helper reorders this kernel's prologue)
  const int nrl = blockDim.x / c4n;
  float4 s1, s2;
  bn1_reduce_parts(part, nb, C, cl, rl, nrl, sm, &s1, &s2, C, 0);
  const float4 sh = *reinterpret_cast<const float4*>(x + cl * 4);
  const float inv_n = 1.f / (float)n;
  float d[4] = {s1.x * inv_n, s1.y * inv_n, s1.z * inv_n, s1.w * inv_n};
  float q[4] = {s2.x * inv_n, s2.y * inv_n, s2.z * inv_n, s2.w * inv_n};
  float shv[4] = {sh.x, sh.y, sh.z, sh.w};
  float mu[4], va[4], is[4], g[4], bt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mu[j] = shv[j] + d[j];
    va[j] = fmaxf(q[j] - d[j] * d[j], 0.f);
    is[j] = 1.f / sqrtf(va[j] + eps);
    g[j] = gamma ? gamma[cl * 4 + j] : 1.f;
    bt[j] = beta ? beta[cl * 4 + j] : 0.f;
  }
  if (blockIdx.x == 0 && rl == 0) {
    *reinterpret_cast<float4*>(mean_out + cl * 4) = make_float4(mu[0], mu[1], mu[2], mu[3]);
    *reinterpret_cast<float4*>(var_out + cl * 4) = make_float4(va[0], va[1], va[2], va[3]);
    if (cl == 0) { cnt_out[0] = (float)n; if (nbt) nbt[0] += 1; }
    if (rmean) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bn_running_update(rmean, rvar, cl * 4 + j, mu[j], va[j], (float)n, momentum);
    }
  }
  const auto [r0, r1] = row_span(rpb, n);
  for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (int64_t)nrl) {      // four rows in flight per thread
    float v[4][4], rs[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      const int64_t rc = r < r1 ? r : r0;
      *reinterpret_cast<float4*>(v[u]) = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
      if (residual) *reinterpret_cast<float4*>(rs[u]) = *reinterpret_cast<const float4*>(residual + rc * C + cl * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      if (r >= r1) continue;
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = norm_act_elem(v[u][j], mu[j], is[j], g[j], bt[j], residual ? &rs[u][j] : nullptr, act);
      const int q = add_inv ? add_inv[r] : -1;
      if (q >= 0) {
        const float4 f = *reinterpret_cast<const float4*>(add_src + (int64_t)q * C + cl * 4);
        o[0] += f.x; o[1] += f.y; o[2] += f.z; o[3] += f.w;
      }
      *reinterpret_cast<float4*>(y + r * C + cl * 4) = *reinterpret_cast<float4*>(o);
    }
  }
}

// general-size BatchNorm statistics, finalisation: one 1024-thread block per 64 channels reduces the
// [nb][2][C] shifted partial sums of k_bn1_partial (fixed order), writes mean / biased var / count and applies the
// nn.BatchNorm1d running-buffer update — 3 launches per training-mode BatchNorm forward instead of 6.
__global__ __launch_bounds__(1024) void k_bn_finalize(const float* __restrict__ part, int nb, int C, int64_t n,
                                                      const float* __restrict__ x, float momentum, float* __restrict__ mean,
                                                      float* __restrict__ var, float* __restrict__ cnt,
                                                      float* __restrict__ rmean, float* __restrict__ rvar,
                                                      long long* __restrict__ nbt) {
  __shared__ float r1[16][65], r2[16][65];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), j = threadIdx.x >> 6;
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    float p1[4] = {0.f, 0.f, 0.f, 0.f}, p2[4] = {0.f, 0.f, 0.f, 0.f};      // four blocks' partials in flight (see k_stats_final)
    int b = j;
    for (; b + 48 < nb; b += 64) {
      float u[4], w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        u[q] = fc_ld(&part[((int64_t)(b + 16 * q) * 2) * C + c]);
        w[q] = fc_ld(&part[((int64_t)(b + 16 * q) * 2 + 1) * C + c]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) { p1[q] += u[q]; p2[q] += w[q]; }
    }
    for (; b < nb; b += 16) {
      p1[0] += fc_ld(&part[((int64_t)b * 2) * C + c]);
      p2[0] += fc_ld(&part[((int64_t)b * 2 + 1) * C + c]);
    }
    a1 = (p1[0] + p1[1]) + (p1[2] + p1[3]);
    a2 = (p2[0] + p2[1]) + (p2[2] + p2[3]);
  }
  r1[j][threadIdx.x & 63] = a1;
  r2[j][threadIdx.x & 63] = a2;
  __syncthreads();
  if (j == 0 && c < C) {
    float s1 = 0.f, s2 = 0.f;
    for (int q = 0; q < 16; ++q) { s1 += r1[q][threadIdx.x & 63]; s2 += r2[q][threadIdx.x & 63]; }
    const float inv_n = 1.f / (float)n;
    float d = s1 * inv_n;
    float mu = x[c] + d;
    float va = fmaxf(s2 * inv_n - d * d, 0.f);
    mean[c] = mu;
    var[c] = va;
    if (c == 0) { cnt[0] = (float)n; if (nbt) nbt[0] += 1; }
    if (rmean) bn_running_update(rmean, rvar, c, mu, va, (float)n, momentum);
  }
}

// backward launch 2: reduce the partials of k_norm_bwd_partial (nseg = 1, layout [nb][1][2][C]) and apply
__global__ void k_bn1_bwd_apply(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                const float* __restrict__ gy2, int64_t n, int C, int64_t rpb, const float* __restrict__ part, int nb,
                                const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                const float* __restrict__ gamma, const float* __restrict__ beta, int act,
                                float* __restrict__ gx, float* __restrict__ gres, float* __restrict__ sums /*[2][C]*/, int CG,
                                unsigned* __restrict__ amax_out) {
  // r6: grid.y channel windows of CG channels (few rows x many channels — 872 x 512 — used to be 14 blocks of 2 row lanes, 49 us)
  extern __shared__ float sm[];
  const int c0 = blockIdx.y * CG;
  x += c0; gy += c0; gx += c0; mean += c0; var += c0;
  if (y) y += c0;
  if (gy2) gy2 += c0;
  if (gres) gres += c0;
  if (gamma) gamma += c0;
  if (beta) beta += c0;
  const int c4n = CG / 4;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;      // (a copy of lane_coord, as in k_bn1_apply)
  const int nrl = blockDim.x / c4n;
  float4 t1, t2;
  bn1_reduce_parts(part, nb, C, cl, rl, nrl, sm, &t1, &t2, CG, c0);
  if (blockIdx.x == 0 && rl == 0) {
    *reinterpret_cast<float4*>(sums + c0 + cl * 4) = t1;
    *reinterpret_cast<float4*>(sums + C + c0 + cl * 4) = t2;
  }
  const float inv_n = 1.f / (float)n;
  float s1[4] = {t1.x * inv_n, t1.y * inv_n, t1.z * inv_n, t1.w * inv_n};
  float s2[4] = {t2.x * inv_n, t2.y * inv_n, t2.z * inv_n, t2.w * inv_n};
  float mu[4], is[4], g[4], bt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mu[j] = mean[cl * 4 + j];
    is[j] = 1.f / sqrtf(var[cl * 4 + j] + eps);
    g[j] = gamma ? gamma[cl * 4 + j] : 1.f;
    bt[j] = beta ? beta[cl * 4 + j] : 0.f;
  }
  const bool from_y = act && y;
  const auto [r0, r1] = row_span(rpb, n);
  unsigned am = 0u;
  for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (int64_t)nrl) {      // four rows (x, gy, y of each) in flight per thread
    float xv[4][4], gv[4][4], yv[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      const int64_t rc = r < r1 ? r : r0;
      *reinterpret_cast<float4*>(xv[u]) = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
      *reinterpret_cast<float4*>(gv[u]) = *reinterpret_cast<const float4*>(gy + rc * C + cl * 4);
      if (gy2) {
        const float4 t2 = *reinterpret_cast<const float4*>(gy2 + rc * C + cl * 4);
        gv[u][0] += t2.x; gv[u][1] += t2.y; gv[u][2] += t2.z; gv[u][3] += t2.w;
      }
      if (from_y) *reinterpret_cast<float4*>(yv[u]) = *reinterpret_cast<const float4*>(y + rc * C + cl * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      if (r >= r1) continue;
      float o[4], gr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gg = gv[u][j];
        if (from_y) gg *= act_bwd_from_y(yv[u][j], act);
        else if (act) gg *= act_bwd_from_pre(bn_pre(xv[u][j], mu[j], is[j], g[j], bt[j]), act);
        float xh = (xv[u][j] - mu[j]) * is[j];
        gr[j] = gg;
        o[j] = g[j] * is[j] * (gg - s1[j] - xh * s2[j]);
      }
      *reinterpret_cast<float4*>(gx + r * C + cl * 4) = *reinterpret_cast<float4*>(o);
      if (gres) *reinterpret_cast<float4*>(gres + r * C + cl * 4) = *reinterpret_cast<float4*>(gr);
#pragma unroll
      for (int j = 0; j < 4; ++j) amax_fold(am, o[j]);
    }
  }
  if (amax_out) amax_commit(am, amax_out);
}

// ================================================================================================
// r5: BatchNorm statistics out of the PRODUCER's epilogue.  The kernel that writes a convolution's result (the MFMA tile epilogue
// of k_conv_x6, or the fixed-order sums k_sum_parts_stats / k_sum_pairs_stats of an offset-split / pair-list launch) also leaves,
// per row block, the column sums of x and x^2 of the rows it wrote: part[nb][2][G * C] (plain fp32 sums over <= a few hundred
// rows; G > 1: the (n, G C) matrix of a generative transposed convolution's GEMM viewed as (G n, C): channel c collects the
// columns g C + c).  They are combined in fp64 in a fixed order — mean = S1 / n, var = S2 / n - mean^2 (bn2_stats, norm_elem.h) —
// either in the prologue of the apply kernel (<= BN1_MAXB partial blocks: ONE launch per BatchNorm) or by k_bn2_finalize (two
// launches).  The read pass over x of k_bn1_partial is gone (r4: 46 launches, 0.32 ms alone / 0.56 ms beside the weight-gradient stream).
__global__ void k_bn2_apply(const float* __restrict__ x, int64_t n, int C, int64_t rpb, const float* __restrict__ part, int nb, int G,
                            float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                            const float* __restrict__ residual, int act, float momentum, float* __restrict__ y,
                            float* __restrict__ mean_out, float* __restrict__ var_out, float* __restrict__ cnt_out,
                            float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ nbt, int CG,
                            const int* __restrict__ add_inv, const float* __restrict__ add_src, unsigned* __restrict__ amax_out) {
  // r6: grid.y channel windows of CG channels (see k_bn1_bwd_apply); add_inv / add_src: see k_norm_act_fwd
  extern __shared__ double smd[];             // [nrl][2][CG]
  const int c0 = blockIdx.y * CG;
  x += c0; y += c0; part += c0; mean_out += c0; var_out += c0;
  if (add_src) add_src += c0;
  if (residual) residual += c0;
  if (gamma) gamma += c0;
  if (beta) beta += c0;
  if (rmean) { rmean += c0; rvar += c0; }
  const auto [cl, rl, nrl] = lane_coord(CG / 4);
  double a1[4] = {0., 0., 0., 0.}, a2[4] = {0., 0., 0., 0.};
  const int GC = G * C;
  for (int t = rl; t < nb * G; t += nrl) {            // (block, group) pairs, fixed order per row lane
    const int b = t / G, g = t % G;
    const float* src = part + ((int64_t)b * 2) * GC + g * C + cl * 4;
    const float4 u = fc_ld4(src), w = fc_ld4(src + GC);
    a1[0] += u.x; a1[1] += u.y; a1[2] += u.z; a1[3] += u.w;
    a2[0] += w.x; a2[1] += w.y; a2[2] += w.z; a2[3] += w.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    smd[(rl * 2 + 0) * CG + cl * 4 + j] = a1[j];
    smd[(rl * 2 + 1) * CG + cl * 4 + j] = a2[j];
  }
  __syncthreads();
  float mu[4], va[4], is[4], g[4], bt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double t1 = 0., t2 = 0.;
    for (int q = 0; q < nrl; ++q) { t1 += smd[(q * 2 + 0) * CG + cl * 4 + j]; t2 += smd[(q * 2 + 1) * CG + cl * 4 + j]; }
    bn2_stats(t1, t2, n, &mu[j], &va[j]);
    is[j] = 1.f / sqrtf(va[j] + eps);
    g[j] = gamma ? gamma[cl * 4 + j] : 1.f;
    bt[j] = beta ? beta[cl * 4 + j] : 0.f;
  }
  if (blockIdx.x == 0 && rl == 0) {
    *reinterpret_cast<float4*>(mean_out + cl * 4) = make_float4(mu[0], mu[1], mu[2], mu[3]);
    *reinterpret_cast<float4*>(var_out + cl * 4) = make_float4(va[0], va[1], va[2], va[3]);
    if (cl == 0 && blockIdx.y == 0) { cnt_out[0] = (float)n; if (nbt) nbt[0] += 1; }
    if (rmean) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bn_running_update(rmean, rvar, cl * 4 + j, mu[j], va[j], (float)n, momentum);
    }
  }
  const auto [r0, r1] = row_span(rpb, n);
  unsigned am = 0u;
  for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (int64_t)nrl) {      // four rows in flight per thread
    float v[4][4], rs[4][4];
    int q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      const int64_t rc = r < r1 ? r : r0;
      *reinterpret_cast<float4*>(v[u]) = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
      if (residual) *reinterpret_cast<float4*>(rs[u]) = *reinterpret_cast<const float4*>(residual + rc * C + cl * 4);
      q[u] = add_inv ? add_inv[rc] : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      if (r >= r1) continue;
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = norm_act_elem(v[u][j], mu[j], is[j], g[j], bt[j], residual ? &rs[u][j] : nullptr, act);
      if (q[u] >= 0) {
        const float4 f = *reinterpret_cast<const float4*>(add_src + (int64_t)q[u] * C + cl * 4);
        o[0] += f.x; o[1] += f.y; o[2] += f.z; o[3] += f.w;
      }
      *reinterpret_cast<float4*>(y + r * C + cl * 4) = *reinterpret_cast<float4*>(o);
#pragma unroll
      for (int j = 0; j < 4; ++j) amax_fold(am, o[j]);
    }
  }
  if (amax_out) amax_commit(am, amax_out);
}

// many partial blocks: one 256-thread block per 4 channels (64 slices of the table each) adds them (fp64, fixed order) and writes
// mean / biased var / count + the nn.BatchNorm1d running-buffer update; follow with k_norm_act_fwd
__global__ __launch_bounds__(256) void k_bn2_finalize(const float* __restrict__ part, int nb, int C, int G, int64_t n, float momentum,
                                                       float* __restrict__ mean, float* __restrict__ var, float* __restrict__ cnt,
                                                       float* __restrict__ rmean, float* __restrict__ rvar,
                                                       long long* __restrict__ nbt) {
  __shared__ double r1[FIN_SL][FIN_CB + 1], r2[FIN_SL][FIN_CB + 1];
  const int cl = threadIdx.x & (FIN_CB - 1), j = threadIdx.x / FIN_CB;
  const int c = blockIdx.x * FIN_CB + cl;
  const int GC = G * C;
  double a1 = 0., a2 = 0.;
  if (c < C) {
    double p1[4] = {0., 0., 0., 0.}, p2[4] = {0., 0., 0., 0.};      // four partial blocks in flight
    const int total = nb * G;
    int t = j;
    for (; t + 3 * FIN_SL < total; t += 4 * FIN_SL) {
      float u[4], w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int tt = t + FIN_SL * q, b = tt / G, g = tt % G;
        u[q] = fc_ld(&part[((int64_t)b * 2) * GC + g * C + c]);
        w[q] = fc_ld(&part[((int64_t)b * 2 + 1) * GC + g * C + c]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) { p1[q] += u[q]; p2[q] += w[q]; }
    }
    for (; t < total; t += FIN_SL) {
      const int b = t / G, g = t % G;
      p1[0] += fc_ld(&part[((int64_t)b * 2) * GC + g * C + c]);
      p2[0] += fc_ld(&part[((int64_t)b * 2 + 1) * GC + g * C + c]);
    }
    a1 = (p1[0] + p1[1]) + (p1[2] + p1[3]);
    a2 = (p2[0] + p2[1]) + (p2[2] + p2[3]);
  }
  r1[j][cl] = a1;
  r2[j][cl] = a2;
  __syncthreads();
  if (j == 0 && c < C) {
    double s1 = 0., s2 = 0.;
    for (int q = 0; q < FIN_SL; ++q) { s1 += r1[q][cl]; s2 += r2[q][cl]; }
    float mu, va;
    bn2_stats(s1, s2, n, &mu, &va);
    mean[c] = mu;
    var[c] = va;
    if (c == 0) { cnt[0] = (float)n; if (nbt) nbt[0] += 1; }
    if (rmean) bn_running_update(rmean, rvar, c, mu, va, (float)n, momentum);
  }
}

// BatchNorm1d running statistics (momentum update with the unbiased variance) + num_batches_tracked, one launch
extern "C" __global__ void k_bn_running(const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ cnt,
                             float momentum, int C, float* __restrict__ rmean, float* __restrict__ rvar,
                             long long* __restrict__ nbt) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) nbt[0] += 1;
  if (c >= C) return;
  float n = cnt[0];
  float unbias = n / fmaxf(n - 1.f, 1.f);
  rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean[c];      // (a copy of bn_running_update: with mean / var read from memory the helper orders the loads differently)
  rvar[c] = (1.f - momentum) * rvar[c] + momentum * var[c] * unbias;
}
