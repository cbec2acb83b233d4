// Segmented column statistics (included by norm.hip): row-blocked partial sums, and the two kernels that add a table of partials in a fixed order.
#pragma once

// ---- pass 1: partial sums of f(x) per (block, segment, channel) --------------------------------
// sq == false: sum x, part layout [block][seg][C] ; sq (r5): sum x AND sum x^2 in one pass, part layout [block][seg][2][C]
// block = (C/4 lanes of float4) x (row lanes); C % 4 == 0, C <= 1024; rows [b*rpb, (b+1)*rpb)
__global__ void k_stats_partial(const float* __restrict__ x, const int* __restrict__ seg, int seg_stride, int64_t n, int C,
                                int nseg, bool sq, int64_t rpb, float* __restrict__ part, float* __restrict__ part_cnt) {
  extern __shared__ float sm[];               // [rl][C] staging for the cross-row-lane reduction
  __shared__ int srange[2];
  const int c4n = C / 4;
  const auto [cl, rl, nrl] = lane_coord(c4n);
  const auto [r0, r1] = row_span(rpb, n);
  int s_lo, s_hi;
  seg_range(seg, seg_stride, r0, r1, &s_lo, &s_hi, srange);
  // a row range inside ONE segment (almost every block: rows are nearly segment-contiguous) needs no per-row segment test —
  // r2: the test is a dependent 4-byte load in front of every row load (InstanceNorm of the 580k-row stem: 1.4 TB/s)
  const bool chk = seg && s_lo != s_hi;
  for (int s = 0; s < nseg; ++s) {
    float4 acc[4];
    float4 sqs = make_float4(0.f, 0.f, 0.f, 0.f);
    float cnt = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s >= s_lo && s <= s_hi) {
      for (int64_t rb = r0 + rl; rb < r1; rb += 4 * nrl) {
        float4 vv[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                     // the four rows are requested together (see k_norm_bwd_partial)
          const int64_t r = rb + (int64_t)u * nrl;
          ok[u] = r < r1;
          const int64_t rc = ok[u] ? r : r0;
          if (chk) ok[u] = ok[u] && seg[rc * seg_stride] == s;
          vv[u] = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!ok[u]) continue;
          float4 v = vv[u];
          if (sq) { sqs.x += v.x * v.x; sqs.y += v.y * v.y; sqs.z += v.z * v.z; sqs.w += v.w * v.w; }
          acc[u].x += v.x; acc[u].y += v.y; acc[u].z += v.z; acc[u].w += v.w;
          cnt += 1.f;
        }
      }
    }
    float4 a;
    a.x = (acc[0].x + acc[1].x) + (acc[2].x + acc[3].x);
    a.y = (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y);
    a.z = (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z);
    a.w = (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w);
    __syncthreads();
    *reinterpret_cast<float4*>(&sm[(rl * c4n + cl) * 4]) = a;
    float* smc = sm + nrl * C;
    if (cl == 0) smc[rl] = cnt;
    __syncthreads();
    const int64_t slot = (int64_t)blockIdx.x * nseg + s;
    float* dst = sq ? part + slot * 2 * C : part + slot * C;
    if (rl == 0) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < nrl; ++j) {
        float4 u = *reinterpret_cast<const float4*>(&sm[(j * c4n + cl) * 4]);
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      }
      *reinterpret_cast<float4*>(dst + cl * 4) = t;
      if (cl == 0 && part_cnt) {
        float c = 0.f;
        for (int j = 0; j < nrl; ++j) c += smc[j];
        part_cnt[slot] = c;
      }
    }
    if (sq) {                                    // the squares through the same staging buffer
      __syncthreads();
      *reinterpret_cast<float4*>(&sm[(rl * c4n + cl) * 4]) = sqs;
      __syncthreads();
      if (rl == 0) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < nrl; ++j) {
          float4 u = *reinterpret_cast<const float4*>(&sm[(j * c4n + cl) * 4]);
          t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        *reinterpret_cast<float4*>(dst + C + cl * 4) = t;
      }
    }
  }
}

// r5: per-segment mean / biased variance / count from the one-pass partials of k_stats_partial with squares ([block][seg][2][C] +
// counts [block][seg]): 4 channels x 64 slices per 256-thread block, fp64 accumulation in a fixed order (the instance norm of the
// stem read its 148 MB input twice — mean, then centred squares — in four launches; now once, in two)
static_assert(FIN_CB == 4 && FIN_SL == 64, "k_seg_meanvar_final spells out the 4 channels x 64 slices its launch (final_launch) gives it");
__global__ __launch_bounds__(256) void k_seg_meanvar_final(const float* __restrict__ part, const float* __restrict__ part_cnt,
                                                           int64_t nblocks, int nseg, int C, float* __restrict__ mean,
                                                           float* __restrict__ var, float* __restrict__ cnt_out) {
  __shared__ double r1[64][5], r2[64][5], rc[64];
  const int cgroups = (C + 3) / 4;
  const int s = blockIdx.x / cgroups, cg = blockIdx.x % cgroups;
  const int cl = threadIdx.x & 3, j = threadIdx.x >> 2;
  const int c = cg * 4 + cl;
  double a1 = 0., a2 = 0., ac = 0.;
  if (c < C) {
    for (int64_t b = j; b < nblocks; b += 64) {
      const float* src = part + ((b * nseg + s) * 2) * C;
      a1 += fc_ld(&src[c]);
      a2 += fc_ld(&src[C + c]);
      if (cl == 0) ac += fc_ld(&part_cnt[b * nseg + s]);
    }
  }
  r1[j][cl] = a1; r2[j][cl] = a2;
  if (cl == 0) rc[j] = ac;
  __syncthreads();
  if (j == 0 && c < C) {
    double s1 = 0., s2 = 0., n = 0.;
    for (int q = 0; q < 64; ++q) { s1 += r1[q][cl]; s2 += r2[q][cl]; n += rc[q]; }
    double m = 0., v = 0.;
    if (n > 0.) {
      m = s1 / n;
      v = s2 / n - m * m;
      if (v < 0.) v = 0.;
    }
    mean[(int64_t)s * C + c] = (float)m;
    var[(int64_t)s * C + c] = (float)v;
    if (c == 0) cnt_out[s] = (float)n;
  }
}

// ---- pass 2: out[seg][c] = the sum of part[block][seg][c] over the blocks (fixed order); block = FIN_CB channels x FIN_SL slices (256
// threads since r5: norm_route.h)
__global__ __launch_bounds__(256) void k_stats_final(const float* __restrict__ part, int64_t nblocks, int nseg, int C, float* __restrict__ out) {
  __shared__ float red[FIN_SL][FIN_CB + 1];
  const int cgroups = (C + FIN_CB - 1) / FIN_CB;
  const int s = blockIdx.x / cgroups, cg = blockIdx.x % cgroups;
  const int cl = threadIdx.x & (FIN_CB - 1), j = threadIdx.x / FIN_CB;
  const int c = cg * FIN_CB + cl;
  // four partials in flight per thread (r3: one dependent load per iteration made these tiny launches 13 us each); the
  // summation order is fixed by the code, hence still deterministic
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < C) {
    const float* p = part + (int64_t)s * C + c;      // (one block reads the table once: past the L1)
    const int64_t st = (int64_t)nseg * C;
    int64_t b = j;
    for (; b + 3 * FIN_SL < nblocks; b += 4 * FIN_SL) {
      const float v0 = fc_ld(&p[b * st]), v1 = fc_ld(&p[(b + FIN_SL) * st]);
      const float v2 = fc_ld(&p[(b + 2 * FIN_SL) * st]), v3 = fc_ld(&p[(b + 3 * FIN_SL) * st]);
      a0 += v0; a1 += v1; a2 += v2; a3 += v3;
    }
    for (; b < nblocks; b += FIN_SL) a0 += fc_ld(&p[b * st]);
  }
  red[j][cl] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (j == 0 && c < C) {
    float t = 0.f;
    for (int q = 0; q < FIN_SL; ++q) t += red[q][cl];
    out[(int64_t)s * C + c] = t;
  }
}
