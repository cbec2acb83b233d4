// Bandwidth-bound feature-matrix ops on gfx950: segmented column statistics (BatchNorm over all
// voxels / InstanceNorm per scene), fused normalise + affine + residual + ReLU/ELU forward and
// backward, max pooling over the k2s2 kernel map, row gather / scatter.
// All reductions are two-level with a fixed summation order (deterministic, no float atomics).
//
// Replaces MinkowskiBatchNorm / MinkowskiInstanceNorm / MinkowskiReLU / MinkowskiELU /
// MinkowskiMaxPooling / MinkowskiPruning feature paths used at me_resnet.py:22-24,63,
// BasicBlock (MinkowskiEngine.modules.resnet_block), fcaf3d_neck_with_head.py:53-54,67-71,76,125.
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "norm_route.h"      // every launch's geometry, the row-block caps, FIN_CB x FIN_SL

__device__ static inline int seg_of(const int* seg, int seg_stride, int64_t row) {
  return seg ? seg[row * seg_stride] : 0;
}

// segment range touched by rows [r0,r1) — block-parallel min/max (rows are nearly segment-contiguous)
__device__ static inline void seg_range(const int* seg, int seg_stride, int64_t r0, int64_t r1, int* lo, int* hi,
                                        int* sh /*[2] shared*/) {
  if (!seg) { *lo = 0; *hi = 0; return; }
  if (threadIdx.x == 0) { sh[0] = 0x7fffffff; sh[1] = -1; }
  __syncthreads();
  int l = 0x7fffffff, h = -1;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    int s = seg[r * seg_stride];
    l = s < l ? s : l;
    h = s > h ? s : h;
  }
  if (h >= 0) { atomicMin(&sh[0], l); atomicMax(&sh[1], h); }
  __syncthreads();
  *lo = sh[0]; *hi = sh[1];
  __syncthreads();
}

// ---- pass 1: partial sums of f(x) per (block, segment, channel) --------------------------------
// mode 0: sum x ; mode 1: sum (x-mean[seg])^2 ; mode 2 (r5): sum x AND sum x^2 in one pass, part layout [block][seg][2][C]
// block = (C/4 lanes of float4) x (row lanes); C % 4 == 0, C <= 1024; rows [b*rpb, (b+1)*rpb)
__global__ void k_stats_partial(const float* __restrict__ x, const int* __restrict__ seg, int seg_stride, int64_t n, int C,
                                int nseg, const float* __restrict__ mean, int mode, int64_t rpb, float* __restrict__ part,
                                float* __restrict__ part_cnt) {
  extern __shared__ float sm[];               // [rl][C] staging for the cross-row-lane reduction
  __shared__ int srange[2];
  const int c4n = C / 4;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  const int nrl = blockDim.x / c4n;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t r1 = r0 + rpb;
  if (r1 > n) r1 = n;
  int s_lo, s_hi;
  seg_range(seg, seg_stride, r0, r1, &s_lo, &s_hi, srange);
  // a row range inside ONE segment (almost every block: rows are nearly segment-contiguous) needs no per-row segment test —
  // r2: the test is a dependent 4-byte load in front of every row load (InstanceNorm of the 580k-row stem: 1.4 TB/s)
  const bool chk = seg && s_lo != s_hi;
  for (int s = 0; s < nseg; ++s) {
    float4 acc[4];
    float4 sq = make_float4(0.f, 0.f, 0.f, 0.f);
    float cnt = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s >= s_lo && s <= s_hi) {
      float4 mu = make_float4(0.f, 0.f, 0.f, 0.f);
      if (mode == 1) mu = *reinterpret_cast<const float4*>(mean + (int64_t)s * C + cl * 4);
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
          if (mode == 1) {
            v.x -= mu.x; v.y -= mu.y; v.z -= mu.z; v.w -= mu.w;
            v.x *= v.x; v.y *= v.y; v.z *= v.z; v.w *= v.w;
          }
          if (mode == 2) { sq.x += v.x * v.x; sq.y += v.y * v.y; sq.z += v.z * v.z; sq.w += v.w * v.w; }
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
    float* dst = mode == 2 ? part + slot * 2 * C : part + slot * C;
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
    if (mode == 2) {                             // the squares through the same staging buffer
      __syncthreads();
      *reinterpret_cast<float4*>(&sm[(rl * c4n + cl) * 4]) = sq;
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

// r5: per-segment mean / biased variance / count from the one-pass partials of k_stats_partial mode 2 ([block][seg][2][C] +
// counts [block][seg]): 4 channels x 64 slices per 256-thread block, fp64 accumulation in a fixed order (the instance norm of the
// stem read its 148 MB input twice — mean, then centred squares — in four launches; now once, in two)
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

// ---- pass 2: sum partials over blocks (fixed order); block = 16 channels x 64 slices -----------------
// mode 0: out = sum / cnt (mean), also writes cnt[seg];  mode 1: out = sum / cnt (biased variance); mode 2: out = sum
// (FIN_CB channels x FIN_SL slices per block, 256 threads since r5: norm_route.h)
__global__ __launch_bounds__(256) void k_stats_final(const float* __restrict__ part, const float* __restrict__ part_cnt,
                                                      int64_t nblocks, int nseg, int C, int mode, float* __restrict__ out,
                                                      float* __restrict__ cnt_io) {
  __shared__ float red[FIN_SL][FIN_CB + 1];
  __shared__ float redc[FIN_SL];
  const int cgroups = (C + FIN_CB - 1) / FIN_CB;
  const int s = blockIdx.x / cgroups, cg = blockIdx.x % cgroups;
  const int cl = threadIdx.x & (FIN_CB - 1), j = threadIdx.x / FIN_CB;
  const int c = cg * FIN_CB + cl;
  // four partials in flight per thread (r3: one dependent load per iteration made these tiny launches 13 us each); the
  // summation order is fixed by the code, hence still deterministic
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (c < C) {
    int64_t b = j;
    for (; b + 3 * FIN_SL < nblocks; b += 4 * FIN_SL) {
      const float v0 = fc_ld(&part[(b * nseg + s) * C + c]), v1 = fc_ld(&part[((b + FIN_SL) * nseg + s) * C + c]);      // (one block reads the
      const float v2 = fc_ld(&part[((b + 2 * FIN_SL) * nseg + s) * C + c]), v3 = fc_ld(&part[((b + 3 * FIN_SL) * nseg + s) * C + c]);   //  table once: past the L1)
      a0 += v0; a1 += v1; a2 += v2; a3 += v3;
    }
    for (; b < nblocks; b += FIN_SL) a0 += fc_ld(&part[(b * nseg + s) * C + c]);
  }
  float acc = (a0 + a1) + (a2 + a3);
  red[j][cl] = acc;
  if (mode == 0 && cl == 0) {
    float cc = 0.f;
    for (int64_t b = j; b < nblocks; b += FIN_SL) cc += fc_ld(&part_cnt[b * nseg + s]);
    redc[j] = cc;
  }
  __syncthreads();
  if (j == 0 && c < C) {
    float t = 0.f;
    for (int q = 0; q < FIN_SL; ++q) t += red[q][cl];
    float cnt = 1.f;
    if (mode == 0) {
      float cc = 0.f;
      for (int q = 0; q < FIN_SL; ++q) cc += redc[q];
      if (c == 0) cnt_io[s] = cc;
      cnt = cc;
    } else if (mode == 1) {
      cnt = cnt_io[s];
    }
    out[(int64_t)s * C + c] = (mode == 2) ? t : (cnt > 0.f ? t / cnt : 0.f);
  }
}

__device__ static inline float act_fwd(float v, int act) {
  if (act == 1) return v > 0.f ? v : 0.f;
  if (act == 2) return v > 0.f ? v : expm1f(v);
  return v;
}
// derivative expressed through the OUTPUT y (ReLU: y>0 ; ELU(alpha=1): y>0 ? 1 : y+1)
__device__ static inline float act_bwd_from_y(float y, int act) {
  if (act == 1) return y > 0.f ? 1.f : 0.f;
  if (act == 2) return y > 0.f ? 1.f : y + 1.f;
  return 1.f;
}

// The pre-activation of a normalised element, ONE instruction sequence for the forward kernels and for the backward
// kernels that recompute it (r3: without a residual the backward pass derives act'(.) from x instead of reading y —
// 2 of 7 passes over the matrix gone; the explicit fmaf keeps the recomputed sign bit-identical to the forward's)
__device__ static inline float bn_pre(float v, float mu, float is, float g, float b) { return fmaf((v - mu) * is, g, b); }
// derivative of the activation from its PRE-activation p (ReLU: p > 0; ELU(alpha=1): p > 0 ? 1 : exp(p) = y + 1)
__device__ static inline float act_bwd_from_pre(float p, int act) {
  if (act == 1) return p > 0.f ? 1.f : 0.f;
  if (act == 2) return p > 0.f ? 1.f : expf(p);
  return 1.f;
}

// ---- r6: max |.| of what a kernel writes, for the convolution that will gather it (csrc/conv_x6.h h3: the operand's scale) ----------
// A producer that is told where (fc_amax_out_hint -> amax_out, a ZEROED slot of FC_AMAX_SUB sub-words) folds the finite elements it
// stores into one integer atomicMax per block on its block's sub-word — skipped when that already holds a larger value — instead of
// the consumer reading the tensor once more (fc_amax).  Integer max: order-independent, bit-reproducible.  EVERY lane of the wave must reach amax_commit.
thread_local unsigned* t_fc_amax_out = nullptr;          // fc_amax_out_hint: consumed by the next producer entry point of this thread (fc_common.h)

// y = act( (x-mean[seg])*invstd[seg]*gamma + beta (+ residual) ) ; invstd = 1/sqrt(var+eps)
// add_inv (nullable, r7): y[r] += add_src[add_inv[r]] where add_inv[r] >= 0, behind the activation — the neck's sparse sum
// `inputs[i] + x` written by the up block's last normalisation instead of a copy + scatter-add + amax pass over the union
__global__ void k_norm_act_fwd(const float* __restrict__ x, const int* __restrict__ seg, int seg_stride, int64_t n, int C,
                               const float* __restrict__ mean, const float* __restrict__ var, float eps,
                               const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ residual, int act, const int* __restrict__ add_inv,
                               const float* __restrict__ add_src, float* __restrict__ y, unsigned* __restrict__ amax_out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  unsigned am = 0u;
  if (t < n * c4n) {
  int64_t r = t / c4n;
  int c = (int)(t % c4n) * 4;
  int s = seg_of(seg, seg_stride, r);
  const int q = add_inv ? add_inv[r] : -1;
  float4 v = *reinterpret_cast<const float4*>(x + r * C + c);
  float4 mu = *reinterpret_cast<const float4*>(mean + (int64_t)s * C + c);
  float4 va = *reinterpret_cast<const float4*>(var + (int64_t)s * C + c);
  float4 g = gamma ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f);
  float4 b = beta ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 o;
  o.x = bn_pre(v.x, mu.x, 1.f / sqrtf(va.x + eps), g.x, b.x);
  o.y = bn_pre(v.y, mu.y, 1.f / sqrtf(va.y + eps), g.y, b.y);
  o.z = bn_pre(v.z, mu.z, 1.f / sqrtf(va.z + eps), g.z, b.z);
  o.w = bn_pre(v.w, mu.w, 1.f / sqrtf(va.w + eps), g.w, b.w);
  if (residual) {
    float4 rs = *reinterpret_cast<const float4*>(residual + r * C + c);
    o.x += rs.x; o.y += rs.y; o.z += rs.z; o.w += rs.w;
  }
  o.x = act_fwd(o.x, act); o.y = act_fwd(o.y, act); o.z = act_fwd(o.z, act); o.w = act_fwd(o.w, act);
  if (q >= 0) {                                  // the sparse sum behind the activation: + add_src[add_inv[r]] (one fp32 add, as fc_scatter_rows_add)
    const float4 f = *reinterpret_cast<const float4*>(add_src + (int64_t)q * C + c);
    o.x += f.x; o.y += f.y; o.z += f.z; o.w += f.w;
  }
  *reinterpret_cast<float4*>(y + r * C + c) = o;
  amax_fold(am, o.x); amax_fold(am, o.y); amax_fold(am, o.z); amax_fold(am, o.w);
  }
  if (amax_out) amax_commit(am, amax_out);
}

// backward pass 1: per (block, seg, channel) partial sums of g' and g'*xhat, g' = gy * act'(y)
// part layout: [block][seg][2][C]
// y == NULL (no residual in the forward): act'(.) is recomputed from x with gamma / beta (bn_pre) instead of read from y
// gy2 (nullable, r5): a second contribution to the incoming gradient — g = gy + gy2 is formed on the fly here and, with the same
// operands in the same order, in the apply kernels: the executor no longer materialises the sum where a normalised tensor has
// two consumers (k_add_inplace: 22 launches per step in r4)
// pool_parent / pool_arg (nullable, r7): the layer's output went through a k2s2 max pool and gy is the gradient of the POOLED tensor —
// row r's incoming gradient is gy[pool_parent[r]][c] where pool_arg[pool_parent[r]][c] == r, else 0: what fc_maxpool_bwd scatters into a
// zeroed matrix, formed on the fly.  Only the loads differ: the sums run over the same rows in the same order, hence the same bits.
// (A template parameter, not a run-time test: the plain instantiation is the kernel every other layer runs and keeps its code.)
template <bool POOL>
__global__ void k_norm_bwd_partial(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                   const float* __restrict__ gy2, const int* __restrict__ pool_parent,
                                   const int* __restrict__ pool_arg, const int* __restrict__ seg, int seg_stride, int64_t n, int C, int nseg,
                                   const float* __restrict__ mean, const float* __restrict__ var, float eps, int act,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   int64_t rpb, float* __restrict__ part) {
  extern __shared__ float sm[];               // [rl][2][C]
  __shared__ int srange[2];
  const int c4n = C / 4;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  const int nrl = blockDim.x / c4n;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t r1 = r0 + rpb;
  if (r1 > n) r1 = n;
  int s_lo, s_hi;
  seg_range(seg, seg_stride, r0, r1, &s_lo, &s_hi, srange);
  // a row range inside ONE segment (almost every block: rows are nearly segment-contiguous) needs no per-row segment test —
  // r2: the test is a dependent 4-byte load in front of every row load (InstanceNorm of the 580k-row stem: 1.4 TB/s)
  const bool chk = seg && s_lo != s_hi;
  for (int s = 0; s < nseg; ++s) {
    float4 a1[4], a2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { a1[u] = make_float4(0.f, 0.f, 0.f, 0.f); a2[u] = a1[u]; }
    if (s >= s_lo && s <= s_hi) {
      float4 mu = *reinterpret_cast<const float4*>(mean + (int64_t)s * C + cl * 4);
      float4 va = *reinterpret_cast<const float4*>(var + (int64_t)s * C + cl * 4);
      float4 is = make_float4(1.f / sqrtf(va.x + eps), 1.f / sqrtf(va.y + eps), 1.f / sqrtf(va.z + eps),
                              1.f / sqrtf(va.w + eps));
      const float4 gm = gamma ? *reinterpret_cast<const float4*>(gamma + cl * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 bt = beta ? *reinterpret_cast<const float4*>(beta + cl * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      const bool from_y = act && y;
      for (int64_t rb = r0 + rl; rb < r1; rb += 4 * nrl) {
        // branch-free batch: the 4 x (x, gy, y) rows are requested together (rows past the range re-read row r0 and are
        // dropped by `ok`), r3 — a `continue` in front of each load serialised them
        float4 xv[4], gv[4], yv[4], g2[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t r = rb + (int64_t)u * nrl;
          ok[u] = r < r1;
          const int64_t rc = ok[u] ? r : r0;
          if (chk) ok[u] = ok[u] && seg[rc * seg_stride] == s;
          xv[u] = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
          if (POOL) {
            const int64_t o = pool_parent[rc];
            const int4 a = *reinterpret_cast<const int4*>(pool_arg + o * C + cl * 4);
            gv[u] = *reinterpret_cast<const float4*>(gy + o * C + cl * 4);
            gv[u].x = a.x == rc ? gv[u].x : 0.f; gv[u].y = a.y == rc ? gv[u].y : 0.f;
            gv[u].z = a.z == rc ? gv[u].z : 0.f; gv[u].w = a.w == rc ? gv[u].w : 0.f;
          } else {
            gv[u] = *reinterpret_cast<const float4*>(gy + rc * C + cl * 4);
          }
          if (gy2) g2[u] = *reinterpret_cast<const float4*>(gy2 + rc * C + cl * 4);
          if (from_y) yv[u] = *reinterpret_cast<const float4*>(y + rc * C + cl * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!ok[u]) continue;
          float4 g = gv[u];
          if (gy2) { g.x += g2[u].x; g.y += g2[u].y; g.z += g2[u].z; g.w += g2[u].w; }
          if (from_y) {
            g.x *= act_bwd_from_y(yv[u].x, act); g.y *= act_bwd_from_y(yv[u].y, act);
            g.z *= act_bwd_from_y(yv[u].z, act); g.w *= act_bwd_from_y(yv[u].w, act);
          } else if (act) {
            g.x *= act_bwd_from_pre(bn_pre(xv[u].x, mu.x, is.x, gm.x, bt.x), act);
            g.y *= act_bwd_from_pre(bn_pre(xv[u].y, mu.y, is.y, gm.y, bt.y), act);
            g.z *= act_bwd_from_pre(bn_pre(xv[u].z, mu.z, is.z, gm.z, bt.z), act);
            g.w *= act_bwd_from_pre(bn_pre(xv[u].w, mu.w, is.w, gm.w, bt.w), act);
          }
          a1[u].x += g.x; a1[u].y += g.y; a1[u].z += g.z; a1[u].w += g.w;
          a2[u].x += g.x * (xv[u].x - mu.x) * is.x; a2[u].y += g.y * (xv[u].y - mu.y) * is.y;
          a2[u].z += g.z * (xv[u].z - mu.z) * is.z; a2[u].w += g.w * (xv[u].w - mu.w) * is.w;
        }
      }
    }
    float4 b1 = make_float4((a1[0].x + a1[1].x) + (a1[2].x + a1[3].x), (a1[0].y + a1[1].y) + (a1[2].y + a1[3].y),
                            (a1[0].z + a1[1].z) + (a1[2].z + a1[3].z), (a1[0].w + a1[1].w) + (a1[2].w + a1[3].w));
    float4 b2 = make_float4((a2[0].x + a2[1].x) + (a2[2].x + a2[3].x), (a2[0].y + a2[1].y) + (a2[2].y + a2[3].y),
                            (a2[0].z + a2[1].z) + (a2[2].z + a2[3].z), (a2[0].w + a2[1].w) + (a2[2].w + a2[3].w));
    __syncthreads();
    *reinterpret_cast<float4*>(&sm[(rl * 2 + 0) * C + cl * 4]) = b1;
    *reinterpret_cast<float4*>(&sm[(rl * 2 + 1) * C + cl * 4]) = b2;
    __syncthreads();
    if (rl == 0) {
      float4 t1 = make_float4(0.f, 0.f, 0.f, 0.f), t2 = t1;
      for (int j = 0; j < nrl; ++j) {
        float4 u = *reinterpret_cast<const float4*>(&sm[(j * 2 + 0) * C + cl * 4]);
        float4 w = *reinterpret_cast<const float4*>(&sm[(j * 2 + 1) * C + cl * 4]);
        t1.x += u.x; t1.y += u.y; t1.z += u.z; t1.w += u.w;
        t2.x += w.x; t2.y += w.y; t2.z += w.z; t2.w += w.w;
      }
      float* dst = part + (((int64_t)blockIdx.x * nseg + s) * 2) * C;
      *reinterpret_cast<float4*>(dst + cl * 4) = t1;
      *reinterpret_cast<float4*>(dst + C + cl * 4) = t2;
    }
  }
}

// backward pass 3:  gx = gamma*invstd*( g' - sum_g/cnt - xhat * sum_gx/cnt ) ; gres = g'
// pool_parent / pool_arg: see k_norm_bwd_partial
template <bool POOL>
__global__ void k_norm_bwd_apply(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                 const float* __restrict__ gy2, const int* __restrict__ pool_parent,
                                 const int* __restrict__ pool_arg, const int* __restrict__ seg, int seg_stride, int64_t n, int C,
                                 const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                 const float* __restrict__ sums /*[seg][2][C]*/,
                                 const float* __restrict__ cnt, int act, float* __restrict__ gx, float* __restrict__ gres,
                                 unsigned* __restrict__ amax_out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  unsigned am = 0u;
  if (t < n * c4n) {
  int64_t r = t / c4n;
  int c = (int)(t % c4n) * 4;
  int s = seg_of(seg, seg_stride, r);
  float inv_n = 1.f / cnt[s];
  float xv[4], gv[4], muv[4], vav[4], gam[4], bet[4] = {0.f, 0.f, 0.f, 0.f}, s1[4], s2[4], yv[4], o[4], gr[4];
  *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(x + r * C + c);
  if (POOL) {
    const int64_t o = pool_parent[r];
    const int4 a = *reinterpret_cast<const int4*>(pool_arg + o * C + c);
    *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(gy + o * C + c);
    gv[0] = a.x == r ? gv[0] : 0.f; gv[1] = a.y == r ? gv[1] : 0.f; gv[2] = a.z == r ? gv[2] : 0.f; gv[3] = a.w == r ? gv[3] : 0.f;
  } else {
    *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(gy + r * C + c);
  }
  if (gy2) {
    const float4 t2 = *reinterpret_cast<const float4*>(gy2 + r * C + c);
    gv[0] += t2.x; gv[1] += t2.y; gv[2] += t2.z; gv[3] += t2.w;
  }
  *reinterpret_cast<float4*>(muv) = *reinterpret_cast<const float4*>(mean + (int64_t)s * C + c);
  *reinterpret_cast<float4*>(vav) = *reinterpret_cast<const float4*>(var + (int64_t)s * C + c);
  *reinterpret_cast<float4*>(s1) = *reinterpret_cast<const float4*>(sums + ((int64_t)s * 2) * C + c);
  *reinterpret_cast<float4*>(s2) = *reinterpret_cast<const float4*>(sums + ((int64_t)s * 2 + 1) * C + c);
  if (gamma) *reinterpret_cast<float4*>(gam) = *reinterpret_cast<const float4*>(gamma + c);
  else gam[0] = gam[1] = gam[2] = gam[3] = 1.f;
  const bool from_y = act && y;
  if (from_y) *reinterpret_cast<float4*>(yv) = *reinterpret_cast<const float4*>(y + r * C + c);
  if (beta) *reinterpret_cast<float4*>(bet) = *reinterpret_cast<const float4*>(beta + c);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float g = gv[j];
    float is = 1.f / sqrtf(vav[j] + eps);
    if (from_y) g *= act_bwd_from_y(yv[j], act);
    else if (act) g *= act_bwd_from_pre(bn_pre(xv[j], muv[j], is, gam[j], bet[j]), act);
    float xh = (xv[j] - muv[j]) * is;
    gr[j] = g;
    o[j] = gam[j] * is * (g - s1[j] * inv_n - xh * s2[j] * inv_n);
  }
  *reinterpret_cast<float4*>(gx + r * C + c) = *reinterpret_cast<float4*>(o);
  if (gres) *reinterpret_cast<float4*>(gres + r * C + c) = *reinterpret_cast<float4*>(gr);
#pragma unroll
  for (int j = 0; j < 4; ++j) amax_fold(am, o[j]);
  }
  if (amax_out) amax_commit(am, amax_out);
}

// ---- max pooling over a (K, n_out) neighbour table ---------------------------------------------
__global__ void k_maxpool_fwd(const float* __restrict__ in, const int* __restrict__ nbr, int64_t n_out, int K, int C,
                              float* __restrict__ out, int* __restrict__ argrow) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out * C) return;
  int64_t o = t / C;
  int c = (int)(t % C);
  float best = -INFINITY;
  int arg = -1;
  for (int k = 0; k < K; ++k) {
    int i = nbr[(int64_t)k * n_out + o];
    if (i < 0) continue;
    float v = in[(int64_t)i * C + c];
    if (arg < 0 || v > best) { best = v; arg = i; }   // first max in offset order wins ties (A.5)
  }
  out[t] = arg < 0 ? 0.f : best;
  argrow[t] = arg;
}

// k2s2 (K == 8), C % 4 == 0: one thread per (output row, 4 channels); the 8 child rows are looked up first, then their
// 8 x 16 B are in flight together (the scalar kernel above keeps one dependent 4-byte load per lane in flight: 1.6 TB/s)
__global__ void k_maxpool8_fwd(const float* __restrict__ in, const int* __restrict__ nbr, int64_t n_out, int C,
                               float* __restrict__ out, int* __restrict__ argrow, unsigned* __restrict__ amax_out) {
  const int c4n = C / 4;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned am = 0u;
  if (t < n_out * c4n) {
  const int64_t o = t / c4n;
  const int c = (int)(t % c4n) * 4;
  int idx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) idx[k] = nbr[(int64_t)k * n_out + o];
  float4 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = idx[k] < 0 ? 0 : idx[k];
    v[k] = *reinterpret_cast<const float4*>(in + (int64_t)i * C + c);
  }
  float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int arg[4] = {-1, -1, -1, -1};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (idx[k] < 0) continue;
    const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (arg[j] < 0 || e[j] > best[j]) { best[j] = e[j]; arg[j] = idx[k]; }   // first max in offset order wins ties (A.5)
  }
  float4 ob = make_float4(arg[0] < 0 ? 0.f : best[0], arg[1] < 0 ? 0.f : best[1], arg[2] < 0 ? 0.f : best[2], arg[3] < 0 ? 0.f : best[3]);
  *reinterpret_cast<float4*>(out + o * C + c) = ob;
  *reinterpret_cast<int4*>(argrow + o * C + c) = make_int4(arg[0], arg[1], arg[2], arg[3]);
  amax_fold(am, ob.x); amax_fold(am, ob.y); amax_fold(am, ob.z); amax_fold(am, ob.w);
  }
  if (amax_out) amax_commit(am, amax_out);
}

__global__ void k_maxpool_bwd(const float* __restrict__ gout, const int* __restrict__ argrow, int64_t n_out, int C,
                              float* __restrict__ gin) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out * C) return;
  int i = argrow[t];
  // k2s2 children are disjoint between output cells -> each (row, channel) receives at most one write
  if (i >= 0) gin[(int64_t)i * C + (t % C)] = gout[t];
}

// ---- r7: the stem's tail without its two n1-row intermediates ------------------------------------------------------------------
// Forward: instance norm + activation + k2s2 max pool in one pass.  One thread per (pooled row, 4 channels), as k_maxpool8_fwd; the
// 8 children's x values go through the SAME bn_pre / act_fwd sequence as k_norm_act_fwd before they are compared, so out / argrow
// (and y, when asked for) are bit for bit those of fc_norm_act_fwd + fc_maxpool_fwd.  The children of a pooled row lie in one
// scene (seg of the first present child).  y (nullable): the normalised tensor itself — every child has one parent, so every
// row is written once.  parent (nullable): parent[child row] = pooled row, for the backward pass (k_norm_bwd_* pool_parent).
__global__ void k_norm_act_maxpool8_fwd(const float* __restrict__ x, const int* __restrict__ seg, int seg_stride, int C,
                                        const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                        const float* __restrict__ gamma, const float* __restrict__ beta, int act,
                                        const int* __restrict__ nbr, int64_t n_out, float* __restrict__ out, int* __restrict__ argrow,
                                        float* __restrict__ y, int* __restrict__ parent, unsigned* __restrict__ amax_out) {
  const int c4n = C / 4;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned am = 0u;
  if (t < n_out * c4n) {
  const int64_t o = t / c4n;
  const int c = (int)(t % c4n) * 4;
  int idx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) idx[k] = nbr[(int64_t)k * n_out + o];
  if (parent) {                                  // one store per lane: the lane of channel group k writes child k's entry
    int mine = -1;
#pragma unroll
    for (int k = 0; k < 8; ++k) mine = (c == 4 * k) ? idx[k] : mine;
    if (mine >= 0) parent[mine] = (int)o;
  }
  float4 v[8];
  int first = -1;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = idx[k] < 0 ? 0 : idx[k];
    if (first < 0 && idx[k] >= 0) first = idx[k];
    v[k] = *reinterpret_cast<const float4*>(x + (int64_t)i * C + c);
  }
  float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int arg[4] = {-1, -1, -1, -1};
  if (first >= 0) {
    const int s = seg_of(seg, seg_stride, first);
    float mu[4], va[4], is[4], g[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<float4*>(mu) = *reinterpret_cast<const float4*>(mean + (int64_t)s * C + c);
    *reinterpret_cast<float4*>(va) = *reinterpret_cast<const float4*>(var + (int64_t)s * C + c);
    if (gamma) *reinterpret_cast<float4*>(g) = *reinterpret_cast<const float4*>(gamma + c);
    if (beta) *reinterpret_cast<float4*>(b) = *reinterpret_cast<const float4*>(beta + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) is[j] = 1.f / sqrtf(va[j] + eps);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (idx[k] < 0) continue;
      float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = act_fwd(bn_pre(e[j], mu[j], is[j], g[j], b[j]), act);
        if (arg[j] < 0 || e[j] > best[j]) { best[j] = e[j]; arg[j] = idx[k]; }   // first max in offset order wins ties (A.5)
      }
      if (y) *reinterpret_cast<float4*>(y + (int64_t)idx[k] * C + c) = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  float4 ob = make_float4(arg[0] < 0 ? 0.f : best[0], arg[1] < 0 ? 0.f : best[1], arg[2] < 0 ? 0.f : best[2], arg[3] < 0 ? 0.f : best[3]);
  *reinterpret_cast<float4*>(out + o * C + c) = ob;
  *reinterpret_cast<int4*>(argrow + o * C + c) = make_int4(arg[0], arg[1], arg[2], arg[3]);
  amax_fold(am, ob.x); amax_fold(am, ob.y); amax_fold(am, ob.z); amax_fold(am, ob.w);
  }
  if (amax_out) amax_commit(am, amax_out);
}

// inv[rows[i]] = i (inv pre-filled with -1; rows unique): generated row -> backbone row of a neck level's sparse sum
__global__ void k_inverse_rows(const int* __restrict__ rows, int64_t n, int64_t n_inv, int* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = rows[i];
  if (r >= 0 && r < n_inv) inv[r] = (int)i;
}

// ---- row gather / scatter ----------------------------------------------------------------------
__global__ void k_gather_rows(const float* __restrict__ src, const int* __restrict__ idx, int64_t n, int C,
                              float* __restrict__ dst) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * C) return;
  int64_t r = t / C;
  int i = idx[r];
  dst[t] = i >= 0 ? src[(int64_t)i * C + (t % C)] : 0.f;
}

// dst[idx[r]] += src[r]   (idx unique -> race free)
__global__ void k_scatter_rows_add(const float* __restrict__ src, const int* __restrict__ idx, int64_t n, int C,
                                   float* __restrict__ dst) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * C) return;
  int64_t r = t / C;
  int i = idx[r];
  if (i >= 0) dst[(int64_t)i * C + (t % C)] += src[t];
}

// ================================================================================================
// Small-tensor BatchNorm (n*C <= 4 M elements: backbone levels 2-4, coarse neck levels): TWO launches per
// direction instead of six / three.  Launch 1 writes per-block partial sums; launch 2 lets every block
// re-reduce the (<= 64) partials in its prologue (a few hundred KB out of L2) and apply straight away.
// Forward statistics in one pass: sums of (x - s) and (x - s)^2 with the shift s = x[0][c] (a sample of the
// column, so |mean - s| ~ sigma and E[(x-s)^2] - E[x-s]^2 loses no digits).

// part [nb][2][C]
__global__ void k_bn1_partial(const float* __restrict__ x, int64_t n, int C, int64_t rpb, float* __restrict__ part) {
  extern __shared__ float sm[];               // [rl][2][C]
  const int c4n = C / 4;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  const int nrl = blockDim.x / c4n;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t r1 = r0 + rpb;
  if (r1 > n) r1 = n;
  const float4 sh = *reinterpret_cast<const float4*>(x + cl * 4);
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
  for (int64_t rb = r0 + rl; rb < r1; rb += 4 * (int64_t)nrl) {      // four rows in flight per thread (padding rows read the shift: 0)
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = rb + (int64_t)u * nrl;
      v[u] = r < r1 ? *reinterpret_cast<const float4*>(x + r * C + cl * 4) : sh;
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
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
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
      float unbias = (float)n / fmaxf((float)n - 1.f, 1.f);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rmean[cl * 4 + j] = (1.f - momentum) * rmean[cl * 4 + j] + momentum * mu[j];
        rvar[cl * 4 + j] = (1.f - momentum) * rvar[cl * 4 + j] + momentum * va[j] * unbias;
      }
    }
  }
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t r1 = r0 + rpb;
  if (r1 > n) r1 = n;
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
      for (int j = 0; j < 4; ++j) {
        o[j] = bn_pre(v[u][j], mu[j], is[j], g[j], bt[j]);
        if (residual) o[j] += rs[u][j];
        o[j] = act_fwd(o[j], act);
      }
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
    if (rmean) {
      float unbias = (float)n / fmaxf((float)n - 1.f, 1.f);
      rmean[c] = (1.f - momentum) * rmean[c] + momentum * mu;
      rvar[c] = (1.f - momentum) * rvar[c] + momentum * va * unbias;
    }
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
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
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
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t r1 = r0 + rpb;
  if (r1 > n) r1 = n;
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
// columns g C + c).  They are combined in fp64 in a fixed order — mean = S1 / n, var = S2 / n - mean^2 — either in the prologue
// of the apply kernel (<= BN1_MAXB partial blocks: ONE launch per BatchNorm) or by k_bn2_finalize (two launches).  The
// read pass over x of k_bn1_partial is gone (r4: 46 launches, 0.32 ms alone / 0.56 ms beside the weight-gradient stream).
__device__ static inline void bn2_stats(double s1, double s2, int64_t n, float* mu, float* va) {
  const double m = s1 / (double)n;
  double v = s2 / (double)n - m * m;
  if (v < 0.0) v = 0.0;
  *mu = (float)m;
  *va = (float)v;
}

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
  const int c4n = CG / 4;
  const int cl = threadIdx.x % c4n, rl = threadIdx.x / c4n;
  const int nrl = blockDim.x / c4n;
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
      float unbias = (float)n / fmaxf((float)n - 1.f, 1.f);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rmean[cl * 4 + j] = (1.f - momentum) * rmean[cl * 4 + j] + momentum * mu[j];
        rvar[cl * 4 + j] = (1.f - momentum) * rvar[cl * 4 + j] + momentum * va[j] * unbias;
      }
    }
  }
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  int64_t r1 = r0 + rpb;
  if (r1 > n) r1 = n;
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
      for (int j = 0; j < 4; ++j) {
        o[j] = bn_pre(v[u][j], mu[j], is[j], g[j], bt[j]);
        if (residual) o[j] += rs[u][j];
        o[j] = act_fwd(o[j], act);
      }
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
    if (rmean) {
      float unbias = (float)n / fmaxf((float)n - 1.f, 1.f);
      rmean[c] = (1.f - momentum) * rmean[c] + momentum * mu;
      rvar[c] = (1.f - momentum) * rvar[c] + momentum * va * unbias;
    }
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
  rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean[c];
  rvar[c] = (1.f - momentum) * rvar[c] + momentum * var[c] * unbias;
}

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
// incoming gradient; table: gy's producer's [nb_part][2][C]; POOL: gy is the pooled gradient, read through parent / argrow; amax (nullable):
// max |gx| into the caller's (zeroed) word — late_hint: the word of fc_amax_out_hint, consumed once the checks have passed
template <bool POOL>
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
    k_norm_bwd_partial<POOL><<<FC_GRID(r.red, stream)>>>(x, y, gy, gy2, parent, argrow, seg, seg_stride, n, C, nseg, mean, var, eps, act, gamma, beta, r.red_rpb, (float*)ws);
    FC_CHECK_LAUNCH();
    table = (const float*)ws;
  }
  if (r.apply == FC_NBAPPLY_PROLOGUE) {
    k_bn1_bwd_apply<<<FC_GRID(r.ap, stream)>>>(x, y, gy, gy2, n, C, r.rpb, table, (int)r.np, mean, var, eps, gamma, beta, act, gx, gres, sums, r.cg, amax);
  } else {
    k_stats_final<<<FC_GRID(r.fin, stream)>>>(table, nullptr, r.np, nseg, 2 * C, 2, sums, nullptr);
    FC_CHECK_LAUNCH();
    k_norm_bwd_apply<POOL><<<FC_GRID(r.ap, stream)>>>(x, y, gy, gy2, parent, argrow, seg, seg_stride, n, C, mean, var, eps, gamma, beta, sums, cnt, act, gx, gres, amax);
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}

static int route_out(const NormRoute& r, int* out) {
  const int f[16] = {r.sums, r.apply, r.amax, (int)r.np, (int)r.nb, (int)r.rpb, r.cg, r.ap.threads, (int)r.ap.lds, (int)r.ap.grid_x, (int)r.ap.grid_y,
                     (int)r.ws_bytes, (r.red.threads != 0) + (r.fin.threads != 0) + (r.ap.threads != 0)};
  for (int i = 0; i < 16; ++i) out[i] = f[i];
  return r.sums ? FC_OK : FC_EINVAL;
}

extern "C" {

int64_t fc_col_stats_ws_bytes(int64_t n, int C, int nseg) {
  return row_blocks(n, MAXBLOCKS).nb * nseg * (2 * (int64_t)C + 1) * (int64_t)sizeof(float);
}

// mean (nseg,C), var (nseg,C) biased, cnt (nseg) ; seg = per-row segment id pointer (NULL -> one segment)
int fc_col_stats(const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* mean, float* var,
                 float* cnt, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (n < 0 || nseg < 1 || nseg > MAXSEG) return FC_EINVAL;
  StatsGeometry g;
  if (!stats_geometry(C, &g)) return FC_EINVAL;
  if (ws_bytes < fc_col_stats_ws_bytes(n, C, nseg)) return FC_EWS;
  const RowBlocks b = row_blocks(n, MAXBLOCKS);
  float* part = (float*)ws;
  float* part_cnt = part + b.nb * nseg * 2 * C;
  if (n == 0) {
    FC_HIP(hipMemsetAsync(mean, 0, sizeof(float) * nseg * C, stream));
    FC_HIP(hipMemsetAsync(var, 0, sizeof(float) * nseg * C, stream));
    FC_HIP(hipMemsetAsync(cnt, 0, sizeof(float) * nseg, stream));
    return FC_OK;
  }
  // r5: ONE pass over x (sums of x and of x^2 per block and segment), combined in fp64 — r1-r4 read x twice (mean, then the
  // centred squares), four launches
  k_stats_partial<<<(unsigned)b.nb, g.threads, g.lds_fwd, stream>>>(x, seg, seg_stride, n, C, nseg, nullptr, 2, b.rpb, part, part_cnt);
  FC_CHECK_LAUNCH();
  k_seg_meanvar_final<<<(unsigned)(nseg * ((C + 3) / 4)), 256, 0, stream>>>(part, part_cnt, b.nb, nseg, C, mean, var, cnt);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// out (nseg,C) = per-segment column sums of x (N,C) — deterministic two-level reduction
int fc_seg_col_sums(const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* out, void* ws,
                    int64_t ws_bytes, hipStream_t stream) {
  if (n < 0 || nseg < 1 || nseg > MAXSEG) return FC_EINVAL;
  StatsGeometry g;
  if (!stats_geometry(C, &g)) return FC_EINVAL;
  if (ws_bytes < fc_col_stats_ws_bytes(n, C, nseg)) return FC_EWS;
  if (n == 0) {
    FC_HIP(hipMemsetAsync(out, 0, sizeof(float) * nseg * C, stream));
    return FC_OK;
  }
  const RowBlocks b = row_blocks(n, MAXBLOCKS);
  float* part = (float*)ws;
  k_stats_partial<<<(unsigned)b.nb, g.threads, g.lds_fwd, stream>>>(x, seg, seg_stride, n, C, nseg, nullptr, 0, b.rpb, part, nullptr);
  FC_CHECK_LAUNCH();
  k_stats_final<<<(unsigned)(nseg * ((C + FIN_CB - 1) / FIN_CB)), FIN_CB * FIN_SL, 0, stream>>>(part, nullptr, b.nb, nseg, C, 2, out, nullptr);
  FC_CHECK_LAUNCH();
  return FC_OK;
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
  return norm_bwd<false>(FC_NFORM_SMALL, x, y, gy, nullptr, nullptr, nullptr, nullptr, 0, n, C, 1, mean, var, nullptr, eps, gamma, beta, act, gx, gres, sums,
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
  unsigned* ao = take_amax_out();                // fc_amax_out_hint: max |y| into the caller's (zeroed) word
  if (n < 0 || C < 4 || C % 4 || act < 0 || act > 2) return FC_EINVAL;
  if (n == 0) return FC_OK;
  k_norm_act_fwd<<<FC_GRID(rows_launch(n, C), stream)>>>(x, seg, seg_stride, n, C, mean, var, eps, gamma, beta, residual, act, nullptr, nullptr, y, ao);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// sums (nseg,2,C): [.,0,.] = sum g' (= d beta per segment), [.,1,.] = sum g'*xhat (= d gamma per segment); max |gx| into the hint's word
int fc_norm_act_bwd(const float* x, const float* y, const float* gy, const int* seg, int seg_stride, int64_t n, int C,
                    int nseg, const float* mean, const float* var, const float* cnt, float eps, const float* gamma,
                    const float* beta, int act, float* gx, float* gres, float* sums, void* ws, int64_t ws_bytes,
                    hipStream_t stream) {
  unsigned* ao = take_amax_out();
  return norm_bwd<false>(FC_NFORM_SEG, x, y, gy, nullptr, nullptr, nullptr, seg, seg_stride, n, C, nseg, mean, var, cnt, eps, gamma, beta, act, gx, gres, sums,
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
  unsigned* ao = take_amax_out();
  return bn_fwd(x, n, C, eps, gamma, beta, residual, act, momentum, y, mean, var, cnt, running_mean, running_var, num_batches_tracked, part, nb_part, groups,
                small_elems, nullptr, nullptr, ws, ws_bytes, stream, ao);
}

// Backward.  gy2 (nullable): a second contribution to the incoming gradient, added on the fly.  part == NULL: the sums of g' and
// g' xhat are reduced here (two or three launches by size); part != NULL: nb_part blocks [nb_part][2][C] written by the producer of gy.
int fc_bn_train_bwd(const float* x, const float* y, const float* gy, const float* gy2, int64_t n, int C, const float* mean,
                    const float* var, const float* cnt, float eps, const float* gamma, const float* beta, int act, float* gx,
                    float* gres, float* sums, const float* part, int64_t nb_part, int64_t small_elems, void* ws, int64_t ws_bytes,
                    hipStream_t stream) {
  unsigned* ao = take_amax_out();
  return norm_bwd<false>(FC_NFORM_TRAIN, x, y, gy, gy2, nullptr, nullptr, nullptr, 0, n, C, 1, mean, var, cnt, eps, gamma, beta, act, gx, gres, sums, part, nb_part,
                         small_elems, ws, ws_bytes, stream, ao);
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
  if (K == 8 && C % 4 == 0) k_maxpool8_fwd<<<(unsigned)fc_cdiv(n_out * (C / 4), 256), 256, 0, stream>>>(in, nbr, n_out, C, out, argrow, ao);
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

// ---- r7: the stem's tail fused (kernels above) ------------------------------------------------------------------------------------
int fc_norm_act_maxpool8_fwd(const float* x, const int* seg, int seg_stride, int C, const float* mean, const float* var, float eps,
                             const float* gamma, const float* beta, int act, const int* nbr, int64_t n_out, float* out,
                             int* argrow, float* y, int* parent, hipStream_t stream) {
  unsigned* ao = take_amax_out();                // fc_amax_out_hint: max |out| into the caller's (zeroed) word
  if (n_out < 0 || C < 4 || C % 4 || act < 0 || act > 2) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  k_norm_act_maxpool8_fwd<<<(unsigned)fc_cdiv(n_out * (C / 4), 256), 256, 0, stream>>>(x, seg, seg_stride, C, mean, var, eps, gamma, beta,
                                                                                      act, nbr, n_out, out, argrow, y, parent, ao);
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
  return norm_bwd<true>(FC_NFORM_SEG, x, nullptr, gout, nullptr, parent, argrow, seg, seg_stride, n_in, C, nseg, mean, var, cnt, eps, gamma, beta, act, gx, nullptr,
                        sums, nullptr, 0, 0, ws, ws_bytes, stream, nullptr);      // (the hint is not consumed)
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
