// The normalisation kernels for any size and any number of segments (included by norm.hip): the forward, the backward's partial sums and apply.
#pragma once

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
  float4 o;                                      // (norm_act_elem written out per float4: the helper changes this kernel's code)
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
// POOL_MASK (r7, C == 64): pool_arg points at the per-child mask the forward kernel wrote instead (k_norm_act_maxpool8_fwd<true>), one 64-bit word
// per INPUT row, bit c set exactly where pool_arg[pool_parent[r]][c] == r.  The select takes the same values, so the sums keep their bits; the
// 16 gathered bytes of arg-max rows per float4 group become 4 linear ones (a lane reads the 32-bit half that holds its nibble).
enum { POOL_NONE, POOL_ARG, POOL_MASK };
__device__ __forceinline__ unsigned pool_mask_nibble(const int* __restrict__ pool_mask, int64_t r, int cl) {
  return (reinterpret_cast<const unsigned*>(pool_mask)[2 * r + (cl >> 3)] >> ((cl & 7) * 4)) & 15u;
}
// v where keep, else +0.f — the value of `keep ? v : 0.f` as an AND on the bits: written as a select, the compiler turns the 16-byte row load behind it
// into 12 bytes + a 4-byte load under the predicate, which waits for the predicate's own load before it is even issued
__device__ __forceinline__ float keep_if(float v, bool keep) { return __uint_as_float(__float_as_uint(v) & (keep ? 0xffffffffu : 0u)); }
// FROM_Y (act && y) / GY2 (gy2 != NULL), r7: whether the y and gy2 rows are read at all is compile-time too.  Four rows of every operand are in flight
// per thread beside eight float4 accumulators; as run-time tests the kernel was allocated for the case that reads all four operands and spilled
// in every case (168 / 220 bytes of scratch per lane under the 128-register cap of a kernel without a launch bound).  An instantiation now
// holds the row registers it loads and no others; the bound tells the compiler the 256 threads it is launched with, and four waves per SIMD are
// asked for because the grid (at most 1 024 blocks of 4 waves) is exactly one resident round at four and two rounds at fewer.  The forms that read
// three row operands (gy2, or the pooled gather) keep a few spilled values in the segment loop and none in the row loop; the one that reads all four
// (y and gy2, which the training step does not launch) has three spill instructions in the row loop as well (profiles/r7_notes.md section 12).
template <int POOL, bool FROM_Y, bool GY2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_norm_bwd_partial(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                   const float* __restrict__ gy2, const int* __restrict__ pool_parent,
                                   const int* __restrict__ pool_arg, const int* __restrict__ seg, int seg_stride, int64_t n, int C_rt, int nseg,
                                   const float* __restrict__ mean, const float* __restrict__ var, float eps, int act,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   int64_t rpb, float* __restrict__ part) {
  const int C = POOL == POOL_MASK ? 64 : C_rt;      // (the mask form exists for 64 channels only: its row geometry folds into constants)
  extern __shared__ float sm[];               // [rl][2][C]
  __shared__ int srange[2];
  const auto [cl, rl, nrl] = lane_coord(C / 4);
  const auto [r0, r1] = row_span(rpb, n);
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
      for (int64_t rb = r0 + rl; rb < r1; rb += 4 * nrl) {
        // branch-free batch: the 4 x (x, gy, y) rows are requested together (rows past the range re-read row r0 and are
        // dropped by `ok`), r3 — a `continue` in front of each load serialised them
        float4 xv[4], gv[4], yv[4], g2[4];
        bool ok[4];
        int po[4];
        if (POOL) {                              // the four parent rows first: the gathers wait for them, and one wait serves all four
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int64_t r = rb + (int64_t)u * nrl;
            po[u] = pool_parent[r < r1 ? r : r0];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t r = rb + (int64_t)u * nrl;
          ok[u] = r < r1;
          const int64_t rc = ok[u] ? r : r0;
          if (chk) ok[u] = ok[u] && seg[rc * seg_stride] == s;
          xv[u] = *reinterpret_cast<const float4*>(x + rc * C + cl * 4);
          if (POOL == POOL_MASK) {
            const int64_t o = po[u];
            const unsigned m = pool_mask_nibble(pool_arg, rc, cl);
            gv[u] = *reinterpret_cast<const float4*>(gy + o * C + cl * 4);
            gv[u].x = keep_if(gv[u].x, m & 1u); gv[u].y = keep_if(gv[u].y, m & 2u);
            gv[u].z = keep_if(gv[u].z, m & 4u); gv[u].w = keep_if(gv[u].w, m & 8u);
          } else if (POOL == POOL_ARG) {
            const int64_t o = po[u];
            const int4 a = *reinterpret_cast<const int4*>(pool_arg + o * C + cl * 4);
            gv[u] = *reinterpret_cast<const float4*>(gy + o * C + cl * 4);
            const int ri = (int)rc;            // (pool_arg names rows in 32 bits, so a pooled matrix has fewer than 2^31 of them)
            gv[u].x = keep_if(gv[u].x, a.x == ri); gv[u].y = keep_if(gv[u].y, a.y == ri);
            gv[u].z = keep_if(gv[u].z, a.z == ri); gv[u].w = keep_if(gv[u].w, a.w == ri);
          } else {
            gv[u] = *reinterpret_cast<const float4*>(gy + rc * C + cl * 4);
          }
          if (GY2) g2[u] = *reinterpret_cast<const float4*>(gy2 + rc * C + cl * 4);
          if (FROM_Y) yv[u] = *reinterpret_cast<const float4*>(y + rc * C + cl * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!ok[u]) continue;
          float4 g = gv[u];
          if (GY2) { g.x += g2[u].x; g.y += g2[u].y; g.z += g2[u].z; g.w += g2[u].w; }
          if (FROM_Y) {
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
// pool_parent / pool_arg, POOL_MASK: see k_norm_bwd_partial
template <int POOL>
__global__ void k_norm_bwd_apply(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gy,
                                 const float* __restrict__ gy2, const int* __restrict__ pool_parent,
                                 const int* __restrict__ pool_arg, const int* __restrict__ seg, int seg_stride, int64_t n, int C_rt,
                                 const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                 const float* __restrict__ sums /*[seg][2][C]*/,
                                 const float* __restrict__ cnt, int act, float* __restrict__ gx, float* __restrict__ gres,
                                 unsigned* __restrict__ amax_out) {
  const int C = POOL == POOL_MASK ? 64 : C_rt;      // (see k_norm_bwd_partial)
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
  if (POOL == POOL_MASK) {
    const int64_t o = pool_parent[r];
    const unsigned m = pool_mask_nibble(pool_arg, r, c >> 2);
    *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(gy + o * C + c);
    gv[0] = (m & 1u) ? gv[0] : 0.f; gv[1] = (m & 2u) ? gv[1] : 0.f; gv[2] = (m & 4u) ? gv[2] : 0.f; gv[3] = (m & 8u) ? gv[3] : 0.f;
  } else if (POOL == POOL_ARG) {
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
