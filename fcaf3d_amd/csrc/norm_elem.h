// What the normalisation kernels share (included by norm.hip in front of them): the segment of a row, the activations and their derivatives, the
// pre-activation, the fp64 statistics, and the blocks that leave every kernel using them with the device code it had with the block written out
// (tools/device_asm_diff.py, profiles/r7_notes.md section 11).  A kernel whose code a helper changes keeps its text, with a comment naming the helper.
#pragma once

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

// rows [r0, r1) of block blockIdx.x at rpb rows per block (row_blocks, norm_route.h)
struct RowSpan { int64_t r0, r1; };
__device__ __forceinline__ RowSpan row_span(int64_t rpb, int64_t n) {
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb;
  return {r0, r1 > n ? n : r1};
}

// a thread of the row-blocked kernels (stats_geometry, norm_route.h): channel lane cl of c4n float4 lanes, row lane rl of nrl
struct LaneCoord { int cl, rl, nrl; };
__device__ __forceinline__ LaneCoord lane_coord(int c4n) {
  return {(int)(threadIdx.x % c4n), (int)(threadIdx.x / c4n), (int)(blockDim.x / c4n)};
}

// nn.BatchNorm1d running buffers of channel c after a batch of n rows: momentum update with the unbiased variance
__device__ __forceinline__ void bn_running_update(float* __restrict__ rmean, float* __restrict__ rvar, int c, float mu, float va, float n, float momentum) {
  const float unbias = n / fmaxf(n - 1.f, 1.f);
  rmean[c] = (1.f - momentum) * rmean[c] + momentum * mu;
  rvar[c] = (1.f - momentum) * rvar[c] + momentum * va * unbias;
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

// one element of the row-blocked forward apply kernels: pre-activation, + *res (nullptr: no residual; the kernels' residual registers are
// unset then, hence a pointer and no value), activation
__device__ __forceinline__ float norm_act_elem(float v, float mu, float is, float g, float b, const float* res, int act) {
  float o = bn_pre(v, mu, is, g, b);
  if (res) o += *res;
  return act_fwd(o, act);
}

__device__ static inline void bn2_stats(double s1, double s2, int64_t n, float* mu, float* va) {
  const double m = s1 / (double)n;
  double v = s2 / (double)n - m * m;
  if (v < 0.0) v = 0.0;
  *mu = (float)m;
  *va = (float)v;
}
