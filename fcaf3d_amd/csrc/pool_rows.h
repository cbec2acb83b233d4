// Max pooling over a neighbour table, the stem's fused normalise + activation + pool, row gather / scatter (included by norm.hip).
#pragma once

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
// MASK (C == 64: the 16 threads of a pooled row are adjacent lanes): mask[child row] = one 64-bit word, bit c set exactly where
// argrow[pooled row][c] == child row, for the backward pass (norm_rows.h POOL_MASK), which then reads 8 linear bytes per input row instead
// of gathering the arg-max rows; argrow may then be NULL and is not stored.  out, parent and the amax word are those of <false>.
template <bool MASK>
__global__ void k_norm_act_maxpool8_fwd(const float* __restrict__ x, const int* __restrict__ seg, int seg_stride, int C,
                                        const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                        const float* __restrict__ gamma, const float* __restrict__ beta, int act,
                                        const int* __restrict__ nbr, int64_t n_out, float* __restrict__ out, int* __restrict__ argrow,
                                        float* __restrict__ y, int* __restrict__ parent, unsigned long long* __restrict__ mask,
                                        unsigned* __restrict__ amax_out) {
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
  if (!MASK || argrow) *reinterpret_cast<int4*>(argrow + o * C + c) = make_int4(arg[0], arg[1], arg[2], arg[3]);
  if (MASK) {
    // this lane's four channels: which child won each, a nibble per child slot k at bits 4k .. 4k + 3 (absent children and rows without
    // children: 0)
    unsigned won = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned nib = (unsigned)(arg[0] == idx[k]) | (unsigned)(arg[1] == idx[k]) << 1 | (unsigned)(arg[2] == idx[k]) << 2 |
                           (unsigned)(arg[3] == idx[k]) << 3;
      won |= (idx[k] < 0 ? 0u : nib) << (4 * k);
    }
    // lane k of the row's 16 stores child k's word, as the parent store above: bits 4L .. 4L + 3 are lane L's nibble of slot k.  (The 16
    // lanes of a pooled row are all inside `t < n_out * c4n` or all outside, so every lane read is active.)
    const int k = (c >> 2) & 7;
    unsigned long long word = 0ull;
#pragma unroll
    for (int L = 0; L < 16; ++L) word |= (unsigned long long)((__shfl(won, L, 16) >> (4 * k)) & 15u) << (4 * L);
    int mine = -1;
#pragma unroll
    for (int q = 0; q < 8; ++q) mine = (c == 4 * q) ? idx[q] : mine;
    if (mine >= 0) mask[mine] = word;
  }
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
