// The input side of a training step for a whole batch in ONE launch: B scenes that live in a resident arena of raw points are
// sampled, aligned, flipped, rotated, scaled, translated and voxelised into the collated coords / feats of the batch, driven by a
// descriptor table on the device.  What the reference does per scene on DataLoader workers —
//   IndoorPointSample (mmdet3d/datasets/pipelines/transforms_3d.py:821-895), GlobalAlignment (:409-490), RandomFlip3D (:59-170),
//   GlobalRotScaleTrans (:493-645), then the collate of extract_feat (mmdet3d/models/detectors/single_stage_sparse.py:34-36)
// — and what fc_augment_voxelize (csrc/coords.hip) does with one launch per scene from an index buffer somebody else drew.
//
// Kept apart from csrc/ as eval.hip and merge.hip are: the kernel is not part of the profiled step, so source_hash() does not cover
// it.  The transform behind the row gather is k_augment_voxelize's own (csrc/aug_point.h, shared with csrc/coords.hip), followed by
// the same collate: true fp32 divisions, no FMA contraction.  coords / feats are bit-equal to B calls of fc_augment_voxelize with
// the same row indices (tests/test_gpu_batch.py).
//
// The sampler (BATCH_* below; tests/test_batch_cpu.py restates it in numpy from this text) — all arithmetic on 32-bit unsigned
// words, wrapping:
//   mix(x):  x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16        (murmur3's finaliser)
//   key[i] = mix(lo ^ mix(hi + (i + 1) * 0x9E3779B9)),  lo / hi the halves of the scene's 64-bit seed, i = 0 .. 3
//   n_src >= n_out (IndoorPointSample, replace=False): output row j reads source row perm(j).  perm is a keyed bijection of
//     [0, n_src): with m = the number of bits of n_src - 1 (at least 1) and h = (m + 1) / 2, a balanced Feistel network on 2 h bits,
//         (L, R) = (x >> h, x & (2^h - 1));  four rounds  (L, R) <- (R, L ^ (mix(R * 0x9E3779B1 + key[i]) & (2^h - 1)));  x' = L << h | R
//     is a bijection F of [0, 2^(2h)), and perm(j) = the first of F(j), F(F(j)), ... that lies below n_src (cycle walking).
//     Termination: F is a bijection of a finite set, so j lies on a cycle of F; the walk follows that cycle and the cycle returns to
//     j itself, which is below n_src — so an element below n_src is met after at most the cycle's length.  Restricted to
//     [0, n_src) the map "next element of my cycle below n_src" is again a bijection: n_out distinct j give n_out DISTINCT rows, as
//     np.random.choice(replace=False) does.  Expected length: 2^(2h) <= 2^(m+1) < 4 n_src, so a step lands below n_src with
//     probability > 1/4 and the expected number of iterations is under 4 (under 2 when m is even).
//   n_src < n_out (replace=True): row = (mix(mix(j ^ key[0]) + key[1]) * n_src) >> 32 (the high word of the 64-bit product):
//     independent draws with replacement, as the reference's.
//   sample_idx != NULL: the rows are read from it instead (scene s: sample_idx[idx_off + j]), nothing is drawn.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "../csrc/aug_point.h"
// exact products and sums, as csrc/coords.hip k_augment_voxelize and torch's elementwise kernels compute them: no FMA contraction
#pragma clang fp contract(off)

#define BATCH_THREADS 256
#define BATCH_MAX_SCENES 256        // one descriptor per thread of the workgroup: the prefix of the output counts is one block scan
#define BATCH_DESC_WORDS 18         // int64 words per scene (include/fcaf3d_hip.h FC_BATCH_DESC_WORDS)

namespace {

// a thread per output row of the batch, rows of all scenes back to back (a workgroup may straddle scenes)
inline unsigned batch_blocks(int64_t total_out) { return (unsigned)((total_out + BATCH_THREADS - 1) / BATCH_THREADS); }

__device__ inline unsigned batch_mix(unsigned x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

struct BatchKeys { unsigned k[4]; };

__device__ inline BatchKeys batch_keys(unsigned long long seed) {
  const unsigned lo = (unsigned)seed, hi = (unsigned)(seed >> 32);
  BatchKeys r;
#pragma unroll
  for (unsigned i = 0; i < 4; ++i) r.k[i] = batch_mix(lo ^ batch_mix(hi + (i + 1u) * 0x9E3779B9u));
  return r;
}

// half width h of the Feistel network for [0, n): m = bits of n - 1 (at least 1), h = (m + 1) / 2  (1 <= h <= 16 for n <= 2^31)
__device__ inline int batch_half_bits(unsigned n) {
  int m = 1;
  while (m < 32 && ((n - 1u) >> m) != 0u) ++m;
  return (m + 1) / 2;
}

__device__ inline unsigned batch_perm(unsigned j, unsigned n, int h, const BatchKeys& key) {
  const unsigned mask = (1u << h) - 1u;
  unsigned x = j;
  do {                                                     // cycle walking: ends, see the head of the file
    unsigned l = x >> h, r = x & mask;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned t = l ^ (batch_mix(r * 0x9E3779B1u + key.k[i]) & mask);
      l = r; r = t;
    }
    x = (l << h) | r;
  } while (x >= n);
  return x;
}

__device__ inline unsigned batch_draw(unsigned j, unsigned n, const BatchKeys& key) {
  const unsigned hsh = batch_mix(batch_mix(j ^ key.k[0]) + key.k[1]);
  return (unsigned)(((unsigned long long)hsh * (unsigned long long)n) >> 32);
}

// A scene's output count as the kernel will honour it: 0 unless every range of the descriptor lies inside its array (the caller
// checks them; a bad descriptor must still not reach outside).
__device__ inline int64_t batch_live_rows(const int64_t* __restrict__ d, int64_t arena_rows, int64_t out_rows, bool has_idx,
                                          int64_t n_idx) {
  const int64_t src_off = d[0], n_src = d[1], n_out = d[2], out_off = d[3], idx_off = d[5];
  bool ok = n_out > 0 && n_out <= 0x7fffffff && n_src >= 1 && n_src <= 0x7fffffff;
  ok = ok && src_off >= 0 && src_off <= arena_rows - n_src;
  ok = ok && out_off >= 0 && out_off <= out_rows - n_out;
  if (has_idx) ok = ok && idx_off >= 0 && idx_off <= n_idx - n_out;
  return ok ? n_out : 0;
}

__global__ __launch_bounds__(BATCH_THREADS) void k_batch_augment_voxelize(
    const float* __restrict__ arena, int64_t arena_rows, int pt_stride, const int64_t* __restrict__ desc, int B,
    const int* __restrict__ sample_idx, int64_t n_idx, int64_t out_rows, float vs, float feat_div, int nfeat,
    int* __restrict__ coords, float* __restrict__ feats, int* __restrict__ sample_out, float* __restrict__ points_out) {
  // inclusive prefix of the scenes' output counts (Hillis-Steele over one descriptor per thread, two buffers)
  __shared__ int64_t s_pre[2][BATCH_MAX_SCENES];
  const int t = (int)threadIdx.x;
  s_pre[0][t] = t < B ? batch_live_rows(desc + (int64_t)t * BATCH_DESC_WORDS, arena_rows, out_rows, sample_idx != nullptr, n_idx) : 0;
  __syncthreads();
  int cur = 0;
  for (int step = 1; step < BATCH_MAX_SCENES; step <<= 1) {
    s_pre[cur ^ 1][t] = s_pre[cur][t] + (t >= step ? s_pre[cur][t - step] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int64_t* pre = s_pre[cur];
  const int64_t v = (int64_t)blockIdx.x * BATCH_THREADS + t;           // row of the virtual concatenation
  if (v >= pre[BATCH_MAX_SCENES - 1]) return;
  // the scene of row v: the first s with v < pre[s]
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v < pre[mid]) hi = mid; else lo = mid + 1;
  }
  const int s = lo;
  const int64_t j = v - (s ? pre[s - 1] : 0);
  const int64_t* d = desc + (int64_t)s * BATCH_DESC_WORDS;
  const int64_t src_off = d[0], n_src = d[1], n_out = d[2], out_off = d[3];
  int64_t src;
  if (sample_idx) {
    src = sample_idx[d[5] + j];
    if (src < 0 || src >= n_src) return;                               // not a row of the scene: the output row keeps what it held
  } else {
    const BatchKeys key = batch_keys((unsigned long long)d[4]);
    src = n_src >= n_out ? (int64_t)batch_perm((unsigned)j, (unsigned)n_src, batch_half_bits((unsigned)n_src), key)
                         : (int64_t)batch_draw((unsigned)j, (unsigned)n_src, key);
  }
  const int64_t i = out_off + j;
  if (sample_out) sample_out[i] = (int)src;
  // from here on as k_augment_voxelize (csrc/coords.hip): the shared transform, then the collate
  const float* p = arena + (src_off + src) * pt_stride;
  const AugP q = aug_point(p[0], p[1], p[2], reinterpret_cast<const float*>(d + 6));
  const float x = q.x, y = q.y, z = q.z;
  int4 cd;
  cd.x = s;
  cd.y = (int)floorf(x / vs);
  cd.z = (int)floorf(y / vs);
  cd.w = (int)floorf(z / vs);
  reinterpret_cast<int4*>(coords)[i] = cd;
  for (int f = 0; f < nfeat; ++f) feats[i * nfeat + f] = p[3 + f] / feat_div;
  if (points_out) {
    float* o = points_out + i * (3 + nfeat);
    o[0] = x; o[1] = y; o[2] = z;
    for (int f = 0; f < nfeat; ++f) o[3 + f] = p[3 + f];
  }
}

}  // namespace

extern "C" {

int fc_batch_augment_voxelize(const float* arena, int64_t arena_rows, int pt_stride, const int64_t* desc, int B, int64_t total_out,
                              int64_t out_rows, const int* sample_idx, int64_t n_idx, float voxel_size, float feat_div, int nfeat,
                              int* coords, float* feats, int* sample_out, float* points_out, hipStream_t stream) {
  if (B < 0 || B > BATCH_MAX_SCENES || total_out < 0 || out_rows < 0 || arena_rows < 0 || n_idx < 0) return FC_EINVAL;
  if (nfeat < 0 || pt_stride < 3 + nfeat || !(voxel_size > 0.f)) return FC_EINVAL;
  if (total_out > out_rows) return FC_EINVAL;
  if (B == 0 || total_out == 0) return FC_OK;
  if (!arena || !desc || !coords || (nfeat > 0 && !feats)) return FC_EINVAL;
  if (sample_idx && n_idx < total_out) return FC_EINVAL;
  if (total_out > (int64_t)0x7fffffff * BATCH_THREADS) return FC_EINVAL;
  k_batch_augment_voxelize<<<batch_blocks(total_out), BATCH_THREADS, 0, stream>>>(
      arena, arena_rows, pt_stride, desc, B, sample_idx, n_idx, out_rows, voxel_size, feat_div, nfeat, coords, feats, sample_out,
      points_out);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
