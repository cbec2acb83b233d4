// Test-time augmentation merge (mmdet3d/core/post_processing/merge_augs.py:7-91): a stable k-way merge of descending-sorted
// segments, with the box mapping-back of core/bbox/transforms.py:4-23 fused into the copy.
//
// Kept apart from csrc/ on purpose: these kernels never run in the training step whose profiles csrc/ is pinned to
// (build.source_hash()).  Used twice per TTA batch by Fcaf3DNeckWithHead.get_bboxes_aug:
//   (scene, class): K = A first-stage survivor lists of the scene's augmented copies, mapped back   (merge_augs.py:36-47)
//   scene:          K = C merge-NMS survivor lists, identity transform, cap = max_num               (merge_augs.py:65-89)
//
// Output segment o merges input segments g = o*K + k, k = 0..K-1.  The rank of element p of input segment k is
//     p + sum_{k' < k} #{x in k' : x >= s} + sum_{k' > k} #{x in k' : x > s}
// (binary searches in descending lists), which is exactly `cat` in input-segment order followed by a STABLE descending sort:
// no atomics, deterministic.  Two launches: (1) every input score is gathered once into a contiguous per-output-segment row of
// the workspace (the searches then read plain arrays instead of chasing keep -> ord -> score indices), (2) rank + scatter.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"

#define MERGE_THREADS 256
#define MERGE_MAX_K 4096
#define MERGE_MAX_GX 1024

namespace {

constexpr float kPi = 3.14159265358979323846f;        // fp32(np.pi): what `-yaw + np.pi` adds to an fp32 tensor

// pre[k] = first concatenated position of input segment k of output segment o, pre[K] = total (LDS, K + 1 ints); tile: 256 ints
__device__ void seg_prefix(const int64_t* __restrict__ desc, const int* __restrict__ counts, int cap_in, int o, int K,
                           int* pre, int* tile) {
  int carry = 0;
  for (int base = 0; base < K; base += MERGE_THREADS) {
    const int k = base + (int)threadIdx.x;
    int c = 0;
    if (k < K) c = min(max(counts[desc[((int64_t)o * K + k) * 4]], 0), cap_in);
    tile[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < MERGE_THREADS; off <<= 1) {     // Hillis-Steele inclusive scan
      const int v = (int)threadIdx.x >= off ? tile[threadIdx.x - off] : 0;
      __syncthreads();
      tile[threadIdx.x] += v;
      __syncthreads();
    }
    if (k < K) pre[k + 1] = carry + tile[threadIdx.x];
    carry += tile[MERGE_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) pre[0] = 0;
  __syncthreads();
}

// input segment of concatenated position e: the last k with pre[k] <= e (pre[K] > e)
__device__ inline int seg_of(const int* pre, int K, int e) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// table row of element p of an input segment whose descriptor row is `row`: keep -> ord -> row (each level optional)
__device__ inline int64_t src_row(int64_t row, const int* __restrict__ keep, int keep_stride, const int64_t* __restrict__ ord,
                                  int ord_stride, int p) {
  const int64_t j = keep ? (int64_t)keep[row * keep_stride + p] : (int64_t)p;
  return ord ? ord[row * ord_stride + j] : j;
}

__global__ __launch_bounds__(MERGE_THREADS) void k_merge_gather(
    const int64_t* __restrict__ desc, int K, const int* __restrict__ counts, int cap_in, const int* __restrict__ keep,
    int keep_stride, const int64_t* __restrict__ ord, int ord_stride, const float* __restrict__ scores, int score_stride,
    int max_total, float* __restrict__ ws) {
  extern __shared__ int smem[];
  int* tile = smem;
  int* pre = smem + MERGE_THREADS;
  const int o = blockIdx.y;
  seg_prefix(desc, counts, cap_in, o, K, pre, tile);
  const int total = min(pre[K], max_total);
  float* wo = ws + (int64_t)o * max_total;
  for (int e = blockIdx.x * MERGE_THREADS + threadIdx.x; e < total; e += gridDim.x * MERGE_THREADS) {
    const int k = seg_of(pre, K, e);
    const int64_t* d = desc + ((int64_t)o * K + k) * 4;
    const int64_t r = src_row(d[0], keep, keep_stride, ord, ord_stride, e - pre[k]);
    wo[e] = scores[d[2] + r * score_stride];
  }
}

__global__ __launch_bounds__(MERGE_THREADS) void k_merge_scatter(
    const int64_t* __restrict__ desc, int K, const int* __restrict__ counts, int cap_in, const int* __restrict__ keep,
    int keep_stride, const int64_t* __restrict__ ord, int ord_stride, const float* __restrict__ boxes, int flags,
    int max_total, int limit, const float* __restrict__ ws, float* __restrict__ out_boxes, float* __restrict__ out_scores,
    int* __restrict__ out_src, int* __restrict__ out_count, int stride_out) {
  extern __shared__ int smem[];
  int* tile = smem;
  int* pre = smem + MERGE_THREADS;
  const int o = blockIdx.y;
  seg_prefix(desc, counts, cap_in, o, K, pre, tile);
  const int total = min(pre[K], max_total);
  if (blockIdx.x == 0 && threadIdx.x == 0) out_count[o] = min(total, limit);
  const float* wo = ws + (int64_t)o * max_total;
  for (int e = blockIdx.x * MERGE_THREADS + threadIdx.x; e < total; e += gridDim.x * MERGE_THREADS) {
    const int k = seg_of(pre, K, e);
    const int p = e - pre[k];
    const float s = wo[e];
    int rank = p;
    for (int kk = 0; kk < K; ++kk) {
      const int a = pre[kk], n = min(pre[kk + 1], total) - a;
      if (kk == k || n <= 0) continue;
      const float* lst = wo + a;
      int lo = 0, hi = n;
      if (kk < k) {                                   // earlier segments win ties: count x >= s
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (lst[mid] >= s) lo = mid + 1; else hi = mid; }
      } else {                                        // later segments lose ties: count x > s
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (lst[mid] > s) lo = mid + 1; else hi = mid; }
      }
      rank += lo;
    }
    if (rank >= limit) continue;
    const int64_t* d = desc + ((int64_t)o * K + k) * 4;
    const int64_t r = src_row(d[0], keep, keep_stride, ord, ord_stride, p);
    const float* src = boxes + (d[1] + r) * 7;
    float b[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) b[i] = src[i];
    // bbox3d_mapping_back on the bottom-centre tensor: DepthInstance3DBoxes(origin=(.5,.5,.5)) first (base_box3d.py:62-66:
    // z += h * (0 - 0.5), exact in fp32), then flip('horizontal'), flip('vertical') (depth_box3d.py:189-197), scale(1 / s)
    // (base_box3d.py:215-222: tensor[:, :6] *= fp32(1 / s))
    const uint64_t xf = (uint64_t)d[3];
    if (flags & FC_MERGE_TO_BOTTOM) b[2] = b[2] + b[5] * -0.5f;
    if (xf & FC_MERGE_XF_FLIP_H) {
      b[0] = -b[0];
      if (flags & FC_MERGE_WITH_YAW) b[6] = -b[6] + kPi;
    }
    if (xf & FC_MERGE_XF_FLIP_V) {
      b[1] = -b[1];
      if (flags & FC_MERGE_WITH_YAW) b[6] = -b[6];
    }
    const float f = __uint_as_float((unsigned)(xf & 0xffffffffull));
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = b[i] * f;
    const int64_t q = (int64_t)o * stride_out + rank;
#pragma unroll
    for (int i = 0; i < 7; ++i) out_boxes[q * 7 + i] = b[i];
    out_scores[q] = s;
    if (out_src) {
      out_src[q * 2] = k;
      out_src[q * 2 + 1] = p;
    }
  }
}

}  // namespace

extern "C" {

int64_t fc_merge_sorted_segments_ws_bytes(int nseg_out, int max_total) {
  if (nseg_out < 0 || max_total < 0) return 0;
  return fc_align((int64_t)nseg_out * max_total * (int64_t)sizeof(float), 256);
}

int fc_merge_sorted_segments(const int64_t* desc, int nseg_out, int K, const int* counts_dev, const int* keep, int keep_stride,
                             const int64_t* ord, int ord_stride, const float* scores, int score_stride, const float* boxes,
                             int flags, int max_total, int cap, float* out_boxes, float* out_scores, int* out_src,
                             int* out_count, int stride_out, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (nseg_out < 0 || nseg_out > 65535 || K < 1 || K > MERGE_MAX_K || max_total < 0 || stride_out < 1 || score_stride < 1)
    return FC_EINVAL;
  if ((keep && keep_stride < 1) || (ord && ord_stride < 1)) return FC_EINVAL;
  if (nseg_out == 0) return FC_OK;
  if (!desc || !counts_dev || !scores || !boxes || !out_boxes || !out_scores || !out_count) return FC_EINVAL;
  if (ws_bytes < fc_merge_sorted_segments_ws_bytes(nseg_out, max_total)) return FC_EWS;
  // an input segment never holds more rows than the index table it is read through
  const int cap_in = keep ? keep_stride : ord ? ord_stride : 0x7fffffff;
  const int limit = cap >= 0 ? min(cap, stride_out) : stride_out;
  const int gx = (int)std::min<int64_t>(std::max<int64_t>(fc_cdiv(max_total, MERGE_THREADS), 1), MERGE_MAX_GX);
  const dim3 grid(gx, nseg_out);
  const size_t lds = (size_t)(MERGE_THREADS + K + 1) * sizeof(int);
  float* wsf = (float*)ws;
  if (max_total > 0) {
    k_merge_gather<<<grid, MERGE_THREADS, lds, stream>>>(desc, K, counts_dev, cap_in, keep, keep_stride, ord, ord_stride, scores,
                                                          score_stride, max_total, wsf);
    FC_CHECK_LAUNCH();
  }
  k_merge_scatter<<<grid, MERGE_THREADS, lds, stream>>>(desc, K, counts_dev, cap_in, keep, keep_stride, ord, ord_stride, boxes,
                                                         flags, max_total, limit, wsf, out_boxes, out_scores, out_src, out_count,
                                                         stride_out);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
