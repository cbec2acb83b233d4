// Per-class BEV NMS on gfx950 — all classes of a scene in two launches, nothing copied to the host.
//
// Replaces mmdet3d/ops/pcdet_nms: nms_gpu / nms_normal_gpu (src/iou3d_nms.cpp:90-186) and their
// kernels nms_kernel / nms_normal_kernel (src/iou3d_nms_kernel.cu:267-372) with the device
// functions they call (:35-234, :314-325), as driven per class by
// Fcaf3DNeckWithHead._nms (fcaf3d_neck_with_head.py:332-353).
//
// Kernel 1: one wavefront per (row block, column block, class): thread = row box, 64 column boxes in
//           LDS, 64-bit suppression word per (row, column block) — wave64 makes the word one lane each.
// Kernel 2: one wavefront per class runs the greedy scan on the device (the reference copies the whole
//           mask to the host and scans there, iou3d_nms.cpp:111-132): lane j owns removed-word j.
#include "fc_common.h"
#include "bev_geom.h"     // the rotated / aligned BEV IoU, shared with csrc_post/eval.hip and vote.hip (sets its own contraction)
// exact products as in the reference's torch / host code: no FMA contraction
#pragma clang fp contract(off)

// grid (block pairs of the UPPER triangle, 1, classes), 64 threads.  The greedy scan only reads the words of column blocks at or
// after a row's own block (a box can only suppress boxes that come later), so the lower triangle is never computed (r4: half
// the IoU work and half the workgroups of the r1-r3 (col blocks, row blocks) grid; the reference computes the full matrix,
// iou3d_nms_kernel.cu:267-313, and its host scan likewise only acts on later boxes).  Pair t = cb (cb + 1) / 2 + rb, rb <= cb.
__global__ __launch_bounds__(64) void k_nms_mask(const float* __restrict__ boxes, const int* __restrict__ counts,
                                                 int stride, float thresh, int rotated,
                                                 unsigned long long* __restrict__ mask) {
  const int seg = blockIdx.z;
  const int n = counts[seg];
  const int t = blockIdx.x;
  int cb = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((cb + 1) * (cb + 2) / 2 <= t) ++cb;           // float rounding: settle on cb (cb + 1) / 2 <= t < (cb + 1)(cb + 2) / 2
  while (cb * (cb + 1) / 2 > t) --cb;
  const int rblk = t - cb * (cb + 1) / 2;
  const int row0 = rblk * 64, col0 = cb * 64;
  if (row0 >= n || col0 >= n) return;
  const int words = (stride + 63) / 64;
  const float* sb = boxes + (int64_t)seg * stride * 7;
  __shared__ float cbox[64 * 7];
  int col_size = min(n - col0, 64);
  if ((int)threadIdx.x < col_size)
    for (int e = 0; e < 7; ++e) cbox[threadIdx.x * 7 + e] = sb[(int64_t)(col0 + threadIdx.x) * 7 + e];
  __syncthreads();
  int row = row0 + threadIdx.x;
  if (row >= n) return;
  float rb[7];
  for (int e = 0; e < 7; ++e) rb[e] = sb[(int64_t)row * 7 + e];
  unsigned long long bits = 0;
  int start = (row0 == col0) ? (int)threadIdx.x + 1 : 0;
  for (int j = start; j < col_size; ++j) {
    float v = rotated ? evg::iou_bev_rotated(rb, cbox + j * 7) : evg::iou_bev_aligned(rb, cbox + j * 7);
    if (v > thresh) bits |= 1ull << j;
  }
  mask[((int64_t)seg * stride + row) * words + cb] = bits;
}

// grid (classes), 64 threads: lane j holds removed-words j, j+64, ...
__global__ __launch_bounds__(64) void k_nms_greedy(const unsigned long long* __restrict__ mask, const int* __restrict__ counts,
                                                   int stride, int* __restrict__ keep, int* __restrict__ keep_count) {
  const int seg = blockIdx.x;
  const int n = counts[seg];
  const int words = (stride + 63) / 64;
  const int lane = threadIdx.x;
  constexpr int MAXW = 16;                    // up to 64*16 words = 65536 boxes per class
  unsigned long long remv[MAXW];
#pragma unroll
  for (int w = 0; w < MAXW; ++w) remv[w] = 0ull;
  const unsigned long long* sm = mask + (int64_t)seg * stride * words;
  int* sk = keep + (int64_t)seg * stride;
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    int nblock = i >> 6, inblock = i & 63;
    // the word that holds box i lives in lane nblock%64, slot nblock/64
    unsigned long long word = 0ull;
#pragma unroll
    for (int w = 0; w < MAXW; ++w)
      if (w == (nblock >> 6)) word = remv[w];
    word = __shfl(word, nblock & 63, 64);
    if (word & (1ull << inblock)) continue;     // wave-uniform
    if (lane == 0) sk[kept] = i;
    ++kept;
    const unsigned long long* row = sm + (int64_t)i * words;
    const int nwords_used = (n + 63) >> 6;
#pragma unroll
    for (int w = 0; w < MAXW; ++w) {
      int j = w * 64 + lane;
      if (j >= nblock && j < nwords_used) remv[w] |= row[j];
    }
  }
  if (lane == 0) keep_count[seg] = kept;
}

extern "C" {

int64_t fc_nms_bev_ws_bytes(int nseg, int stride) {
  return (int64_t)nseg * stride * ((stride + 63) / 64) * (int64_t)sizeof(unsigned long long);
}

// boxes (nseg, stride, 7) — segment s holds counts[s] boxes sorted by descending score.
// keep (nseg, stride): ascending positions of the surviving boxes; keep_count (nseg).
int fc_nms_bev(const float* boxes, const int* counts_dev, int nseg, int stride, float thresh, int rotated,
               unsigned long long* mask_ws, int64_t ws_bytes, int* keep, int* keep_count, hipStream_t stream) {
  if (nseg < 1 || stride < 1 || stride > 65536 || nseg > 65535) return FC_EINVAL;
  if (ws_bytes < fc_nms_bev_ws_bytes(nseg, stride)) return FC_EWS;
  int nb = (stride + 63) / 64;
  dim3 grid(nb * (nb + 1) / 2, 1, nseg);
  k_nms_mask<<<grid, 64, 0, stream>>>(boxes, counts_dev, stride, thresh, rotated, mask_ws);
  FC_CHECK_LAUNCH();
  k_nms_greedy<<<nseg, 64, 0, stream>>>(mask_ws, counts_dev, stride, keep, keep_count);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// pairwise BEV IoU matrix (N,M) — pcdet `boxes_iou_bev_gpu` (iou3d_nms_kernel.cu:251-265); used by the parity tests
__global__ void k_iou_bev_matrix(const float* __restrict__ a, int n, const float* __restrict__ b, int m, int rotated,
                                 float* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n * m) return;
  int i = (int)(t / m), j = (int)(t % m);
  out[t] = rotated ? evg::iou_bev_rotated(a + i * 7, b + j * 7) : evg::iou_bev_aligned(a + i * 7, b + j * 7);
}

int fc_boxes_iou_bev(const float* boxes_a, int n, const float* boxes_b, int m, int rotated, float* out,
                     hipStream_t stream) {
  if (n < 0 || m < 0) return FC_EINVAL;
  if (n == 0 || m == 0) return FC_OK;
  k_iou_bev_matrix<<<(unsigned)fc_cdiv((int64_t)n * m, 128), 128, 0, stream>>>(boxes_a, n, boxes_b, m, rotated, out);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
