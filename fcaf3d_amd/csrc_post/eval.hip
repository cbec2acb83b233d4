// Detection-to-ground-truth matching of indoor_eval (mmdet3d/core/evaluation/indoor_eval.py:86-146) for ALL scenes and classes of
// a validation set in one call: three launches, nothing read back.
//
// The reference walks the detections of a class in descending confidence; a detection is a true positive at a threshold when
// its best-overlapping ground-truth box of its class and scene exceeds the threshold and no earlier detection has claimed that
// box.  A detection only ever claims its BEST box (:131-146: a later claimant is a false positive, it does not fall back to
// another box), and only detections whose best IoU exceeds the threshold claim.  So per (ground-truth box, threshold) the true
// positive is the first claimant in the order — an order-independent minimum:
//   key = (~ordered(score) << 32) | position in the scene       (ordered: the order-preserving bit transform of an fp32)
//   smallest key = highest score, equal scores to the lowest position.
// Launch 1 presets the outputs and the key table; launch 2 finds every detection's best box (first maximum in scene order, the
// strict '>' scan of :131-136) and folds its key into the table with a 64-bit unsigned atomicMin (the minimum does not depend on
// arrival order: deterministic); launch 3 turns winners into bits.
//
// Kept apart from csrc/ as merge.hip is: it never runs in the training step whose profiles csrc/ is pinned to.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "../csrc/bev_geom.h"     // the NMS's BEV IoU (sets its own contraction)
// exact products, as csrc/nms.hip and torch's elementwise kernels compute them: no FMA contraction
#pragma clang fp contract(off)

#define EVAL_THREADS 256
#define EVAL_GT_CHUNK 64          // ground-truth boxes staged in LDS at a time
#define EVAL_MAX_GY 64            // detection tiles of a scene walked in parallel (grid-stride beyond)
#define EVAL_MAX_THR 8

namespace {

// The launch shapes, stated once (tools/eval_host_emu.cpp walks the same grids from this text).
// k_eval_init: a thread per detection and per key.
inline unsigned eval_init_blocks(int64_t n_det, int64_t n_keys) {
  const int64_t n = n_det > n_keys ? n_det : n_keys;
  return (unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS);
}
// k_eval_best / k_eval_bits: detection tiles per scene.  seg lives on the device, so the host does not know the largest scene:
// the grid is sized for twice the MEAN scene and a larger scene's tiles are walked by the grid-stride loop.
inline unsigned eval_tiles_y(int64_t n_det, int64_t n_scenes) {
  const int64_t mean = (n_det + n_scenes - 1) / n_scenes;
  const int64_t tiles = (2 * mean + EVAL_THREADS - 1) / EVAL_THREADS;
  return (unsigned)(tiles < 1 ? 1 : tiles > EVAL_MAX_GY ? EVAL_MAX_GY : tiles);
}

struct SceneSeg { int ds, dc, gs, gc; };

// the scene's ranges, cut to the arrays (the caller checks them; a bad row must still not reach outside)
__device__ inline SceneSeg load_seg(const int64_t* __restrict__ seg, int s, int64_t n_det, int64_t n_gt) {
  const int64_t ds = seg[(int64_t)s * 4], dc = seg[(int64_t)s * 4 + 1], gs = seg[(int64_t)s * 4 + 2], gc = seg[(int64_t)s * 4 + 3];
  SceneSeg r;
  const bool dok = ds >= 0 && dc > 0 && ds < n_det;
  const bool gok = gs >= 0 && gc > 0 && gs < n_gt;
  r.ds = dok ? (int)ds : 0;
  r.dc = dok ? (int)(dc < n_det - ds ? dc : n_det - ds) : 0;
  r.gs = gok ? (int)gs : 0;
  r.gc = gok ? (int)(gc < n_gt - gs ? gc : n_gt - gs) : 0;
  return r;
}

__device__ inline unsigned long long claim_key(float score, int pos) {
  const unsigned u = __float_as_uint(score + 0.f);                   // -0 -> +0
  const unsigned ordered = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)(~ordered) << 32) | (unsigned long long)(unsigned)pos;
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_init(int64_t n_det, int64_t n_keys, float* __restrict__ best_iou,
                                                            int* __restrict__ best_gt, unsigned char* __restrict__ tp_bits,
                                                            unsigned long long* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (i < n_det) {
    best_iou[i] = -INFINITY;
    best_gt[i] = -1;
    tp_bits[i] = 0;
  }
  if (i < n_keys) keys[i] = FC_EMPTY_KEY;
}

// grid (scenes, detection tiles), 256 threads: thread = detection
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_best(
    const float* __restrict__ det_boxes, int det_dim, const float* __restrict__ det_scores, const int64_t* __restrict__ det_labels,
    const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels, const int64_t* __restrict__ seg, int64_t n_det,
    int64_t n_gt, const double* __restrict__ thr, int n_thr, int flags, float* __restrict__ best_iou, int* __restrict__ best_gt,
    unsigned long long* __restrict__ keys) {
  __shared__ float s_box[EVAL_GT_CHUNK * 7];
  __shared__ int s_lab[EVAL_GT_CHUNK];
  const SceneSeg sg = load_seg(seg, blockIdx.x, n_det, n_gt);
  for (int tile = blockIdx.y; (int64_t)tile * EVAL_THREADS < sg.dc; tile += gridDim.y) {
    const int p = tile * EVAL_THREADS + (int)threadIdx.x;
    const bool live = p < sg.dc;
    const int64_t d = (int64_t)sg.ds + p;
    float a[7];
    int64_t lab = -1;
    if (live) {
      const float* src = det_boxes + d * det_dim;
#pragma unroll
      for (int e = 0; e < 6; ++e) a[e] = src[e];
      a[6] = det_dim == 7 ? src[6] : 0.f;
      if (flags & FC_EVAL_DET_BOTTOM) a[2] = a[2] + a[5] * 0.5f;
      lab = det_labels[d];
    } else {
#pragma unroll
      for (int e = 0; e < 7; ++e) a[e] = 0.f;
    }
    float bi = -INFINITY;
    int bj = -1;
    for (int g0 = 0; g0 < sg.gc; g0 += EVAL_GT_CHUNK) {
      const int m = min(sg.gc - g0, EVAL_GT_CHUNK);
      __syncthreads();                                  // the previous chunk has been read
      for (int e = threadIdx.x; e < m * 7; e += EVAL_THREADS) s_box[e] = gt_boxes[((int64_t)sg.gs + g0) * 7 + e];
      if ((int)threadIdx.x < m) s_lab[threadIdx.x] = gt_labels[(int64_t)sg.gs + g0 + threadIdx.x];
      __syncthreads();
      if (live)
        for (int j = 0; j < m; ++j) {
          if ((int64_t)s_lab[j] != lab) continue;
          const float v = evg::iou3d_rotated(a, s_box + j * 7);
          if (v > bi) { bi = v; bj = g0 + j; }
        }
    }
    if (live) {
      best_iou[d] = bi;
      best_gt[d] = bj;
      if (bj >= 0) {
        const unsigned long long key = claim_key(det_scores[d], p);
        for (int t = 0; t < n_thr; ++t)
          if ((double)bi > thr[t]) atomicMin(&keys[((int64_t)sg.gs + bj) * n_thr + t], key);
      }
    }
  }
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_bits(
    const float* __restrict__ det_scores, const int64_t* __restrict__ seg, int64_t n_det, int64_t n_gt,
    const double* __restrict__ thr, int n_thr, const float* __restrict__ best_iou, const int* __restrict__ best_gt,
    const unsigned long long* __restrict__ keys, unsigned char* __restrict__ tp_bits) {
  const SceneSeg sg = load_seg(seg, blockIdx.x, n_det, n_gt);
  for (int tile = blockIdx.y; (int64_t)tile * EVAL_THREADS < sg.dc; tile += gridDim.y) {
    const int p = tile * EVAL_THREADS + (int)threadIdx.x;
    if (p >= sg.dc) continue;
    const int64_t d = (int64_t)sg.ds + p;
    const int bj = best_gt[d];
    unsigned bits = 0;
    if (bj >= 0) {
      const float bi = best_iou[d];
      const unsigned long long key = claim_key(det_scores[d], p);
      for (int t = 0; t < n_thr; ++t)
        if ((double)bi > thr[t] && keys[((int64_t)sg.gs + bj) * n_thr + t] == key) bits |= 1u << t;
    }
    tp_bits[d] = (unsigned char)bits;
  }
}

}  // namespace

extern "C" {

int64_t fc_eval_match_ws_bytes(int64_t n_det, int64_t n_gt, int n_thr) {
  if (n_det < 0 || n_gt < 0 || n_thr < 1 || n_thr > EVAL_MAX_THR) return 0;
  return fc_align(n_gt * n_thr * (int64_t)sizeof(unsigned long long), 256);
}

int fc_eval_match(const float* det_boxes, int det_dim, const float* det_scores, const int64_t* det_labels, const float* gt_boxes,
                  const int* gt_labels, const int64_t* seg, int n_scenes, int64_t n_det, int64_t n_gt, const double* thr, int n_thr,
                  int flags, float* best_iou, int* best_gt, unsigned char* tp_bits, void* ws, int64_t ws_bytes,
                  hipStream_t stream) {
  if (det_dim != 6 && det_dim != 7) return FC_EINVAL;
  if (n_thr < 1 || n_thr > EVAL_MAX_THR) return FC_EINVAL;
  if (n_scenes < 0 || n_det < 0 || n_gt < 0 || n_det > 0x7fffffff || n_gt > 0x7fffffff) return FC_EINVAL;
  if (flags & ~FC_EVAL_DET_BOTTOM) return FC_EINVAL;
  if (n_det == 0) return FC_OK;
  if (!det_boxes || !det_scores || !det_labels || !thr || !best_iou || !best_gt || !tp_bits) return FC_EINVAL;
  if (n_scenes > 0 && !seg) return FC_EINVAL;
  if (n_gt > 0 && (!gt_boxes || !gt_labels || !ws)) return FC_EINVAL;
  if (ws_bytes < fc_eval_match_ws_bytes(n_det, n_gt, n_thr)) return FC_EWS;
  unsigned long long* keys = (unsigned long long*)ws;
  const int64_t n_keys = n_gt * n_thr;
  k_eval_init<<<eval_init_blocks(n_det, n_keys), EVAL_THREADS, 0, stream>>>(n_det, n_keys, best_iou, best_gt, tp_bits, keys);
  FC_CHECK_LAUNCH();
  if (n_scenes == 0) return FC_OK;
  const dim3 grid((unsigned)n_scenes, eval_tiles_y(n_det, n_scenes));
  k_eval_best<<<grid, EVAL_THREADS, 0, stream>>>(det_boxes, det_dim, det_scores, det_labels, gt_boxes, gt_labels, seg, n_det, n_gt,
                                                  thr, n_thr, flags, best_iou, best_gt, keys);
  FC_CHECK_LAUNCH();
  k_eval_bits<<<grid, EVAL_THREADS, 0, stream>>>(det_scores, seg, n_det, n_gt, thr, n_thr, best_iou, best_gt, keys, tp_bits);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
