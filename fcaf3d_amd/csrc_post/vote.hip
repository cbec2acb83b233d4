// Box voting for the test-time augmentation merge (No reference counterpart: merge_augs.py:7-91 keeps the NMS survivors as they
// are).  Between the merge NMS and the per-scene merge of Fcaf3DNeckWithHead.get_bboxes_aug every KEPT box of a (scene, class)
// segment becomes the score-weighted mean of the segment's candidates that overlap it:
//   M      = {i} ∪ { j != i, j < count : iou(i, j) >= vote_thr }          iou: the merge NMS's fp32 BEV IoU (bev_geom.h), a = box i
//   out[k] = fp32( Σ_{j∈M} score_j box_j[k] / Σ_{j∈M} score_j ), k = 0..5   both sums in fp64, ascending j (a product of two fp32
//                                                                          values is exact in fp64); column 6 keeps box i's yaw
// With yaws, d = remainder(yaw_j - yaw_i, fp32 π); |d| > π/4: member j contributes (l_j, w_j) in place of (w_j, l_j) — a rectangle
// written with its sides exchanged votes for the right sides.  A weight sum that is not positive and finite leaves box i as it is.
// Rows that are not kept are copied; rows at or past a segment's count are neither read nor written.
//
// Mapping.  Segments are short (about 230 candidates, about 90 kept at A = 4) and many (B·C).  Grid (kept groups, segments), 256
// threads: ONE WAVE64 PER KEPT BOX.  A workgroup stages the segment's boxes and scores in LDS tiles of VOTE_TILE candidates (row
// stride 7 floats: odd, so the 32-bank ds_read_b32 of lane = candidate is conflict-free); the wave's lanes take one candidate each,
// __ballot turns the 64 membership tests into a word, and lanes 0..5 walk the set bits of that word in ascending order, each summing
// its own column (and the weights) in fp64.  The order of a box's sum is therefore ascending j whatever the segment's length, the
// grid or the wave that serves it: deterministic, no atomics.  A thread per kept box would leave a segment to two waves that each
// run 230 divergent rotated-IoU evaluations back to back; a wave per box runs 4 rounds of 64 and fills the machine with B·C·kept/4
// workgroups' worth of waves.
//
// Kept apart from csrc/ as merge.hip is: it never runs in the training step whose profiles csrc/ is pinned to.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "../csrc/bev_geom.h"     // the NMS's BEV IoU (sets its own contraction)
// exact products, as csrc/nms.hip computes them: no FMA contraction
#pragma clang fp contract(off)

#define VOTE_THREADS 256
#define VOTE_WAVE 64
#define VOTE_WAVES (VOTE_THREADS / VOTE_WAVE)      // kept boxes a workgroup votes for at once
#define VOTE_TILE 128                              // candidates staged in LDS at a time
#define VOTE_KEPT_PER_BLOCK 32                     // the grid is sized for 8 rounds of a workgroup at max_keep kept boxes
#define VOTE_MAX_GX 256

namespace {

constexpr float kVotePi = 3.14159265358979323846f;    // fp32(π)

// The launch shape, stated once (tools/vote_host_emu.cpp walks the same grid from this text): kept-box groups per segment.
// keep_counts lives on the device, so the grid is sized by the host bound; the rounds loop walks whatever is there.
inline unsigned vote_blocks_x(int max_keep) {
  const int g = (max_keep + VOTE_KEPT_PER_BLOCK - 1) / VOTE_KEPT_PER_BLOCK;
  return (unsigned)(g < 1 ? 1 : g > VOTE_MAX_GX ? VOTE_MAX_GX : g);
}

// is row p one of the kept positions sk[0 .. kc) (ascending, as fc_nms_bev writes them)
__device__ inline bool vote_is_kept(const int* __restrict__ sk, int kc, int p) {
  int lo = 0, hi = kc;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sk[mid] < p) lo = mid + 1; else hi = mid;
  }
  return lo < kc && sk[lo] == p;
}

__global__ __launch_bounds__(VOTE_THREADS) void k_vote_boxes(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ counts, int stride, int max_count,
    const int* __restrict__ keep, const int* __restrict__ keep_counts, int keep_stride, int max_keep, float thr, int flags,
    float* __restrict__ out, int* __restrict__ members) {
  __shared__ float s_box[VOTE_TILE * 7];
  __shared__ float s_score[VOTE_TILE];
  const int s = blockIdx.y;
  const int tid = threadIdx.x;
  const int n = min(max(counts[s], 0), max_count);             // max_count <= stride, max_keep <= keep_stride (checked by the host)
  const int kc = min(max(keep_counts[s], 0), max_keep);
  const float* sb = boxes + (int64_t)s * stride * 7;
  const float* ss = scores + (int64_t)s * stride;
  const int* sk = keep + (int64_t)s * keep_stride;
  float* so = out + (int64_t)s * stride * 7;
  // rows that are not kept: copied as they are (a kept row is written below, by the wave that votes for it)
  for (int p = blockIdx.x * VOTE_THREADS + tid; p < n; p += gridDim.x * VOTE_THREADS) {
    if (vote_is_kept(sk, kc, p)) continue;
#pragma unroll
    for (int e = 0; e < 7; ++e) so[(int64_t)p * 7 + e] = sb[(int64_t)p * 7 + e];
  }
  const int wave = tid / VOTE_WAVE, lane = tid % VOTE_WAVE;
  const int per_pass = gridDim.x * VOTE_WAVES;
  for (int q0 = blockIdx.x * VOTE_WAVES; q0 < kc; q0 += per_pass) {       // block-uniform: every wave meets every barrier
    const int q = q0 + wave;
    int i = -1;
    if (q < kc) {
      i = sk[q];
      if (i < 0 || i >= n) i = -1;                                        // a bad position votes for nothing and writes nothing
    }
    float bi[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) bi[e] = i >= 0 ? sb[(int64_t)i * 7 + e] : 0.f;
    double acc = 0.0, den = 0.0;
    int cnt = 0;
    for (int t0 = 0; t0 < n; t0 += VOTE_TILE) {
      const int m = min(n - t0, VOTE_TILE);
      __syncthreads();                                                    // the previous tile has been read
      for (int e = tid; e < m * 7; e += VOTE_THREADS) s_box[e] = sb[(int64_t)t0 * 7 + e];
      for (int e = tid; e < m; e += VOTE_THREADS) s_score[e] = ss[t0 + e];
      __syncthreads();
      for (int h0 = 0; h0 < m; h0 += VOTE_WAVE) {                         // wave-uniform
        const int jl = h0 + lane;
        bool mem = false;
        if (i >= 0 && jl < m) {
          if (t0 + jl == i) {
            mem = true;                                                   // by definition, not by iou(i, i)
          } else {
            float bj[7];
#pragma unroll
            for (int e = 0; e < 7; ++e) bj[e] = s_box[jl * 7 + e];
            const float v = (flags & FC_VOTE_ROTATED) ? evg::iou_bev_rotated(bi, bj) : evg::iou_bev_aligned(bi, bj);
            mem = v >= thr;                                               // a NaN is not a member
          }
        }
        unsigned long long bits = __ballot(mem);
        cnt += __popcll(bits);
        if (lane < 6) {
          while (bits) {                                                  // ascending j
            const int l = h0 + __ffsll(bits) - 1;
            bits &= bits - 1;
            int col = lane;
            if ((flags & FC_VOTE_WITH_YAW) && (lane == 3 || lane == 4)) {
              const float d = remainderf(s_box[l * 7 + 6] - bi[6], kVotePi);
              if (fabsf(d) > kVotePi * 0.25f) col = 7 - lane;
            }
            const double w = (double)s_score[l];
            acc += w * (double)s_box[l * 7 + col];
            den += w;
          }
        }
      }
    }
    if (i >= 0) {
      if (lane < 6) {
        const bool ok = den > 0.0 && den <= 1.7976931348623157e308;       // positive and finite (a NaN fails both)
        float v = bi[0];
#pragma unroll
        for (int e = 1; e < 6; ++e) v = lane == e ? bi[e] : v;
        so[(int64_t)i * 7 + lane] = ok ? (float)(acc / den) : v;
      } else if (lane == 6) {
        so[(int64_t)i * 7 + 6] = bi[6];
      } else if (lane == 7 && members) {
        members[(int64_t)s * keep_stride + q] = cnt;
      }
    }
  }
}

}  // namespace

extern "C" {

int fc_vote_boxes(const float* boxes, const float* scores, const int* counts_dev, int nseg, int stride, int max_count,
                  const int* keep, const int* keep_counts_dev, int keep_stride, int max_keep, float vote_thr, int flags,
                  float* out_boxes, int* out_members, hipStream_t stream) {
  if (nseg < 0 || nseg > 65535 || stride < 0 || keep_stride < 0 || max_count < 0 || max_keep < 0) return FC_EINVAL;
  if (stride < max_count || keep_stride < max_keep) return FC_EINVAL;
  if (!(vote_thr > 0.f && vote_thr <= 1.f)) return FC_EINVAL;
  if (flags & ~(FC_VOTE_ROTATED | FC_VOTE_WITH_YAW)) return FC_EINVAL;
  if (nseg == 0 || max_count == 0) return FC_OK;
  if (!boxes || !scores || !counts_dev || !keep_counts_dev || !out_boxes || (max_keep > 0 && !keep)) return FC_EINVAL;
  const dim3 grid(vote_blocks_x(max_keep), (unsigned)nseg);
  k_vote_boxes<<<grid, VOTE_THREADS, 0, stream>>>(boxes, scores, counts_dev, stride, max_count, keep, keep_counts_dev, keep_stride,
                                                  max_keep, vote_thr, flags, out_boxes, out_members);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
