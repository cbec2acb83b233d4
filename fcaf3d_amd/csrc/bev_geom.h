// Rotated-BEV rectangle overlap, stated once: the NMS (csrc/nms.hip) and the post-processing kernels that must agree with it to the
// bit (csrc_post/eval.hip, csrc_post/vote.hip) all compile these functions.  The header lives in csrc/ because a csrc/ kernel depends
// on it, so build.source_hash() has to cover it; a change here is a change of the NMS.
//
// Exact products, as the reference's torch / host code computes them (e.g. num == 0 for parallel edges): every function that does
// arithmetic switches FMA contraction off in its own body, so the result does not depend on the including file and the including
// file's setting is left alone.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

#define EVG_EPS 1e-8f

namespace evg {

struct P2 { float x, y; };

__device__ static inline float cross3(P2 p1, P2 p2, P2 p0) {
#pragma clang fp contract(off)
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// proper crossing of segments p0p1 and q0q1 (touching / collinear do not count)
__device__ static inline bool seg_cross(P2 p1, P2 p0, P2 q1, P2 q0, P2* out) {
#pragma clang fp contract(off)
  bool overlap = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                 fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
  if (!overlap) return false;
  float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0);
  float s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
  float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > EVG_EPS) {
    out->x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    out->y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    float D = a0 * b1 - a1 * b0;
    out->x = (b0 * c1 - b1 * c0) / D;
    out->y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

__device__ static inline bool in_box_bev(const float* box, P2 p) {
#pragma clang fp contract(off)
  const float MARGIN = 1e-2f;
  float c = cosf(-box[6]), s = sinf(-box[6]);
  float rx = (p.x - box[0]) * c + (p.y - box[1]) * (-s);
  float ry = (p.x - box[0]) * s + (p.y - box[1]) * c;
  return fabsf(rx) < box[3] / 2 + MARGIN && fabsf(ry) < box[4] / 2 + MARGIN;
}

__device__ static inline void box_corners(const float* box, P2* c /*[5]*/) {
#pragma clang fp contract(off)
  float hx = box[3] / 2, hy = box[4] / 2;
  float cs = cosf(box[6]), sn = sinf(box[6]);
  const float sx[4] = {-1.f, 1.f, 1.f, -1.f}, sy[4] = {-1.f, -1.f, 1.f, 1.f};
  for (int k = 0; k < 4; ++k) {
    // axis-aligned corner, then rotation about the centre
    float px = box[0] + sx[k] * hx, py = box[1] + sy[k] * hy;
    c[k].x = (px - box[0]) * cs + (py - box[1]) * (-sn) + box[0];
    c[k].y = (px - box[0]) * sn + (py - box[1]) * cs + box[1];
  }
  c[4] = c[0];
}

// area of the intersection polygon of two rotated BEV rectangles (x,y,_,dx,dy,_,heading)
__device__ static float bev_overlap_rotated(const float* a, const float* b) {
#pragma clang fp contract(off)
  P2 ca[5], cb[5], pts[24];
  box_corners(a, ca);
  box_corners(b, cb);
  int cnt = 0;
  P2 ctr = {0.f, 0.f};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 x;
      if (seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], &x)) {
        pts[cnt++] = x;
        ctr.x += x.x; ctr.y += x.y;
      }
    }
  for (int k = 0; k < 4; ++k) {
    if (in_box_bev(a, cb[k])) { pts[cnt++] = cb[k]; ctr.x += cb[k].x; ctr.y += cb[k].y; }
    if (in_box_bev(b, ca[k])) { pts[cnt++] = ca[k]; ctr.x += ca[k].x; ctr.y += ca[k].y; }
  }
  if (cnt < 3) return 0.f;
  ctr.x /= cnt; ctr.y /= cnt;
  float ang[24];
  for (int k = 0; k < cnt; ++k) ang[k] = atan2f(pts[k].y - ctr.y, pts[k].x - ctr.x);
  for (int k = 1; k < cnt; ++k) {            // stable insertion sort by polar angle
    P2 p = pts[k]; float g = ang[k];
    int m = k - 1;
    while (m >= 0 && ang[m] > g) { pts[m + 1] = pts[m]; ang[m + 1] = ang[m]; --m; }
    pts[m + 1] = p; ang[m + 1] = g;
  }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; ++k) {
    float ux = pts[k].x - pts[0].x, uy = pts[k].y - pts[0].y;
    float vx = pts[k + 1].x - pts[0].x, vy = pts[k + 1].y - pts[0].y;
    area += ux * vy - uy * vx;
  }
  return fabsf(area) / 2.f;
}

// the two BEV IoUs of the NMS: what fc_nms_bev compares with its threshold and fc_boxes_iou_bev stores (csrc_post/vote.hip: a = the
// kept box, b = the candidate)
__device__ static inline float iou_bev_rotated(const float* a, const float* b) {
#pragma clang fp contract(off)
  float sa = a[3] * a[4], sb = b[3] * b[4];
  float ov = bev_overlap_rotated(a, b);
  return ov / fmaxf(sa + sb - ov, EVG_EPS);
}

__device__ static inline float iou_bev_aligned(const float* a, const float* b) {
#pragma clang fp contract(off)
  float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
  float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
  float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
  float inter = w * h;
  return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, EVG_EPS);
}

// iou_bev_rotated's value, then fcaf3d_amd/nms.py:86-96 (boxes_iou3d_gpu) on it, the same fp32 operations in the same order
// (csrc_post/eval.hip only): a = detection, b = ground truth, both (x, y, z, dx, dy, dz, heading) gravity centre
__device__ static inline float iou3d_rotated(const float* a, const float* b) {
#pragma clang fp contract(off)
  const float sa = a[3] * a[4], sb = b[3] * b[4];
  const float ov = bev_overlap_rotated(a, b);
  const float iou = ov / fmaxf(sa + sb - ov, EVG_EPS);
  const float ov_bev = iou * (sa + sb) / (1.f + iou);
  const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2;
  const float b_max = b[2] + b[5] / 2, b_min = b[2] - b[5] / 2;
  const float ov_h = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
  const float ov3 = ov_bev * ov_h;
  const float vol_a = a[3] * a[4] * a[5], vol_b = b[3] * b[4] * b[5];
  return ov3 / fmaxf(vol_a + vol_b - ov3, 1e-6f);
}

}  // namespace evg
