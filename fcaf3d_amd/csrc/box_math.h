// Scalar pieces the box losses share: csrc/loss.hip (k_riou3d, k_sort_v, aiou3d_eval) and csrc_post/eiou.hip (eiou7_row, eiou6_row).
// Values in, values out; every function that does arithmetic switches FMA contraction off in its own body.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

// Angular sort key of sort_v ("sign of y, then |x| x / (x^2 + y^2)", eps 1e-8): monotone in
// atan2(y, x) over (-pi, pi], built from +, *, / only — with contraction off (set here, whatever the including file has set) it is
// bit-identical to the numpy restatement (oracle/loss_oracle.py::sort_key), so the index order is EXACT across machines (r1/r2 used
// atan2f: two libms ordered ~0.5 % of near-tied vertices differently).
__device__ static inline float sort_key(float y, float x) {
#pragma clang fp contract(off)
  const float r = x * fabsf(x) / (x * x + y * y + 1e-8f);
  return y < 0.f ? r - 3.f : 1.f - r;
}

// torch.max / torch.min split the gradient evenly on ties; clamp(min=0) passes it at x >= 0.
__device__ static inline void tie_max(float a, float b, float* v, float* wa) {
  *v = a > b ? a : b;
  *wa = a > b ? 1.f : (a == b ? 0.5f : 0.f);
}
__device__ static inline void tie_min(float a, float b, float* v, float* wa) {
  *v = a < b ? a : b;
  *wa = a < b ? 1.f : (a == b ? 0.5f : 0.f);
}

// One axis of the axis-aligned IoU (iou3d_calculator.py:201-330): the two intervals [p1, p2] (centre pc, size ps) and [t1, t2], their
// overlap wh = clamp(min(p2, t2) - max(p1, t1), 0) and its derivatives w.r.t. pc and ps (d/dc = wr - wl, d/ds = wr/2 + wl/2).
struct AxisOverlap { float p1, p2, t1, t2, wh, dwh_dc, dwh_ds; };
__device__ static inline AxisOverlap axis_overlap(float pc, float ps, float tc, float ts) {
#pragma clang fp contract(off)
  AxisOverlap r;
  r.p1 = pc - ps / 2; r.p2 = pc + ps / 2;
  r.t1 = tc - ts / 2; r.t2 = tc + ts / 2;
  float lt, rb, wl, wr;
  tie_max(r.p1, r.t1, &lt, &wl);       // d lt / d p1
  tie_min(r.p2, r.t2, &rb, &wr);       // d rb / d p2
  float d = rb - lt;
  float pass = d >= 0.f ? 1.f : 0.f;
  r.wh = d > 0.f ? d : 0.f;
  r.dwh_dc = pass * (wr - wl);
  r.dwh_ds = pass * 0.5f * (wr + wl);
  return r;
}

// d IoU / d (centre, size) of one axis, IoU = ov / U with U = max(a1 + a2 - ov, eps) (upass = 1 where the max passes the union):
// wh_b, wh_c = the other two axes' overlaps, sp_b, sp_c = the other two axes' sizes of p
struct AxisIouGrad { float dU_dc, dU_ds, diou_dc, diou_ds; };
__device__ static inline AxisIouGrad axis_iou_grad(float wh_b, float wh_c, float dwh_dc, float dwh_ds, float sp_b, float sp_c, float ov, float U,
                                                   float upass) {
#pragma clang fp contract(off)
  AxisIouGrad r;
  float dov_dwh = wh_b * wh_c;
  float dov_dc = dov_dwh * dwh_dc;
  float dov_ds = dov_dwh * dwh_ds;
  float da1_ds = sp_b * sp_c;          // area1 = prod (p2-p1): d/ds_a = prod of the others
  r.dU_dc = upass * (-dov_dc);
  r.dU_ds = upass * (da1_ds - dov_ds);
  r.diou_dc = (dov_dc * U - ov * r.dU_dc) / (U * U);
  r.diou_ds = (dov_ds * U - ov * r.dU_ds) / (U * U);
  return r;
}
