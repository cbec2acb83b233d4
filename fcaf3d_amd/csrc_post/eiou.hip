// Enclosing-box 3D IoU losses (GIoU, DIoU) with their gradient w.r.t. the prediction, fused, on gfx950:
//   * rotated boxes — rotated_iou/oriented_iou_loss.py:112-152 (cal_giou_3d, cal_diou_3d) over cal_iou_3d (:86-109) and
//     min_enclosing_box.py:142-172 (smallest_bounding_box over the 24 candidate lines of generate_table, :25-48);
//   * axis-aligned boxes — iou3d_calculator.py:290-319 (mode='giou', is_aligned=True, eps = 1e-6); the aligned DIoU has no
//     reference function: it is cal_diou_3d(enclosing_type='aligned') at yaw 0 up to the IoU's eps.
// This file lives in csrc_post/ because its kernel is not part of the profiled training step: build.source_hash() — the hash every
// profile under profiles/ is pinned to — does not cover it.  What it has in common with csrc/loss.hip is shared, not copied: the
// forward-mode D7 numbers (csrc/dual7.h), and sort_key, tie_max / tie_min and the per-axis steps of the aligned IoU (csrc/box_math.h).
// The rotated intersection follows k_riou3d's arithmetic graph on those operations (contraction off), so the values of iou3d / u3d
// agree with k_riou3d's to the bit.
//
// What differs from k_riou3d's layout: the 24 polygon vertices are kept as plain floats (192 bytes per thread) and the derivative is
// carried only through the <= 8 vertices of the clipped polygon, each rebuilt from the box parameters when the shoelace sum needs it;
// k_riou3d's `V2 vert[24]` of D7 is 1 536 bytes of scratch per thread.  The 24 enclosing-rectangle candidates are evaluated on plain
// floats and the derivative goes through the winner only.
//
// One deliberate difference from the reference: the extent along a candidate line uses the line's unit direction,
// (x dx + y dy) / sqrt(dx^2 + dy^2 + 1e-14), where the reference uses the slope k = dy / (dx + 1e-8); in fp32 the slope form loses the
// gradient of near-vertical edges.
//
// Degenerate pairs (v_c == 0 for GIoU, c2 == 0 for DIoU: both boxes without extent) give what IEEE gives — NaN or inf, as the
// reference does — without a fault: nothing is indexed by a computed value.
//
// Lanes: in the head ~1 % of the rows carry weight.  A workgroup owns EIOU_ROWS consecutive rows; it lists its active rows in LDS
// (a ballot and a prefix per wave, in row order), writes the zeros of the inactive rows in a coalesced pass, and then walks the list
// with consecutive lanes, so that the geometry runs on full waves as far as the workgroup has active rows.
#include "../csrc/fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "../csrc/box_math.h"     // sort_key, tie_max / tie_min, axis_overlap, axis_iou_grad
#include "../csrc/dual7.h"        // D7 and its operators, V2
// exact products as in the reference's torch code and in k_riou3d (e.g. num == 0 for parallel edges): no FMA contraction
#pragma clang fp contract(off)

#define EIOU_THREADS 256
#ifndef EIOU_ROWS
#define EIOU_ROWS 1024                             // rows per workgroup, a multiple of EIOU_THREADS (chosen by measurement: DESIGN.md section 16)
#endif
namespace {
constexpr int EIOU_RPT = EIOU_ROWS / EIOU_THREADS;   // rows per thread in the listing pass
constexpr int EIOU_WAVES = EIOU_THREADS / 64;
static_assert(EIOU_ROWS % EIOU_THREADS == 0 && EIOU_THREADS % 64 == 0, "a workgroup lists whole waves of rows");

static inline unsigned eiou_blocks(int64_t n) { return (unsigned)((n + EIOU_ROWS - 1) / EIOU_ROWS); }

// the box whose derivative is carried: its parameters and the sine / cosine of its yaw (box2corners_th order: corner k has the
// signs sx = +,-,-,+ and sy = +,+,-,-)
struct Box1 {
  D7 cx, cy, w, h, cs, sn;
};
__device__ static inline float corner_sx(int k) { return (k == 0 || k == 3) ? 0.5f : -0.5f; }
__device__ static inline float corner_sy(int k) { return k < 2 ? 0.5f : -0.5f; }
__device__ static inline V2 corner_d(const Box1& b, int k) {
  D7 x4 = dscale(b.w, corner_sx(k)), y4 = dscale(b.h, corner_sy(k));
  V2 r;
  r.x = x4 * b.cs - y4 * b.sn + b.cx;
  r.y = x4 * b.sn + y4 * b.cs + b.cy;
  return r;
}
// the same arithmetic on plain floats (what corner_d(...).v is)
__device__ static inline void corners_f(float cx, float cy, float w, float h, float alpha, float* x, float* y) {
  const float cs = cosf(alpha), sn = sinf(alpha);
  for (int k = 0; k < 4; ++k) {
    const float x4 = w * corner_sx(k), y4 = h * corner_sy(k);
    x[k] = x4 * cs - y4 * sn + cx;
    y[k] = x4 * sn + y4 * cs + cy;
  }
}

// corner (mx, my) lies inside the rectangle with corners q[0..3] (box_intersection_2d.py:57-82)
__device__ static inline bool corner_in_rect(float mx, float my, const float* qx, const float* qy) {
  float abx = qx[1] - qx[0], aby = qy[1] - qy[0];
  float adx = qx[3] - qx[0], ady = qy[3] - qy[0];
  float amx = mx - qx[0], amy = my - qy[0];
  float pab = (abx * amx + aby * amy) / (abx * abx + aby * aby);
  float pad = (adx * amx + ady * amy) / (adx * adx + ady * ady);
  return pab > -1e-6f && pab < 1.f + 1e-6f && pad > -1e-6f && pad < 1.f + 1e-6f;
}

// vertex k of the 24 (0..3 corners of box 1, 4..7 corners of box 2, 8 + 4a + b = edge a of box 1 with edge b of box 2) with its
// derivative; vx / vy hold the values of all 24
__device__ static V2 vertex_d(const Box1& b1, const float* vx, const float* vy, int k) {
  if (k < 4) return corner_d(b1, k);
  V2 r;
  if (k < 8) {
    r.x = dconst(vx[k]);
    r.y = dconst(vy[k]);
    return r;
  }
  const int a = (k - 8) >> 2, b = (k - 8) & 3;
  const V2 p1 = corner_d(b1, a), p2 = corner_d(b1, (a + 1) & 3);
  const D7 p3x = dconst(vx[4 + b]), p3y = dconst(vy[4 + b]);
  const D7 p4x = dconst(vx[4 + ((b + 1) & 3)]), p4y = dconst(vy[4 + ((b + 1) & 3)]);
  D7 num = (p1.x - p2.x) * (p3y - p4y) - (p1.y - p2.y) * (p3x - p4x);
  D7 den_t = (p1.x - p3x) * (p3y - p4y) - (p1.y - p3y) * (p3x - p4x);
  D7 ts = den_t / (num + dconst(1e-8f));
  r.x = p1.x + ts * (p2.x - p1.x);
  r.y = p1.y + ts * (p2.y - p1.y);
  return r;
}

// the 8 corners as D7 for the enclosing rectangle: 0..3 carry the derivative, 4..7 are constants
__device__ static inline V2 corner8_d(const Box1& b1, const float* vx, const float* vy, int k) {
  if (k < 4) return corner_d(b1, k);
  V2 r;
  r.x = dconst(vx[k]);
  r.y = dconst(vy[k]);
  return r;
}

// signed distance of (x, y) from the line (x1,y1)-(x2,y2) times the line's length, and the extent along the line times it
__device__ static inline float line_den(float x1, float y1, float x2, float y2, float x, float y) {
  return (y2 - y1) * x - (x2 - x1) * y + x2 * y1 - y2 * x1;
}

// p, t: [cx,cy,cz,w,l,h,yaw]; writes loss, iou and d loss / d p[0..6]
__device__ static void eiou7_row(const float* __restrict__ p, const float* __restrict__ t, int kind, float* loss_o, float* iou_o,
                                 float* dp) {
  D7 P[7];
  for (int e = 0; e < 7; ++e) P[e] = dvar(p[e], e);
  Box1 b1;
  b1.cx = P[0]; b1.cy = P[1]; b1.w = P[3]; b1.h = P[4];
  b1.cs.v = cosf(p[6]); b1.sn.v = sinf(p[6]);
  for (int i = 0; i < 7; ++i) { b1.cs.d[i] = -b1.sn.v * P[6].d[i]; b1.sn.d[i] = b1.cs.v * P[6].d[i]; }
  float vx[24], vy[24];
  bool valid[24];
  corners_f(p[0], p[1], p[3], p[4], p[6], vx, vy);
  corners_f(t[0], t[1], t[3], t[4], t[6], vx + 4, vy + 4);
  // 16 edge-edge intersections (box_intersection_2d.py:13-54), values only
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      const float p1x = vx[a], p1y = vy[a], p2x = vx[(a + 1) & 3], p2y = vy[(a + 1) & 3];
      const float p3x = vx[4 + b], p3y = vy[4 + b], p4x = vx[4 + ((b + 1) & 3)], p4y = vy[4 + ((b + 1) & 3)];
      float num = (p1x - p2x) * (p3y - p4y) - (p1y - p2y) * (p3x - p4x);
      float den_t = (p1x - p3x) * (p3y - p4y) - (p1y - p3y) * (p3x - p4x);
      float den_u = (p1x - p2x) * (p1y - p3y) - (p1y - p2y) * (p1x - p3x);
      float tt = num == 0.f ? -1.f : den_t / num;
      float uu = num == 0.f ? -1.f : -den_u / num;
      bool m = tt > 0.f && tt < 1.f && uu > 0.f && uu < 1.f;
      int k = 8 + a * 4 + b;
      valid[k] = m;
      if (m) {
        float ts = den_t / (num + 1e-8f);
        vx[k] = p1x + ts * (p2x - p1x);
        vy[k] = p1y + ts * (p2y - p1y);
      } else {
        vx[k] = 0.f;
        vy[k] = 0.f;
      }
    }
  for (int k = 0; k < 4; ++k) {
    valid[k] = corner_in_rect(vx[k], vy[k], vx + 4, vy + 4);
    valid[4 + k] = corner_in_rect(vx[4 + k], vy[4 + k], vx, vy);
  }
  // order the valid vertices by polar angle about their mean (sort_v)
  int nv = 0;
  float mx = 0.f, my = 0.f;
  for (int k = 0; k < 24; ++k)
    if (valid[k]) { mx += vx[k]; my += vy[k]; ++nv; }
  int order[24];
  int cnt = 0;
  if (nv >= 3) {
    mx /= nv; my /= nv;
    float ang[24];
    for (int k = 0; k < 24; ++k) {
      if (!valid[k]) continue;
      float g = sort_key(vy[k] - my, vx[k] - mx);
      int m = cnt - 1;
      while (m >= 0 && ang[m] > g) { ang[m + 1] = ang[m]; order[m + 1] = order[m]; --m; }   // stable insertion
      ang[m + 1] = g; order[m + 1] = k;
      ++cnt;
    }
    // drop coincident neighbours (identical boxes list every corner twice)
    int kept = 0;
    for (int k = 0; k < cnt; ++k) {
      if (kept > 0) {
        int q = order[kept - 1];
        if (fmaxf(fabsf(vx[order[k]] - vx[q]), fabsf(vy[order[k]] - vy[q])) <= 1e-6f) continue;
      }
      order[kept++] = order[k];
    }
    if (kept > 1) {
      int a0 = order[0], q = order[kept - 1];
      if (fmaxf(fabsf(vx[a0] - vx[q]), fabsf(vy[a0] - vy[q])) <= 1e-6f) --kept;
    }
    cnt = kept > 8 ? 8 : kept;
  }
  D7 total = dconst(0.f);
  if (cnt >= 3) {
    const V2 first = vertex_d(b1, vx, vy, order[0]);
    V2 a = first;
    for (int k = 0; k < cnt; ++k) {
      const V2 b = k + 1 < cnt ? vertex_d(b1, vx, vy, order[k + 1]) : first;
      total = total + (a.x * b.y - a.y * b.x);
      a = b;
    }
  }
  D7 inter = dscale(total, total.v > 0.f ? 0.5f : (total.v < 0.f ? -0.5f : 0.f));
  D7 area1 = P[3] * P[4];
  D7 u2d = area1 + dconst(t[3] * t[4]) - inter;
  D7 iou2d = inter / u2d;
  D7 zmax1 = P[2] + dscale(P[5], 0.5f), zmin1 = P[2] - dscale(P[5], 0.5f);
  D7 zmax2 = dconst(t[2] + t[5] * 0.5f), zmin2 = dconst(t[2] - t[5] * 0.5f);
  D7 zo = dclamp0(dmin_tie(zmax1, zmax2) - dmax_tie(zmin1, zmin2));
  D7 inter3d = iou2d * u2d * zo;
  D7 v1 = P[3] * P[4] * P[5];
  D7 u3d = v1 + dconst(t[3] * t[4] * t[5]) - inter3d;
  D7 iou3d = inter3d / u3d;
  D7 z_range = dclamp0(dmax_tie(zmax1, zmax2) - dmin_tie(zmin1, zmin2));

  // ---- smallest_bounding_box (min_enclosing_box.py:142-172): the 24 candidate lines on plain floats, first minimum wins -------------
  int bi = 0, bj = 1;
  float best = 0.f;
  bool have = false;
  for (int i = 0; i < 8; ++i)
    for (int j = i + 1; j < 8; ++j) {
      if (j == i + 2 && (i & 3) < 2) continue;                   // (0,2) (1,3) (4,6) (5,7): a box's diagonals
      const float x1 = vx[i], y1 = vy[i], x2 = vx[j], y2 = vy[j];
      const float len = sqrtf((y2 - y1) * (y2 - y1) + (x2 - x1) * (x2 - x1) + 1e-14f);
      float dmx = 0.f, dmn = 0.f, dab = 0.f, pmx = 0.f, pmn = 0.f;
      bool fd = true;
      for (int m = 0; m < 8; ++m) {
        const float pr = (vx[m] * (x2 - x1) + vy[m] * (y2 - y1)) / len;
        if (m == 0 || pr > pmx) pmx = pr;
        if (m == 0 || pr < pmn) pmn = pr;
        if (m == i || m == j) continue;
        const float d = line_den(x1, y1, x2, y2, vx[m], vy[m]) / len;
        if (fd || d > dmx) dmx = d;
        if (fd || d < dmn) dmn = d;
        if (fd || fabsf(d) > dab) dab = fabsf(d);
        fd = false;
      }
      const float d1 = dmx - dmn;
      const float dist = d1 > dab ? d1 : dab;
      float area = (pmx - pmn) * dist;
      if (area == 0.f) area += 1e8f;                             // the two points of the line coincide
      if (!have || area < best) { best = area; bi = i; bj = j; have = true; }
    }
  // the winner once more with the derivative: the extreme points are selected by value, the first one on a tie
  D7 w_enc, h_enc;
  {
    const V2 q1 = corner8_d(b1, vx, vy, bi), q2 = corner8_d(b1, vx, vy, bj);
    const D7 dx = q2.x - q1.x, dy = q2.y - q1.y;
    const D7 len = dsqrt(dy * dy + dx * dx + dconst(1e-14f));
    const D7 off = q2.x * q1.y - q2.y * q1.x;
    int imx = -1, imn = -1, iab = -1, jmx = 0, jmn = 0;
    float dmx = 0.f, dmn = 0.f, dab = 0.f, pmx = 0.f, pmn = 0.f;
    for (int m = 0; m < 8; ++m) {
      const float pr = (vx[m] * dx.v + vy[m] * dy.v) / len.v;
      if (m == 0 || pr > pmx) { pmx = pr; jmx = m; }
      if (m == 0 || pr < pmn) { pmn = pr; jmn = m; }
      if (m == bi || m == bj) continue;
      const float d = (dy.v * vx[m] - dx.v * vy[m] + off.v) / len.v;
      if (imx < 0 || d > dmx) { dmx = d; imx = m; }
      if (imn < 0 || d < dmn) { dmn = d; imn = m; }
      if (iab < 0 || fabsf(d) > dab) { dab = fabsf(d); iab = m; }
    }
    D7 dsel[3], psel[2];
    const int di[3] = {imx, imn, iab}, pi[2] = {jmx, jmn};
    for (int s = 0; s < 3; ++s) {
      const V2 q = corner8_d(b1, vx, vy, di[s]);
      dsel[s] = (dy * q.x - dx * q.y + off) / len;
    }
    for (int s = 0; s < 2; ++s) {
      const V2 q = corner8_d(b1, vx, vy, pi[s]);
      psel[s] = (q.x * dx + q.y * dy) / len;
    }
    h_enc = dmax_tie(dsel[0] - dsel[1], dabs(dsel[2]));
    w_enc = psel[0] - psel[1];
  }
  D7 loss;
  if (kind == FC_EIOU_GIOU) {
    D7 v_c = z_range * w_enc * h_enc;
    loss = dconst(1.f) - iou3d + (v_c - u3d) / v_c;
  } else {
    D7 xo = P[0] - dconst(t[0]), yo = P[1] - dconst(t[1]), zf = P[2] - dconst(t[2]);
    D7 d2 = xo * xo + yo * yo + zf * zf;
    D7 c2 = w_enc * w_enc + h_enc * h_enc + z_range * z_range;
    loss = dconst(1.f) - iou3d + d2 / c2;
  }
  *loss_o = loss.v;
  *iou_o = iou3d.v;
  for (int e = 0; e < 7; ++e) dp[e] = loss.d[e];
}

// ---- axis-aligned: the per-axis overlap and IoU gradient of aiou3d_eval (csrc/box_math.h, shared with csrc/loss.hip), with the
// enclosing box in the same per-axis loops -------------------------------------------------------------------------------------------
// p, t: [cx,cy,cz,w,l,h]; writes loss, iou and d loss / d p[0..5]
__device__ static void eiou6_row(const float* __restrict__ p, const float* __restrict__ t, int kind, float* loss_o, float* iou_o,
                                 float* dp) {
  const float eps = 1e-6f;
  float wh[3], dwh_dc[3], dwh_ds[3], sp[3], ew[3], dew_dc[3], dew_ds[3];
  float a1 = 1.f, a2 = 1.f, ov = 1.f, enc = 1.f, d2 = 0.f, c2 = 0.f;
  for (int a = 0; a < 3; ++a) {
    const AxisOverlap o = axis_overlap(p[a], p[3 + a], t[a], t[3 + a]);
    wh[a] = o.wh; dwh_dc[a] = o.dwh_dc; dwh_ds[a] = o.dwh_ds;
    sp[a] = o.p2 - o.p1;
    a1 *= sp[a];
    a2 *= (o.t2 - o.t1);
    ov *= wh[a];
    // the enclosing box: lt = min, rb = max (iou3d_calculator.py:290-319)
    float elt, erb, el, er;
    tie_min(o.p1, o.t1, &elt, &el);
    tie_max(o.p2, o.t2, &erb, &er);
    float e = erb - elt;
    float epass = e >= 0.f ? 1.f : 0.f;
    ew[a] = e > 0.f ? e : 0.f;
    dew_dc[a] = epass * (er - el);
    dew_ds[a] = epass * 0.5f * (er + el);
    enc *= ew[a];
    c2 += ew[a] * ew[a];
    d2 += (p[a] - t[a]) * (p[a] - t[a]);
  }
  float un = a1 + a2 - ov;
  float upass = un > eps ? 1.f : 0.f;     // torch.max(union, eps)
  float U = un > eps ? un : eps;
  const float iou = ov / U;
  const bool giou = kind == FC_EIOU_GIOU;
  const float raw = giou ? enc : c2;
  const float Epass = raw > eps ? 1.f : 0.f;
  const float E = raw > eps ? raw : eps;
  for (int a = 0; a < 3; ++a) {
    int b = (a + 1) % 3, c = (a + 2) % 3;
    const AxisIouGrad g = axis_iou_grad(wh[b], wh[c], dwh_dc[a], dwh_ds[a], sp[b], sp[c], ov, U, upass);
    if (giou) {                            // loss = 1 - iou + (E - U) / E
      float dE_dc = Epass * ew[b] * ew[c] * dew_dc[a], dE_ds = Epass * ew[b] * ew[c] * dew_ds[a];
      dp[a] = -g.diou_dc + (U * dE_dc - g.dU_dc * E) / (E * E);
      dp[3 + a] = -g.diou_ds + (U * dE_ds - g.dU_ds * E) / (E * E);
    } else {                               // loss = 1 - iou + d2 / E, E = max(c2, eps)
      float dE_dc = Epass * 2.f * ew[a] * dew_dc[a], dE_ds = Epass * 2.f * ew[a] * dew_ds[a];
      dp[a] = -g.diou_dc + (2.f * (p[a] - t[a]) * E - d2 * dE_dc) / (E * E);
      dp[3 + a] = -g.diou_ds + (-d2 * dE_ds) / (E * E);
    }
  }
  *iou_o = iou;
  *loss_o = giou ? 1.f - (iou - (E - U) / E) : 1.f - iou + d2 / E;
}

// pred (n, BD); target rows of `tstride` floats whose first BD are the box; weight (n) or NULL
template <int BD>
__global__ __launch_bounds__(EIOU_THREADS) void k_eiou3d(const float* __restrict__ pred, const float* __restrict__ target, int tstride,
                                                         const float* __restrict__ weight, int64_t n, int kind,
                                                         float* __restrict__ loss, float* __restrict__ iou, float* __restrict__ dpred) {
  __shared__ int s_list[EIOU_ROWS];                                    // local indices of the active rows, ascending
  __shared__ unsigned long long s_mask[EIOU_RPT * EIOU_WAVES];         // activity of local rows 64 w .. 64 w + 63
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * EIOU_ROWS;
  bool act[EIOU_RPT];
  for (int r = 0; r < EIOU_RPT; ++r) {
    const int64_t row = base + r * EIOU_THREADS + tid;
    act[r] = row < n && (!weight || weight[row] > 0.f);
    const unsigned long long m = __ballot(act[r]);
    if (lane == 0) s_mask[r * EIOU_WAVES + wave] = m;
  }
  __syncthreads();
  int total = 0;
  for (int r = 0; r < EIOU_RPT; ++r) {
    int off = 0;
    for (int w = 0; w < EIOU_RPT * EIOU_WAVES; ++w) {
      const int c = __popcll(s_mask[w]);
      if (w < r * EIOU_WAVES + wave) off += c;
      if (r == 0) total += c;
    }
    if (act[r]) {
      const unsigned long long below = s_mask[r * EIOU_WAVES + wave] & ((1ull << lane) - 1ull);
      s_list[off + __popcll(below)] = r * EIOU_THREADS + tid;
    }
  }
  // the zeros of the inactive rows, coalesced (an active row's words are written below, by one thread each)
  for (int r = 0; r < EIOU_RPT; ++r) {
    const int64_t row = base + r * EIOU_THREADS + tid;
    if (row < n && !act[r]) { loss[row] = 0.f; iou[row] = 0.f; }
  }
  for (int e = tid; e < EIOU_ROWS * BD; e += EIOU_THREADS) {
    const int lr = e / BD;
    if (base + lr < n && !((s_mask[lr >> 6] >> (lr & 63)) & 1ull)) dpred[base * BD + e] = 0.f;
  }
  __syncthreads();
  for (int k = tid; k < total; k += EIOU_THREADS) {
    const int64_t row = base + s_list[k];
    float dp[BD], l, u;
    if constexpr (BD == 7) eiou7_row(pred + row * 7, target + row * tstride, kind, &l, &u, dp);
    else eiou6_row(pred + row * 6, target + row * tstride, kind, &l, &u, dp);
    loss[row] = l;
    iou[row] = u;
    for (int e = 0; e < BD; ++e) dpred[row * BD + e] = dp[e];
  }
}
}  // namespace

extern "C" int fc_eiou3d_fwd_bwd(const float* pred, const float* target, int target_stride, const float* weight, int64_t n,
                                 int box_dim, int kind, float* loss, float* iou, float* dpred, hipStream_t stream) {
  if (n < 0 || (box_dim != 6 && box_dim != 7) || target_stride < box_dim || (kind != FC_EIOU_GIOU && kind != FC_EIOU_DIOU))
    return FC_EINVAL;
  if (n == 0) return FC_OK;
  if (box_dim == 7)
    k_eiou3d<7><<<eiou_blocks(n), EIOU_THREADS, 0, stream>>>(pred, target, target_stride, weight, n, kind, loss, iou, dpred);
  else
    k_eiou3d<6><<<eiou_blocks(n), EIOU_THREADS, 0, stream>>>(pred, target, target_stride, weight, n, kind, loss, iou, dpred);
  FC_CHECK_LAUNCH();
  return FC_OK;
}
