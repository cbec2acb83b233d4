// Forward-mode derivative w.r.t. the 7 parameters of a predicted box: a value and its 7 partials, carried through +, -, *, / and the
// tie-splitting min / max of torch.  Shared by k_riou3d (csrc/loss.hip) and the enclosing-box losses (csrc_post/eiou.hip), whose
// iou3d / u3d agree with k_riou3d's to the bit because both run these operations.
//
// Exact products and sums, as torch's elementwise kernels compute them: every function that does arithmetic switches FMA contraction
// off in its own body, whatever the including file has set.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

struct D7 {
  float v;
  float d[7];
};
__device__ static inline D7 dconst(float c) { D7 r; r.v = c; for (int i = 0; i < 7; ++i) r.d[i] = 0.f; return r; }
__device__ static inline D7 dvar(float c, int i) { D7 r = dconst(c); r.d[i] = 1.f; return r; }
__device__ static inline D7 operator+(const D7& a, const D7& b) {
#pragma clang fp contract(off)
  D7 r; r.v = a.v + b.v; for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] + b.d[i]; return r;
}
__device__ static inline D7 operator-(const D7& a, const D7& b) {
#pragma clang fp contract(off)
  D7 r; r.v = a.v - b.v; for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] - b.d[i]; return r;
}
__device__ static inline D7 operator*(const D7& a, const D7& b) {
#pragma clang fp contract(off)
  D7 r; r.v = a.v * b.v; for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r;
}
__device__ static inline D7 operator/(const D7& a, const D7& b) {
#pragma clang fp contract(off)
  D7 r; r.v = a.v / b.v; float inv = 1.f / b.v;
  for (int i = 0; i < 7; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
__device__ static inline D7 dscale(const D7& a, float s) {
#pragma clang fp contract(off)
  D7 r; r.v = a.v * s; for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * s; return r;
}
__device__ static inline D7 dmin_tie(const D7& a, const D7& b) {     // torch.min(a,b): ties split the gradient
  if (a.v < b.v) return a;
  if (b.v < a.v) return b;
  return dscale(a + b, 0.5f);
}
__device__ static inline D7 dmax_tie(const D7& a, const D7& b) {
  if (a.v > b.v) return a;
  if (b.v > a.v) return b;
  return dscale(a + b, 0.5f);
}

struct V2 { D7 x, y; };

// ---- csrc_post/eiou.hip only ----
__device__ static inline D7 dsqrt(const D7& a) {
#pragma clang fp contract(off)
  D7 r; r.v = sqrtf(a.v); float h = 0.5f / r.v; for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * h; return r;
}
__device__ static inline D7 dabs(const D7& a) { return dscale(a, a.v > 0.f ? 1.f : (a.v < 0.f ? -1.f : 0.f)); }      // torch.abs: sign(0) = 0
__device__ static inline D7 dclamp0(D7 a) {                          // clamp_min(0): the gradient passes at x >= 0
  if (!(a.v >= 0.f)) return dconst(0.f);
  if (a.v == 0.f) a.v = 0.f;
  return a;
}
