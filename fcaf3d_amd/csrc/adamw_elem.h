// torch.optim.AdamW (decoupled weight decay, no amsgrad) for ONE element, the arithmetic of torch's own kernels:
//   p *= decay (= 1 - lr * wd) ; m += (g - m) * (1 - b1) ; v = b2 * v + (1 - b2) * g * g ;
//   p -= step_size (= lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)          with g scaled by the clip coefficient c first
// Shared by k_adamw (csrc/optim.hip) and k_adamw_groups (csrc_post/optim_groups.hip), which differ only in where decay and step_size
// come from.  Values in, values out; the stores stay with the kernels.  Contraction is the compiler's default for device code (fast),
// as it was in both kernels: stated in the body so that it does not depend on the including file.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

struct AdamwElem { float p, m, v; };

__device__ static inline AdamwElem adamw_elem(float p, float g, float m, float v, float c, float decay, float step_size, float b1,
                                              float b2, float eps, float bc2_sqrt) {
#pragma clang fp contract(fast)
  const float gg = g * c;
  float pp = p * decay;
  const float mm = m + (gg - m) * (1.f - b1);
  const float v2 = v * b2 + (1.f - b2) * gg * gg;
  const float denom = sqrtf(v2) / bc2_sqrt + eps;
  pp -= step_size * (mm / denom);
  return AdamwElem{pp, mm, v2};
}
