// mmcv GradientCumulativeOptimizerHook (mmcv/runner/hooks/optimizer.py, third party: not in the reference tree) for ONE element of
// the flat gradient buffers, with the factor applied AFTER the backward pass (s = fl32(1 / f), formed by the caller):
//   first micro-iteration of a group   acc <- fl32(g * s)
//   every later one                    acc <- fl32( acc + fl32(g * s) )
// Two fp32 roundings, NO fused multiply-add: the rule every path is held to bit for bit (the kernels of optim_accum.hip, the host
// emulator tools/accum_host_emu.cpp, torch.mul then torch.add in the tests' twins and the numpy replays).  For f a power of two
// g * s is exact and the sum is mmcv's, which scales the loss instead; for other f it differs by the rounding of this one product.
// Values in, value out; the stores stay with the kernels.  Contraction is switched off in the bodies so that it does not depend on
// the including file.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

__device__ static inline float accum_first_elem(float g, float s) {
#pragma clang fp contract(off)
  return g * s;
}

__device__ static inline float accum_elem(float acc, float g, float s) {
#pragma clang fp contract(off)
  const float scaled = g * s;
  return acc + scaled;
}
