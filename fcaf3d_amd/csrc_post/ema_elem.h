// mmcv EMAHook (mmcv/runner/hooks/ema.py, third party: not in the reference tree) for ONE element, after the optimizer has written
// the new parameter p_new:   e <- fl32( fl32(e * keep) + fl32(mu * p_new) )        keep = fl32(1 - mu), formed by the caller
// Three fp32 roundings, NO fused multiply-add: the rule every path is held to bit for bit (the kernel of optim_ema.hip, the host
// emulator tools/ema_host_emu.cpp, torch's three ops in runner.WeightEma and the numpy replays of the tests).  Values in, value
// out; the store stays with the kernel.  Contraction is switched off in the body so that it does not depend on the including file.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

__device__ static inline float ema_elem(float e, float p_new, float mu, float keep) {
#pragma clang fp contract(off)
  const float kept = e * keep;
  const float added = mu * p_new;
  return kept + added;
}
