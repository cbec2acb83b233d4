// The ORDER of the global gradient norm of csrc/optim.hip (k_sqsum_partial / k_sqsum_final), for a kernel that forms the gradient
// in the pass that sums its squares (csrc_post/optim_accum.hip): the blocks fc_grad_norm launches, the squares of one 16-byte
// vector in one float, a thread's doubles in sweep order, the butterfly over the wave, the four waves as (0 + 1) + (2 + 3), and
// the final reduce with its clip coefficient.  A kernel that walks float4 j = i + u * stride (i = block * 256 + thread, then
// + 4 * stride; u = 0 .. 3; stride = blocks * 256) and feeds sqo_vec / sqo_block_store / sqo_final gets fc_grad_norm's two floats
// bit for bit (tests/test_gpu_accum.py holds it to that on the device, tests/test_accum_cpu.py to the order in numpy).
//
// csrc/optim.hip does not include this header and keeps its own text: csrc/ is under source_hash(), which the committed profiles
// are pinned to, and its kernels are not to be recompiled for a feature outside the profiled step.
// sqo_vec: optim.hip's expression.  Its compile packs the four squares into two v_pk_mul_f32 and adds them up unfused
// ((x0^2 + x1^2) + x2^2) + x3^2 — four products, three sums, seven roundings; contraction is switched off here so that this text
// gives the same seven on the device, in the host emulator and in numpy.
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#define SQO_BLOCKS 1024             // csrc/optim.hip SQ_BLOCKS: the cap of the partial pass's grid, and the doubles of its workspace
#define SQO_THREADS 256
#define SQO_FINAL_THREADS 1024

typedef float sqo4 __attribute__((ext_vector_type(4)));

// the grid of the partial pass over n4 16-byte vectors
static inline int sqo_blocks(int64_t n4) {
  const int64_t nb = ((n4 > 0 ? n4 : 1) + SQO_THREADS * 4 - 1) / (SQO_THREADS * 4);
  return nb > SQO_BLOCKS ? SQO_BLOCKS : (int)nb;
}

__device__ static inline float sqo_vec(sqo4 v) {
#pragma clang fp contract(off)
  return v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
}

// every thread of the 256-thread block calls this with its sum; red: 4 doubles of LDS
__device__ static inline void sqo_block_store(double acc, double* red, double* __restrict__ part) {
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one block of 1024 threads; red: 16 doubles of LDS.  out[0] = the norm, out[1] = min(1, max_norm / (norm + 1e-6))  (max_norm <= 0: 1)
__device__ static inline void sqo_final(const double* __restrict__ part, int nb, float max_norm, float* __restrict__ out, double* red) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += SQO_FINAL_THREADS) acc += fc_ld(&part[i]);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w];
    const float norm = (float)sqrt(t);
    out[0] = norm;
    float c = 1.f;
    if (max_norm > 0.f) c = fminf(max_norm / (norm + 1e-6f), 1.f);
    out[1] = c;
  }
}
