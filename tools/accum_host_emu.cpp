// Host emulation of the kernels of fcaf3d_amd/csrc_post/optim_accum.hip, as tools/ema_host_emu.cpp emulates optim_ema.hip's: one
// std::thread per GPU thread of a workgroup, a std::barrier for __syncthreads, workgroups one after the other, the grids
// fc_grad_accum / fc_grad_accum_norm launch.  __shfl_xor is an exchange through a per-workgroup array between two barriers (every
// thread of the norm kernels reaches every shuffle).  tests/test_accum_cpu.py cuts the kernels' text (optim_accum.hip from its
// ACC_THREADS constant to the end of its anonymous namespace, so nothing of them is restated here; the cut holds no #include) into
// accum_kernels.inc and builds this file with clang++ -std=c++20 -ffp-contract=off -fsanitize=address,undefined: the loads, the
// masked second sweep of the norm pass and the bounds of the last, partially filled workgroup are checked without a GPU, on
// exact-size heap arrays.  A stand-alone program: it is run, never loaded.
//
//   accum_host_emu IN OUT   IN: int64[4] n first has_ema mode, float[4] scale mu keep max_norm
//                           mode 0 (k_grad_accum):  acc, g (n floats each), then ema, p if has_ema     OUT: acc, g, then ema if has_ema
//                           mode 1 (k_accum_sqsum_partial + k_accum_sqsum_final): g, acc               OUT: g, acc, out2 (2 floats)
//                           mode 2 (k_grad_accum_sum): g, acc                                          OUT: g, acc
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
struct D3 { unsigned x, y, z; };
static thread_local D3 threadIdx;
static D3 blockIdx, gridDim;
static std::barrier<>* g_bar;
static void __syncthreads() { g_bar->arrive_and_wait(); }
static double g_lanes[1024];
static double __shfl_xor(double v, int off, int width) {
  g_lanes[threadIdx.x] = v;
  g_bar->arrive_and_wait();
  const unsigned lane = threadIdx.x % (unsigned)width;
  const double got = g_lanes[threadIdx.x - lane + (lane ^ (unsigned)off)];
  g_bar->arrive_and_wait();
  return got;
}
static double fc_ld(const double* p) { return *p; }
#pragma clang fp contract(off)
#include "../fcaf3d_amd/csrc_post/accum_elem.h"       // optim_accum.hip includes the three above the cut
#include "../fcaf3d_amd/csrc_post/ema_elem.h"
#include "../fcaf3d_amd/csrc_post/sqsum_order.h"
#include "accum_kernels.inc"

template <class F> static void launch(unsigned gx, unsigned threads, F f) {
  gridDim = {gx, 1, 1};
  for (unsigned bx = 0; bx < gx; ++bx) {
    blockIdx = {bx, 0, 0};
    std::barrier<> bar(threads);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; ++t) th.emplace_back([&, t] { threadIdx = {t, 0, 0}; f(); });
    for (auto& x : th) x.join();
  }
}
// exact-size heap arrays (ASan sees every access past them), 16-byte aligned for the kernels' vector accesses
template <class T> static T* rd(FILE* f, size_t n) {
  void* v = nullptr;
  if (posix_memalign(&v, 16, std::max<size_t>(n * sizeof(T), 1))) abort();
  if (n && fread(v, sizeof(T), n, f) != n) abort();
  return static_cast<T*>(v);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t* h = rd<int64_t>(f, 4);
  const int64_t n = h[0], first = h[1], has_ema = h[2], mode = h[3];
  if (n < 0 || n % 4 || mode < 0 || mode > 2) return 3;
  float* s = rd<float>(f, 4);
  const int64_t n4 = n / 4;
  const unsigned grid = (unsigned)((n4 + ACC_THREADS - 1) / ACC_THREADS);
  FILE* o = nullptr;
  if (mode == 0) {
    float* acc = rd<float>(f, n);
    float* g = rd<float>(f, n);
    float* e = has_ema ? rd<float>(f, n) : nullptr;
    float* p = has_ema ? rd<float>(f, n) : nullptr;
    fclose(f);
    if (n4)      // (fc_grad_accum launches nothing for n == 0)
      launch(grid, ACC_THREADS, [&] {
        if (has_ema && first) k_grad_accum<true, true>((oa4*)acc, (const oa4*)g, n4, s[0], (oa4*)e, (const oa4*)p, s[1], s[2]);
        else if (has_ema) k_grad_accum<false, true>((oa4*)acc, (const oa4*)g, n4, s[0], (oa4*)e, (const oa4*)p, s[1], s[2]);
        else if (first) k_grad_accum<true, false>((oa4*)acc, (const oa4*)g, n4, s[0], nullptr, nullptr, 0.f, 0.f);
        else k_grad_accum<false, false>((oa4*)acc, (const oa4*)g, n4, s[0], nullptr, nullptr, 0.f, 0.f);
      });
    if (!(o = fopen(argv[2], "wb"))) return 2;
    fwrite(acc, 4, n, o); fwrite(g, 4, n, o);
    if (has_ema) fwrite(e, 4, n, o);
    free(acc); free(g); free(e); free(p);
  } else {
    float* g = rd<float>(f, n);
    float* acc = rd<float>(f, n);
    fclose(f);
    float out2[2] = {-1.f, -1.f};
    if (n4 && mode == 1) {
      const int nb = sqo_blocks(n4);
      double* part = static_cast<double*>(malloc(sizeof(double) * (size_t)nb));      // exactly the words the launch may touch
      launch((unsigned)nb, SQO_THREADS, [&] { k_accum_sqsum_partial((oa4*)g, (const oa4*)acc, n4, s[0], part); });
      launch(1, SQO_FINAL_THREADS, [&] { k_accum_sqsum_final(part, nb, s[3], out2); });
      free(part);
    } else if (n4) {
      launch(grid, ACC_THREADS, [&] { k_grad_accum_sum((oa4*)g, (const oa4*)acc, n4, s[0]); });
    }
    if (!(o = fopen(argv[2], "wb"))) return 2;
    fwrite(g, 4, n, o); fwrite(acc, 4, n, o);
    if (mode == 1) fwrite(out2, 4, 2, o);
    free(g); free(acc);
  }
  fclose(o);
  free(h); free(s);
  return 0;
}
