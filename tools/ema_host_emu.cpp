// Host emulation of the kernels of fcaf3d_amd/csrc_post/optim_ema.hip, as tools/optim_host_emu.cpp emulates optim_groups.hip's: one
// std::thread per GPU thread of a workgroup, a std::barrier for __syncthreads, workgroups one after the other, the grids
// fc_adamw_ema_step / fc_swap_f32 launch.  tests/test_ema_cpu.py cuts the kernels' text (optim_ema.hip from its EMA_* constants to the
// end of its anonymous namespace: the constants, the run search and both kernels, so nothing of them is restated here; the cut
// holds no #include) into ema_kernels.inc and builds this file with clang++ -std=c++20 -ffp-contract=off
// -fsanitize=address,undefined: the five loads, the staging of the run table, the search and the bounds of the last, partially
// filled workgroup are checked without a GPU, on exact-size heap arrays.  A stand-alone program: it is run, never loaded.
//
//   ema_host_emu IN OUT     IN: int64[4] n R has_clip mode, float[12] lr beta1 beta2 eps weight_decay bc1 bc2 norm clip mu keep 0
//                           mode 0 (k_adamw_ema): the packed run table of fc_adamw_groups_pack (3 R words; R == 0: none), then
//                                   p, g, m, v, ema (n floats each)                        OUT: p, m, v, ema
//                           mode 1 (k_swap_f32):  a, b (n floats each)                     OUT: a, b
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
static float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static float fc_ld(const float* p) { return *p; }
#pragma clang fp contract(off)
#include "../fcaf3d_amd/csrc/adamw_elem.h"       // optim_ema.hip includes both above the cut
#include "../fcaf3d_amd/csrc_post/ema_elem.h"
#include "ema_kernels.inc"

template <class F> static void launch(unsigned gx, F f) {
  gridDim = {gx, 1, 1};
  for (unsigned bx = 0; bx < gx; ++bx) {
    blockIdx = {bx, 0, 0};
    std::barrier<> bar(EMA_THREADS);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < EMA_THREADS; ++t) th.emplace_back([&, t] { threadIdx = {t, 0, 0}; f(); });
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
  const int64_t n = h[0], R = h[1], has_clip = h[2], mode = h[3];
  if (n < 0 || n % 4 || R < 0 || R > EMA_MAX_RUNS || (mode != 0 && mode != 1)) return 3;
  float* s = rd<float>(f, 12);
  const int64_t n4 = n / 4;
  const unsigned grid = (unsigned)((n4 + EMA_THREADS - 1) / EMA_THREADS);
  FILE* o = nullptr;
  if (mode == 1) {
    float* a = rd<float>(f, n);
    float* b = rd<float>(f, n);
    fclose(f);
    if (n4) launch(grid, [&] { k_swap_f32((oe4*)a, (oe4*)b, n4); });      // (fc_swap_f32 launches nothing for n == 0)
    if (!(o = fopen(argv[2], "wb"))) return 2;
    fwrite(a, 4, n, o); fwrite(b, 4, n, o);
    free(a); free(b);
  } else {
    unsigned* table = R ? rd<unsigned>(f, 3 * R) : nullptr;      // R == 0: fc_adamw_ema_step passes a null table
    float* p = rd<float>(f, n);
    float* g = rd<float>(f, n);
    float* m = rd<float>(f, n);
    float* v = rd<float>(f, n);
    float* e = rd<float>(f, n);
    fclose(f);
    if (n4)
      launch(grid, [&] {
        k_adamw_ema((oe4*)p, (const oe4*)g, (oe4*)m, (oe4*)v, (oe4*)e, n4, s[0], s[1], s[2], s[3], s[4], s[5], s[0] / s[5], sqrtf(s[6]),
                    has_clip ? s + 7 : nullptr, table, (int)R, s[9], s[10]);
      });
    if (!(o = fopen(argv[2], "wb"))) return 2;
    fwrite(p, 4, n, o); fwrite(m, 4, n, o); fwrite(v, 4, n, o); fwrite(e, 4, n, o);
    free(table); free(p); free(g); free(m); free(v); free(e);
  }
  fclose(o);
  free(h); free(s);
  return 0;
}
