// Host emulation of the kernel of fcaf3d_amd/csrc_post/optim_groups.hip: one std::thread per GPU thread of a workgroup, a
// std::barrier for __syncthreads, workgroups one after the other, the grid fc_adamw_step_groups launches.  tests/test_finetune_cpu.py
// cuts the kernel's text (optim_groups.hip from its ADAMW_* constants to the end of its anonymous namespace: the constants, the run
// search and the kernel, so nothing of them is restated here; the cut holds no #include) into kernels.inc and builds this file with
// clang++ -std=c++20 -ffp-contract=off -fsanitize=address,undefined: the staging of the run table, the search and the bounds of
// the last, partially filled workgroup are checked without a GPU, on exact-size heap arrays.
//
//   optim_host_emu IN OUT     IN: int64[4] n R has_clip 0, float[10] lr beta1 beta2 eps weight_decay bc1 bc2 norm clip 0, the packed
//                             run table of fc_adamw_groups_pack (3 R words), then p, g, m, v (n floats each)
//                             OUT: p, m, v
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
#include "../fcaf3d_amd/csrc/adamw_elem.h"  // optim_groups.hip includes it above the cut
#include "kernels.inc"

template <class F> static void launch(unsigned gx, F f) {
  gridDim = {gx, 1, 1};
  for (unsigned bx = 0; bx < gx; ++bx) {
    blockIdx = {bx, 0, 0};
    std::barrier<> bar(ADAMW_THREADS);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < ADAMW_THREADS; ++t) th.emplace_back([&, t] { threadIdx = {t, 0, 0}; f(); });
    for (auto& x : th) x.join();
  }
}
// exact-size heap arrays (ASan sees every access past them), 16-byte aligned for the kernel's vector accesses
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
  const int64_t n = h[0], R = h[1], has_clip = h[2];
  if (n < 0 || n % 4 || R < 1 || R > ADAMW_MAX_RUNS) return 3;
  float* s = rd<float>(f, 10);
  unsigned* table = rd<unsigned>(f, 3 * R);
  float* p = rd<float>(f, n);
  float* g = rd<float>(f, n);
  float* m = rd<float>(f, n);
  float* v = rd<float>(f, n);
  fclose(f);
  const int64_t n4 = n / 4;
  if (n4)      // (fc_adamw_step_groups launches nothing for n == 0)
    launch((unsigned)((n4 + ADAMW_THREADS - 1) / ADAMW_THREADS), [&] {
      k_adamw_groups((og4*)p, (const og4*)g, (og4*)m, (og4*)v, n4, s[0], s[1], s[2], s[3], s[4], s[5], sqrtf(s[6]),
                     has_clip ? s + 7 : nullptr, table, (int)R);
    });
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(p, 4, n, o); fwrite(m, 4, n, o); fwrite(v, 4, n, o);
  fclose(o);
  free(h); free(s); free(table); free(p); free(g); free(m); free(v);
  return 0;
}
