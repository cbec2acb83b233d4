// Host emulation of the kernel of fcaf3d_amd/csrc_post/vote.hip: one std::thread per GPU thread of a workgroup, a std::barrier for
// __syncthreads, a barrier per 64 threads for the wave's __ballot, workgroups one after the other, the grid fc_vote_boxes launches.
// tests/test_vote_cpu.py cuts the kernel's text (vote.hip from its VOTE_* constants to the end of its anonymous namespace: the
// constants, the grid helper and the kernel, so nothing of the configuration is restated here) into kernels.inc, puts an empty
// hip/hip_runtime.h beside it, builds this file with clang++ -std=c++20 -fsanitize=address,undefined and compares the outputs with
// merge_augs.vote_boxes: the index arithmetic, the LDS staging, the order of the sums and every bound of the kernel are checked
// without a GPU.  The tables are allocated at their exact sizes, so an access outside them is an AddressSanitizer report.
//
//   vote_host_emu IN OUT      IN: int64[8] nseg stride max_count keep_stride max_keep flags members thr_bits, then boxes f32
//                             (nseg,stride,7), scores f32 (nseg,stride), counts i32, keep i32 (nseg,keep_stride), keep_counts i32,
//                             out_init f32 (nseg,stride,7): what the output holds before the launch
//                             OUT: out f32 (nseg,stride,7), members i32 (nseg,keep_stride)
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
#include "fcaf3d_hip.h"  // FC_VOTE_ROTATED, FC_VOTE_WITH_YAW
struct D3 { unsigned x, y, z; };
static thread_local D3 threadIdx;
static D3 blockIdx, gridDim;
static std::barrier<>* g_bar;
static void __syncthreads() { g_bar->arrive_and_wait(); }
static unsigned long long __ballot(int pred);
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
using std::max;
using std::min;
#pragma clang fp contract(off)
#include "../fcaf3d_amd/csrc/bev_geom.h"
#include "kernels.inc"

static std::barrier<>* g_wave_bar[VOTE_WAVES];
static unsigned char g_pred[VOTE_THREADS];
// every lane of the wave arrives (the kernel calls it in wave-uniform flow only: a lane that did not would hang the emulator)
static unsigned long long __ballot(int pred) {
  const unsigned t = threadIdx.x, w = t / VOTE_WAVE;
  g_pred[t] = pred ? 1 : 0;
  g_wave_bar[w]->arrive_and_wait();
  unsigned long long m = 0;
  for (unsigned l = 0; l < VOTE_WAVE; ++l)
    if (g_pred[w * VOTE_WAVE + l]) m |= 1ull << l;
  g_wave_bar[w]->arrive_and_wait();
  return m;
}

template <class F> static void launch(unsigned gx, unsigned gy, F f) {
  gridDim = {gx, gy, 1};
  for (unsigned by = 0; by < gy; ++by)
    for (unsigned bx = 0; bx < gx; ++bx) {
      blockIdx = {bx, by, 0};
      std::barrier<> bar(VOTE_THREADS);
      g_bar = &bar;
      std::vector<std::unique_ptr<std::barrier<>>> wb;
      for (int w = 0; w < VOTE_WAVES; ++w) {
        wb.emplace_back(new std::barrier<>(VOTE_WAVE));
        g_wave_bar[w] = wb.back().get();
      }
      std::vector<std::thread> th;
      for (unsigned t = 0; t < VOTE_THREADS; ++t) th.emplace_back([&, t] { threadIdx = {t, 0, 0}; f(); });
      for (auto& x : th) x.join();
    }
}
// exact-size heap arrays (a std::vector's spare capacity would hide an overrun of a few elements)
template <class T> static std::unique_ptr<T[]> rd(FILE* f, size_t n) {
  std::unique_ptr<T[]> v(new T[n]);
  if (n && fread(v.get(), sizeof(T), n, f) != n) abort();
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  auto h = rd<int64_t>(f, 8);
  const int64_t nseg = h[0], stride = h[1], max_count = h[2], keep_stride = h[3], max_keep = h[4], flags = h[5], want_members = h[6];
  float thr;
  const uint32_t tb = (uint32_t)h[7];
  memcpy(&thr, &tb, 4);
  auto boxes = rd<float>(f, nseg * stride * 7);
  auto scores = rd<float>(f, nseg * stride);
  auto counts = rd<int>(f, nseg);
  auto keep = rd<int>(f, nseg * keep_stride);
  auto kcounts = rd<int>(f, nseg);
  auto out = rd<float>(f, nseg * stride * 7);
  fclose(f);
  std::unique_ptr<int[]> members(new int[nseg * keep_stride]);
  for (int64_t i = 0; i < nseg * keep_stride; ++i) members[i] = -1;
  if (nseg > 0 && max_count > 0)
    launch(vote_blocks_x((int)max_keep), (unsigned)nseg, [&] {
      k_vote_boxes(boxes.get(), scores.get(), counts.get(), (int)stride, (int)max_count, keep.get(), kcounts.get(), (int)keep_stride,
                   (int)max_keep, thr, (int)flags, out.get(), want_members ? members.get() : nullptr);
    });
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(out.get(), 4, nseg * stride * 7, o);
  fwrite(members.get(), 4, nseg * keep_stride, o);
  fclose(o);
  return 0;
}
