// Host emulation of the kernels of fcaf3d_amd/csrc_post/eval.hip: one std::thread per GPU thread of a workgroup, a std::barrier for
// __syncthreads, workgroups one after the other, the grids fc_eval_match launches.  tests/test_eval_cpu.py cuts the kernels' text
// (eval.hip from its EVAL_* constants to the end of its anonymous namespace: the constants, the grid helpers and the kernels, so
// nothing of the configuration is restated here) into kernels.inc behind fc_common.h's own FC_EMPTY_KEY line, puts an empty
// hip/hip_runtime.h beside it, builds this file with
// clang++ -std=c++20 -fsanitize=address,undefined and compares the outputs with evaluation.match_table_host: the index arithmetic,
// the LDS staging and every bound of the kernels are checked without a GPU (not their floating-point results to the bit: the
// host's sinf / cosf / atan2f are not the device's).
//
//   eval_host_emu IN OUT      IN: int64[6] n_det det_dim n_gt n_scenes n_thr flags, then det_boxes f32, det_scores f32, det_labels
//                             i64, gt_boxes f32 (n_gt,7), gt_labels i32, seg i64 (n_scenes,4), thr f64
//                             OUT: best_iou f32, best_gt i32, tp_bits u8
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
#include "fcaf3d_hip.h"  // FC_EVAL_DET_BOTTOM
struct D3 { unsigned x, y, z; };
static thread_local D3 threadIdx;
static D3 blockIdx, gridDim;
static std::barrier<>* g_bar;
static void __syncthreads() { g_bar->arrive_and_wait(); }
static unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
using std::min;
static void atomicMin(unsigned long long* p, unsigned long long v) {
  unsigned long long o = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
#pragma clang fp contract(off)
#include "../fcaf3d_amd/csrc/bev_geom.h"
#include "kernels.inc"

template <class F> static void launch(unsigned gx, unsigned gy, F f) {
  gridDim = {gx, gy, 1};
  for (unsigned by = 0; by < gy; ++by)
    for (unsigned bx = 0; bx < gx; ++bx) {
      blockIdx = {bx, by, 0};
      std::barrier<> bar(EVAL_THREADS);
      g_bar = &bar;
      std::vector<std::thread> th;
      for (unsigned t = 0; t < EVAL_THREADS; ++t) th.emplace_back([&, t] { threadIdx = {t, 0, 0}; f(); });
      for (auto& x : th) x.join();
    }
}
template <class T> static std::vector<T> rd(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) abort(); return v; }

int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  auto h = rd<int64_t>(f, 6);
  const int64_t n_det = h[0], det_dim = h[1], n_gt = h[2], n_scenes = h[3], n_thr = h[4], flags = h[5];
  auto boxes = rd<float>(f, n_det * det_dim); auto scores = rd<float>(f, n_det); auto labels = rd<int64_t>(f, n_det);
  auto gb = rd<float>(f, n_gt * 7); auto gl = rd<int>(f, n_gt); auto seg = rd<int64_t>(f, n_scenes * 4); auto thr = rd<double>(f, n_thr);
  std::vector<float> best_iou(n_det); std::vector<int> best_gt(n_det); std::vector<unsigned char> bits(n_det);
  std::vector<unsigned long long> keys(n_gt * n_thr);
  const int64_t n_keys = n_gt * n_thr;
  launch(eval_init_blocks(n_det, n_keys), 1, [&] { k_eval_init(n_det, n_keys, best_iou.data(), best_gt.data(), bits.data(), keys.data()); });
  const unsigned gy = eval_tiles_y(n_det, n_scenes);
  launch((unsigned)n_scenes, gy, [&] { k_eval_best(boxes.data(), (int)det_dim, scores.data(), labels.data(), gb.data(), gl.data(), seg.data(), n_det, n_gt, thr.data(), (int)n_thr, (int)flags, best_iou.data(), best_gt.data(), keys.data()); });
  launch((unsigned)n_scenes, gy, [&] { k_eval_bits(scores.data(), seg.data(), n_det, n_gt, thr.data(), (int)n_thr, best_iou.data(), best_gt.data(), keys.data(), bits.data()); });
  FILE* o = fopen(argv[2], "wb");
  fwrite(best_iou.data(), 4, n_det, o); fwrite(best_gt.data(), 4, n_det, o); fwrite(bits.data(), 1, n_det, o);
  fclose(o);
  return 0;
}
