// Host emulation of the kernel of fcaf3d_amd/csrc_post/batch.hip: one std::thread per GPU thread of a workgroup, a std::barrier for
// __syncthreads, workgroups one after the other, the grid fc_batch_augment_voxelize launches.  tests/test_batch_cpu.py cuts the
// kernel's text (batch.hip from its BATCH_* constants to the end of its anonymous namespace: the constants, the grid helper, the
// sampler and the kernel, so nothing of them is restated here; the cut holds no #include) into kernels.inc and builds
// this file with clang++ -std=c++20 -ffp-contract=off -fsanitize=address,undefined: the ragged indexing, the prefix, the scene search
// and every bound of the kernel are checked without a GPU, and the rows it draws are the kernel's own integer arithmetic.
//
//   batch_host_emu IN OUT     IN: int64[8] arena_rows pt_stride B total_out out_rows n_idx (-1: no sample_idx) nfeat want_points, then
//                             float[2] voxel_size feat_div, arena f32, desc i64 (B, 18), sample_idx i32, then the POISON the outputs
//                             start from: coords i32 (out_rows,4), feats f32 (out_rows,nfeat), sample_out i32, points_out f32
//                             OUT: coords, feats, sample_out, points_out (if wanted)
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
struct alignas(16) int4 { int x, y, z, w; };
static thread_local D3 threadIdx;
static D3 blockIdx, gridDim;
static std::barrier<>* g_bar;
static void __syncthreads() { g_bar->arrive_and_wait(); }
#pragma clang fp contract(off)
#include "../fcaf3d_amd/csrc/aug_point.h"  // batch.hip includes it above the cut
#include "kernels.inc"

template <class F> static void launch(unsigned gx, F f) {
  gridDim = {gx, 1, 1};
  for (unsigned bx = 0; bx < gx; ++bx) {
    blockIdx = {bx, 0, 0};
    std::barrier<> bar(BATCH_THREADS);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < BATCH_THREADS; ++t) th.emplace_back([&, t] { threadIdx = {t, 0, 0}; f(); });
    for (auto& x : th) x.join();
  }
}
// exact-size heap arrays (ASan sees every access past them), 16-byte aligned for the kernel's int4 store
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
  int64_t* h = rd<int64_t>(f, 8);
  const int64_t arena_rows = h[0], pt_stride = h[1], B = h[2], total_out = h[3], out_rows = h[4], n_idx = h[5], nfeat = h[6], want = h[7];
  float* fl = rd<float>(f, 2);
  float* arena = rd<float>(f, arena_rows * pt_stride);
  int64_t* desc = rd<int64_t>(f, B * BATCH_DESC_WORDS);
  int* idx = n_idx >= 0 ? rd<int>(f, n_idx) : nullptr;
  int* coords = rd<int>(f, out_rows * 4);
  float* feats = rd<float>(f, out_rows * nfeat);
  int* sample_out = rd<int>(f, out_rows);
  float* points_out = want ? rd<float>(f, out_rows * (3 + nfeat)) : nullptr;
  fclose(f);
  launch(batch_blocks(total_out), [&] {
    k_batch_augment_voxelize(arena, arena_rows, (int)pt_stride, desc, (int)B, idx, n_idx >= 0 ? n_idx : 0, out_rows, fl[0], fl[1], (int)nfeat,
                             coords, feats, sample_out, points_out);
  });
  FILE* o = fopen(argv[2], "wb");
  fwrite(coords, 4, out_rows * 4, o); fwrite(feats, 4, out_rows * nfeat, o); fwrite(sample_out, 4, out_rows, o);
  if (want) fwrite(points_out, 4, out_rows * (3 + nfeat), o);
  fclose(o);
  free(h); free(fl); free(arena); free(desc); free(idx); free(coords); free(feats); free(sample_out); free(points_out);
  return 0;
}
