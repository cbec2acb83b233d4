// The stable argsort of 27-bit keys behind the mask-sorted tables of the native coordinate phase (fc_plan_maps) and fc_argsort27:
// an LSD radix sort, all sort jobs of a plan per launch.
#ifndef FCAF3D_PLAN_RADIX_H
#define FCAF3D_PLAN_RADIX_H
#include "plan_batch.h"

namespace {

// one (27, n) table that gets a mask-sorted copy: its occupancy masks, their argsort (`order`), the permuted table; ka / kb / va / hist
// are the argsort's workspace (sort_job_ws)
struct SortJob { const int* tab; int* masks; int* order; int* sorted; int* ka; int* kb; int* va; int* hist; int64_t n; int nblk, nbx; };

// ---- LSD radix argsort of 27-bit keys (the occupancy masks), stable: 3 passes of 9 bits; all sort jobs of a plan per launch -------
constexpr int RB = 9, RBINS = 1 << RB, RTILE = 4096;
struct RadixIO { const int* kin; const int* vin; int* kout; int* vout; };
// p0: (masks, identity) -> (ka, order); p1: (ka, order) -> (kb, va); p2: (kb, va) -> (ka, order): the result lands in `order`.
// PASS is a template parameter: with a run-time pass hipcc 7.2 left the key pointer of the third pass undefined in k_radix_scatter
// (the switch lowering assigned it on one of two default paths only: it read job 0's `tab` — found with a null `tab`, r6_notes.md)
template <int PASS> __device__ __forceinline__ RadixIO radix_io(const SortJob& j) {
  if (PASS == 0) return {j.masks, nullptr, j.ka, j.order};
  if (PASS == 1) return {j.ka, j.order, j.kb, j.va};
  return {j.kb, j.va, j.ka, j.order};
}
template <int PASS> __global__ __launch_bounds__(256) void k_radix_hist(Batch<SortJob> bt) {
  constexpr int pass = PASS;
  __shared__ int h[RBINS];
  int64_t lb;
  const SortJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int* keys = radix_io<PASS>(j).kin;
  const int shift = pass * RB;
  for (int b = threadIdx.x; b < RBINS; b += 256) h[b] = 0;
  __syncthreads();
  const int64_t base = lb * RTILE;
  for (int r = 0; r < RTILE / 256; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    if (i < j.n) atomicAdd(&h[(keys[i] >> shift) & (RBINS - 1)], 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < RBINS; b += 256) j.hist[lb * RBINS + b] = h[b];
}

// one block of RBINS threads per job: hist[blk][d] -> global start of (d, blk) in (digit, block) order
__global__ __launch_bounds__(RBINS) void k_radix_scan(Batch<SortJob> bt) {
  __shared__ int tot[RBINS];
  const SortJob& j = bt.j[blockIdx.x];
  int* hist = j.hist;
  const int nblk = j.nblk;
  const int d = threadIdx.x;
  int run = 0;
  for (int b = 0; b < nblk; ++b) {
    const int v = hist[(int64_t)b * RBINS + d];
    hist[(int64_t)b * RBINS + d] = run;
    run += v;
  }
  tot[d] = run;
  __syncthreads();
  int x = run;                                     // inclusive scan of the digit totals (Hillis-Steele over RBINS threads)
  for (int o = 1; o < RBINS; o <<= 1) {
    const int t = d >= o ? tot[d - o] : 0;
    __syncthreads();
    x += t;
    tot[d] = x;
    __syncthreads();
  }
  const int dbase = x - run;
  for (int b = 0; b < nblk; ++b) hist[(int64_t)b * RBINS + d] += dbase;
}

// rank inside the tile in row order (stable) and scatter.  vin == nullptr: the identity (first pass).
template <int PASS> __global__ __launch_bounds__(256) void k_radix_scatter(Batch<SortJob> bt) {
  constexpr int pass = PASS;
  __shared__ int offs[RBINS];
  int64_t lb;
  const SortJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const RadixIO io = radix_io<PASS>(j);
  const int shift = pass * RB;
  const int64_t n = j.n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = threadIdx.x; b < RBINS; b += 256) offs[b] = j.hist[lb * RBINS + b];
  __syncthreads();
  const int64_t base = lb * RTILE;
  for (int r = 0; r < RTILE / 256; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    const bool live = i < n;
    const int key = live ? io.kin[i] : 0;
    const int d = (key >> shift) & (RBINS - 1);
    unsigned long long peers = __ballot(live);     // lanes of this wave with the same digit
    for (int b = 0; b < RB; ++b) {
      const unsigned long long m = __ballot((d >> b) & 1);
      peers &= ((d >> b) & 1) ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    const int cnt = __popcll(peers);
    int dst = 0;
    for (int ww = 0; ww < 4; ++ww) {               // waves in row order
      if (w == ww && live && rank == 0) { dst = offs[d]; offs[d] = dst + cnt; }
      __syncthreads();
    }
    const int leader = __ffsll((long long)peers) - 1;
    dst = __shfl(dst, live ? leader : 0, 64);
    if (live) {
      io.kout[dst + rank] = key;
      io.vout[dst + rank] = io.vin ? io.vin[i] : (int)i;
    }
  }
}

int64_t argsort27_ws_bytes(int64_t n) { return fc_align(4 * n, 256) * 3 + fc_align(4 * fc_cdiv(n > 0 ? n : 1, RTILE) * RBINS, 256); }
// masks must be filled already (job.masks); ws of every job: ka, kb, va, hist
int argsort27_batch(const Batch<SortJob>& bt, hipStream_t s) {
  static_assert(sizeof(Batch<SortJob>) <= 1536, "batch descriptor too large for the kernel-argument block");
  if (bt.overflow) return FC_EINVAL;
  if (!bt.count || !bt.blocks()) return 0;
  Batch<SortJob> tiles = bt;                       // blocks = RTILE tiles
  tiles.count = 0; tiles.blk0[0] = 0;
  for (int i = 0; i < bt.count; ++i) tiles.add(bt.j[i], bt.j[i].nblk);
  const unsigned g = (unsigned)tiles.blocks(), nj = (unsigned)tiles.count;
#define FC_RADIX_PASS(P)                                  \
  k_radix_hist<P><<<g, 256, 0, s>>>(tiles);               \
  FC_CHECK_LAUNCH();                                      \
  k_radix_scan<<<nj, RBINS, 0, s>>>(tiles);               \
  FC_CHECK_LAUNCH();                                      \
  k_radix_scatter<P><<<g, 256, 0, s>>>(tiles);            \
  FC_CHECK_LAUNCH();
  FC_RADIX_PASS(0)
  FC_RADIX_PASS(1)
  FC_RADIX_PASS(2)
#undef FC_RADIX_PASS
  return 0;
}
// rows of all jobs, and the compulsory bytes of the three passes: per pass keys + values read twice-ish, written once
inline double sort_rows(const Batch<SortJob>& b) { double t = 0; for (int i = 0; i < b.count; ++i) t += (double)b.j[i].n; return t; }
inline double probe_bytes_radix(const Batch<SortJob>& b) { return sort_rows(b) * 3.0 * (8.0 + 4.0 + 8.0); }
void sort_job_ws(SortJob& j, void* ws) {
  char* w = (char*)ws;
  j.ka = (int*)w; w = at(w, fc_align(4 * j.n, 256));
  j.kb = (int*)w; w = at(w, fc_align(4 * j.n, 256));
  j.va = (int*)w; w = at(w, fc_align(4 * j.n, 256));
  j.hist = (int*)w;
  j.nblk = (int)fc_cdiv(j.n > 0 ? j.n : 1, RTILE);
  j.nbx = (int)fc_cdiv(j.n > 0 ? j.n : 1, 256);
}

}  // namespace

#endif
