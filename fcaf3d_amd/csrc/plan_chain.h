// Stage 1 of the native coordinate phase (fc_plan_levels): the collate, the voxel hash and the whole pyramid of strided sets as ONE
// chain of kernels with DEVICE-resident row counts — every kernel is launched for the upper bound and reads the live count from the
// previous set's meta word (plan_layout.h META_*; behind all sets: rows per (set, scene)).
#ifndef FCAF3D_PLAN_CHAIN_H
#define FCAF3D_PLAN_CHAIN_H
#include "fc_common.h"
#include "plan_layout.h"
#include "coord_rules.h"     // the quantiser, the range predicate, the hash insert: shared with coords.hip

namespace {

constexpr int CH = 32;              // scenes per launch of the point kernel
struct SceneArgs { const float* p[CH]; int n[CH]; int off[CH]; int b0, stride, nfeat; float vs, feat_div; };

// capacity of the table of a set whose INPUT has n rows: next_pow2(2 n) — the per-operator path's rule (sparse.CoordMap.from_coords)
__host__ __device__ inline unsigned long long table_mask(int64_t n_in) {
  int64_t cap = 2;
  while (cap < 2 * n_in) cap *= 2;
  return (unsigned long long)(cap - 1);
}

// all tables of the chain in one launch: keys (S, cap) / vals (S, cap) contiguous, two key slots per thread
__global__ void k_plan_tables_init(unsigned long long* __restrict__ keys, int* __restrict__ vals, int64_t total) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (i + 1 < total) {
    *reinterpret_cast<ulonglong2*>(keys + i) = make_ulonglong2(FC_EMPTY_KEY, FC_EMPTY_KEY);
    *reinterpret_cast<int2*>(vals + i) = make_int2(0x7fffffff, 0x7fffffff);
  } else if (i < total) {
    keys[i] = FC_EMPTY_KEY; vals[i] = 0x7fffffff;
  }
}

// the collate (single_stage_sparse.py:34-36: floor(xyz / voxel_size), features / 255, batch index = scene) fused with the hash
// insert of level 0 — blockIdx.y = scene of the chunk.  (true fp32 division, as fc_voxelize.)
__global__ void k_plan_voxelize_insert(SceneArgs sc, int4* __restrict__ coords, float* __restrict__ feats, unsigned long long* keys,
                                       int* vals, unsigned long long mask, int* __restrict__ meta_s, int* __restrict__ slot) {
  const int j = blockIdx.y;
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= sc.n[j]) return;
  const float* p = sc.p[j] + (int64_t)l * sc.stride;
  const int i = sc.off[j] + l;
  int4 c;
  c.x = sc.b0 + j;
  c.y = (int)floorf(p[0] / sc.vs); c.z = (int)floorf(p[1] / sc.vs); c.w = (int)floorf(p[2] / sc.vs);
  coords[i] = c;
  for (int f = 0; f < sc.nfeat; ++f) feats[(int64_t)i * sc.nfeat + f] = p[3 + f] / sc.feat_div;
  if (fc_coord_out_of_range(c)) meta_s[META_BAD] = 1;
  fc_hash_insert(keys, vals, mask, c, i, slot);
}

// level 0 from a pre-voxelised coordinate array
__global__ void k_plan_insert(const int4* __restrict__ coords, int64_t n, unsigned long long* keys, int* vals, unsigned long long mask,
                              int* __restrict__ meta_s, int* __restrict__ slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 c = coords[i];
  if (fc_coord_out_of_range(c)) meta_s[META_BAD] = 1;
  fc_hash_insert(keys, vals, mask, c, (int)i, slot);
}

// winners: flags + the count of every 256-row sub-block (blocksums: a wave quad of k_plan_finalize) and of every 1 024-row block
// (coarse: a block of k_plan_finalize).  No scan here: every block of k_plan_finalize adds up the (L2-resident, <= a few thousand) counts in front of it — and all
// of them, for the set's row count — itself.  (Until r6's last take the LAST block to finish scanned the counts in place: a
// device-scope fence and a same-line atomic per block, 28 us for an EMPTY set and ~60 of the ~100 us of a full one.)
__global__ __launch_bounds__(256) void k_plan_flags(const int* __restrict__ slot, const int* __restrict__ vals, const int* __restrict__ n_dev,
                                                    int64_t n_host, unsigned char* __restrict__ flags, int* __restrict__ blocksums,
                                                    int* __restrict__ coarse) {
  const int64_t n = n_dev ? *n_dev : n_host;
  if ((int64_t)blockIdx.x * 1024 >= n) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ int wsr[4][4];
  // the four dependent read pairs of a thread (slot, table value) are issued together
  int f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + r * 256 + threadIdx.x;
    f[r] = i < n ? (vals[slot[i]] == (int)i) : 0;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + r * 256 + threadIdx.x;
    if (i < n) flags[i] = (unsigned char)f[r];
    const unsigned long long bal = __ballot(f[r]);
    if (lane == 0) wsr[r][w] = __popcll(bal);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int r = threadIdx.x;
    blocksums[4 * blockIdx.x + r] = wsr[r][0] + wsr[r][1] + wsr[r][2] + wsr[r][3];
  } else if (threadIdx.x == 64) {
    int t = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) t += wsr[r][0] + wsr[r][1] + wsr[r][2] + wsr[r][3];
    coarse[blockIdx.x] = t;
  }
}

// positions + the set itself: winner row i -> out row p: coordinates (with its feature row for level 0), table value = p,
// rows-per-scene counters — and, fused, the hash insert of the NEXT set of the chain: row p of this set, quantised to the next
// stride, goes into the next table with value p (first occurrence = smallest p, as an insert pass over the finished set would
// give).  A block covers the 1 024 input rows of one block of k_plan_flags, one row per thread, waves 4r .. 4r + 3 its sub-block r.
// The block's first output row = the winners in front of it = the coarse counts of the blocks before its own, a sub-block's
// = + the sub-block counts before it; the set's row count (the next table's mask; block 0 leaves it in meta_s[META_ROWS] for
// the kernels behind) = all coarse counts.
//
// Rows per scene: rows of one scene are consecutive, so a block's winners belong to a short run of scenes that begins at
// the scene of the block's first input row.  Each wave adds its count per scene to one of PF_SCENE_SLOTS counters in LDS
// (scene - first scene), and the block sends ONE global atomic per occupied slot; a scene outside the slots (more than
// PF_SCENE_SLOTS scenes inside 1 024 rows, or rows that are not in scene order) takes one global atomic per wave.  All
// counters of a set share one cache line: one atomic per wave and scene — 12 500 of them for the level-0 set of eight
// 100 000-point scenes — queued up at that line; a block now sends one or two (~800 for that set).  The sums are
// integers: any grouping is exact.  (profiles/r7_notes.md section 14: the seven launches of the benchmark's chain 540 -> 239 us,
// what the kernel without any counter takes.)
//
// Knock-outs (tools/planbench.py --ko; never the product library, the plans are wrong):
//   -DFC_KO_PF_NOCOUNT: no scene counters      -DFC_KO_PF_NOVALS: no vals[slot[i]] = p
//   -DFC_KO_PF_NOINSERT: no insert into the next table (slot 0 for every row: the sets behind come out empty)
constexpr int PF_SCENE_SLOTS = 4;
__global__ __launch_bounds__(1024) void k_plan_finalize(const int4* __restrict__ coords, const int* __restrict__ n_dev, int64_t n_host, int q,
                                                        const unsigned char* __restrict__ flags, const int* __restrict__ blocksums,
                                                        const int* __restrict__ coarse, const int* __restrict__ slot, int* vals,
                                                        int4* __restrict__ out_coords, const float* __restrict__ feats_in,
                                                        float* __restrict__ feats_out, int nfeat, int* __restrict__ scene_cnt, int B,
                                                        int* __restrict__ meta_s, unsigned long long* next_keys, int* next_vals,
                                                        int* __restrict__ next_slot) {
  __shared__ int ws[16];
  __shared__ int red[2][16];
  __shared__ int cnt[PF_SCENE_SLOTS];
  const int64_t n = n_dev ? *n_dev : n_host;
  const int64_t base = (int64_t)blockIdx.x * 1024;
  if (base >= n) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = w >> 2;
  const int64_t i = base + threadIdx.x;
  const int f = i < n ? (int)flags[i] : 0;
  const unsigned long long bal = __ballot(f);
  if (lane == 0) ws[w] = __popcll(bal);
  if (threadIdx.x < PF_SCENE_SLOTS) cnt[threadIdx.x] = 0;
  const int first_scene = coords[base].x;
  const int nc = (int)((n + 1023) >> 10), mine = (int)blockIdx.x;
  int sub = 0;                                     // winners of the sub-blocks in front of this wave's
  for (int k = 0; k < r; ++k) sub += blocksums[4 * mine + k];
  int before = 0, all = 0;
  for (int j = threadIdx.x; j < nc; j += 1024) {
    const int v = coarse[j];
    all += v;
    if (j < mine) before += v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o, 64);
    all += __shfl_xor(all, o, 64);
  }
  if (lane == 0) { red[0][w] = before; red[1][w] = all; }
  __syncthreads();
  int pre = sub, total = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { pre += red[0][k]; total += red[1][k]; }
  if (blockIdx.x == 0 && threadIdx.x == 0) meta_s[META_ROWS] = total;
  const unsigned long long nmask = next_keys ? table_mask(total) : 0ull;
  for (int k = 4 * r; k < w; ++k) pre += ws[k];
  int b = -1;
  if (f) {
    const int p = pre + __popcll(bal & ((1ull << lane) - 1ull));
    const int4 c = fc_quantize(coords[i], q);
    out_coords[p] = c;
#ifndef FC_KO_PF_NOVALS
    vals[slot[i]] = p;                             // the table now maps key -> row of the new set
#endif
    if (feats_out)
      for (int k = 0; k < nfeat; ++k) feats_out[(int64_t)p * nfeat + k] = feats_in[i * nfeat + k];
    b = c.x;
#ifndef FC_KO_PF_NOINSERT
    if (next_keys) fc_hash_insert(next_keys, next_vals, nmask, fc_quantize(c, 2 * q), p, next_slot);
#else
    if (next_keys) next_slot[p] = 0;
#endif
  }
#ifndef FC_KO_PF_NOCOUNT
  unsigned long long rem = bal;                    // rows per scene
  while (rem) {
    const int leader = __ffsll((long long)rem) - 1;
    const int lb = __shfl(b, leader, 64);
    const unsigned long long same = __ballot(f && b == lb);
    if (lane == leader) {
      const unsigned k = (unsigned)lb - (unsigned)first_scene;
      if (k < (unsigned)PF_SCENE_SLOTS) atomicAdd(&cnt[k], __popcll(same));
      else if (lb >= 0 && lb < B) atomicAdd(&scene_cnt[lb], __popcll(same));
    }
    rem &= ~same;
  }
  __syncthreads();
  if (threadIdx.x < PF_SCENE_SLOTS) {
    const int64_t sc = (int64_t)first_scene + threadIdx.x;
    const int v = cnt[threadIdx.x];
    if (v && sc >= 0 && sc < B) atomicAdd(&scene_cnt[sc], v);
  }
#endif
}

}  // namespace

#endif
