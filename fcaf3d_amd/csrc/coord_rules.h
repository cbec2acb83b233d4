// One body per coordinate rule that both coordinate phases apply: the per-operator entry points (coords.hip) and the native plan
// (plan_chain.h) must give the same sets and tables bit for bit (tests/test_gpu_plan.py), so the rules they share are stated here
// once.  Each kernel keeps its own signature, indexing and launch; everything here inlines into it and leaves its device code as it
// was.  (Not here: the row masks and the pair-list count / fill — coords.hip indexes them by the unsigned block index and a run-time
// K, the plan's batched kernels by a signed block of a job and K = 27, and one body for both changes the code of one of them.)
#ifndef FCAF3D_COORD_RULES_H
#define FCAF3D_COORD_RULES_H
#include "fc_common.h"

// a voxel of stride q: every axis rounded down to a multiple of q
__device__ static inline int4 fc_quantize(int4 c, int q) {
  if (q > 1) {
    c.y = fc_floor_div(c.y, q) * q;
    c.z = fc_floor_div(c.z, q) * q;
    c.w = fc_floor_div(c.w, q) * q;
  }
  return c;
}

// a coordinate that does not fit fc_pack's 16 bits per axis (with room for the largest kernel offset) or a batch index that does not
// fit its 16 bits — e.g. an inf / far-outlier point: such a key would alias another voxel
__device__ static inline bool fc_coord_out_of_range(int4 c) {
  return c.x < 0 || c.x > 32767 || c.y < -FC_COORD_LIMIT || c.y > FC_COORD_LIMIT || c.z < -FC_COORD_LIMIT || c.z > FC_COORD_LIMIT ||
         c.w < -FC_COORD_LIMIT || c.w > FC_COORD_LIMIT;
}

// the same for a voxel ALREADY rounded down to stride q (fc_hash_unique builds a strided set from an accepted one): rounding takes
// -FC_COORD_LIMIT to -(FC_COORD_LIMIT + 1) = -510 * 64, a multiple of every stride of the pyramid, and that voxel is a member of the
// set like any other — its key fields still hold the largest kernel offset (128 - 64 >= 0).  The plan's chain checks the raw rows of
// level 0 only and accepts it; held to the raw limit, the per-operator path refused every scene with a voxel at -32 639 as soon as
// it was strided (tests/test_gpu_coords_exact.py: range_limit, edge_*_neg_32639).  q = 1 is the raw rule.
__device__ static inline bool fc_voxel_out_of_range(int4 c, int q) {
  const int lo = q > 1 ? -(FC_COORD_LIMIT + 1) : -FC_COORD_LIMIT;
  return c.x < 0 || c.x > 32767 || c.y < lo || c.y > FC_COORD_LIMIT || c.z < lo || c.z > FC_COORD_LIMIT || c.w < lo || c.w > FC_COORD_LIMIT;
}

// row i into the voxel hash (linear probing): the first occurrence (smallest row) wins — SURVEY.md Appendix A.2; slot[i] = where.
// I: the caller's row index type
template <typename I>
__device__ static inline void fc_hash_insert(unsigned long long* keys, int* vals, unsigned long long mask, int4 c, I i, int* slot) {
  const unsigned long long key = fc_pack(c.x, c.y, c.z, c.w);
  unsigned long long h = fc_mix(key) & mask;
  while (true) {
    const unsigned long long prev = atomicCAS(&keys[h], FC_EMPTY_KEY, key);
    if (prev == FC_EMPTY_KEY || prev == key) {
      atomicMin(&vals[h], (int)i);
      slot[i] = (int)h;
      return;
    }
    h = (h + 1) & mask;
  }
}

#endif
