// What the tiled convolution kernels share (k_conv_mfma / _p / k_conv_glds: conv_f32.h; k_conv_x6: conv_x6.h; k_conv_h3r: conv_h3r.h)
// — the pair-mode tile walk and the offset mask of a tile — and what the weight-gradient kernels share (k_wgrad_mfma / _p /
// k_wgrad_multi: wgrad_f32.h; k_wgrad_x6t: wgrad_x6.h): the workgroup decode.
// The kernels compile to the device code they had with these blocks written out (tools/device_asm_diff.py, profiles/r7_notes.md
// section 10).  That holds only for helpers that take and return VALUES: the compiler inlines them after its first round of scalar
// promotion and simplification, and a kernel local handed over by reference (bx, n_out, the accumulators) stays in memory through that
// round, after which every kernel that calls the helper is allocated and laid out differently.  So the helpers get the values the
// kernel already holds (tid, lane, m0, ...) and hand results back in small structs.
#pragma once

// ---- pair mode (fc_conv_fwd_pairs) -----------------------------------------------------------------------------------------------
// `nbr` row z lists the input rows of offset z's cnt[z] pairs and the tile computes those compacted rows only:
// T_z[j] = in[pair_in[z][j]] @ W[z], written to slab z of the workspace.  From here on it is a one-offset convolution over cnt[z]
// rows.  Two grid shapes: (row tiles, column tiles, K) with the workgroups beyond cnt[z] exiting at once, or — gridDim.z == 1, the
// caller knows sum_k ceil(cnt[k] / BM) — a LINEAR list of the live tiles only, offset-major (r2: the dead workgroups of the 3-D grid
// skew the round-robin placement, a few shader engines overflow and their last workgroups start a whole round late: 115 -> 88 us on
// the 3.5k-row level).
// The walk of that list: offset z and row tile bx of this workgroup (the 3-D grid: as they came in).  The kernel then sets
// n_out = cnt[z], returns if bx * BM lies past it, rebases nbr / W or kbase / out and goes on with K = 1, S = 1, z = 0.
struct PairTile { int64_t bx; int z; };
template <int BM>
__device__ __forceinline__ PairTile tile_pair_walk(const int* cnt, int K, int64_t bx, int z) {
  if (gridDim.z == 1 && K > 1) {
    int k = 0;
    for (; k < K - 1; ++k) {
      const int64_t t = ((int64_t)cnt[k] + BM - 1) / BM;
      if (bx < t) break;
      bx -= t;
    }
    z = k;
  }
  return {bx, z};
}

// ---- which of this split's offsets (z, z + S, ... < K) have a neighbour anywhere in the tile's BM rows from m0 ------------------------
// (offsets without one are skipped outright.)  OR within each wave, one LDS atomic per wave into *kmask_s — any LDS word that nothing
// else touches before the second barrier here.
template <int BM, bool HAS_NBR>
__device__ __forceinline__ unsigned int tile_offset_mask(unsigned int* kmask_s, const int* nbr, int64_t m0, int64_t n_out,
                                                         int z, int K, int S, int tid, int lane) {
  if (tid == 0) *kmask_s = 0u;
  __syncthreads();
  if (tid < BM) {
    unsigned int mk = 0u;
    int64_t row = m0 + tid;
    if (row < n_out) {
      if (HAS_NBR) {
        for (int k = z; k < K; k += S)
          if (nbr[(int64_t)k * n_out + row] >= 0) mk |= 1u << k;
      } else {
        mk = 1u;
      }
    }
    for (int off = 32; off > 0; off >>= 1) mk |= __shfl_xor(mk, off, 64);
    if (lane == 0 && mk) atomicOr(kmask_s, mk);
  }
  __syncthreads();
  return *kmask_s;
}

// ---- weight gradient: what a workgroup works on ---------------------------------------------------------------------------------------
// blockIdx.y = ((first offset / KO) * Cin tiles + Cin tile) * Cout tiles + Cout tile
struct WgradTile { int k0, ci0, co0; };
template <int BMc, int BNc>
__device__ __forceinline__ WgradTile wgrad_tile(int Cin, int Cout, int KO) {
  const int tiles_n = Cout / BNc, tiles_m = Cin / BMc;
  int y = blockIdx.y;
  const int tn = y % tiles_n; y /= tiles_n;
  const int tm = y % tiles_m; y /= tiles_m;
  return {y * KO, tm * BMc, tn * BNc};
}
// ... and its rows [begin, end) of the reduction: split blockIdx.x of n_out rows, rows_per_split each; PAIRS: of offset k's cnt[k]
// pairs, split evenly over gridDim.x in whole chunks of BKR rows
struct WgradRows { int64_t begin, end; };
template <bool PAIRS, int BKR>
__device__ __forceinline__ WgradRows wgrad_rows(const int* __restrict__ cnt, int k, int64_t n_out, int64_t rows_per_split) {
  int64_t total = n_out;
  if (PAIRS) {
    total = cnt[k];
    rows_per_split = ((total + gridDim.x - 1) / gridDim.x + BKR - 1) / BKR * BKR;
  }
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_split;
  int64_t r_end = r_begin + rows_per_split;
  if (r_end > total) r_end = total;
  return {r_begin, r_end};
}
