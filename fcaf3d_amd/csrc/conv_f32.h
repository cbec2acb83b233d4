// The fp32 convolution kernels on the matrix cores (v_mfma_f32_32x32x2_f32: an exact fp32 FMA chain) — k_conv_mfma, its deeper-pipelined
// variant k_conv_mfma_p and the LDS-DMA variant k_conv_glds — and the untiled fallback k_conv_fma.  Included by conv.hip, which holds
// what they use (g_zero_row, g_fc_prio, the trace points of fc_trace.h) and launches them (launch_conv).
#pragma once

#define BK 32            // reduction slab (input channels per stage / rows per stage for wgrad)
#define LDA (BK + 4)     // A row stride in floats: 16B-aligned rows, conflict-free ds_read_b128 (9r mod 16)

// ------------------------------------------------------------------------------------------------
// Pipeline per workgroup: (1) which kernel offsets have any neighbour among the tile's rows (offsets without one are
// skipped outright), OR-reduced over the tile's rows; (2) walk the surviving (offset,
// Cin-slab) stages with the NEXT stage's gathers + weight loads issued into registers before the current stage's MFMAs
// run (single LDS buffer, global-load latency hidden behind the matrix pipe).
// gridDim.z > 1 = split over kernel offsets (offset k handled by split k % gridDim.z) for layers whose
// row count cannot fill the chip; partial tiles go to `out` + z*n_out*Cout and are summed by k_sum_parts.
// WM = waves along the rows (2: 2 x 2 waves; 4: 4 x 1 — the 256 x 64 tile for 64-wide outputs: every wave still owns a
// 64 x 64 quadrant, i.e. the operand re-use of the 128 x 128 tile, where a 128 x 64 tile halves it).
// WT: the weights are given TRANSPOSED, W[k] as (Cout, Cin) row-major — the backward-data pass reads the layer's own
// (K, Cin, Cout) kernel as the (Cout -> Cin) operator it needs, no per-step transpose launch.  Only the staging differs:
// a thread loads 4 reduction-consecutive floats of one output column and stores them as 4 ds_write_b32 (conflict-free:
// consecutive lanes = consecutive columns); the LDS image, the fragment reads and the results are the same.
template <int BM, int BN, int BKT, bool HAS_NBR, int WM = 2, bool WT = false>
__global__ __launch_bounds__(256, (BM == 128 && BN == 128 && BKT == 32) ? 4 : (WM == 4 ? 3 : 2)) void k_conv_mfma(const float* __restrict__ in, const float* __restrict__ W,
                                                   const int* __restrict__ nbr,
                                                   const int* __restrict__ out_index, const int* __restrict__ cnt,
                                                   float* __restrict__ out, int64_t n_out, int K, int Cin, int Cout) {
  constexpr int WN = 4 / WM;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);      // 32x32 MFMA tiles per wave
  constexpr int RW = BM / WM, CW = BN / WN;      // rows / columns of a wave's part of the tile
  constexpr int LDAT = BKT + 4;                  // (BKT+4)/4 odd -> conflict-free ds_read_b128 of the A fragments
  constexpr int A4 = BKT / 4;                    // float4 per gathered row slab
  constexpr int APASS = 256 / A4;                // rows staged per pass
  constexpr int AR = BM / APASS;                 // float4 gathers per thread per stage
  constexpr int BR = BKT * BN / 1024;            // float4 weight loads per thread per stage
  __shared__ __attribute__((aligned(16))) float As[BM * LDAT];
  __shared__ __attribute__((aligned(16))) float Bs[BKT * BN];
  __shared__ unsigned int kmask_s;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = WM == 4 ? wave : wave >> 1, wc = WM == 4 ? 0 : wave & 1;
  const int r = lane & 31, h = lane >> 5;
  int64_t bx = blockIdx.x;
  const int n0 = blockIdx.y * BN;
  int S = gridDim.z, z = blockIdx.z;
  TR_DECL;
  TR(0);
  int tr_units = 0;
  (void)tr_units;
  if (cnt) {                                     // pair mode: tile_pair_walk (conv_tile.h)
    const PairTile pt = tile_pair_walk<BM>(cnt, K, bx, z);
    bx = pt.bx; z = pt.z;
    const int64_t stride = n_out;
    n_out = cnt[z];
    if (bx * BM >= n_out) return;
    nbr += (int64_t)z * stride;
    W += (int64_t)z * Cin * Cout;
    out += (int64_t)z * stride * Cout;
    K = 1; S = 1; z = 0;
  }
  const int64_t m0 = bx * BM;
  const int a_c4 = tid % A4, a_r = tid / A4;     // A staging: A4 float4 per row, APASS rows per pass

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // ---- (1) which of this split's offsets have a neighbour anywhere in the tile ---------------------
  unsigned int kmask = tile_offset_mask<BM, HAS_NBR>(&kmask_s, nbr, m0, n_out, z, K, S, tid, lane);
  TR(1);

  // ---- (2) software-pipelined stage loop -------------------------------------------------------------
  if (kmask) {
    int k = __ffs(kmask) - 1;
    kmask &= kmask - 1;
    int c0 = 0;
    f32x4 av[AR], bv[BR];
    // Prefetch of one stage, written branch-free so that the compiler issues it as batches (the AR neighbour
    // indices, the weights, then the AR gathers) instead of AR serialised index->wait->gather chains with the data
    // waited for on the spot (r1 ISA reading).  An absent neighbour gathers from a row of zeros (pointer select
    // BEFORE the load), so nothing touches the loaded registers until the next stage's LDS store.
    auto load_stage = [&](int kk, int cc) {
      const float* Wk = W + (int64_t)kk * Cin * Cout;
      int v[AR];
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        int64_t row = m0 + a_r + APASS * i;
        int64_t rc = row < n_out ? row : n_out - 1;
        int t = HAS_NBR ? nbr[(int64_t)kk * n_out + rc] : (int)rc;    // compile-time: no null test between the loads
        v[i] = row < n_out ? t : -1;
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        int lin = tid + 256 * i;
        if (WT) {
          bv[i] = *reinterpret_cast<const f32x4*>(Wk + (int64_t)(n0 + lin % BN) * Cin + cc + (lin / BN) * 4);
        } else {
          int kr = lin / (BN / 4), c4 = lin % (BN / 4);
          bv[i] = *reinterpret_cast<const f32x4*>(Wk + (int64_t)(cc + kr) * Cout + n0 + c4 * 4);
        }
      }
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const float* src = v[i] < 0 ? g_zero_row + a_c4 * 4 : in + (int64_t)v[i] * Cin + cc + a_c4 * 4;
        av[i] = *reinterpret_cast<const f32x4*>(src);
      }
    };
    load_stage(k, c0);
    const bool prio = g_fc_prio >= 0;             // see g_fc_prio
    while (true) {
#ifdef FC_TRACE
      if (tr_units == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TR(2); }
      tr_units += BKT / 8;
#endif
      __syncthreads();                           // previous stage fully consumed
#pragma unroll
      for (int i = 0; i < AR; ++i)
        *reinterpret_cast<f32x4*>(&As[(a_r + APASS * i) * LDAT + a_c4 * 4]) = av[i];
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        int lin = tid + 256 * i;
        if (WT) {
#pragma unroll
          for (int e = 0; e < 4; ++e) Bs[((lin / BN) * 4 + e) * BN + lin % BN] = bv[i][e];
        } else {
          int kr = lin / (BN / 4), c4 = lin % (BN / 4);
          *reinterpret_cast<f32x4*>(&Bs[kr * BN + c4 * 4]) = bv[i];
        }
      }
      __syncthreads();
      // issue the next stage's global loads before computing this one
      int nk = k, nc0 = c0 + BKT;
      if (nc0 >= Cin) {
        nc0 = 0;
        nk = kmask ? __ffs(kmask) - 1 : -1;
        kmask &= kmask - 1;
      }
      // unconditional (the last iteration re-reads its own stage): a conditionally assigned float4 array is not
      // promoted to registers by the compiler and lands in scratch
      load_stage(nk >= 0 ? nk : k, nk >= 0 ? nc0 : c0);
      if (prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < BKT / 8; ++q) {
        f32x4 a[TM];
        float b[TN][4];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          a[i] = *reinterpret_cast<const f32x4*>(&As[(wr * RW + i * 32 + r) * LDAT + 8 * q + 4 * h]);
        // sub-tile j of the wave owns the INTERLEAVED columns TN*r + j of its half of the tile: one ds_read_b64 per
        // (k, lane) instead of two ds_read_b32 (conflict-free: 32 lanes x 8 B = 64 banks), and 8-byte output stores
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (TN == 2) {
            const f32x2 bb = *reinterpret_cast<const f32x2*>(&Bs[(8 * q + 4 * h + e) * BN + wc * CW + 2 * r]);
            b[0][e] = bb[0];
            b[TN - 1][e] = bb[1];
          } else {
            b[0][e] = Bs[(8 * q + 4 * h + e) * BN + wc * CW + r];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            float ae = a[i][e];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae, b[j][e], acc[i][j], 0, 0, 0);
          }
        }
      }
      if (prio) __builtin_amdgcn_s_setprio(0);
      if (nk < 0) break;
      k = nk;
      c0 = nc0;
    }
  }
  // epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  TR(3);
  float* dst = out + (int64_t)z * n_out * Cout + n0 + wc * CW + TN * r;
  int orow[TM][16];                              // looked up in one batch ahead of the stores
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t row = m0 + wr * RW + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      int o = -1;
      if (row < n_out) o = out_index ? out_index[row] : (int)row;      // rows are processed in mask-sorted order
      orow[i][e] = o;
    }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (orow[i][e] >= 0) {
        if (TN == 2) {
          f32x2 v = {acc[i][0][e], acc[i][TN - 1][e]};
          *reinterpret_cast<f32x2*>(dst + (int64_t)orow[i][e] * Cout) = v;
        } else {
          dst[(int64_t)orow[i][e] * Cout] = acc[i][0][e];
        }
      }
    }
  TR(5);
  TR_FLUSH(tr_units);
}

// Deeper-pipelined variant of k_conv_mfma (same tiles, same LDS layout, same results) at 3 waves per SIMD (168 VGPRs):
//  * the neighbour rows of the NEXT kernel offset are requested one offset ahead (vnxt), so that a stage's gathers are
//    issued at once instead of behind an exposed index round trip (r2 ISA reading of k_conv_mfma: index loads ->
//    s_waitcnt vmcnt(0) -> gathers in front of every stage's MFMA block; the 128-VGPR budget of 4 waves/SIMD had no
//    room for the look-ahead — r1 dead end);
//  * the MFMA fragments of 8-channel step q+1 are read from LDS while step q multiplies (double-buffered fragment
//    registers) instead of read -> s_waitcnt lgkmcnt(0) -> multiply.
template <int BM, int BN, int BKT, bool HAS_NBR, int WM = 2, bool WT = false>
__global__ __launch_bounds__(256, 3) void k_conv_mfma_p(const float* __restrict__ in, const float* __restrict__ W,
                                                   const int* __restrict__ nbr,
                                                   const int* __restrict__ out_index, const int* __restrict__ cnt,
                                                   float* __restrict__ out, int64_t n_out, int K, int Cin, int Cout) {
  constexpr int WN = 4 / WM;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);      // 32x32 MFMA tiles per wave
  constexpr int RW = BM / WM, CW = BN / WN;      // rows / columns of a wave's part of the tile
  constexpr int LDAT = BKT + 4;                  // (BKT+4)/4 odd -> conflict-free ds_read_b128 of the A fragments
  constexpr int A4 = BKT / 4;                    // float4 per gathered row slab
  constexpr int APASS = 256 / A4;                // rows staged per pass
  constexpr int AR = BM / APASS;                 // float4 gathers per thread per stage
  constexpr int BR = BKT * BN / 1024;            // float4 weight loads per thread per stage
  __shared__ __attribute__((aligned(16))) float As[BM * LDAT];
  __shared__ __attribute__((aligned(16))) float Bs[BKT * BN];
  __shared__ unsigned int kmask_s;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = WM == 4 ? wave : wave >> 1, wc = WM == 4 ? 0 : wave & 1;
  const int r = lane & 31, h = lane >> 5;
  int64_t bx = blockIdx.x;
  const int n0 = blockIdx.y * BN;
  int S = gridDim.z, z = blockIdx.z;
  TR_DECL;
  TR(0);
  int tr_units = 0;
  (void)tr_units;
  if (cnt) {                                     // pair mode: tile_pair_walk (conv_tile.h)
    const PairTile pt = tile_pair_walk<BM>(cnt, K, bx, z);
    bx = pt.bx; z = pt.z;
    const int64_t stride = n_out;
    n_out = cnt[z];
    if (bx * BM >= n_out) return;
    nbr += (int64_t)z * stride;
    W += (int64_t)z * Cin * Cout;
    out += (int64_t)z * stride * Cout;
    K = 1; S = 1; z = 0;
  }
  const int64_t m0 = bx * BM;
  const int a_c4 = tid % A4, a_r = tid / A4;     // A staging: A4 float4 per row, APASS rows per pass

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // ---- (1) which of this split's offsets have a neighbour anywhere in the tile ---------------------
  unsigned int kmask = tile_offset_mask<BM, HAS_NBR>(&kmask_s, nbr, m0, n_out, z, K, S, tid, lane);
  TR(1);

  // ---- (2) software-pipelined stage loop -------------------------------------------------------------
  if (kmask) {
    const int nst = __popc(kmask) * (Cin / BKT);         // stages of this tile
    unsigned int rem = kmask;
    int lk = __ffs(rem) - 1;                              // load cursor: offset / channel slab of the stage requested next
    rem &= rem - 1;
    int lnk = rem ? __ffs(rem) - 1 : lk;                  // ... and the offset after it (its rows are already on their way)
    if (rem) rem &= rem - 1;
    int lc0 = 0;
    bool sw = false;                                      // the cursor has left lk: switch to lnk at the next request
    f32x4 av[AR], bv[BR];
    int vcur[AR], vnxt[AR];
    int64_t arow[AR];
    bool aok[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int64_t row = m0 + a_r + APASS * i;
      aok[i] = row < n_out;
      arow[i] = aok[i] ? row : n_out - 1;
    }
    // raw table entries only: nothing touches a requested index until the stage that uses it
    auto fetch_idx = [&](int kk, int (&v)[AR]) {
#pragma unroll
      for (int i = 0; i < AR; ++i) v[i] = HAS_NBR ? nbr[(int64_t)kk * n_out + arow[i]] : (int)arow[i];
    };
    fetch_idx(lk, vcur);
    fetch_idx(lnk, vnxt);
    auto load_stage = [&]() {
      if (sw) {                                           // first slab of a new offset: its rows were requested an offset ago
        sw = false;
        lk = lnk;
#pragma unroll
        for (int i = 0; i < AR; ++i) vcur[i] = vnxt[i];
        if (rem) {
          lnk = __ffs(rem) - 1;
          rem &= rem - 1;
        }
        fetch_idx(lnk, vnxt);
      }
      const float* Wk = W + (int64_t)lk * Cin * Cout;
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        int lin = tid + 256 * i;
        if (WT) {
          bv[i] = *reinterpret_cast<const f32x4*>(Wk + (int64_t)(n0 + lin % BN) * Cin + lc0 + (lin / BN) * 4);
        } else {
          int kr = lin / (BN / 4), c4 = lin % (BN / 4);
          bv[i] = *reinterpret_cast<const f32x4*>(Wk + (int64_t)(lc0 + kr) * Cout + n0 + c4 * 4);
        }
      }
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const float* src = (vcur[i] < 0 || !aok[i]) ? g_zero_row + a_c4 * 4 : in + (int64_t)vcur[i] * Cin + lc0 + a_c4 * 4;
        av[i] = *reinterpret_cast<const f32x4*>(src);
      }
    };
    load_stage();
    const bool prio = g_fc_prio >= 0;
    for (int st = 0; st < nst; ++st) {
#ifdef FC_TRACE
      if (tr_units == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TR(2); }
      tr_units += BKT / 8;
#endif
      __syncthreads();                           // previous stage fully consumed
#pragma unroll
      for (int i = 0; i < AR; ++i)
        *reinterpret_cast<f32x4*>(&As[(a_r + APASS * i) * LDAT + a_c4 * 4]) = av[i];
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        int lin = tid + 256 * i;
        if (WT) {
#pragma unroll
          for (int e = 0; e < 4; ++e) Bs[((lin / BN) * 4 + e) * BN + lin % BN] = bv[i][e];
        } else {
          int kr = lin / (BN / 4), c4 = lin % (BN / 4);
          *reinterpret_cast<f32x4*>(&Bs[kr * BN + c4 * 4]) = bv[i];
        }
      }
      __syncthreads();
      // request the next stage before multiplying this one (the last iteration re-reads its own stage: a conditionally
      // assigned staging array lands in scratch)
      if (st + 1 < nst) {
        lc0 += BKT;
        if (lc0 >= Cin) {
          lc0 = 0;
          sw = true;
        }
      }
      load_stage();
      f32x4 fa[2][TM];
      float fb[2][TN][4];
      auto read_frag = [&](int q, int u) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          fa[u][i] = *reinterpret_cast<const f32x4*>(&As[(wr * RW + i * 32 + r) * LDAT + 8 * q + 4 * h]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (TN == 2) {
            const f32x2 bb = *reinterpret_cast<const f32x2*>(&Bs[(8 * q + 4 * h + e) * BN + wc * CW + 2 * r]);
            fb[u][0][e] = bb[0];
            fb[u][TN - 1][e] = bb[1];
          } else {
            fb[u][0][e] = Bs[(8 * q + 4 * h + e) * BN + wc * CW + r];
          }
        }
      };
      read_frag(0, 0);
      if (prio) __builtin_amdgcn_s_setprio(1);
      // (r2: sched_group_barrier pins that issue the LDS reads of step q+1 ahead of step q's MFMAs measured +-1 % on 50 of 58
      // launch shapes and -10.5 % at the VGPR limit: the fragment reads are not what the loop waits for.)
#pragma unroll
      for (int q = 0; q < BKT / 8; ++q) {
        if (q + 1 < BKT / 8) read_frag(q + 1, (q + 1) & 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const float ae = fa[q & 1][i][e];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae, fb[q & 1][j][e], acc[i][j], 0, 0, 0);
          }
        }
      }
      if (prio) __builtin_amdgcn_s_setprio(0);
    }
  }
  // epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  TR(3);
  float* dst = out + (int64_t)z * n_out * Cout + n0 + wc * CW + TN * r;
  int orow[TM][16];                              // looked up in one batch ahead of the stores
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t row = m0 + wr * RW + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      int o = -1;
      if (row < n_out) o = out_index ? out_index[row] : (int)row;      // rows are processed in mask-sorted order
      orow[i][e] = o;
    }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (orow[i][e] >= 0) {
        if (TN == 2) {
          f32x2 v = {acc[i][0][e], acc[i][TN - 1][e]};
          *reinterpret_cast<f32x2*>(dst + (int64_t)orow[i][e] * Cout) = v;
        } else {
          dst[(int64_t)orow[i][e] * Cout] = acc[i][0][e];
        }
      }
    }
  TR(5);
  TR_FLUSH(tr_units);
}

// LDS-DMA variant (r2; VERDICT r1 item 1a — double-buffered LDS, one barrier per stage): the gathered rows and the weight slab go
// from global memory STRAIGHT into LDS (`global_load_lds_dwordx4`, 1 KiB per wave instruction: 8 gathered rows x 128 B, or
// 1 KiB of a weight slab), no staging registers and no ds_write pass, into one of TWO stage buffers; a stage is
//     wait for my own DMAs -> barrier -> issue stage s+1's DMAs into the other buffer -> multiply stage s.
// The DMA's LDS image is lane-linear (wave-uniform base + lane x 16 B: MI355X guide), so the A tile cannot be padded; its
// rows are XOR-swizzled instead ON THE SOURCE SIDE: the lane that fills 16-byte slot p of row j fetches the row's slot
// p ^ ((j >> 1) & 7), and the MFMA fragment read of slot c of row j addresses slot c ^ ((j >> 1) & 7) — conflict-free for
// ds_read_b128's 16-lane groups.  Same tiles, prologue, epilogue, grid shapes and results as k_conv_mfma / _p.
template <int BM, int BN, bool HAS_NBR, int WM = 2>
__global__ __launch_bounds__(256, 2) void k_conv_glds(const float* __restrict__ in, const float* __restrict__ W,
                                                      const int* __restrict__ nbr,
                                                      const int* __restrict__ out_index, const int* __restrict__ cnt,
                                                      float* __restrict__ out, int64_t n_out, int K, int Cin, int Cout) {
  constexpr int BKT = 32;
  constexpr int WN = 4 / WM;
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
  constexpr int RW = BM / WM, CW = BN / WN;
  constexpr int AR = BM / 32;                    // row DMAs per thread per stage (8 rows per wave instruction)
  constexpr int BR = BN / 32;                    // weight DMAs per thread per stage
  constexpr int BRPI = 256 / BN;                 // weight-slab rows per wave instruction
  constexpr int STAGE = BM * BKT + BKT * BN;     // floats per stage buffer
  __shared__ __attribute__((aligned(1024))) float smem[2 * STAGE];         // ONE array (a second one costs vmcnt(0)s: guide §5)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = WM == 4 ? wave : wave >> 1, wc = WM == 4 ? 0 : wave & 1;
  const int r = lane & 31, h = lane >> 5;
  int64_t bx = blockIdx.x;
  const int n0 = blockIdx.y * BN;
  int S = gridDim.z, z = blockIdx.z;
  if (cnt) {                                     // pair mode: tile_pair_walk (conv_tile.h)
    const PairTile pt = tile_pair_walk<BM>(cnt, K, bx, z);
    bx = pt.bx; z = pt.z;
    const int64_t stride = n_out;
    n_out = cnt[z];
    if (bx * BM >= n_out) return;
    nbr += (int64_t)z * stride;
    W += (int64_t)z * Cin * Cout;
    out += (int64_t)z * stride * Cout;
    K = 1; S = 1; z = 0;
  }
  const int64_t m0 = bx * BM;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // the tile-mask word lives in stage buffer 1: nothing is written there before every wave has passed stage 0's barrier
  unsigned int kmask = tile_offset_mask<BM, HAS_NBR>(reinterpret_cast<unsigned int*>(&smem[STAGE]), nbr, m0, n_out, z, K, S, tid, lane);

  if (kmask) {
    const int nst = __popc(kmask) * (Cin / BKT);
    unsigned int rem = kmask;
    int lk = __ffs(rem) - 1;
    rem &= rem - 1;
    int lnk = rem ? __ffs(rem) - 1 : lk;
    if (rem) rem &= rem - 1;
    int lc0 = 0;
    bool sw = false;
    // this lane's part of a row DMA: row (i*4 + wave)*8 + lane/8 of the tile, LDS slot lane%8, source slot swizzled
    const int a_j = lane >> 3;
    int vcur[AR], vnxt[AR], a_src4[AR];
    int64_t arow[AR];
    bool aok[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int lrow = (i * 4 + wave) * 8 + a_j;
      const int64_t row = m0 + lrow;
      aok[i] = row < n_out;
      arow[i] = aok[i] ? row : n_out - 1;
      a_src4[i] = (((lane & 7) ^ ((lrow >> 1) & 7))) * 4;
    }
    auto fetch_idx = [&](int kk, int (&v)[AR]) {
#pragma unroll
      for (int i = 0; i < AR; ++i) v[i] = HAS_NBR ? nbr[(int64_t)kk * n_out + arow[i]] : (int)arow[i];
    };
    fetch_idx(lk, vcur);
    fetch_idx(lnk, vnxt);
    const int b_kr = lane / (BN / 4), b_c4 = lane % (BN / 4);
    auto issue_stage = [&](int buf) {
      if (sw) {
        sw = false;
        lk = lnk;
#pragma unroll
        for (int i = 0; i < AR; ++i) vcur[i] = vnxt[i];
        if (rem) {
          lnk = __ffs(rem) - 1;
          rem &= rem - 1;
        }
        fetch_idx(lnk, vnxt);
      }
      float* As = smem + buf * STAGE;
      float* Bs = As + BM * BKT;
      const float* Wk = W + (int64_t)lk * Cin * Cout;
      // every source address first (this consumes the index registers: hipcc waits vmcnt(0) at the first use of an ordinary
      // load's result while a DMA is in flight — here nothing is, the loop-top wait has just drained the queue), then the
      // DMAs back to back
      const float* asrc[AR];
      const float* bsrc[BR];
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const bool ok = vcur[i] >= 0 && aok[i];
        const int64_t off = ok ? (int64_t)vcur[i] * Cin + lc0 : 0;
        asrc[i] = (ok ? in : g_zero_row) + off + a_src4[i];
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) bsrc[i] = Wk + (int64_t)(lc0 + (i * 4 + wave) * BRPI + b_kr) * Cout + n0 + b_c4 * 4;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < BR; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)bsrc[i],
                                         (__attribute__((address_space(3))) void*)(Bs + (i * 4 + wave) * BRPI * BN), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < AR; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)asrc[i],
                                         (__attribute__((address_space(3))) void*)(As + (i * 4 + wave) * 8 * BKT), 16, 0, 0);
    };
    issue_stage(0);
    const int fsw = (r >> 1) & 7;                // the fragment rows' swizzle (tile row = 32-aligned base + r)
    for (int st = 0; st < nst; ++st) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my DMAs of stage st have landed ...
      __syncthreads();                                      // ... and everyone's; stage st-1 is fully consumed
      if (st + 1 < nst) {
        lc0 += BKT;
        if (lc0 >= Cin) {
          lc0 = 0;
          sw = true;
        }
        issue_stage((st + 1) & 1);
      }
      const float* As = smem + (st & 1) * STAGE;
      const float* Bs = As + BM * BKT;
      f32x4 fa[2][TM];
      float fb[2][TN][4];
      auto read_frag = [&](int q, int u) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          fa[u][i] = *reinterpret_cast<const f32x4*>(&As[(wr * RW + i * 32 + r) * BKT + 4 * ((2 * q + h) ^ fsw)]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (TN == 2) {
            const f32x2 bb = *reinterpret_cast<const f32x2*>(&Bs[(8 * q + 4 * h + e) * BN + wc * CW + 2 * r]);
            fb[u][0][e] = bb[0];
            fb[u][TN - 1][e] = bb[1];
          } else {
            fb[u][0][e] = Bs[(8 * q + 4 * h + e) * BN + wc * CW + r];
          }
        }
      };
      read_frag(0, 0);
#pragma unroll
      for (int q = 0; q < BKT / 8; ++q) {
        if (q + 1 < BKT / 8) read_frag(q + 1, (q + 1) & 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const float ae = fa[q & 1][i][e];
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae, fb[q & 1][j][e], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  }
  float* dst = out + (int64_t)z * n_out * Cout + n0 + wc * CW + TN * r;
  int orow[TM][16];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t row = m0 + wr * RW + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      int o = -1;
      if (row < n_out) o = out_index ? out_index[row] : (int)row;
      orow[i][e] = o;
    }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (orow[i][e] >= 0) {
        if (TN == 2) {
          f32x2 v = {acc[i][0][e], acc[i][TN - 1][e]};
          *reinterpret_cast<f32x2*>(dst + (int64_t)orow[i][e] * Cout) = v;
        } else {
          dst[(int64_t)orow[i][e] * Cout] = acc[i][0][e];
        }
      }
    }
}

// generic fallback (any Cin/Cout): one thread per (row, cout).  Used for the Cin=3 stem and as the
// cross-check path of the parity tests (FC_CONV_FMA).
__global__ void k_conv_fma(const float* __restrict__ in, const float* __restrict__ W, const int* __restrict__ nbr,
                           float* __restrict__ out, int64_t n_out, int K, int Cin, int Cout, int wt) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out * Cout) return;
  int64_t o = t / Cout;
  int co = (int)(t % Cout);
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    int i = nbr ? nbr[(int64_t)k * n_out + o] : (int)o;
    if (i < 0) continue;
    const float* x = in + (int64_t)i * Cin;
    const float* w = W + (int64_t)k * Cin * Cout + (wt ? (int64_t)co * Cin : co);
    const int64_t ws = wt ? 1 : Cout;             // wt: W[k] stored (Cout, Cin)
    for (int ci = 0; ci < Cin; ++ci) acc = fmaf(x[ci], w[ci * ws], acc);
  }
  out[t] = acc;
}
