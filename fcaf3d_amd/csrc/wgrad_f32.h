// The fp32 weight-gradient kernels — k_wgrad_mfma, k_wgrad_mfma_p, k_wgrad_multi on the matrix cores, the untiled k_wgrad_fma.
// Included by conv.hip (after conv_f32.h: BK), which launches them (launch_wgrad) and sums their partial products.
#pragma once

// ------------------------------------------------------------------------------------------------
// wgrad:  gW[k][ci][co] = sum_o in[nbr[k][o]][ci] * gout[o][co]
// GEMM with M = Cin, N = Cout and the reduction over output rows, split over `S` row ranges whose
// partial products are written to the workspace and summed by k_wgrad_reduce in a fixed order
// (deterministic, no atomics).
// PAIRS: `nbr` / `row_index` are the exact pair lists of fc_kernel_map_pairs (input row, output row; `cnt[k]` valid
// entries per offset) and the reduction runs over the pairs only, split evenly over gridDim.x on the device.
template <int BMc, int BNc, bool HAS_NBR, int BKR, bool PAIRS>
__global__ __launch_bounds__(256, 2) void k_wgrad_mfma(const float* __restrict__ in, const float* __restrict__ gout,
                                                    const int* __restrict__ nbr, const int* __restrict__ row_index,
                                                    const int* __restrict__ cnt,
                                                    float* __restrict__ part, int64_t n_out, int K, int Cin, int Cout,
                                                    int64_t rows_per_split) {
  constexpr int TM = BMc / 64, TN = BNc / 64;
  constexpr int AR = BMc * BKR / 1024, GR = BNc * BKR / 1024;    // float4 loads per thread per stage (BKR rows)
  __shared__ __attribute__((aligned(16))) float As[BKR * BMc];
  __shared__ __attribute__((aligned(16))) float Gs[BKR * BNc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const WgradTile wt = wgrad_tile<BMc, BNc>(Cin, Cout, 1);
  const int k = wt.k0, ci0 = wt.ci0, co0 = wt.co0;
  const WgradRows rows = wgrad_rows<PAIRS, BKR>(cnt, k, n_out, rows_per_split);
  const int64_t r_begin = rows.begin, r_end = rows.end;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // register-prefetch pipeline: the gathers + gout rows of chunk t+1 are in flight while chunk t is multiplied.
  // (Measured r1: processing wgrad rows in occupancy-mask order with per-chunk skipping LOSES 15-35 % — gout rows stop
  //  being sequential and the skip test costs a barrier per chunk — so wgrad always walks rows in natural order
  //  and row_index must be NULL.)
  f32x4 av[AR], gv[GR];
  auto load_chunk = [&](int64_t rb) {        // branch-free, batched (see k_conv_mfma): indices, gout rows, gathers
    int src[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int lin = tid + 256 * i;
      int rr = lin / (BMc / 4);
      int64_t row = rb + rr;
      int64_t rc = row < r_end ? row : r_end - 1;
      int t = HAS_NBR ? nbr[(int64_t)k * n_out + rc] : (int)rc;      // compile-time: no null test between the loads
      src[i] = row < r_end ? t : -1;
    }
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      int lin = tid + 256 * i;
      int rr = lin / (BNc / 4), c4 = lin % (BNc / 4);
      int64_t row = rb + rr;
      int64_t rc = row < r_end ? row : r_end - 1;
      if (PAIRS) rc = row_index[(int64_t)k * n_out + rc];
      const float* gp = row < r_end ? gout + rc * Cout + co0 + c4 * 4 : g_zero_row + (c4 & 15) * 4;
      gv[i] = *reinterpret_cast<const f32x4*>(gp);
    }
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int lin = tid + 256 * i;
      int c4 = lin % (BMc / 4);
      const float* ap = src[i] < 0 ? g_zero_row + (c4 & 15) * 4 : in + (int64_t)src[i] * Cin + ci0 + c4 * 4;
      av[i] = *reinterpret_cast<const f32x4*>(ap);
    }
  };
  if (r_begin < r_end) load_chunk(r_begin);
  for (int64_t rb = r_begin; rb < r_end; rb += BKR) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int lin = tid + 256 * i;
      int rr = lin / (BMc / 4), c4 = lin % (BMc / 4);
      *reinterpret_cast<f32x4*>(&As[rr * BMc + c4 * 4]) = av[i];
    }
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      int lin = tid + 256 * i;
      int rr = lin / (BNc / 4), c4 = lin % (BNc / 4);
      *reinterpret_cast<f32x4*>(&Gs[rr * BNc + c4 * 4]) = gv[i];
    }
    __syncthreads();
    if (rb + BKR < r_end) load_chunk(rb + BKR);
#pragma unroll
    for (int q = 0; q < BKR / 8; ++q) {
      float a[TM][4], b[TN][4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i][e] = As[(8 * q + 4 * h + e) * BMc + wr * (BMc / 2) + i * 32 + r];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j][e] = Gs[(8 * q + 4 * h + e) * BNc + wc * (BNc / 2) + j * 32 + r];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
  }
  float* dst = part + ((int64_t)blockIdx.x * K + k) * Cin * Cout;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        int row = ci0 + wr * (BMc / 2) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        int col = co0 + wc * (BNc / 2) + j * 32 + r;
        dst[(int64_t)row * Cout + col] = acc[i][j][e];
      }
}

// Deeper-pipelined weight gradient (64-channel Cin tile x BNc, 32-row chunks; same partial layout and results as
// k_wgrad_mfma).  r2 ISA reading of the pair-list path of k_wgrad_mfma: every gout row of a chunk went through its own
// `row index load -> s_waitcnt vmcnt(0) -> row load` chain (a bounds branch per load) — five exposed round trips in front of
// 2 048 MFMA cycles.  Here the (input row, output row) indices of chunk t+2 are requested while chunk t+1's rows are
// (branch-free: out-of-range rows read the zero row), and the MFMA fragments of 8-row step q+1 are read from LDS while step
// q multiplies.  3 waves per SIMD.
template <int BNc, bool HAS_NBR, bool PAIRS>
__global__ __launch_bounds__(256, 3) void k_wgrad_mfma_p(const float* __restrict__ in, const float* __restrict__ gout,
                                                          const int* __restrict__ nbr, const int* __restrict__ row_index,
                                                          const int* __restrict__ cnt, float* __restrict__ part,
                                                          int64_t n_out, int K, int Cin, int Cout, int64_t rows_per_split) {
  constexpr int BMc = 64, BKR = 32;
  constexpr int TN = BNc / 64;
  constexpr int AR = 2, GR = BNc * BKR / 1024;   // float4 loads per thread per chunk
  __shared__ __attribute__((aligned(16))) float As[BKR * BMc];
  __shared__ __attribute__((aligned(16))) float Gs[BKR * BNc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const WgradTile wt = wgrad_tile<BMc, BNc>(Cin, Cout, 1);
  const int k = wt.k0, ci0 = wt.ci0, co0 = wt.co0;
  const WgradRows rows = wgrad_rows<PAIRS, BKR>(cnt, k, n_out, rows_per_split);
  const int64_t r_begin = rows.begin, r_end = rows.end;

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  if (r_begin < r_end) {
    const int* tab_in = HAS_NBR ? nbr + (int64_t)k * n_out : nullptr;
    const int* tab_out = PAIRS ? row_index + (int64_t)k * n_out : nullptr;
    const int a_rr[AR] = {tid / 16, (tid + 256) / 16};
    const int a_c4 = tid % 16;
    int g_rr[GR];
#pragma unroll
    for (int i = 0; i < GR; ++i) g_rr[i] = (tid + 256 * i) / (BNc / 4);
    const int g_c4 = tid % (BNc / 4);
    // indices of a chunk (raw table entries; rows beyond the range are clamped here and zeroed at the row load)
    int ia[AR], ig[GR], ian[AR], ign[GR];
    auto fetch_idx = [&](int64_t rb, int (&va)[AR], int (&vg)[GR]) {
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        int64_t row = rb + a_rr[i];
        if (row >= r_end) row = r_end - 1;
        va[i] = HAS_NBR ? tab_in[row] : (int)row;
      }
#pragma unroll
      for (int i = 0; i < GR; ++i) {
        int64_t row = rb + g_rr[i];
        if (row >= r_end) row = r_end - 1;
        vg[i] = PAIRS ? tab_out[row] : (int)row;
      }
    };
    f32x4 av[AR], gv[GR];
    auto load_rows = [&](int64_t rb) {          // rows of chunk rb from the indices in ia / ig
#pragma unroll
      for (int i = 0; i < GR; ++i) {
        const bool ok = rb + g_rr[i] < r_end;
        const float* gp = ok ? gout + (int64_t)ig[i] * Cout + co0 + g_c4 * 4 : g_zero_row + (g_c4 & 15) * 4;
        gv[i] = *reinterpret_cast<const f32x4*>(gp);
      }
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const bool ok = rb + a_rr[i] < r_end && ia[i] >= 0;
        const float* ap = ok ? in + (int64_t)ia[i] * Cin + ci0 + a_c4 * 4 : g_zero_row + a_c4 * 4;
        av[i] = *reinterpret_cast<const f32x4*>(ap);
      }
    };
    fetch_idx(r_begin, ia, ig);
    fetch_idx(r_begin + BKR < r_end ? r_begin + BKR : r_begin, ian, ign);
    load_rows(r_begin);
    for (int64_t rb = r_begin; rb < r_end; rb += BKR) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < AR; ++i) *reinterpret_cast<f32x4*>(&As[a_rr[i] * BMc + a_c4 * 4]) = av[i];
#pragma unroll
      for (int i = 0; i < GR; ++i) *reinterpret_cast<f32x4*>(&Gs[g_rr[i] * BNc + g_c4 * 4]) = gv[i];
      __syncthreads();
      // chunk t+1: its indices arrived a chunk ago; request chunk t+2's indices, then t+1's rows (unconditional: past the
      // end the last chunk is re-read and never used)
      const int64_t nb = rb + BKR < r_end ? rb + BKR : rb;
      const int64_t nnb = nb + BKR < r_end ? nb + BKR : nb;
#pragma unroll
      for (int i = 0; i < AR; ++i) ia[i] = ian[i];
#pragma unroll
      for (int i = 0; i < GR; ++i) ig[i] = ign[i];
      fetch_idx(nnb, ian, ign);
      load_rows(nb);
      float fa[2][4], fb[2][TN][4];
      auto read_frag = [&](int q, int u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          fa[u][e] = As[(8 * q + 4 * h + e) * BMc + wr * 32 + r];
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[u][j][e] = Gs[(8 * q + 4 * h + e) * BNc + wc * (BNc / 2) + j * 32 + r];
        }
      };
      read_frag(0, 0);
#pragma unroll
      for (int q = 0; q < BKR / 8; ++q) {
        if (q + 1 < BKR / 8) read_frag(q + 1, (q + 1) & 1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q & 1][e], fb[q & 1][j][e], acc[j], 0, 0, 0);
      }
    }
  }
  float* dst = part + ((int64_t)blockIdx.x * K + k) * Cin * Cout;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = ci0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const int col = co0 + wc * (BNc / 2) + j * 32 + r;
      dst[(int64_t)row * Cout + col] = acc[j][e];
    }
}

// Dense-table weight gradient with KO kernel offsets per workgroup sharing ONE gout chunk.  With 64 input channels the
// one-offset kernel above moves 24 KB (8 KB gathered rows + 16 KB of gout) per 0.5 MFLOP chunk = 22 FLOP/B and sits on
// the fabric at ~4.3 TB/s (r2 measurement: 88 TF on the 437k-row level); re-using the staged gout rows for KO = 3 offsets
// lifts that to 39 FLOP/B.  64 x BNc tile of gW[k] per offset, 4 waves as 2 x 2, reduction over rows in natural order.
template <int BNc, int KO>
__global__ __launch_bounds__(256, (BNc == 128) ? 2 : 3) void k_wgrad_multi(const float* __restrict__ in, const float* __restrict__ gout,
                                                         const int* __restrict__ nbr, float* __restrict__ part, int64_t n_out,
                                                         int K, int Cin, int Cout, int64_t rows_per_split) {
  constexpr int TN = BNc / 64;
  constexpr int GR = BNc * 32 / 1024;            // float4 gout loads per thread per 32-row chunk
  __shared__ __attribute__((aligned(16))) float As[KO][32 * 64];
  __shared__ __attribute__((aligned(16))) float Gs[32 * BNc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const WgradTile wt = wgrad_tile<64, BNc>(Cin, Cout, KO);
  const int k0 = wt.k0, ci0 = wt.ci0, co0 = wt.co0;
  const WgradRows rows = wgrad_rows<false, 32>(nullptr, k0, n_out, rows_per_split);
  const int64_t r_begin = rows.begin, r_end = rows.end;

  f32x16 acc[KO][TN];
#pragma unroll
  for (int o = 0; o < KO; ++o)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[o][j][e] = 0.f;

  f32x4 av[KO][2], gv[GR];
  auto load_chunk = [&](int64_t rb) {        // branch-free, batched: indices, gout rows, gathers
    int src[KO][2];
#pragma unroll
    for (int o = 0; o < KO; ++o)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rr = (tid + 256 * i) / 16;
        const int64_t row = rb + rr;
        const int64_t rc = row < r_end ? row : r_end - 1;
        const int kk = k0 + o < K ? k0 + o : K - 1;
        const int t = nbr[(int64_t)kk * n_out + rc];
        src[o][i] = (row < r_end && k0 + o < K) ? t : -1;
      }
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      const int lin = tid + 256 * i;
      const int rr = lin / (BNc / 4), c4 = lin % (BNc / 4);
      const int64_t row = rb + rr;
      const float* gp = row < r_end ? gout + row * Cout + co0 + c4 * 4 : g_zero_row + (c4 & 15) * 4;
      gv[i] = *reinterpret_cast<const f32x4*>(gp);
    }
#pragma unroll
    for (int o = 0; o < KO; ++o)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c4 = (tid + 256 * i) % 16;
        const float* ap = src[o][i] < 0 ? g_zero_row + c4 * 4 : in + (int64_t)src[o][i] * Cin + ci0 + c4 * 4;
        av[o][i] = *reinterpret_cast<const f32x4*>(ap);
      }
  };
  if (r_begin < r_end) load_chunk(r_begin);
  const bool prio = g_fc_prio == 0;               // see g_fc_prio (mode 1: forward / backward-data kernels only)
  for (int64_t rb = r_begin; rb < r_end; rb += 32) {
    __syncthreads();
#pragma unroll
    for (int o = 0; o < KO; ++o)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int lin = tid + 256 * i;
        *reinterpret_cast<f32x4*>(&As[o][(lin / 16) * 64 + (lin % 16) * 4]) = av[o][i];
      }
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      const int lin = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&Gs[(lin / (BNc / 4)) * BNc + (lin % (BNc / 4)) * 4]) = gv[i];
    }
    __syncthreads();
    load_chunk(rb + 32 < r_end ? rb + 32 : rb);            // unconditional (see k_conv_mfma)
    if (prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float b[TN][4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j][e] = Gs[(8 * q + 4 * h + e) * BNc + wc * (BNc / 2) + j * 32 + r];
#pragma unroll
      for (int o = 0; o < KO; ++o) {
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = As[o][(8 * q + 4 * h + e) * 64 + wr * 32 + r];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[o][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[j][e], acc[o][j], 0, 0, 0);
      }
    }
    if (prio) __builtin_amdgcn_s_setprio(0);
  }
#pragma unroll
  for (int o = 0; o < KO; ++o) {
    if (k0 + o >= K) break;
    float* dst = part + ((int64_t)blockIdx.x * K + k0 + o) * Cin * Cout;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = ci0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int col = co0 + wc * (BNc / 2) + j * 32 + r;
        dst[(int64_t)row * Cout + col] = acc[o][j][e];
      }
  }
}

// generic wgrad: block = (row range, k); each thread owns (ci,co) pairs strided by blockDim.
__global__ void k_wgrad_fma(const float* __restrict__ in, const float* __restrict__ gout, const int* __restrict__ nbr,
                            float* __restrict__ part, int64_t n_out, int K, int Cin, int Cout, int64_t rows_per_split) {
  const int k = blockIdx.y;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_split;
  int64_t r_end = r_begin + rows_per_split;
  if (r_end > n_out) r_end = n_out;
  float* dst = part + ((int64_t)blockIdx.x * K + k) * Cin * Cout;
  for (int p = threadIdx.x; p < Cin * Cout; p += blockDim.x) {
    int ci = p / Cout, co = p % Cout;
    float acc = 0.f;
    for (int64_t o = r_begin; o < r_end; ++o) {
      int i = nbr ? nbr[(int64_t)k * n_out + o] : (int)o;
      if (i >= 0) acc = fmaf(in[(int64_t)i * Cin + ci], gout[o * Cout + co], acc);
    }
    dst[p] = acc;
  }
}
