// The stem convolution (3 -> 64 channels): forward, and the weight gradient with gathered or saved inputs.  Included by conv.hip.
#pragma once

// ------------------------------------------------------------------------------------------------
// Stem convolution (Cin = 3 colour channels -> 64, k3 s2; me_resnet.py:19-21): bound by the 148 MB output
// write.  64 output rows per workgroup; the 27x3 gathered inputs of every row and the whole (81,64) kernel sit in
// LDS, zero-padded to a reduction depth of 96, and each wave multiplies one 32x32 tile on the matrix cores.
#define STEM_CIN 3
#define STEM_COUT 64
#define STEM_ROWS 64
#define STEM_FWD_LDA 97
#define STEM_COL_LD 84      // row stride of the saved gathered inputs: 27 x 3 = 81 floats, padded to 21 float4
__global__ __launch_bounds__(256) void k_stem_fwd(const float* __restrict__ in, const float* __restrict__ W,
                                                  const int* __restrict__ nbr, float* __restrict__ out,
                                                  float* __restrict__ col, int64_t n_out, int K) {
  // out[64 rows][64] = A[64][81 -> 96] x W[96][64] on the matrix cores: one 32x32 tile per wave, 48 MFMA steps.
  extern __shared__ float sm[];
  constexpr int SLD = STEM_FWD_LDA;          // odd row stride -> conflict-free column reads of A
  const int KC = K * STEM_CIN;
  float* in_s = sm;                          // [STEM_ROWS][SLD]   (columns >= KC are zero)
  float* W_s = sm + STEM_ROWS * SLD;         // [96][64]           (rows >= KC are zero)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * STEM_ROWS;
  for (int t = tid; t < STEM_ROWS * (SLD - KC); t += 256) {
    int row = t / (SLD - KC), c = KC + t % (SLD - KC);
    in_s[row * SLD + c] = 0.f;
  }
  for (int t = tid; t < STEM_ROWS * K; t += 256) {
    int k = t / STEM_ROWS, row = t % STEM_ROWS;
    int64_t o = m0 + row;
    int64_t oc = o < n_out ? o : n_out - 1;
    int i = nbr[(int64_t)k * n_out + oc];
    if (o >= n_out) i = -1;
    const float* src = i < 0 ? g_zero_row : in + (int64_t)i * 3;
    float a = src[0], b = src[1], c = src[2];       // (r2: one 12-byte load instead of three dwords is no faster)
    in_s[row * SLD + k * 3] = a; in_s[row * SLD + k * 3 + 1] = b; in_s[row * SLD + k * 3 + 2] = c;
  }
  for (int t = tid; t < 96 * 16; t += 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t < KC * 16) v = reinterpret_cast<const f32x4*>(W)[t];
    reinterpret_cast<f32x4*>(W_s)[t] = v;
  }
  __syncthreads();
  if (col) {
    // training: the gathered inputs of the tile go out as rows of `col` (n_out, 84) — the weight gradient then streams them
    // instead of repeating 27 scattered 12-byte reads per output row (r2: 390 -> ~100 us; the forward pays one 195 MB write)
    for (int t = tid; t < STEM_ROWS * (STEM_COL_LD / 4); t += 256) {
      const int row = t / (STEM_COL_LD / 4), c = (t % (STEM_COL_LD / 4)) * 4;
      const int64_t o = m0 + row;
      if (o < n_out) {
        const float* sp = in_s + row * SLD + c;
        f32x4 v = {sp[0], sp[1], sp[2], sp[3]};
        *reinterpret_cast<f32x4*>(col + o * STEM_COL_LD + c) = v;
      }
    }
  }
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const float* ap = in_s + (wr * 32 + r) * SLD + h;
  const float* bp = W_s + h * 64 + wc * 32 + r;
#pragma unroll 8
  for (int sidx = 0; sidx < 48; ++sidx)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * sidx], bp[2 * sidx * 64], acc, 0, 0, 0);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    int64_t o = m0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (o < n_out) out[o * 64 + wc * 32 + r] = acc[e];
  }
}

// stem wgrad on the matrix cores: part[block][j][co] = sum over the block's rows of A[row][j] * gout[row][co], with
// A[row][j = 3k+c] = in[nbr[k][row]][c] staged in LDS (81 real columns padded to 96 = 3 MFMA tiles, gout 64 = 2 tiles).
// Each of the 4 waves owns a quarter of every 64-row chunk as its reduction slice and all 6 tiles; the four partial
// tiles are summed through LDS in wave order (deterministic) at the end.
#define STEM_JP 96
__global__ __launch_bounds__(256) void k_stem_wgrad(const float* __restrict__ in, const float* __restrict__ gout,
                                                    const int* __restrict__ nbr, float* __restrict__ part, int64_t n_out,
                                                    int K, int64_t rows_per_block) {
  extern __shared__ float sm[];
  const int KC = K * STEM_CIN;
  float* in_s = sm;                          // [STEM_ROWS][STEM_JP]   (columns >= KC stay zero)
  float* g_s = sm + STEM_ROWS * STEM_JP;     // [STEM_ROWS][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  int64_t r_end = r_begin + rows_per_block;
  if (r_end > n_out) r_end = n_out;
  for (int t = tid; t < STEM_ROWS * STEM_JP; t += 256) in_s[t] = 0.f;
  f32x16 acc[3][2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // register-prefetch pipeline (as k_conv_mfma): the 27 x 3 gathered inputs and the gout rows of chunk t+1 are in flight
  // while chunk t is multiplied (r2: without it the index -> gather chain of every 64-row chunk was exposed: 0.6 TB/s)
  constexpr int NG = (STEM_ROWS * 27 + 255) / 256;          // gathers per thread per chunk (K <= 27)
  float pa[NG][3];
  f32x4 pg[4];
  auto load_chunk = [&](int64_t rb) {
    int idx[NG];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
      const int t = tid + 256 * u;
      const int k = t / STEM_ROWS, row = t % STEM_ROWS;
      const int64_t o = rb + row;
      const int64_t oc = o < r_end ? o : r_end - 1;
      const int kk = k < K ? k : K - 1;
      int i = nbr[(int64_t)kk * n_out + oc];
      idx[u] = (o < r_end && k < K) ? i : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = tid + 256 * u;
      const int64_t o = rb + (t >> 4);
      const float* gp = o < r_end ? gout + o * 64 + (t & 15) * 4 : g_zero_row;
      pg[u] = *reinterpret_cast<const f32x4*>(gp);
    }
#pragma unroll
    for (int u = 0; u < NG; ++u) {
      const float* src = idx[u] < 0 ? g_zero_row : in + (int64_t)idx[u] * 3;
      pa[u][0] = src[0]; pa[u][1] = src[1]; pa[u][2] = src[2];
    }
  };
  if (r_begin < r_end) load_chunk(r_begin);
  for (int64_t rb = r_begin; rb < r_end; rb += STEM_ROWS) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NG; ++u) {
      const int t = tid + 256 * u;
      const int k = t / STEM_ROWS, row = t % STEM_ROWS;
      if (k < K) {
        in_s[row * STEM_JP + k * 3] = pa[u][0]; in_s[row * STEM_JP + k * 3 + 1] = pa[u][1]; in_s[row * STEM_JP + k * 3 + 2] = pa[u][2];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) reinterpret_cast<f32x4*>(g_s)[tid + 256 * u] = pg[u];
    __syncthreads();
    load_chunk(rb + STEM_ROWS < r_end ? rb + STEM_ROWS : rb);          // unconditional (see k_conv_mfma)
#pragma unroll
    for (int sidx = 0; sidx < 8; ++sidx) {
      const int row = wave * 16 + 2 * sidx + h;
      float a[3], b[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) a[i] = in_s[row * STEM_JP + i * 32 + r];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = g_s[row * 64 + j * 32 + r];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // cross-wave sum in wave order through LDS ([96][64] floats = 24 KB, reusing the staging area)
  __syncthreads();
  float* red = sm;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            int jj = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h, co = j * 32 + r;
            float v = acc[i][j][e];
            if (w > 0) v += red[jj * 64 + co];
            red[jj * 64 + co] = v;
          }
    }
    __syncthreads();
  }
  float* dst = part + (int64_t)blockIdx.x * KC * 64;
  for (int t = tid; t < KC * 64; t += 256) dst[t] = red[t];
}

// The same reduction with the gathered inputs read back from `col` (k_stem_fwd) — no neighbour table, no gathers.
__global__ __launch_bounds__(256) void k_stem_wgrad_col(const float* __restrict__ col, const float* __restrict__ gout,
                                                        float* __restrict__ part, int64_t n_out, int K, int64_t rows_per_block) {
  extern __shared__ float sm[];
  const int KC = K * STEM_CIN;
  float* in_s = sm;                          // [STEM_ROWS][STEM_JP]   (columns >= KC stay zero)
  float* g_s = sm + STEM_ROWS * STEM_JP;     // [STEM_ROWS][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  int64_t r_end = r_begin + rows_per_block;
  if (r_end > n_out) r_end = n_out;
  for (int t = tid; t < STEM_ROWS * STEM_JP; t += 256) in_s[t] = 0.f;
  f32x16 acc[3][2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // the gathered inputs come as rows of `col` (saved by k_stem_fwd): two coalesced streams, prefetched one chunk ahead
  constexpr int NC = (STEM_ROWS * (STEM_COL_LD / 4) + 255) / 256;      // float4 per thread per chunk
  f32x4 pc[NC], pg[4];
  auto load_chunk = [&](int64_t rb) {
#pragma unroll
    for (int u = 0; u < NC; ++u) {
      const int t = tid + 256 * u;
      const int row = t / (STEM_COL_LD / 4), c = (t % (STEM_COL_LD / 4)) * 4;
      const int64_t o = rb + row;
      const float* cp = (o < r_end && row < STEM_ROWS) ? col + o * STEM_COL_LD + c : g_zero_row;
      pc[u] = *reinterpret_cast<const f32x4*>(cp);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = tid + 256 * u;
      const int64_t o = rb + (t >> 4);
      const float* gp = o < r_end ? gout + o * 64 + (t & 15) * 4 : g_zero_row;
      pg[u] = *reinterpret_cast<const f32x4*>(gp);
    }
  };
  if (r_begin < r_end) load_chunk(r_begin);
  for (int64_t rb = r_begin; rb < r_end; rb += STEM_ROWS) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NC; ++u) {
      const int t = tid + 256 * u;
      const int row = t / (STEM_COL_LD / 4), c = (t % (STEM_COL_LD / 4)) * 4;
      if (row < STEM_ROWS) *reinterpret_cast<f32x4*>(&in_s[row * STEM_JP + c]) = pc[u];      // columns 84..95 stay zero
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) reinterpret_cast<f32x4*>(g_s)[tid + 256 * u] = pg[u];
    __syncthreads();
    load_chunk(rb + STEM_ROWS < r_end ? rb + STEM_ROWS : rb);          // unconditional (see k_conv_mfma)
#pragma unroll
    for (int sidx = 0; sidx < 8; ++sidx) {
      const int row = wave * 16 + 2 * sidx + h;
      float a[3], b[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) a[i] = in_s[row * STEM_JP + i * 32 + r];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = g_s[row * 64 + j * 32 + r];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // cross-wave sum in wave order through LDS ([96][64] floats = 24 KB, reusing the staging area)
  __syncthreads();
  float* red = sm;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            int jj = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h, co = j * 32 + r;
            float v = acc[i][j][e];
            if (w > 0) v += red[jj * 64 + co];
            red[jj * 64 + co] = v;
          }
    }
    __syncthreads();
  }
  float* dst = part + (int64_t)blockIdx.x * KC * 64;
  for (int t = tid; t < KC * 64; t += 256) dst[t] = red[t];
}
