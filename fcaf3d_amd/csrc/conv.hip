// Sparse convolution on gfx950 as an OUTPUT-STATIONARY implicit GEMM over a dense neighbour
// table nbr[k][o] (built by fc_kernel_map):
//     out[o, :] = sum_k  in[nbr[k][o], :] @ W[k]            (rows with nbr < 0 contribute zero)
// Each output row is written exactly once (no atomics, deterministic).  The same kernel computes
// dgrad (gather over the transposed table with W[k]^T) and, with nbr == NULL (identity), the dense
// GEMMs of the generative transposed convolution and the 1x1 head convolutions.
//
// fp32 in / fp32 accumulate on the matrix cores: v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain).
// Workgroup = 256 threads = 4 wave64 in a 2x2 grid; gathered input rows and the W[k] slab are
// staged through LDS with 16-byte coalesced loads.
//
// Replaces MinkowskiEngine's ConvolutionForward/Backward (and ConvolutionTranspose, 1x1 mm) called
// from me_resnet.py:19-21,56-62, BasicBlock, fcaf3d_neck_with_head.py:52,60-69,83-85,257-263.
//
// This file: the process switches, the amax pass, the fixed-order sums, launch_conv / launch_wgrad and the entry points.  The kernels:
// conv_f32.h / wgrad_f32.h (fp32), conv_stem.h, conv_x6.h / wgrad_x6.h / conv_h3r.h (split operands); what they share: conv_tile.h.
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"
#ifdef FC_TRACE
__device__ unsigned long long* g_trace_buf_lds;
__device__ int g_trace_cap_lds;
extern "C" int fc_debug_trace_lds(unsigned long long* buf, int cap) {
  FC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_buf_lds), &buf, sizeof(buf)));
  FC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_cap_lds), &cap, sizeof(cap)));
  return FC_OK;
}
#define TR_BUF g_trace_buf_lds
#define TR_CAP g_trace_cap_lds
#endif
#include "fc_trace.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector: struct float4 copies lower to memcpy and
                                                          // pin the prefetch registers in scratch (r1 finding)

__device__ __attribute__((aligned(16))) float g_zero_row[64];   // what an absent neighbour gathers from (BKT <= 64 floats)

// Wave priority around the MFMA block of a stage (s_setprio 1 ... 0): a wave that is multiplying goes ahead of the waves
// that are staging, so the resident waves of a SIMD drift apart instead of all meeting their barriers together.  r2,
// same box, instruction-identical otherwise: +2.4...3.4 % on the 441k-row launches, +3 % on the 64k-row level, +4 % on
// the 3.5k-row pair mode, +1...4 % on k_wgrad_multi; the one-offset weight-gradient kernels LOSE 2...7 % and the LDS-DMA
// kernel up to 9 %, so those stay at priority 0.  Static per-workgroup priorities (by block index, by hardware wave slot):
// +1 % or -10 %.  g_fc_prio = -1 switches it off (A/B: tools/nbench --prio -1; not a C-ABI entry point).
__device__ int g_fc_prio;
extern "C" int fc_debug_set_prio(int mode) {
  FC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_fc_prio), &mode, sizeof(mode)));
  return FC_OK;
}

// r5, SURVEY.md 8(f) rank 4 "bf16 fast mode" — a flagged NON-PARITY extra, never the benchmark's `value`: with the switch on,
// the split-bf16 launches that read a weight image (k_conv_x6 BSRC 2, 128-row tiles) and k_wgrad_x6t run their FAST variants:
// ONLY plane 0 of either operand = the operand rounded to nearest bf16 (x6_rn2), fp32 accumulate — one v_mfma_f32_32x32x16_bf16
// per 32x32x16 block instead of six.  Process-global host switch (FC_BF16=1 / fc_set_bf16_fast); default off.
static int g_bf16_fast = 0;
extern "C" int fc_set_bf16_fast(int on) {
  g_bf16_fast = on ? 1 : 0;
  return FC_OK;
}

// r6: how the split kernels cut an fp32 operand (conv_x6.h): 2 = two fp16 pieces, three products ("h3", the default), 0 = three
// bf16 pieces, six products (r3-r5).  Process-global (fc_set_split_mode): weight images are built in the mode
// that is current when fc_x6_weight_image(s) runs and MUST be read in that mode — whoever switches rebuilds them (functional.py
// set_split_mode does).  The bf16 fast mode reads plane 0 of a SIX-product image: fc_set_bf16_fast(1) implies mode 0 while it is on.
static int g_split_mode = 2;
static inline int split_mode() { return g_bf16_fast ? 0 : g_split_mode; }
extern "C" int fc_set_split_mode(int mode) {
  if (mode != 0 && mode != 2) return FC_EINVAL;
  g_split_mode = mode;
  return FC_OK;
}
extern "C" int fc_get_split_mode(void) { return split_mode(); }
static int g_h3r = 1;                            // which h3 launches run the register-operand kernel (conv_route.h)
extern "C" int fc_debug_set_h3r(int mode) {
  if (mode < 0 || mode > 2) return FC_EINVAL;
  g_h3r = mode;
  return FC_OK;
}

#include <mutex>
#include "conv_tile.h"
#include "conv_f32.h"
#include "wgrad_f32.h"
#include "conv_stem.h"
#include "conv_x6.h"
#include "wgrad_x6.h"
#include "conv_h3r.h"
#include "conv_route.h"
// the three switches above as every entry point reads them: once, before it computes its route
static inline RouteEnv route_env() { return {split_mode(), g_bf16_fast, g_h3r}; }

// ---- r6: max |x| of an operand tensor (the scale of the h3 split, conv_x6.h) -----------------------------------------------------
// slot = FC_AMAX_SLOT_BYTES (fc_common.h: 32 sub-words, one per 64-byte line; the kernels read their maximum); this pass uses the
// first line: [0] the result (sub-word 0: bit pattern of max |x|), [1] running maximum, [2] finished blocks.
// Every block folds its elements into [1] with ONE integer atomicMax (order-independent: bit-reproducible); the last block to
// finish publishes [1] to [0] and clears [1], [2] for the slot's next use.  Slots must start zeroed (fc_amax_slots / the ring).
__global__ __launch_bounds__(256) void k_amax(const f32x4* __restrict__ x, int64_t n4, const float* __restrict__ tail, int ntail,
                                              unsigned* __restrict__ slot) {
  __shared__ unsigned wm[4];
  __shared__ int last_s;
  unsigned m = 0u;
  // FINITE elements only: an overflowed activation must poison the rows that gather it (inf s = inf -> NaN, as on the six-product
  // route), not flatten the scale of the whole tensor.  Four loads in flight per thread.
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += 4 * stride) {
    f32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = i + q * stride < n4 ? x[i + q * stride] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) { const unsigned u = __float_as_uint(v[q][j]) & 0x7fffffffu; m = (u > m && u < 0x7f800000u) ? u : m; }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) { const unsigned u = __float_as_uint(tail[threadIdx.x]) & 0x7fffffffu; m = (u > m && u < 0x7f800000u) ? u : m; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)m, off, 64); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned b = wm[0];
    for (int w = 1; w < 4; ++w) b = wm[w] > b ? wm[w] : b;
    if (b > __hip_atomic_load(&slot[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&slot[1], b);
    __threadfence();
    last_s = atomicAdd(&slot[2], 1u) == gridDim.x - 1;
    if (last_s) {
      __threadfence();
      slot[0] = atomicExch(&slot[1], 0u);
      slot[2] = 0u;
    }
  }
}

// library-owned ring of slots per device, for the operands whose caller brings no amax word of its own
constexpr int AMAX_RING = 2048;
static unsigned* g_amax_ring[16] = {};
static unsigned g_amax_next[16] = {};
static std::mutex g_amax_ring_mu;
static int amax_ring_slot(unsigned** slot) {
  int dev = 0;
  FC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 16) return FC_EINVAL;
  std::lock_guard<std::mutex> lock(g_amax_ring_mu);          // (two threads' first calls must not both create the ring)
  if (!g_amax_ring[dev]) {
    FC_HIP(hipMalloc((void**)&g_amax_ring[dev], (size_t)AMAX_RING * FC_AMAX_SLOT_BYTES));
    FC_HIP(hipMemset(g_amax_ring[dev], 0, (size_t)AMAX_RING * FC_AMAX_SLOT_BYTES));
  }
  const unsigned i = __atomic_fetch_add(&g_amax_next[dev], 1u, __ATOMIC_RELAXED) % AMAX_RING;
  *slot = g_amax_ring[dev] + (size_t)i * (FC_AMAX_SLOT_BYTES / 4);
  return FC_OK;
}
static int amax_launch(const float* x, int64_t n, unsigned* slot, hipStream_t stream) {
  if (n <= 0) { FC_HIP(hipMemsetAsync(slot, 0, 4, stream)); return FC_OK; }
  const int64_t n4 = n / 4;
  int64_t blocks = fc_cdiv(n4 > 0 ? n4 : 1, 256 * 8);
  if (blocks > 1024) blocks = 1024;
  k_amax<<<(unsigned)blocks, 256, 0, stream>>>(reinterpret_cast<const f32x4*>(x), n4, x + 4 * n4, (int)(n - 4 * n4), slot);
  FC_CHECK_LAUNCH();
  return FC_OK;
}
// the caller's amax words for the NEXT convolution / weight-gradient call of this thread (fc_conv_amax_hint): a0 = the gathered
// operand (`in`), a1 = `gout` (weight gradients); NULL: computed here, into a ring slot.  Consumed by that call.
static thread_local const unsigned* t_amax_hint[2] = {nullptr, nullptr};
struct AmaxHintScope { ~AmaxHintScope() { t_amax_hint[0] = t_amax_hint[1] = nullptr; } };      // every convolution entry point drops the hints when it returns
static int operand_amax(const float* x, int64_t n, int which, hipStream_t stream, const unsigned** out) {
  const unsigned* h = t_amax_hint[which];
  if (h) { *out = h; return FC_OK; }
  unsigned* slot;
  int rc = amax_ring_slot(&slot);
  if (rc) return rc;
  rc = amax_launch(x, n, slot, stream);
  *out = slot;
  return rc;
}
extern "C" int fc_amax(const float* x, int64_t n, unsigned* slot, hipStream_t stream) {
  if (!slot || n < 0 || (n > 0 && !x) || ((uintptr_t)x & 15)) return FC_EINVAL;
  return amax_launch(x, n, slot, stream);
}
extern "C" int fc_conv_amax_hint(const unsigned* amax_in, const unsigned* amax_gout) {
  t_amax_hint[0] = amax_in;
  t_amax_hint[1] = amax_gout;
  return FC_OK;
}

// out[i] = sum_z part[z][i]   (fixed order; elems % 4 == 0)
__global__ void k_sum_parts(const float* __restrict__ part, float* __restrict__ out, int64_t elems4, int S) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= elems4) return;
  float4 a = reinterpret_cast<const float4*>(part)[i];
  for (int s = 1; s < S; ++s) {
    float4 b = reinterpret_cast<const float4*>(part)[(int64_t)s * elems4 + i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  reinterpret_cast<float4*>(out)[i] = a;
}

// out[o] = sum_k T_k[pos[k][o]] over the offsets that have a neighbour at o (fixed k order: deterministic)
__global__ void k_sum_pairs(const float* __restrict__ part, const int* __restrict__ pos, float* __restrict__ out,
                            int64_t n_out, int K, int Cout) {
  const int c4n = Cout / 4;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out * c4n) return;
  int64_t o = t / c4n;
  int c4 = (int)(t % c4n);
  // nine offsets per batch: their positions, then their rows, are requested together (an absent offset reads the zero
  // row), and added in offset order — r3: one dependent (position -> row) chain per offset made this launch 19 us on
  // every level, 1 ms per step
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 9) {
    int j[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) j[u] = k0 + u < K ? pos[(int64_t)(k0 + u) * n_out + o] : -1;
    f32x4 v[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const float* src = j[u] >= 0 ? part + ((int64_t)(k0 + u) * n_out + j[u]) * Cout + c4 * 4 : g_zero_row + (c4 & 15) * 4;
      v[u] = *reinterpret_cast<const f32x4*>(src);
    }
#pragma unroll
    for (int u = 0; u < 9; ++u)
      if (j[u] >= 0) a += v[u];
  }
  *reinterpret_cast<f32x4*>(out + o * Cout + c4 * 4) = a;
}

// ---- r5: the same two sums, leaving the BatchNorm statistics of what they write -----------------------------------------------
// A workgroup = 16 float4 lanes (64 channels) x 16 row lanes; grid (row blocks of RB rows, C / 64).  Besides out, every workgroup
// writes the column sums of its rows' results and of their squares: stats[row block][2][C] (norm.hip k_bn2_apply / k_bn2_finalize
// combine them in fp64).  RB = fc_stat_rb(n): row blocks are sized so that small matrices leave <= 64 of them (then the
// BatchNorm that follows is ONE launch) while every thread still has at most a handful of rows.
__host__ __device__ static inline int fc_stat_rb(int64_t n) { return n <= 1024 ? 16 : (n <= 4096 ? 64 : 32); }

__device__ __forceinline__ void stat_block_reduce(f32x4 a1, f32x4 a2, float* __restrict__ stats, int C, f32x4* sm /*[16][2][16]*/) {
  const int lane = threadIdx.x & 15, rl = threadIdx.x >> 4;
  sm[(rl * 2 + 0) * 16 + lane] = a1;
  sm[(rl * 2 + 1) * 16 + lane] = a2;
  __syncthreads();
  if (rl < 2) {                                  // row lane 0 adds the sums, row lane 1 the sums of squares (fixed order)
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 16; ++q) t += sm[(q * 2 + rl) * 16 + lane];
    *reinterpret_cast<f32x4*>(stats + ((int64_t)blockIdx.x * 2 + rl) * C + blockIdx.y * 64 + lane * 4) = t;
  }
}

// per-thread channel parameters of the backward form of the statistics (X6Epi, conv_x6.h): 4 channels from c on
struct StatCh { f32x4 mu, is, ga, be; bool bwd, from_y, has_add; int act; };
__device__ __forceinline__ StatCh stat_channels(const X6Epi& epi, int c) {
  StatCh p;
  p.bwd = epi.bn_x != nullptr;
  p.act = epi.act;
  p.from_y = p.bwd && epi.bn_y != nullptr && epi.act != 0;
  p.has_add = p.bwd && epi.add != nullptr;
  p.mu = f32x4{0.f, 0.f, 0.f, 0.f}; p.is = f32x4{1.f, 1.f, 1.f, 1.f}; p.ga = p.is; p.be = p.mu;
  if (p.bwd) {
    p.mu = *reinterpret_cast<const f32x4*>(epi.mean + c);
    const f32x4 va = *reinterpret_cast<const f32x4*>(epi.var + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) p.is[j] = 1.f / sqrtf(va[j] + epi.eps);
    if (epi.gamma) p.ga = *reinterpret_cast<const f32x4*>(epi.gamma + c);
    if (epi.beta) p.be = *reinterpret_cast<const f32x4*>(epi.beta + c);
  }
  return p;
}
// `at`: element offset of (row, first channel) in the (n, C) matrices bn_x / add / bn_y
__device__ __forceinline__ void stat_accumulate(const StatCh& p, const X6Epi& epi, const f32x4& a, int64_t at, f32x4& a1, f32x4& a2) {
  f32x4 xv = {0.f, 0.f, 0.f, 0.f}, av = xv, yv = xv;
  if (p.bwd) xv = *reinterpret_cast<const f32x4*>(epi.bn_x + at);
  if (p.has_add) av = *reinterpret_cast<const f32x4*>(epi.add + at);
  if (p.from_y) yv = *reinterpret_cast<const f32x4*>(epi.bn_y + at);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t1, t2;
    x6_epi_terms(p.bwd, p.bwd ? av[j] + a[j] : a[j], xv[j], p.mu[j], p.is[j], p.ga[j], p.be[j], p.act, p.from_y, yv[j], t1, t2);
    a1[j] += t1;
    a2[j] += t2;
  }
}

__global__ __launch_bounds__(256) void k_sum_parts_stats(const float* __restrict__ part, float* __restrict__ out, int64_t n, int C, int S,
                                                         int RB, X6Epi epi) {
  __shared__ f32x4 sm[16 * 2 * 16];
  const int lane = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  const int c = blockIdx.y * 64 + lane * 4;
  const StatCh p = stat_channels(epi, c);
  f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1;
  for (int64_t r = r0 + rl; r < r0 + RB && r < n; r += 16) {
    f32x4 a = *reinterpret_cast<const f32x4*>(part + r * C + c);
    for (int z = 1; z < S; ++z) a += *reinterpret_cast<const f32x4*>(part + ((int64_t)z * n + r) * C + c);
    *reinterpret_cast<f32x4*>(out + r * C + c) = a;
    stat_accumulate(p, epi, a, r * C + c, a1, a2);
  }
  stat_block_reduce(a1, a2, epi.stats, C, sm);
}

__global__ __launch_bounds__(256) void k_sum_pairs_stats(const float* __restrict__ part, const int* __restrict__ pos, float* __restrict__ out,
                                                         int64_t n_out, int K, int Cout, int RB, X6Epi epi) {
  __shared__ f32x4 sm[16 * 2 * 16];
  const int lane = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  const int c = blockIdx.y * 64 + lane * 4;
  const StatCh p = stat_channels(epi, c);
  f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1;
  const int64_t rend = (r0 + RB < n_out) ? r0 + RB : n_out;
  // TWO rows of this thread per pass (rows o and o + 16): their positions, then their partial rows, are requested together — with
  // 64-row blocks (1k...4k result rows) a thread owns four rows, and one row per pass made them a chain of 4 x 3 x 2 dependent loads
  for (int64_t o = r0 + rl; o < rend; o += 32) {
    const int64_t o2 = o + 16;
    const bool two = o2 < rend;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;              // as k_sum_pairs: offsets in order, nine in flight
    for (int k0 = 0; k0 < K; k0 += 9) {
      int j[9], j2[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        j[u] = k0 + u < K ? pos[(int64_t)(k0 + u) * n_out + o] : -1;
        j2[u] = (two && k0 + u < K) ? pos[(int64_t)(k0 + u) * n_out + o2] : -1;
      }
      f32x4 v[9], v2[9];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const float* src = j[u] >= 0 ? part + ((int64_t)(k0 + u) * n_out + j[u]) * Cout + c : g_zero_row + lane * 4;
        const float* src2 = j2[u] >= 0 ? part + ((int64_t)(k0 + u) * n_out + j2[u]) * Cout + c : g_zero_row + lane * 4;
        v[u] = *reinterpret_cast<const f32x4*>(src);
        v2[u] = *reinterpret_cast<const f32x4*>(src2);
      }
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        if (j[u] >= 0) a += v[u];
        if (j2[u] >= 0) b += v2[u];
      }
    }
    *reinterpret_cast<f32x4*>(out + o * Cout + c) = a;
    stat_accumulate(p, epi, a, o * Cout + c, a1, a2);
    if (two) {
      *reinterpret_cast<f32x4*>(out + o2 * Cout + c) = b;
      stat_accumulate(p, epi, b, o2 * Cout + c, a1, a2);
    }
  }
  stat_block_reduce(a1, a2, epi.stats, Cout, sm);
}

static_assert(STEM_CIN == 3 && STEM_COUT == 64 && BK == 32, "conv_route.h spells these shapes out");

// what every tiled convolution kernel takes (k_conv_x6 / k_conv_h3r: and the epilogue)
struct ConvArgs {
  const float *in, *W; const int *nbr, *out_index, *cnt; float* dst;
  int64_t n_rows; int K, Cin, Cout; X6Epi epi; hipStream_t stream;
};
#define FC_LAUNCH(...) __VA_ARGS__<<<grid, 256, 0, a.stream>>>(a.in, a.W, a.nbr, a.out_index, a.cnt, a.dst, a.n_rows, a.K, a.Cin, a.Cout)
#define FC_LAUNCH_EPI(...) __VA_ARGS__<<<grid, 256, 0, a.stream>>>(a.in, a.W, a.nbr, a.out_index, a.cnt, a.dst, a.n_rows, a.K, a.Cin, a.Cout, a.epi)

// the LDS-tiled fp32 MFMA kernels (32-deep slabs; measured r1: 64-deep slabs, 256-row tiles, an LDS index table
// and LDS-padding occupancy caps all lose or are neutral — profiles/r1_conv_pmc.md — and were removed in r2)
template <int BM, int BN, int WM>
static void launch_conv_fp32(const ConvRoute& r, const ConvArgs& a, dim3 grid) {
#define FC_LAUNCH_MFMA(KERNEL)                                                                                              \
  do { if (r.wsrc == FC_WSRC_FP32_T) FC_LAUNCH(KERNEL<BM, BN, 32, true, WM, true>); else if (a.nbr) FC_LAUNCH(KERNEL<BM, BN, 32, true, WM>); \
       else FC_LAUNCH(KERNEL<BM, BN, 32, false, WM>); } while (0)
  if (r.family == FC_FAM_MFMA) FC_LAUNCH_MFMA(k_conv_mfma);
  if constexpr (BM >= 128) {                     // the deeper pipeline and the LDS-DMA kernel have no 64-row tile
    if (r.family == FC_FAM_MFMA_P) FC_LAUNCH_MFMA(k_conv_mfma_p);
    if (r.family == FC_FAM_GLDS) { if (a.nbr) FC_LAUNCH(k_conv_glds<BM, BN, true, WM>); else FC_LAUNCH(k_conv_glds<BM, BN, false, WM>); }
  }
#undef FC_LAUNCH_MFMA
}

// the split-bf16 kernel (conv_x6.h): template arguments <tile, HAS_NBR, WM, BSRC = r.wsrc, MODE, BUF>; bf16-fast and buffer addressing
// exist for 128-row tiles reading an image; k_conv_h3r (conv_h3r.h): h3 on 128-row tiles
template <int BM, int BN, int WM>
static void launch_conv_x6(const ConvRoute& r, const ConvArgs& a, dim3 grid) {
  if (r.family == FC_FAM_H3R) {
    if constexpr (BM == 128) {
      if (r.buf) FC_LAUNCH_EPI(k_conv_h3r<BN, true, true>);
      else if (a.nbr) FC_LAUNCH_EPI(k_conv_h3r<BN, true, false>);
      else FC_LAUNCH_EPI(k_conv_h3r<BN, false, false>);
    }
  } else if (r.wsrc == FC_WSRC_FP32_T) FC_LAUNCH_EPI(k_conv_x6<BM, BN, true, WM, 1>);
  else if (r.wsrc == FC_WSRC_FP32) { if (a.nbr) FC_LAUNCH_EPI(k_conv_x6<BM, BN, true, WM, 0>); else FC_LAUNCH_EPI(k_conv_x6<BM, BN, false, WM, 0>); }
  else if (r.mode == FC_MODE_BF16 || r.buf) {
    if constexpr (BM == 128) {
      if (r.mode == FC_MODE_BF16) { if (a.nbr) FC_LAUNCH_EPI(k_conv_x6<128, BN, true, 2, 2, 1>); else FC_LAUNCH_EPI(k_conv_x6<128, BN, false, 2, 2, 1>); }
      else if (r.mode == FC_MODE_H3) FC_LAUNCH_EPI(k_conv_x6<128, BN, true, 2, 2, 2, true>);
      else FC_LAUNCH_EPI(k_conv_x6<128, BN, true, 2, 2, 0, true>);
    }
  } else if (r.mode == FC_MODE_H3) { if (a.nbr) FC_LAUNCH_EPI(k_conv_x6<BM, BN, true, WM, 2, 2>); else FC_LAUNCH_EPI(k_conv_x6<BM, BN, false, WM, 2, 2>); }
  else { if (a.nbr) FC_LAUNCH_EPI(k_conv_x6<BM, BN, true, WM, 2>); else FC_LAUNCH_EPI(k_conv_x6<BM, BN, false, WM, 2>); }
}

// one convolution launch: nothing but the route's template instantiation (STEM / FMA: a.dst is the output itself)
static int launch_conv(const ConvRoute& r, const ConvArgs& a) {
  const dim3 grid(r.grid[0], r.grid[1], r.grid[2]);
  if (r.family == FC_FAM_STEM) {
    const size_t smem = (size_t)(STEM_ROWS * STEM_FWD_LDA + 96 * 64) * sizeof(float);
    k_stem_fwd<<<(unsigned)fc_cdiv(a.n_rows, STEM_ROWS), 256, smem, a.stream>>>(a.in, a.W, a.nbr, a.dst, nullptr, a.n_rows, a.K);
  } else if (r.family == FC_FAM_FMA) {
    k_conv_fma<<<(unsigned)fc_cdiv(a.n_rows * a.Cout, 256), 256, 0, a.stream>>>(a.in, a.W, a.nbr, a.dst, a.n_rows, a.K, a.Cin, a.Cout, r.wsrc == FC_WSRC_FP32_T ? 1 : 0);
  } else {
#define FC_TILE(BM, BN, WM) do { if (r.family >= FC_FAM_X6) launch_conv_x6<BM, BN, WM>(r, a, grid); else launch_conv_fp32<BM, BN, WM>(r, a, grid); } while (0)
    if (r.bm == 256) FC_TILE(256, 64, 4);
    else if (r.bm == 128 && r.bn == 128) FC_TILE(128, 128, 2);
    else if (r.bm == 128) FC_TILE(128, 64, 2);
    else if (r.bn == 128) launch_conv_fp32<64, 128, 2>(r, a, grid);
    else launch_conv_fp32<64, 64, 2>(r, a, grid);
#undef FC_TILE
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}
#undef FC_LAUNCH
#undef FC_LAUNCH_EPI

extern "C" {

int fc_conv_fwd_route(int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, int table_kind, int64_t live_tiles, int* out) {
  if (!out || n_in < 0 || n_out < 0 || K < 1 || Cin < 1 || Cout < 1) return FC_EINVAL;
  const ConvRoute r = conv_route({n_in, n_out, K, Cin, Cout}, flags, table_kind, live_tiles, route_env());
  const int f[16] = {r.family, r.bm, r.bn, r.wm, r.S, r.wsrc, r.mode, r.buf, r.epi, (int)r.grid[0], (int)r.grid[1], (int)r.grid[2]};
  for (int i = 0; i < 16; ++i) out[i] = f[i];
  return r.family == FC_FAM_INVALID ? FC_EINVAL : FC_OK;
}

int64_t fc_conv_fwd_ws_bytes(int64_t n_out, int K, int Cin, int Cout, int flags) {
  const ConvRoute r = conv_route({n_out, n_out, K, Cin, Cout}, flags, FC_TABLE_DENSE, 0, route_env());
  return r.S > 1 ? (int64_t)r.S * n_out * Cout * (int64_t)sizeof(float) : 0;
}

int64_t fc_conv_fwd_pairs_ws_bytes(int64_t n_out, int K, int Cout) {      // the pair-list route's S is K, whatever the rest of the shape
  return (int64_t)K * n_out * Cout * (int64_t)sizeof(float);
}

// Row blocks of the statistics table a convolution launch leaves for the BatchNorm behind it (fc_conv_fwd_stats /
// fc_conv_fwd_pairs_tiles_stats: stats[blocks][2][Cout], column sums of the result and of its square per row block); 0: this launch
// has no statistics epilogue (not the split-bf16 MFMA route).  pairs != 0: the per-offset pair-list route.
int64_t fc_conv_stats_blocks(int64_t n_out, int K, int Cin, int Cout, int flags, int pairs) {
  if (n_out < 1) return 0;
  const ConvRoute r = conv_route({n_out, n_out, K, Cin, Cout}, flags, pairs ? FC_TABLE_PAIRS : FC_TABLE_DENSE, 0, route_env());
  if (r.epi == FC_EPI_NONE) return 0;
  return r.epi == FC_EPI_SUM ? fc_cdiv(n_out, fc_stat_rb(n_out)) : fc_cdiv(n_out, r.bm);
}

// Every convolution entry point: the route, the workspace, the amax word, the launch, the fixed-order sum of the partial results.
// cnt / pos != NULL: the exact pair lists (nbr = pair_in) — per offset a compacted gather-GEMM into the workspace, then a gather-sum.
static int conv_impl(const float* in, const float* W, const int* nbr, const int* out_index, const int* cnt, const int* pos, float* out,
                     int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags, void* ws, int64_t ws_bytes,
                     hipStream_t stream, const X6Epi* epi) {
  AmaxHintScope hint_scope;
  if (n_in < 0 || n_out < 0 || K < 1 || Cin < 1 || Cout < 1) return FC_EINVAL;
  // nothing to write (an empty table may well be a NULL pointer) and no row block to leave statistics for
  if (n_out == 0 && !cnt) return epi ? FC_EINVAL : FC_OK;
  if (out_index && !nbr) return FC_EINVAL;
  const int table = cnt ? FC_TABLE_PAIRS : out_index ? FC_TABLE_SORTED : nbr ? FC_TABLE_DENSE : FC_TABLE_NONE;
  const ConvRoute r = conv_route({n_in, n_out, K, Cin, Cout}, flags, table | (epi ? FC_TABLE_STATS : 0), live_tiles, route_env());
  if (r.family == FC_FAM_INVALID) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  ConvArgs a = {in, W, nbr, out_index, cnt, out, n_out, K, Cin, Cout, {}, stream};
  if (r.family == FC_FAM_STEM || r.family == FC_FAM_FMA) return launch_conv(r, a);      // untiled: no partial sums
  const bool parts = cnt || r.S > 1;
  if (parts && ws_bytes < (int64_t)r.S * n_out * Cout * (int64_t)sizeof(float)) return FC_EWS;
  if (parts) a.dst = (float*)ws;
  if (epi && r.epi == FC_EPI_KERNEL) a.epi = *epi;
  int rc = FC_OK;
  if (r.mode == FC_MODE_H3) rc = operand_amax(in, n_in * (int64_t)Cin, 0, stream, &a.epi.amax_in);      // the gathered operand's amax word: the caller's hint or a pass of our own
  if (rc == FC_OK) rc = launch_conv(r, a);
  if (rc != FC_OK || !parts) return rc;
  const int rb = fc_stat_rb(n_out);
  const dim3 sgrid((unsigned)fc_cdiv(n_out, rb), Cout / 64);
  if (cnt && epi) k_sum_pairs_stats<<<sgrid, 256, 0, stream>>>(a.dst, pos, out, n_out, K, Cout, rb, *epi);
  else if (cnt) k_sum_pairs<<<(unsigned)fc_cdiv(n_out * (Cout / 4), 256), 256, 0, stream>>>(a.dst, pos, out, n_out, K, Cout);
  else if (epi) k_sum_parts_stats<<<sgrid, 256, 0, stream>>>(a.dst, out, n_out, Cout, r.S, rb, *epi);
  else k_sum_parts<<<(unsigned)fc_cdiv(n_out * Cout / 4, 256), 256, 0, stream>>>(a.dst, out, n_out * Cout / 4, r.S);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

static int conv_pairs_impl(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos, float* out,
                           int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags, void* ws,
                           int64_t ws_bytes, hipStream_t stream, const X6Epi* epi) {
  if (!pair_in || !pair_cnt || !pair_pos || K > 65535) return FC_EINVAL;
  return conv_impl(in, W, pair_in, nullptr, pair_cnt, pair_pos, out, n_in, n_out, K, Cin, Cout, live_tiles, flags, ws, ws_bytes, stream, epi);
}

// the epilogue of the *_stats entry points (conv_x6.h X6Epi); bn_x != NULL: the two backward reductions of the BatchNorm in front
static X6Epi stats_epi(float* stats, const float* bn_x = nullptr, const float* mean = nullptr, const float* var = nullptr, const float* gamma = nullptr,
                       const float* beta = nullptr, float eps = 0.f, int act = 0, const float* add = nullptr, const float* bn_y = nullptr) {
  return {stats, bn_x, mean, var, gamma, beta, eps, act, add, bn_y, nullptr};
}

// flags: FC_CONV_* (include/fcaf3d_hip.h).
int fc_conv_fwd(const float* in, const float* W, const int* nbr, const int* out_index, float* out, int64_t n_in,
                int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, hipStream_t stream) {
  return conv_impl(in, W, nbr, out_index, nullptr, nullptr, out, n_in, n_out, K, Cin, Cout, 0, flags, ws, ws_bytes, stream, nullptr);
}

int fc_conv_fwd_stats(const float* in, const float* W, const int* nbr, const int* out_index, float* out, int64_t n_in,
                      int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, float* stats,
                      hipStream_t stream) {
  const X6Epi e = stats_epi(stats);
  return conv_impl(in, W, nbr, out_index, nullptr, nullptr, out, n_in, n_out, K, Cin, Cout, 0, flags, ws, ws_bytes, stream, stats ? &e : nullptr);
}

// The backward-data pass of a convolution whose INPUT came out of a BatchNorm (+ ReLU / ELU) layer: besides the gradient g it
// writes, the launch leaves that layer's two backward reductions per row block — stats[blocks][2][Cout] = column sums of
// g' = g act'(.) and of g' xhat, xhat from the layer's input bn_x (n_out, Cout) and its batch statistics — for
// fc_bn_train_bwd(part = stats).  act: 0 none, 1 ReLU, 2 ELU; add (nullable): a second contribution to the gradient, g = result + add;
// bn_y (nullable): the layer's output, which act'(.) is taken from (a layer WITH a residual; NULL: recomputed from bn_x).
int fc_conv_fwd_bn_bwd_stats(const float* in, const float* W, const int* nbr, const int* out_index, float* out, int64_t n_in,
                             int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, float* stats,
                             const float* bn_x, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                             int act, const float* add, const float* bn_y, hipStream_t stream) {
  if (!stats || !bn_x || !mean || !var || act < 0 || act > 2) return FC_EINVAL;
  const X6Epi e = stats_epi(stats, bn_x, mean, var, gamma, beta, eps, act, add, bn_y);
  return conv_impl(in, W, nbr, out_index, nullptr, nullptr, out, n_in, n_out, K, Cin, Cout, 0, flags, ws, ws_bytes, stream, &e);
}

int fc_conv_fwd_pairs_tiles(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                            float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags,
                            void* ws, int64_t ws_bytes, hipStream_t stream) {
  return conv_pairs_impl(in, W, pair_in, pair_cnt, pair_pos, out, n_in, n_out, K, Cin, Cout, live_tiles, flags, ws, ws_bytes, stream, nullptr);
}

int fc_conv_fwd_pairs_tiles_stats(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                                  float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags,
                                  void* ws, int64_t ws_bytes, float* stats, hipStream_t stream) {
  const X6Epi e = stats_epi(stats);
  return conv_pairs_impl(in, W, pair_in, pair_cnt, pair_pos, out, n_in, n_out, K, Cin, Cout, live_tiles, flags, ws, ws_bytes, stream,
                         stats ? &e : nullptr);
}

int fc_conv_fwd_pairs_tiles_bn_bwd_stats(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                                         float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags,
                                         void* ws, int64_t ws_bytes, float* stats, const float* bn_x, const float* mean,
                                         const float* var, const float* gamma, const float* beta, float eps, int act,
                                         const float* add, const float* bn_y, hipStream_t stream) {
  if (!stats || !bn_x || !mean || !var || act < 0 || act > 2) return FC_EINVAL;
  const X6Epi e = stats_epi(stats, bn_x, mean, var, gamma, beta, eps, act, add, bn_y);
  return conv_pairs_impl(in, W, pair_in, pair_cnt, pair_pos, out, n_in, n_out, K, Cin, Cout, live_tiles, flags, ws, ws_bytes, stream, &e);
}

int fc_conv_fwd_pairs(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                      float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, void* ws,
                      int64_t ws_bytes, hipStream_t stream) {
  return fc_conv_fwd_pairs_tiles(in, W, pair_in, pair_cnt, pair_pos, out, n_in, n_out, K, Cin, Cout, 0, flags, ws, ws_bytes, stream);
}

// Pre-split weight image for the split-bf16 kernel (FC_CONV_SPLIT | FC_CONV_IMAGE of fc_conv_fwd / fc_conv_fwd_pairs*): R = reduction
// size (Cin of the launch), C = its columns (Cout of the launch); transposed != 0: W[k] is stored (C, R) row-major.
int64_t fc_x6_weight_image_bytes(int K, int R, int C) { return (int64_t)K * R * C * 6; }

int fc_x6_weight_image(const float* W, void* img, int K, int R, int C, int transposed, hipStream_t stream) {
  if (K < 1 || R < 32 || C < 64 || R % 32 != 0 || C % 64 != 0) return FC_EINVAL;
  const int64_t total = (int64_t)K * (R / 32) * (C / 64) * 256;
  const unsigned nb = (unsigned)fc_cdiv(total, 256);
  if (split_mode() == 2) {                       // h3: max |W| into the image's amax word, then the fp16 pieces
    FC_HIP(hipMemsetAsync((char*)img + 4 * X6_IMG_AMAX_WORD, 0, FC_AMAX_SLOT_BYTES, stream));
    k_x6_weight_image<3><<<nb, 256, 0, stream>>>(W, (u32x4*)img, K, R, C, transposed);
    k_x6_weight_image<2><<<nb, 256, 0, stream>>>(W, (u32x4*)img, K, R, C, transposed);
  } else {
    k_x6_weight_image<0><<<nb, 256, 0, stream>>>(W, (u32x4*)img, K, R, C, transposed);
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int64_t fc_x6_amax_units(void) { return X6_AMAX_UNITS; }

// passes: bit 0 zero the amax slots, bit 1 the amax pass, bit 2 the image pass (split mode 2; other modes have the image pass alone)
int fc_x6_weight_images_passes(const int64_t* desc, int n, int64_t total_blocks, const int64_t* amax_chunks, int64_t amax_blocks,
                               int passes, hipStream_t stream) {
  if (!desc || n < 1 || total_blocks < 1 || total_blocks > 0x7fffffffll || amax_blocks < 0 || amax_blocks > 0x7fffffffll ||
      (amax_blocks && !amax_chunks))
    return FC_EINVAL;
  const long long* d = reinterpret_cast<const long long*>(desc);
  if (split_mode() == 2) {
    if (passes & 1) k_x6_weight_images<4><<<(unsigned)fc_cdiv(n, 4), 256, 0, stream>>>(d, n);
    if ((passes & 2) && amax_blocks)
      k_x6_weight_amax<X6_AMAX_UNITS><<<(unsigned)amax_blocks, 256, 0, stream>>>(d, reinterpret_cast<const long long*>(amax_chunks));
    if (passes & 4) k_x6_weight_images<2><<<(unsigned)total_blocks, 256, 0, stream>>>(d, n);
  } else if (passes & 4) {
    k_x6_weight_images<0><<<(unsigned)total_blocks, 256, 0, stream>>>(d, n);
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}

int fc_x6_weight_images(const int64_t* desc, int n, int64_t total_blocks, const int64_t* amax_chunks, int64_t amax_blocks,
                        hipStream_t stream) {
  return fc_x6_weight_images_passes(desc, n, total_blocks, amax_chunks, amax_blocks, 7, stream);
}

}  // extern "C"

// ---- weight gradient: the fixed-order sums of the partial products (kernels: wgrad_f32.h, wgrad_x6.h) ----
__global__ void k_wgrad_reduce(const float* __restrict__ part, float* __restrict__ gW, int64_t elems, int S) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= elems) return;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += part[(int64_t)s * elems + i];
  gW[i] = acc;
}

// The same for elems % 4 == 0 with 16-byte accesses and G slab groups per output (256 threads = 256 / G float4 columns x G
// groups): group g sums slabs [g * ceil(S / G), ...) in slab order with four loads in flight, the G group sums are added in
// group order through LDS — a fixed order, whatever the grid (r3: the stem's 192 x 20 KB slabs went through 5 184 threads
// with one dependent 4-byte load each).  Measured and dropped (r3, profiles/r3_notes.md): combining the partial tiles INSIDE
// the weight-gradient launch (last-arriving workgroup per tile, agent-scope release / ticket / acquire) — the release's
// buffer_wbl2 in each of the ~1 500 workgroups of a launch writes back everything the concurrently running main-stream
// kernels have dirtied in that L2: 32.4 -> 34.3 ms per step.
template <int G>
__global__ __launch_bounds__(256) void k_wgrad_reduce4(const float* __restrict__ part, float* __restrict__ gW, int64_t elems4, int S) {
  __shared__ f32x4 red[256];
  constexpr int COLS = 256 / G;
  const int col = threadIdx.x % COLS, g = threadIdx.x / COLS;
  const int64_t i = (int64_t)blockIdx.x * COLS + col;
  const int per = (S + G - 1) / G;
  const int s0 = g * per, s1 = (s0 + per < S) ? s0 + per : S;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (i < elems4) {
    const f32x4* src = reinterpret_cast<const f32x4*>(part) + i;
    int sl = s0;
    for (; sl + 4 <= s1; sl += 4) {
      const f32x4 v0 = src[(int64_t)sl * elems4], v1 = src[(int64_t)(sl + 1) * elems4];
      const f32x4 v2 = src[(int64_t)(sl + 2) * elems4], v3 = src[(int64_t)(sl + 3) * elems4];
      a += v0; a += v1; a += v2; a += v3;
    }
    for (; sl < s1; ++sl) a += src[(int64_t)sl * elems4];
  }
  if (G == 1) {
    if (i < elems4) reinterpret_cast<f32x4*>(gW)[i] = a;
    return;
  }
  red[threadIdx.x] = a;
  __syncthreads();
  if (g == 0 && i < elems4) {
    for (int q = 1; q < G; ++q) a += red[q * COLS + col];
    reinterpret_cast<f32x4*>(gW)[i] = a;
  }
}

// (K,Cin,Cout) -> (K,Cout,Cin)
__global__ void k_transpose_w(const float* __restrict__ W, float* __restrict__ Wt, int K, int Cin, int Cout) {
  __shared__ float tile[32][33];
  int k = blockIdx.z;
  int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
  int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 32 x 8
  for (int j = ty; j < 32; j += 8) {
    int ci = ci0 + j, co = co0 + tx;
    tile[j][tx] = (ci < Cin && co < Cout) ? W[((int64_t)k * Cin + ci) * Cout + co] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int co = co0 + j, ci = ci0 + tx;
    if (ci < Cin && co < Cout) Wt[((int64_t)k * Cout + co) * Cin + ci] = tile[tx][j];
  }
}

// what every weight-gradient kernel takes (k_wgrad_x6t: and the amax words; the kernels without pair lists: no row_index / cnt)
struct WgradArgs {
  const float *in, *gout; const int *nbr, *row_index, *cnt; float* part;
  int64_t n_out; int K, Cin, Cout; const unsigned *amax_in, *amax_gout; hipStream_t stream;
};
#define FC_LAUNCH(...) __VA_ARGS__<<<grid, 256, 0, a.stream>>>(a.in, a.gout, a.nbr, a.row_index, a.cnt, a.part, a.n_out, a.K, a.Cin, a.Cout, r.rps)
#define FC_LAUNCH_X6T(...) __VA_ARGS__<<<grid, 256, 0, a.stream>>>(a.in, a.gout, a.nbr, a.row_index, a.cnt, a.part, a.n_out, a.K, a.Cin, a.Cout, r.rps, a.amax_in, a.amax_gout, r.wbuf)
#define FC_LAUNCH_TABLE(...) __VA_ARGS__<<<grid, 256, 0, a.stream>>>(a.in, a.gout, a.nbr, a.part, a.n_out, a.K, a.Cin, a.Cout, r.rps)

template <int BM, int BN, int KO, bool PAIRS>          // split-bf16 (wgrad_x6.h): the arithmetic is the last template argument
static void launch_wgrad_x6t(const WgradRoute& r, const WgradArgs& a, dim3 grid) {
  if (r.mode == FC_MODE_BF16) FC_LAUNCH_X6T(k_wgrad_x6t<BM, BN, KO, PAIRS, 1>);
  else if (r.mode == FC_MODE_H3) FC_LAUNCH_X6T(k_wgrad_x6t<BM, BN, KO, PAIRS, 2>);
  else FC_LAUNCH_X6T(k_wgrad_x6t<BM, BN, KO, PAIRS>);
}

template <int BM, int BN>                               // one offset per workgroup: k_wgrad_x6t, k_wgrad_mfma, k_wgrad_mfma_p (64-channel Cin tiles)
static void launch_wgrad_tile(const WgradRoute& r, const WgradArgs& a, dim3 grid) {
  const bool pairs = r.table == FC_TABLE_PAIRS;
  if (r.family == FC_WFAM_X6T) { if (pairs) launch_wgrad_x6t<BM, BN, 1, true>(r, a, grid); else launch_wgrad_x6t<BM, BN, 1, false>(r, a, grid); }
  else if (r.family == FC_WFAM_MFMA && !pairs && r.bkr == 32) { if (a.nbr) FC_LAUNCH(k_wgrad_mfma<BM, BN, true, 32, false>); else FC_LAUNCH(k_wgrad_mfma<BM, BN, false, 32, false>); }
  else if constexpr (BM == 64) {
    if (r.family == FC_WFAM_MFMA) { if (pairs) FC_LAUNCH(k_wgrad_mfma<64, BN, true, 32, true>); else FC_LAUNCH(k_wgrad_mfma<64, BN, true, 64, false>); }
    else if (pairs) FC_LAUNCH(k_wgrad_mfma_p<BN, true, true>);
    else if (a.nbr) FC_LAUNCH(k_wgrad_mfma_p<BN, true, false>);
    else FC_LAUNCH(k_wgrad_mfma_p<BN, false, false>);
  }
}

// one weight-gradient launch: nothing but the route's template instantiation
static int launch_wgrad(const WgradRoute& r, const WgradArgs& a) {
  const dim3 grid((unsigned)r.S, r.grid_y);
  const bool wide = r.bn == 128;
  if (r.family == FC_WFAM_STEM) {
    const size_t smem = (size_t)(STEM_ROWS * STEM_JP + STEM_ROWS * 64) * sizeof(float);
    k_stem_wgrad<<<(unsigned)r.S, 256, smem, a.stream>>>(a.in, a.gout, a.nbr, a.part, a.n_out, a.K, r.rps);
  } else if (r.family == FC_WFAM_FMA) FC_LAUNCH_TABLE(k_wgrad_fma);
  else if (r.family == FC_WFAM_MULTI) { if (wide) FC_LAUNCH_TABLE(k_wgrad_multi<128, WGRAD_KO>); else FC_LAUNCH_TABLE(k_wgrad_multi<64, WGRAD_KO>); }
  else if (r.ko == WGRAD_KO) { if (wide) launch_wgrad_x6t<64, 128, WGRAD_KO, false>(r, a, grid); else launch_wgrad_x6t<64, 64, WGRAD_KO, false>(r, a, grid); }
  else if (r.bm == 128) { if (wide) launch_wgrad_tile<128, 128>(r, a, grid); else launch_wgrad_tile<128, 64>(r, a, grid); }
  else { if (wide) launch_wgrad_tile<64, 128>(r, a, grid); else launch_wgrad_tile<64, 64>(r, a, grid); }
  FC_CHECK_LAUNCH();
  return FC_OK;
}
#undef FC_LAUNCH
#undef FC_LAUNCH_X6T
#undef FC_LAUNCH_TABLE

extern "C" {

// gW = sum of the S partial slabs, fixed order
static int wgrad_reduce(const float* part, float* gW, int64_t elems, int S, hipStream_t stream) {
  if (elems % 4 == 0) {
    const int64_t e4 = elems / 4;
    if (S >= 64) k_wgrad_reduce4<16><<<(unsigned)fc_cdiv(e4, 16), 256, 0, stream>>>(part, gW, e4, S);
    else if (S >= 16) k_wgrad_reduce4<4><<<(unsigned)fc_cdiv(e4, 64), 256, 0, stream>>>(part, gW, e4, S);
    else k_wgrad_reduce4<1><<<(unsigned)fc_cdiv(e4, 256), 256, 0, stream>>>(part, gW, e4, S);
  } else {
    k_wgrad_reduce<<<(unsigned)fc_cdiv(elems, 256), 256, 0, stream>>>(part, gW, elems, S);
  }
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// ---- stem convolution with saved gathered inputs (training): forward writes col (n_out, 84), the weight gradient streams it ----
int fc_stem_conv_fwd(const float* in, const float* W, const int* nbr, float* out, float* col, int64_t n_in, int64_t n_out,
                     int K, hipStream_t stream) {
  if (n_in < 0 || n_out < 0 || K < 1 || K > 27 || !nbr) return FC_EINVAL;
  if (n_out == 0) return FC_OK;
  size_t smem = (size_t)(STEM_ROWS * STEM_FWD_LDA + 96 * 64) * sizeof(float);
  k_stem_fwd<<<(unsigned)fc_cdiv(n_out, STEM_ROWS), 256, smem, stream>>>(in, W, nbr, out, col, n_out, K);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

// ~192 row ranges (multiples of 64 rows): every range ends with a 24 KB cross-wave LDS sum, a 20 KB partial and a pass of
// k_wgrad_reduce over all partials, so FEWER, longer ranges win until the chip runs dry (r2, 580k rows, forward + weight
// gradient: 1 024-row ranges 436 us, 2 048: 365, 3 072: 353, 4 096: 378, 8 192: 512; the gather kernel: 493)
static void stem_col_plan(int64_t n_out, int* S, int64_t* rps) {
  int64_t r = fc_cdiv(fc_cdiv(n_out > 0 ? n_out : 1, 192), STEM_ROWS) * STEM_ROWS;
  *rps = r;
  *S = (int)fc_cdiv(n_out > 0 ? n_out : 1, r);
}

int64_t fc_stem_conv_wgrad_ws_bytes(int64_t n_out, int K) {
  int S; int64_t rps;
  stem_col_plan(n_out, &S, &rps);
  return (int64_t)S * K * STEM_CIN * STEM_COUT * (int64_t)sizeof(float);
}

int fc_stem_conv_wgrad(const float* col, const float* gout, float* gW, int64_t n_out, int K, void* ws, int64_t ws_bytes,
                       hipStream_t stream) {
  if (n_out < 0 || K < 1 || K > 27) return FC_EINVAL;
  const int64_t elems = (int64_t)K * STEM_CIN * STEM_COUT;
  if (n_out == 0) {
    FC_HIP(hipMemsetAsync(gW, 0, elems * sizeof(float), stream));
    return FC_OK;
  }
  int S; int64_t rps;
  stem_col_plan(n_out, &S, &rps);
  if (ws_bytes < (int64_t)S * elems * (int64_t)sizeof(float)) return FC_EWS;
  float* part = (S == 1) ? gW : (float*)ws;
  size_t smem = (size_t)(STEM_ROWS * STEM_JP + STEM_ROWS * 64) * sizeof(float);
  k_stem_wgrad_col<<<(unsigned)S, 256, smem, stream>>>(col, gout, part, n_out, K, rps);
  FC_CHECK_LAUNCH();
  if (S > 1) return wgrad_reduce(part, gW, elems, S, stream);
  return FC_OK;
}

int fc_conv_wgrad_route(int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, int table_kind, int* out) {
  if (!out || n_in < 0 || n_out < 0 || K < 1 || Cin < 1 || Cout < 1) return FC_EINVAL;
  const WgradRoute r = wgrad_route({n_in, n_out, K, Cin, Cout}, flags, table_kind, route_env());
  const int f[16] = {r.family, r.bm, r.bn, r.ko, r.bkr, r.table, r.mode, r.S, (int)(r.rps < 0x7fffffff ? r.rps : 0x7fffffff), r.wbuf, (int)r.grid_y};
  for (int i = 0; i < 16; ++i) out[i] = f[i];
  return r.family == FC_WFAM_INVALID ? FC_EINVAL : FC_OK;
}

int64_t fc_conv_wgrad_ws_bytes(int64_t n_out, int K, int Cin, int Cout, int flags) {
  int S = 0;                                   // the caller's table kind is not known here: the largest split of any route the shape has
  for (int table : {FC_TABLE_NONE, FC_TABLE_DENSE, FC_TABLE_PAIRS}) {      // (dense tables may take the multi-offset kernel)
    const WgradRoute r = wgrad_route({n_out, n_out, K, Cin, Cout}, flags, table, route_env());
    if (r.family != FC_WFAM_INVALID && r.S > S) S = r.S;
  }
  return (int64_t)S * K * Cin * Cout * (int64_t)sizeof(float);
}

static int conv_wgrad_impl(const float* in, const float* gout, const int* nbr, const int* row_index, const int* cnt,
                           float* gW, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, void* ws,
                           int64_t ws_bytes, hipStream_t stream) {
  AmaxHintScope hint_scope;
  if (n_in < 0 || n_out < 0 || K < 1 || Cin < 1 || Cout < 1) return FC_EINVAL;
  const int64_t elems = (int64_t)K * Cin * Cout;
  if (n_out == 0) { FC_HIP(hipMemsetAsync(gW, 0, elems * sizeof(float), stream)); return FC_OK; }
  const WgradRoute r = wgrad_route({n_in, n_out, K, Cin, Cout}, flags, cnt ? FC_TABLE_PAIRS : nbr ? FC_TABLE_DENSE : FC_TABLE_NONE, route_env());
  if (r.family == FC_WFAM_INVALID) return FC_EINVAL;
  if (ws_bytes < (int64_t)r.S * elems * (int64_t)sizeof(float)) return FC_EWS;
  WgradArgs a = {in, gout, nbr, row_index, cnt, (r.S == 1) ? gW : (float*)ws, n_out, K, Cin, Cout, nullptr, nullptr, stream};
  int rc = FC_OK;
  if (r.mode == FC_MODE_H3) {                  // the operands' amax words: the caller's hints or passes of our own
    rc = operand_amax(in, n_in * (int64_t)Cin, 0, stream, &a.amax_in);
    if (rc == FC_OK) rc = operand_amax(gout, n_out * (int64_t)Cout, 1, stream, &a.amax_gout);
  }
  if (rc == FC_OK) rc = launch_wgrad(r, a);
  if (rc == FC_OK && r.S > 1) rc = wgrad_reduce(a.part, gW, elems, r.S, stream);
  return rc;
}

int fc_conv_wgrad(const float* in, const float* gout, const int* nbr, const int* row_index, float* gW, int64_t n_in,
                  int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (row_index) return FC_EINVAL;             // reserved (see k_wgrad_mfma)
  return conv_wgrad_impl(in, gout, nbr, nullptr, nullptr, gW, n_in, n_out, K, Cin, Cout, flags, ws, ws_bytes, stream);
}

int fc_conv_wgrad_pairs(const float* in, const float* gout, const int* pair_in, const int* pair_out, const int* pair_cnt,
                        float* gW, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, void* ws,
                        int64_t ws_bytes, hipStream_t stream) {
  if (!pair_in || !pair_out || !pair_cnt) return FC_EINVAL;
  return conv_wgrad_impl(in, gout, pair_in, pair_out, pair_cnt, gW, n_in, n_out, K, Cin, Cout, flags, ws, ws_bytes, stream);
}

int fc_transpose_weight(const float* W, float* Wt, int K, int Cin, int Cout, hipStream_t stream) {
  if (K < 1 || Cin < 1 || Cout < 1 || K > 65535) return FC_EINVAL;
  dim3 grid((unsigned)fc_cdiv(Cout, 32), (unsigned)fc_cdiv(Cin, 32), (unsigned)K);
  k_transpose_w<<<grid, 256, 0, stream>>>(W, Wt, K, Cin, Cout);
  FC_CHECK_LAUNCH();
  return FC_OK;
}

}  // extern "C"
