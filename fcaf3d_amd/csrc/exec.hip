// Native launch-list executor (r4): the forward / backward pass of the FCAF3D network body as ONE C-ABI call per direction.
//
// r4 host profile (tools/hostprof.py, profiles/r4_hostprof.txt): the training step was HOST-bound at every batch size —
// 16.7 ms of Python per step at 2 scenes (drained 16.75 ms), 20.3 ms at 8 (drained 22.8): ~1 000 launches per step, each
// reached through nn.Module.__call__ -> autograd.Function.apply -> torch.empty -> ctypes (~16 us per launch), where the HIP
// launch itself costs ~3.5 us.  The network body is a STATIC sequence of operators (me_resnet.py:43-50, BasicBlock,
// fcaf3d_neck_with_head.py:94-108; only row counts and addresses change from step to step), so the host side builds the
// operator list once per model (fcaf3d_amd/executor.py) and this interpreter walks it: every operator is one of the
// library's own entry points (the kernels, tiles, routes and results are those of the per-operator path — tests compare the
// two bit for bit in the forward pass), every operand an index into a table of device addresses / row counts that the host
// refreshes per step.  Streams: 0 = the caller's stream (the step's dependent chain), 1 = the head branch of the neck
// (out_block_i + forward_single, i > 0), 2 = weight gradients; cross-stream order through hipEvents owned by the library
// (created once per process, never destroyed: a handful).
//
// Reference: what this replaces is mmcv's per-module Python dispatch of the same graph (mmdet3d/models/detectors/
// single_stage_sparse.py:43-50 `extract_feat`, torch.autograd's backward over it).
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "exec_ops.h"        // opcodes, the fields of every operator row and of the kernel-map descriptor, OPW / MAPW / NSTREAM
#include <vector>

namespace {

constexpr int MAX_EVENTS = 64;

// one event set per DEVICE (an event belongs to the device that was current when it was created; a process that drives
// detectors on two devices must not share them — ADVICE r4).  fc_exec is NOT re-entrant per device: one thread per device at a
// time (the reference's loop is one Python thread per process, SURVEY.md 8(b) "Threading").
constexpr int MAX_DEVICES = 16;
hipEvent_t g_events_dev[MAX_DEVICES][MAX_EVENTS];
bool g_events_ready[MAX_DEVICES] = {};
thread_local hipEvent_t* g_events = nullptr;      // the current call's set

int ensure_events() {
  int dev = 0;
  FC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= MAX_DEVICES) return FC_EINVAL;
  if (!g_events_ready[dev]) {
    for (int i = 0; i < MAX_EVENTS; ++i) FC_HIP(hipEventCreateWithFlags(&g_events_dev[dev][i], hipEventDisableTiming));
    g_events_ready[dev] = true;
  }
  g_events = g_events_dev[dev];
  return 0;
}

// ---- probe: HIP-event brackets around the convolution launches of a call (bench.py's roofline measurement) ----------------
struct ProbeRec { hipEvent_t a, b; int64_t meta[8]; };
std::vector<ProbeRec> g_probe;          // records since the last fc_exec_probe_read
std::vector<hipEvent_t> g_probe_pool;   // timing events, reused

hipEvent_t probe_event() {
  if (!g_probe_pool.empty()) { hipEvent_t e = g_probe_pool.back(); g_probe_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

inline double as_double(int64_t v) { double d; __builtin_memcpy(&d, &v, 8); return d; }

__global__ void k_add_inplace(float* __restrict__ dst, const float* __restrict__ src, int64_t n4) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n4) return;
  float4 a = reinterpret_cast<float4*>(dst)[t];
  const float4 b = reinterpret_cast<const float4*>(src)[t];
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  reinterpret_cast<float4*>(dst)[t] = a;
}

// desc[e] = {src, dst, C, nseg, seg_stride (floats), -, -, -}: dst[c] = sum_s src[s * seg_stride + c]  (the d gamma / d beta sums of every
// normalisation layer, written by the backward kernels into one persistent buffer, land in their gradient slices in ONE launch)
__global__ void k_small_grads(const long long* __restrict__ desc, int n) {
  const int e = blockIdx.x;
  if (e >= n) return;
  const long long* d = desc + 8 * e;
  const float* src = reinterpret_cast<const float*>(d[0]);
  float* dst = reinterpret_cast<float*>(d[1]);
  const int C = (int)d[2], nseg = (int)d[3];
  const long long stride = d[4];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < nseg; ++k) s += fc_ld(src + k * stride + c);
    dst[c] = s;
  }
}

// gW' (Cin, 8 Cout) of the generative transposed convolution's dense GEMM -> the layer's kernel gradient (8, Cin, Cout)
__global__ void k_permute_gent(const float* __restrict__ src, float* __restrict__ dst, int Cin, int Cout) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // index into dst
  const int64_t total = (int64_t)8 * Cin * Cout;
  if (t >= total) return;
  const int d = (int)(t % Cout), c = (int)((t / Cout) % Cin), k = (int)(t / ((int64_t)Cout * Cin));
  dst[t] = src[(int64_t)c * 8 * Cout + (int64_t)k * Cout + d];
}

// the packed head kernel's gradient: sum of the per-level partials (nl, R, ld) -> centerness (R, 1), reg (R, n_reg), cls (R, n_cls)
// ... and (r5) the class-bias gradient: sum over the levels of bias_part (nl, n_cls), the column sums fc_head_split_bwd_sums left
__global__ void k_head_wfin(const float* __restrict__ part, int nl, int R, int ld, int n_reg, int n_cls, float* __restrict__ g_cent,
                            float* __restrict__ g_reg, float* __restrict__ g_cls, const float* __restrict__ bias_part,
                            float* __restrict__ g_bias) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int ncol = 1 + n_reg + n_cls;
  if (g_bias && t < n_cls) {
    float b = 0.f;
    for (int l = 0; l < nl; ++l) b += fc_ld(&bias_part[l * n_cls + t]);
    g_bias[t] = b;
  }
  if (t >= R * ncol) return;
  const int r = t / ncol, c = t % ncol;
  float s = 0.f;
  for (int l = 0; l < nl; ++l) s += part[((int64_t)l * R + r) * ld + c];
  if (c == 0) g_cent[r] = s;
  else if (c <= n_reg) g_reg[r * n_reg + c - 1] = s;
  else g_cls[r * n_cls + c - 1 - n_reg] = s;
}

// dst[c] = sum over n rows of x[r][c] (C columns, any C): one 1024-thread block per column, rows strided over the threads, fixed
// tree order — the head's class-bias gradient (the column sums of d loss / d cls_score over every location of the batch)
__global__ __launch_bounds__(1024) void k_col_sum(const float* __restrict__ x, int64_t n, int C, float* __restrict__ dst) {
  __shared__ float red[1024];
  const int c = blockIdx.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int64_t r = threadIdx.x;
  for (; r + 3 * 1024 < n; r += 4 * 1024) {
    a0 += x[r * C + c]; a1 += x[(r + 1024) * C + c]; a2 += x[(r + 2048) * C + c]; a3 += x[(r + 3072) * C + c];
  }
  for (; r < n; r += 1024) a0 += x[r * C + c];
  red[threadIdx.x] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) dst[c] = red[0];
}

struct Ctx {
  const int64_t* ops;            // the WHOLE operator list (an operator may refer to its producer by index)
  const int64_t* addr;
  const int64_t* dims;
  const int64_t* maps;
  hipStream_t streams[NSTREAM];
  void* ws[NSTREAM];
  int64_t ws_bytes[NSTREAM];
  int64_t need[NSTREAM];
  bool dry;
  bool probe;
  int64_t bn_small_elems;
  int flags;
};

int run_op_impl(Ctx& c, const int64_t* op);

int run_op(Ctx& c, const int64_t* op) {
  if (c.dry || !c.probe || (op[ROW_OP] != OP_CONV && op[ROW_OP] != OP_AMAX)) return run_op_impl(c, op);
  ProbeRec r;
  r.a = probe_event(); r.b = probe_event();
  if (!r.a || !r.b) return run_op_impl(c, op);
  hipStream_t st = c.streams[op[ROW_STREAM]];
  if (op[ROW_OP] == OP_AMAX) {          // the amax pass of a convolution operand (h3): meta[0] = -2, n_in = rows, Cin = columns, no FLOPs
    const int64_t meta[8] = {-2, 0, c.dims[op[AMAX_N]], 0, 0, op[AMAX_C], 0, 0};
    __builtin_memcpy(r.meta, meta, sizeof meta);
  } else if (op[CONV_MAP] < 0) {
    const int64_t n = c.dims[op[CONV_N]];
    const int64_t meta[8] = {-1, op[CONV_DIR], n, n, 1, op[CONV_CIN], op[CONV_COUT], 0};
    __builtin_memcpy(r.meta, meta, sizeof meta);
  } else {
    const int64_t* mp = c.maps + op[CONV_MAP] * MAPW;
    const bool bwd = op[CONV_DIR] != 0;
    const int64_t meta[8] = {op[CONV_MAP], op[CONV_DIR], bwd ? mp[MAP_N_OUT] : mp[MAP_N_IN], bwd ? mp[MAP_N_IN] : mp[MAP_N_OUT], mp[MAP_K],
                             op[CONV_CIN], op[CONV_COUT], (mp[MAP_FLAGS] & (bwd ? MAP_ROUTE_BWD_PAIRS : MAP_ROUTE_FWD_PAIRS)) ? 1 : 0};
    __builtin_memcpy(r.meta, meta, sizeof meta);
  }
  FC_HIP(hipEventRecord(r.a, st));
  const int rc = run_op_impl(c, op);
  FC_HIP(hipEventRecord(r.b, st));
  g_probe.push_back(r);
  return rc;
}

// a field that holds an address index, -1 = none
template <class T>
inline T* P(const Ctx& c, int64_t idx) { return idx < 0 ? nullptr : reinterpret_cast<T*>(c.addr[idx]); }
// a ..._P1 field: address index + 1, 0 = none
template <class T>
inline T* P1(const Ctx& c, int64_t idx1) { return P<T>(c, idx1 - 1); }

// Row blocks of the statistics table the convolution operator `conv` leaves (CONV_STATS_P1): the route logic of OP_CONV below, as a
// pure function of the step's tables — the BatchNorm operator behind it may sit in another segment of a segmented run, so
// nothing is remembered from the launch.
int64_t stats_blocks_of(const Ctx& c, const int64_t* conv) {
  const int Cin = (int)conv[CONV_CIN], Cout = (int)conv[CONV_COUT];
  const int fl = c.flags | FC_CONV_SPLIT | FC_CONV_IMAGE;
  if (conv[CONV_MAP] < 0) return fc_conv_stats_blocks(c.dims[conv[CONV_N]], 1, Cin, Cout, fl, 0);
  const int64_t* m = c.maps + conv[CONV_MAP] * MAPW;
  const bool bwd = conv[CONV_DIR] != 0;
  return fc_conv_stats_blocks(bwd ? m[MAP_N_IN] : m[MAP_N_OUT], (int)m[MAP_K], Cin, Cout, fl,
                              (m[MAP_FLAGS] & (bwd ? MAP_ROUTE_BWD_PAIRS : MAP_ROUTE_FWD_PAIRS)) ? 1 : 0);
}

inline bool want_ws(Ctx& c, int s, int64_t bytes) {     // true: the launch may go ahead
  if (bytes > c.need[s]) c.need[s] = bytes;
  return !c.dry;
}

int run_op_impl(Ctx& c, const int64_t* op) {
  const int s = (int)op[ROW_STREAM];
  hipStream_t st = c.streams[s];
#ifdef FC_KO_EXEC
  // knock-out build (tools/knockout.sh FC_KO_EXEC; never the product library): FC_KO_OPS = bit mask of op families NOT launched
  // (1 weight gradients, 2 convolutions, 4 normalisation) — what the step costs without them (results are garbage)
  {
    static const int ko = getenv("FC_KO_OPS") ? atoi(getenv("FC_KO_OPS")) : 0;
    const int64_t o = op[ROW_OP];
    if (!c.dry && (((ko & 1) && (o == OP_WGRAD || o == OP_STEM_WGRAD)) || ((ko & 2) && o == OP_CONV) ||
                   ((ko & 4) && (o == OP_BN_FWD || o == OP_BN_BWD || o == OP_BN_EVAL_BWD || o == OP_COL_STATS || o == OP_NORM_POOL_FWD || o == OP_POOL_NORM_BWD))))
      return 0;
  }
#endif
  switch (op[ROW_OP]) {
    case OP_STEM_FWD: {
      const int64_t* m = c.maps + op[STEM_FWD_MAP] * MAPW;
      if (c.dry) return 0;
      return fc_stem_conv_fwd(P<const float>(c, op[STEM_FWD_X]), P<const float>(c, op[STEM_FWD_W]), reinterpret_cast<const int*>(m[MAP_NBR]),
                              P<float>(c, op[STEM_FWD_OUT]), P<float>(c, op[STEM_FWD_COL]), m[MAP_N_IN], m[MAP_N_OUT], (int)m[MAP_K], st);
    }
    case OP_COL_STATS: {
      const int64_t n = c.dims[op[COL_STATS_N]];
      const int C = (int)op[COL_STATS_C], nseg = (int)c.dims[op[COL_STATS_NSEG]];
      if (!want_ws(c, s, fc_col_stats_ws_bytes(n, C, nseg))) return 0;
      return fc_col_stats(P<const float>(c, op[COL_STATS_X]), P<const int>(c, op[COL_STATS_SEG]), op[COL_STATS_SEG] >= 0 ? 4 : 0, n, C, nseg,
                          P<float>(c, op[COL_STATS_MEAN]), P<float>(c, op[COL_STATS_VAR]), P<float>(c, op[COL_STATS_CNT]), c.ws[s],
                          c.ws_bytes[s], st);
    }
    case OP_CONV: {
      const int Cin = (int)op[CONV_CIN], Cout = (int)op[CONV_COUT];
      const int fl = c.flags | FC_CONV_SPLIT | FC_CONV_IMAGE;
      float* stats = (op[CONV_STATS_P1] > 0 && stats_blocks_of(c, op) > 0) ? P1<float>(c, op[CONV_STATS_P1]) : nullptr;
      const float* bnx = stats ? P1<const float>(c, op[CONV_BN_X_P1]) : nullptr;
      const float *bmean = P<const float>(c, op[CONV_BN_MEAN]), *bvar = P<const float>(c, op[CONV_BN_VAR]),
                  *bga = P<const float>(c, op[CONV_BN_GAMMA]), *bbe = P<const float>(c, op[CONV_BN_BETA]);
      const float beps = (float)as_double(op[CONV_BN_EPS]);
      const int bact = (int)op[CONV_BN_ACT];
      const float* badd = P1<const float>(c, op[CONV_BN_ADD_P1]);
      const float* bny = P1<const float>(c, op[CONV_BN_Y_P1]);
      const float* in = P<const float>(c, op[CONV_X]);
      const float* img = P<const float>(c, op[CONV_IMG]);
      float* out = P<float>(c, op[CONV_OUT]);
      // the amax word of `in` is consumed by the ONE call below
      if (!c.dry && op[CONV_AMAX_X_P1] > 0) fc_conv_amax_hint(P1<const unsigned>(c, op[CONV_AMAX_X_P1]), nullptr);
      if (op[CONV_MAP] < 0) {
        const int64_t n = c.dims[op[CONV_N]];
        if (!want_ws(c, s, fc_conv_fwd_ws_bytes(n, 1, Cin, Cout, fl))) return 0;
        if (bnx)
          return fc_conv_fwd_bn_bwd_stats(in, img, nullptr, nullptr, out, n, n, 1, Cin, Cout, fl, c.ws[s], c.ws_bytes[s], stats, bnx, bmean, bvar,
                                          bga, bbe, beps, bact, badd, bny, st);
        return fc_conv_fwd_stats(in, img, nullptr, nullptr, out, n, n, 1, Cin, Cout, fl, c.ws[s], c.ws_bytes[s], stats, st);
      }
      const int64_t* m = c.maps + op[CONV_MAP] * MAPW;
      const bool bwd = op[CONV_DIR] != 0;
      const int64_t n_in = bwd ? m[MAP_N_OUT] : m[MAP_N_IN], n_out = bwd ? m[MAP_N_IN] : m[MAP_N_OUT];
      const int K = (int)m[MAP_K];
      if (m[MAP_FLAGS] & (bwd ? MAP_ROUTE_BWD_PAIRS : MAP_ROUTE_FWD_PAIRS)) {                       // per offset over the exact pair lists
        const int64_t* pr = m + (bwd ? MAP_PAIRS_T : MAP_PAIRS);
        const int *pi = reinterpret_cast<const int*>(pr[PAIR_IN]), *pc = reinterpret_cast<const int*>(pr[PAIR_CNT]),
                  *pp = reinterpret_cast<const int*>(pr[PAIR_POS]);
        if (!want_ws(c, s, fc_conv_fwd_pairs_ws_bytes(n_out, K, Cout))) return 0;
        if (bnx)
          return fc_conv_fwd_pairs_tiles_bn_bwd_stats(in, img, pi, pc, pp, out, n_in, n_out, K, Cin, Cout, pr[PAIR_TILES], fl, c.ws[s],
                                                      c.ws_bytes[s], stats, bnx, bmean, bvar, bga, bbe, beps, bact, badd, bny, st);
        return fc_conv_fwd_pairs_tiles_stats(in, img, pi, pc, pp, out, n_in, n_out, K, Cin, Cout, pr[PAIR_TILES], fl, c.ws[s], c.ws_bytes[s],
                                             stats, st);
      }
      const int *tab = reinterpret_cast<const int*>(bwd ? m[MAP_BWD_TAB] : m[MAP_FWD_TAB]),
                *oidx = reinterpret_cast<const int*>(bwd ? m[MAP_BWD_IDX] : m[MAP_FWD_IDX]);
      if (!want_ws(c, s, fc_conv_fwd_ws_bytes(n_out, K, Cin, Cout, fl))) return 0;
      if (bnx)
        return fc_conv_fwd_bn_bwd_stats(in, img, tab, oidx, out, n_in, n_out, K, Cin, Cout, fl, c.ws[s], c.ws_bytes[s], stats, bnx, bmean, bvar,
                                        bga, bbe, beps, bact, badd, bny, st);
      return fc_conv_fwd_stats(in, img, tab, oidx, out, n_in, n_out, K, Cin, Cout, fl, c.ws[s], c.ws_bytes[s], stats, st);
    }
    case OP_BN_FWD: {
      const int64_t n = c.dims[op[BN_FWD_N]];
      const int C = (int)op[BN_FWD_C];
      const float eps = (float)as_double(op[BN_FWD_EPS]), mom = (float)as_double(op[BN_FWD_MOMENTUM]);
      const int* add_inv = P1<const int>(c, op[BN_FWD_ADD_INV_P1]);
      const float* add_src = op[BN_FWD_ADD_INV_P1] > 0 ? P1<const float>(c, op[BN_FWD_ADD_SRC_P1]) : nullptr;
      if (!op[BN_FWD_TRAIN]) {      // eval mode: the running statistics are the statistics
        if (c.dry) return 0;
        if (op[BN_FWD_AMAX_Y_P1] > 0) fc_amax_out_hint(P1<unsigned>(c, op[BN_FWD_AMAX_Y_P1]));
        return fc_norm_act_add_fwd(P<const float>(c, op[BN_FWD_X]), nullptr, 0, n, C, P<const float>(c, op[BN_FWD_RMEAN]),
                                   P<const float>(c, op[BN_FWD_RVAR]), eps, P<const float>(c, op[BN_FWD_GAMMA]),
                                   P<const float>(c, op[BN_FWD_BETA]), P<const float>(c, op[BN_FWD_RES]), (int)op[BN_FWD_ACT], add_inv, add_src,
                                   P<float>(c, op[BN_FWD_Y]), st);
      }
      // training: statistics from the producer's epilogue when the operator names one and that launch has a statistics epilogue;
      // else computed from x (fc_bn_train_fwd)
      const float* part = nullptr;
      int64_t nbp = 0;
      if (op[BN_FWD_PRODUCER_P1] > 0) {
        const int64_t* conv = c.ops + (op[BN_FWD_PRODUCER_P1] - 1) * OPW;
        nbp = conv[CONV_STATS_P1] > 0 ? stats_blocks_of(c, conv) : 0;
        if (nbp > 0) part = P1<const float>(c, conv[CONV_STATS_P1]);
      }
      if (!want_ws(c, s, fc_bn_train_ws_bytes(n, C))) return 0;
      if (op[BN_FWD_AMAX_Y_P1] > 0) fc_amax_out_hint(P1<unsigned>(c, op[BN_FWD_AMAX_Y_P1]));         // (h3: y feeds a convolution)
      return fc_bn_train_add_fwd(P<const float>(c, op[BN_FWD_X]), n, C, eps, P<const float>(c, op[BN_FWD_GAMMA]),
                                 P<const float>(c, op[BN_FWD_BETA]), P<const float>(c, op[BN_FWD_RES]), (int)op[BN_FWD_ACT], mom,
                                 P<float>(c, op[BN_FWD_Y]), P<float>(c, op[BN_FWD_MEAN]), P<float>(c, op[BN_FWD_VAR]),
                                 P<float>(c, op[BN_FWD_CNT]), P<float>(c, op[BN_FWD_RMEAN]), P<float>(c, op[BN_FWD_RVAR]),
                                 P<long long>(c, op[BN_FWD_NBT]), part, nbp, op[BN_FWD_GROUPS] > 0 ? (int)op[BN_FWD_GROUPS] : 1,
                                 c.bn_small_elems, add_inv, add_src, c.ws[s], c.ws_bytes[s], st);
    }
    case OP_HEAD_FWD: {
      if (c.dry) return 0;
      return fc_head_split_fwd(P<const float>(c, op[HEAD_FWD_Y]), (int)op[HEAD_FWD_LD], P<const float>(c, op[HEAD_FWD_BIAS]),
                               P<const float>(c, op[HEAD_FWD_SCALE]), c.dims[op[HEAD_FWD_N]], (int)op[HEAD_FWD_N_REG], (int)op[HEAD_FWD_N_CLS],
                               P<float>(c, op[HEAD_FWD_CENT]), P<float>(c, op[HEAD_FWD_BBOX]), P<float>(c, op[HEAD_FWD_CLS]),
                               P<float>(c, op[HEAD_FWD_CMAX]), st);
    }
    case OP_RECORD:
      if (c.dry) return 0;
      FC_HIP(hipEventRecord(g_events[op[RECORD_EVENT]], st));
      return 0;
    case OP_WAIT:
      if (c.dry) return 0;
      FC_HIP(hipStreamWaitEvent(st, g_events[op[WAIT_EVENT]], 0));
      return 0;
    case OP_HEAD_BWD: {
      const float *y = P<const float>(c, op[HEAD_BWD_Y]), *scale = P<const float>(c, op[HEAD_BWD_SCALE]),
                  *bbox = P<const float>(c, op[HEAD_BWD_BBOX]), *g_cent = P<const float>(c, op[HEAD_BWD_G_CENT]),
                  *g_bbox = P<const float>(c, op[HEAD_BWD_G_BBOX]), *g_cls = P<const float>(c, op[HEAD_BWD_G_CLS]);
      const int64_t n = c.dims[op[HEAD_BWD_N]];
      const int ld = (int)op[HEAD_BWD_LD], n_reg = (int)op[HEAD_BWD_N_REG], n_cls = (int)op[HEAD_BWD_N_CLS];
      if (op[HEAD_BWD_GS_ROW] < 0) {    // with the scale / class-bias reductions of this level (fc_head_split_bwd_sums)
        if (!want_ws(c, s, fc_head_split_bwd_sums_ws_bytes(n))) return 0;
        if (op[HEAD_BWD_AMAX_GY_P1] > 0) fc_amax_out_hint(P1<unsigned>(c, op[HEAD_BWD_AMAX_GY_P1]));
        return fc_head_split_bwd_sums(y, ld, scale, bbox, g_cent, g_bbox, g_cls, n, n_reg, n_cls, P<float>(c, op[HEAD_BWD_GY]),
                                      P<float>(c, op[HEAD_BWD_BIAS_PART]), P<float>(c, op[HEAD_BWD_G_SCALE]), c.ws[s], c.ws_bytes[s], st);
      }
      if (c.dry) return 0;
      return fc_head_split_bwd(y, ld, scale, bbox, g_cent, g_bbox, g_cls, n, n_reg, n_cls, P<float>(c, op[HEAD_BWD_GY]),
                               P<float>(c, op[HEAD_BWD_GS_ROW]), st);
    }
    case OP_WGRAD: {
      const int Cin = (int)op[WGRAD_CIN], Cout = (int)op[WGRAD_COUT];
      const int fl = c.flags | FC_CONV_SPLIT;
      const float *in = P<const float>(c, op[WGRAD_X]), *gout = P<const float>(c, op[WGRAD_GOUT]);
      float* gw = P<float>(c, op[WGRAD_GW]);
      if (!c.dry && (op[WGRAD_AMAX_X_P1] > 0 || op[WGRAD_AMAX_GOUT_P1] > 0))
        fc_conv_amax_hint(P1<const unsigned>(c, op[WGRAD_AMAX_X_P1]), P1<const unsigned>(c, op[WGRAD_AMAX_GOUT_P1]));
      if (op[WGRAD_MAP] < 0) {
        const int64_t n = c.dims[op[WGRAD_N]];
        if (!want_ws(c, s, fc_conv_wgrad_ws_bytes(n, 1, Cin, Cout, fl))) return 0;
        return fc_conv_wgrad(in, gout, nullptr, nullptr, gw, n, n, 1, Cin, Cout, fl, c.ws[s], c.ws_bytes[s], st);
      }
      const int64_t* m = c.maps + op[WGRAD_MAP] * MAPW;
      const int K = (int)m[MAP_K];
      if (!want_ws(c, s, fc_conv_wgrad_ws_bytes(m[MAP_N_OUT], K, Cin, Cout, fl))) return 0;
      if ((m[MAP_FLAGS] & MAP_ROUTE_WGRAD_PAIRS) && Cin % 64 == 0 && Cout % 64 == 0) {
        const int64_t* pr = m + MAP_PAIRS;
        return fc_conv_wgrad_pairs(in, gout, reinterpret_cast<const int*>(pr[PAIR_IN]), reinterpret_cast<const int*>(pr[PAIR_OUT]),
                                   reinterpret_cast<const int*>(pr[PAIR_CNT]), gw, m[MAP_N_IN], m[MAP_N_OUT], K, Cin, Cout, fl, c.ws[s],
                                   c.ws_bytes[s], st);
      }
      return fc_conv_wgrad(in, gout, reinterpret_cast<const int*>(m[MAP_NBR]), nullptr, gw, m[MAP_N_IN], m[MAP_N_OUT], K, Cin, Cout, fl,
                           c.ws[s], c.ws_bytes[s], st);
    }
    case OP_BN_BWD: {
      const int64_t n = c.dims[op[BN_BWD_N]];
      const int C = (int)op[BN_BWD_C];
      const float eps = (float)as_double(op[BN_BWD_EPS]);
      // the backward-data convolution that wrote gy may have left this layer's two reductions in its epilogue (fc_conv_fwd_bn_bwd_stats)
      const float* part = nullptr;
      int64_t nbp = 0;
      if (op[BN_BWD_PRODUCER_P1] > 0) {
        const int64_t* conv = c.ops + (op[BN_BWD_PRODUCER_P1] - 1) * OPW;
        nbp = (conv[CONV_STATS_P1] > 0 && conv[CONV_BN_X_P1] > 0) ? stats_blocks_of(c, conv) : 0;
        if (nbp > 0) part = P1<const float>(c, conv[CONV_STATS_P1]);
      }
      if (!want_ws(c, s, fc_bn_train_ws_bytes(n, C))) return 0;
      if (op[BN_BWD_AMAX_GX_P1] > 0) fc_amax_out_hint(P1<unsigned>(c, op[BN_BWD_AMAX_GX_P1]));
      return fc_bn_train_bwd(P<const float>(c, op[BN_BWD_X]), P<const float>(c, op[BN_BWD_Y]), P<const float>(c, op[BN_BWD_GY]),
                             P1<const float>(c, op[BN_BWD_GY2_P1]), n, C, P<const float>(c, op[BN_BWD_MEAN]),
                             P<const float>(c, op[BN_BWD_VAR]), P<const float>(c, op[BN_BWD_CNT]), eps, P<const float>(c, op[BN_BWD_GAMMA]),
                             P<const float>(c, op[BN_BWD_BETA]), (int)op[BN_BWD_ACT], P<float>(c, op[BN_BWD_GX]),
                             P<float>(c, op[BN_BWD_GRES]), P<float>(c, op[BN_BWD_SUMS]), part, nbp, c.bn_small_elems, c.ws[s],
                             c.ws_bytes[s], st);
    }
    case OP_BN_EVAL_BWD: {
      const int64_t n = c.dims[op[BN_EVAL_BWD_N]];
      const int C = (int)op[BN_EVAL_BWD_C];
      float* sums = P<float>(c, op[BN_EVAL_BWD_SUMS]);
      if (!want_ws(c, s, fc_bn_eval_bwd_ws_bytes(n, C, op[BN_EVAL_BWD_SUMS] >= 0))) return 0;
      return fc_bn_eval_bwd(P<const float>(c, op[BN_EVAL_BWD_X]), P<const float>(c, op[BN_EVAL_BWD_Y]), P<const float>(c, op[BN_EVAL_BWD_GY]),
                            P1<const float>(c, op[BN_EVAL_BWD_GY2_P1]), n, C, P<const float>(c, op[BN_EVAL_BWD_RMEAN]),
                            P<const float>(c, op[BN_EVAL_BWD_RVAR]), (float)as_double(op[BN_EVAL_BWD_EPS]), P<const float>(c, op[BN_EVAL_BWD_GAMMA]),
                            P<const float>(c, op[BN_EVAL_BWD_BETA]), (int)op[BN_EVAL_BWD_ACT], P<float>(c, op[BN_EVAL_BWD_GX]),
                            P<float>(c, op[BN_EVAL_BWD_GRES]), sums, P1<unsigned>(c, op[BN_EVAL_BWD_AMAX_GX_P1]), c.ws[s], c.ws_bytes[s], st);
    }
    case OP_STEM_WGRAD: {
      const int64_t* m = c.maps + op[STEM_WGRAD_MAP] * MAPW;
      if (!want_ws(c, s, fc_stem_conv_wgrad_ws_bytes(m[MAP_N_OUT], (int)m[MAP_K]))) return 0;
      return fc_stem_conv_wgrad(P<const float>(c, op[STEM_WGRAD_COL]), P<const float>(c, op[STEM_WGRAD_GOUT]), P<float>(c, op[STEM_WGRAD_GW]),
                                m[MAP_N_OUT], (int)m[MAP_K], c.ws[s], c.ws_bytes[s], st);
    }
    case OP_GATHER: {
      if (c.dry) return 0;
      return fc_gather_rows(P<const float>(c, op[GATHER_SRC]), P<const int>(c, op[GATHER_IDX]), c.dims[op[GATHER_N]], (int)op[GATHER_C],
                            P<float>(c, op[GATHER_DST]), st);
    }
    case OP_ADD: {
      if (c.dry) return 0;
      const int64_t n4 = c.dims[op[ADD_N]] * op[ADD_C] / 4;
      if (n4 > 0) k_add_inplace<<<(unsigned)fc_cdiv(n4, 256), 256, 0, st>>>(P<float>(c, op[ADD_DST]), P<const float>(c, op[ADD_SRC]), n4);
      FC_CHECK_LAUNCH();
      return 0;
    }
    case OP_SMALL_GRADS: {
      if (c.dry) return 0;
      const int64_t cnt = op[SMALL_GRADS_COUNT];
      if (cnt > 0) k_small_grads<<<(unsigned)cnt, 128, 0, st>>>(P<const long long>(c, op[SMALL_GRADS_DESC]) + 8 * op[SMALL_GRADS_FIRST], (int)cnt);
      FC_CHECK_LAUNCH();
      return 0;
    }
    case OP_COL_SUM: {
      if (c.dry) return 0;
      k_col_sum<<<(unsigned)op[COL_SUM_C], 1024, 0, st>>>(P<const float>(c, op[COL_SUM_X]), c.dims[op[COL_SUM_N]], (int)op[COL_SUM_C],
                                                         P<float>(c, op[COL_SUM_DST]));
      FC_CHECK_LAUNCH();
      return 0;
    }
    case OP_ROW_SUM: {
      if (c.dry) return 0;
      k_col_sum<<<1, 1024, 0, st>>>(P<const float>(c, op[ROW_SUM_X]), c.dims[op[ROW_SUM_N]], 1, P<float>(c, op[ROW_SUM_DST]));
      FC_CHECK_LAUNCH();
      return 0;
    }
    case OP_PERMUTE_GENT: {
      if (c.dry) return 0;
      const int Cin = (int)op[PERMUTE_GENT_CIN], Cout = (int)op[PERMUTE_GENT_COUT];
      const int64_t total = (int64_t)8 * Cin * Cout;
      k_permute_gent<<<(unsigned)fc_cdiv(total, 256), 256, 0, st>>>(P<const float>(c, op[PERMUTE_GENT_SRC]), P<float>(c, op[PERMUTE_GENT_DST]),
                                                                    Cin, Cout);
      FC_CHECK_LAUNCH();
      return 0;
    }
    case OP_HEAD_WFIN: {
      if (c.dry) return 0;
      const int R = (int)op[HEAD_WFIN_R], n_reg = (int)op[HEAD_WFIN_N_REG], n_cls = (int)op[HEAD_WFIN_N_CLS];
      const int total = R * (1 + n_reg + n_cls);
      k_head_wfin<<<(unsigned)fc_cdiv(total, 256), 256, 0, st>>>(P<const float>(c, op[HEAD_WFIN_PART]), (int)op[HEAD_WFIN_NL], R,
                                                                 (int)op[HEAD_WFIN_LD], n_reg, n_cls, P<float>(c, op[HEAD_WFIN_G_CENT]),
                                                                 P<float>(c, op[HEAD_WFIN_G_REG]), P<float>(c, op[HEAD_WFIN_G_CLS]),
                                                                 P<const float>(c, op[HEAD_WFIN_BIAS_PART]), P<float>(c, op[HEAD_WFIN_G_BIAS]));
      FC_CHECK_LAUNCH();
      return 0;
    }
    case OP_AMAX: {
      if (c.dry) return 0;
      return fc_amax(P<const float>(c, op[AMAX_X]), c.dims[op[AMAX_N]] * op[AMAX_C], P<unsigned>(c, op[AMAX_SLOT]), st);
    }
    case OP_CLEAR: {
      if (c.dry) return 0;
      FC_HIP(hipMemsetAsync(P<void>(c, op[CLEAR_DST]), 0, (size_t)op[CLEAR_BYTES], st));
      return 0;
    }
    case OP_NORM_POOL_FWD: {
      const int64_t* m = c.maps + op[NORM_POOL_FWD_MAP] * MAPW;
      if (c.dry) return 0;
      if ((int)m[MAP_K] != 8) return FC_EINVAL;
      if (op[NORM_POOL_FWD_AMAX_OUT_P1] > 0) fc_amax_out_hint(P1<unsigned>(c, op[NORM_POOL_FWD_AMAX_OUT_P1]));
      if (op[NORM_POOL_FWD_MASK_P1] > 0)      // a training program: the per-child mask for the backward pass, the arg-max rows only where kept
        return fc_norm_act_maxpool8_mask_fwd(P<const float>(c, op[NORM_POOL_FWD_X]), P<const int>(c, op[NORM_POOL_FWD_SEG]),
                                             op[NORM_POOL_FWD_SEG] >= 0 ? 4 : 0, (int)op[NORM_POOL_FWD_C], P<const float>(c, op[NORM_POOL_FWD_MEAN]),
                                             P<const float>(c, op[NORM_POOL_FWD_VAR]), (float)as_double(op[NORM_POOL_FWD_EPS]),
                                             P<const float>(c, op[NORM_POOL_FWD_GAMMA]), P<const float>(c, op[NORM_POOL_FWD_BETA]),
                                             (int)op[NORM_POOL_FWD_ACT], reinterpret_cast<const int*>(m[MAP_NBR]), m[MAP_N_OUT],
                                             P<float>(c, op[NORM_POOL_FWD_OUT]), P<int>(c, op[NORM_POOL_FWD_ARG]), P<float>(c, op[NORM_POOL_FWD_Y]),
                                             P<int>(c, op[NORM_POOL_FWD_PARENT]), P1<unsigned long long>(c, op[NORM_POOL_FWD_MASK_P1]), st);
      return fc_norm_act_maxpool8_fwd(P<const float>(c, op[NORM_POOL_FWD_X]), P<const int>(c, op[NORM_POOL_FWD_SEG]),
                                      op[NORM_POOL_FWD_SEG] >= 0 ? 4 : 0, (int)op[NORM_POOL_FWD_C], P<const float>(c, op[NORM_POOL_FWD_MEAN]),
                                      P<const float>(c, op[NORM_POOL_FWD_VAR]), (float)as_double(op[NORM_POOL_FWD_EPS]),
                                      P<const float>(c, op[NORM_POOL_FWD_GAMMA]), P<const float>(c, op[NORM_POOL_FWD_BETA]),
                                      (int)op[NORM_POOL_FWD_ACT], reinterpret_cast<const int*>(m[MAP_NBR]), m[MAP_N_OUT],
                                      P<float>(c, op[NORM_POOL_FWD_OUT]), P<int>(c, op[NORM_POOL_FWD_ARG]), P<float>(c, op[NORM_POOL_FWD_Y]),
                                      P<int>(c, op[NORM_POOL_FWD_PARENT]), st);
    }
    case OP_POOL_NORM_BWD: {
      const int64_t n = c.dims[op[POOL_NORM_BWD_N]];
      const int C = (int)op[POOL_NORM_BWD_C], nseg = (int)c.dims[op[POOL_NORM_BWD_NSEG]];
      if (!want_ws(c, s, fc_maxpool8_norm_act_bwd_ws_bytes(n, C, nseg))) return 0;
      if (op[POOL_NORM_BWD_MASK_P1] > 0)
        return fc_maxpool8_mask_norm_act_bwd(P<const float>(c, op[POOL_NORM_BWD_X]), P<const float>(c, op[POOL_NORM_BWD_G_POOL]),
                                             P1<const unsigned long long>(c, op[POOL_NORM_BWD_MASK_P1]), P<const int>(c, op[POOL_NORM_BWD_PARENT]),
                                             P<const int>(c, op[POOL_NORM_BWD_SEG]), op[POOL_NORM_BWD_SEG] >= 0 ? 4 : 0, n, C, nseg,
                                             P<const float>(c, op[POOL_NORM_BWD_MEAN]), P<const float>(c, op[POOL_NORM_BWD_VAR]),
                                             P<const float>(c, op[POOL_NORM_BWD_CNT]), (float)as_double(op[POOL_NORM_BWD_EPS]),
                                             P<const float>(c, op[POOL_NORM_BWD_GAMMA]), P<const float>(c, op[POOL_NORM_BWD_BETA]),
                                             (int)op[POOL_NORM_BWD_ACT], P<float>(c, op[POOL_NORM_BWD_GX]), P<float>(c, op[POOL_NORM_BWD_SUMS]),
                                             c.ws[s], c.ws_bytes[s], st);
      return fc_maxpool8_norm_act_bwd(P<const float>(c, op[POOL_NORM_BWD_X]), P<const float>(c, op[POOL_NORM_BWD_G_POOL]),
                                      P<const int>(c, op[POOL_NORM_BWD_ARG]), P<const int>(c, op[POOL_NORM_BWD_PARENT]),
                                      P<const int>(c, op[POOL_NORM_BWD_SEG]), op[POOL_NORM_BWD_SEG] >= 0 ? 4 : 0, n, C, nseg,
                                      P<const float>(c, op[POOL_NORM_BWD_MEAN]), P<const float>(c, op[POOL_NORM_BWD_VAR]),
                                      P<const float>(c, op[POOL_NORM_BWD_CNT]), (float)as_double(op[POOL_NORM_BWD_EPS]),
                                      P<const float>(c, op[POOL_NORM_BWD_GAMMA]), P<const float>(c, op[POOL_NORM_BWD_BETA]),
                                      (int)op[POOL_NORM_BWD_ACT], P<float>(c, op[POOL_NORM_BWD_GX]), P<float>(c, op[POOL_NORM_BWD_SUMS]),
                                      c.ws[s], c.ws_bytes[s], st);
    }
    case OP_INV_ROWS: {
      if (c.dry) return 0;
      return fc_inverse_rows(P<const int>(c, op[INV_ROWS_ROWS]), c.dims[op[INV_ROWS_N]], c.dims[op[INV_ROWS_N_INV]], P<int>(c, op[INV_ROWS_INV]), st);
    }
    case OP_COPY: {
      if (c.dry) return 0;
      FC_HIP(hipMemcpyAsync(P<float>(c, op[COPY_DST]), P<const float>(c, op[COPY_SRC]), sizeof(float) * c.dims[op[COPY_N]] * op[COPY_C],
                            hipMemcpyDeviceToDevice, st));
      return 0;
    }
    default:
      return FC_EINVAL;
  }
}

}  // namespace

extern "C" {

int fc_exec_op_words(void) { return OPW; }
int fc_exec_map_words(void) { return MAPW; }

// Runs operators [op_begin, op_end) of `ops` (HOST array, fc_exec_op_words() int64 per operator; layouts: csrc/exec_ops.h).
// addr / dims / maps: HOST arrays of device addresses, row counts and kernel-map descriptors the operators index.
// streams / ws / ws_bytes: 3 entries each (0 main, 1 head branch, 2 weight gradients).  A first pass sizes the scratch space of
// every operator; if a stream's workspace is too small NOTHING is launched, ws_need[3] holds the required sizes and the call
// returns -2.  cfg[0] = bn_small_elems (functional.BN_SMALL_ELEMS), cfg[1] = kernel-variant flags (functional.FLAGS), cfg[2] != 0:
// probe (below), cfg[3] != 0: the sizing pass ONLY (ws_need is filled, -2 if a workspace is too small, nothing is launched).
int fc_exec(const int64_t* ops, int64_t op_begin, int64_t op_end, const int64_t* addr, const int64_t* dims, const int64_t* maps,
            const int64_t* streams, const int64_t* ws, const int64_t* ws_bytes, int64_t* ws_need, const int64_t* cfg) {
  if (!ops || op_begin < 0 || op_end < op_begin) return FC_EINVAL;
  int rc = ensure_events();
  if (rc) return rc;
  Ctx c;
  c.ops = ops;
  c.addr = addr; c.dims = dims; c.maps = maps;
  for (int i = 0; i < NSTREAM; ++i) {
    c.streams[i] = reinterpret_cast<hipStream_t>(streams[i]);
    c.ws[i] = reinterpret_cast<void*>(ws[i]);
    c.ws_bytes[i] = ws_bytes[i];
    c.need[i] = 0;
  }
  c.bn_small_elems = cfg[0];
  c.flags = (int)cfg[1];
  c.probe = cfg[2] != 0;
  c.dry = true;
  for (int64_t i = op_begin; i < op_end; ++i) {
    rc = run_op(c, ops + i * OPW);
    if (rc) return rc;
  }
  bool ok = true;
  for (int i = 0; i < NSTREAM; ++i) {
    if (ws_need) ws_need[i] = c.need[i];
    if (c.need[i] > c.ws_bytes[i]) ok = false;
  }
  if (!ok) return FC_EWS;
  if (cfg[3]) return 0;
  c.dry = false;
  for (int64_t i = op_begin; i < op_end; ++i) {
    rc = run_op(c, ops + i * OPW);
    if (rc) return rc;
  }
  return 0;
}

// Probe read-out (cfg[2] != 0 in fc_exec: a HIP-event pair brackets every convolution operator, on the stream it is launched
// on).  Call after the device has drained: ms[i] = duration of record i, meta[8 i ..] = {map index or -1, direction, n_in, n_out,
// K, Cin, Cout, 1 if the per-offset pair-list route ran}; returns the number of records (at most cap are written) and forgets them.
int64_t fc_exec_probe_read(float* ms, int64_t* meta, int64_t cap) {
  const int64_t n = (int64_t)g_probe.size();
  for (int64_t i = 0; i < n; ++i) {
    ProbeRec& r = g_probe[i];
    if (i < cap) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) t = -1.f;
      ms[i] = t;
      __builtin_memcpy(meta + 8 * i, r.meta, sizeof r.meta);
    }
    g_probe_pool.push_back(r.a);
    g_probe_pool.push_back(r.b);
  }
  g_probe.clear();
  return n;
}

}  // extern "C"
