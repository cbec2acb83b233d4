// The coordinate phase of one step as native host loops (r6): collate + voxel hash + the whole pyramid of coordinate sets,
// then every kernel map and derived table the network body will use — two C-ABI calls per step instead of ~420 launches
// driven from Python with ~25 blocking count read-backs (profiles/r5_notes.md section 16: the step was host-bound on them
// whenever a round trip on the coordinate stream took 0.3 ms longer than usual).
//
//   fc_plan_levels  points of B scenes -> [cm0, m1, m2, L1..Lnl]: the collate of single_stage_sparse.py:34-37 and the strided
//                   output sets of me_resnet.py:19-24, :56-62, built as ONE chain with DEVICE-resident row counts (every kernel
//                   is launched for the upper bound and reads the live count from the previous set's meta word), then ONE
//                   read-back of all counts (rows per set, rows per set and scene, range flags).
//   fc_plan_maps    with those counts: every kernel map of the backbone and the neck (generated sets by index arithmetic),
//                   mask-sorted tables (native LSD radix argsort), pair lists, transposed tables, union rows, the head's
//                   location / scene / level arrays — enqueued back to back, then ONE read-back (pair-list counts, union hits).
//
// Results are the sets, tables and row orders of the per-operator path (fcaf3d_amd/sparse.py -> csrc/coords.hip), bit for
// bit: tests/test_gpu_plan.py compares every buffer.  Reference: what this replaces is ME's CoordinateManager work inside
// ME.SparseTensor(...) and every ME.Minkowski* call of extract_feat (mmdet3d/models/detectors/single_stage_sparse.py:32-40).
// This file is the host side; the kernels live in headers by family, the layout of every host table in plan_layout.h.
#include "fc_common.h"
#include "../../include/fcaf3d_hip.h"
#include "plan_layout.h"     // cfg / out / meta / counter-block words, probe kinds: read by fcaf3d_amd/plan.py too
#include "exec_ops.h"        // MAPW, MAP_*, PAIR_*, MAP_ROUTE_*: the kernel-map descriptors inside a map record
#include "plan_batch.h"      // Bump, Bracket (probe), Batch<J>, batch_find, launch_batch
#include "plan_chain.h"      // stage 1: k_plan_tables_init, k_plan_voxelize_insert, k_plan_insert, k_plan_flags, k_plan_finalize
#include "plan_radix.h"      // SortJob, k_radix_hist / _scan / _scatter, argsort27_batch
#include "plan_maps.h"       // stage 2: k_plan_kernel_maps / _strided_maps / _rows / _gen_coords / _gen_rows / _head_arrays / _row_masks / _permute / _pairs_*
#include <string.h>

static_assert(MW_FLAGS < MW_DESC_F && MW_DESC_F + MAPW <= MW_DESC_B && MW_DESC_B + MAPW <= MAPR, "both descriptors fit inside a map record");
// the pair-list words of a map record are one PAIR_* group each
static_assert(MW_PO - MW_PI == PAIR_OUT && MW_POS - MW_PI == PAIR_POS && MW_CNT - MW_PI == PAIR_CNT && MW_TILES - MW_PI == PAIR_TILES, "MW_PI group");
static_assert(MW_TPO - MW_TPI == PAIR_OUT && MW_TPOS - MW_TPI == PAIR_POS && MW_TCNT - MW_TPI == PAIR_CNT && MW_TTILES - MW_TPI == PAIR_TILES, "MW_TPI group");
static_assert(CNT_T + 27 <= CNT_MAP && 2 + 2 * MAXLV <= MAXSETS, "counter block; chain sets + generated sets");

namespace {

inline double as_double(int64_t v) { double d; memcpy(&d, &v, 8); return d; }
inline int64_t next_pow2(int64_t n) { int64_t p = 2; while (p < n) p *= 2; return p; }
inline int max_maps(int nl) { return MAPS_FIXED + MAPS_PER_LEVEL * nl; }
inline int64_t cnt_words(int nm) { return (int64_t)CNT_MAP * nm + CNT_TAIL; }      // the counter block of nm maps

// one event per thread for the read-backs (created once, never destroyed)
thread_local hipEvent_t t_ev = nullptr;
int sync_readback(void* host, const void* dev, int64_t bytes, hipStream_t s) {
  if (!t_ev) FC_HIP(hipEventCreateWithFlags(&t_ev, hipEventDisableTiming));
  FC_HIP(hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, s));
  FC_HIP(hipEventRecord(t_ev, s));
  FC_HIP(hipEventSynchronize(t_ev));
  return 0;
}

// ---- stage 1 -------------------------------------------------------------------------------------------------------------------
// stage 1 arena: raw collate, scratch of the chain, the sets of [cm0, m1, m2, L1..Lnl] with their tables, the meta block
int64_t stage1_layout(int64_t T, int B, int nl, int nfeat, char* base, void** p /*pointers out*/, int S) {
  Bump a{base, 0};
  int i = 0;
  p[i++] = a.arr<int>(4 * T);                                   // 0 coords_raw
  p[i++] = a.arr<float>((int64_t)nfeat * T);                    // 1 feats_raw
  p[i++] = a.arr<int>(T);                                       // 2 slot (even sets)
  p[i++] = a.take(T);                                           // 3 flags
  p[i++] = a.arr<int>(5 * fc_cdiv(T > 0 ? T : 1, 1024) + 8);    // 4 blocksums (one per 256 rows), then one per 1 024 rows
  p[i++] = a.arr<int>((int64_t)METAW * S + (int64_t)S * B + PAD); // 5 meta
  p[i++] = a.arr<float>((int64_t)nfeat * T);                    // 6 F0
  p[i++] = a.arr<int>(T);                                       // 7 slot (odd sets)
  const int64_t cap = next_pow2(T > 0 ? 2 * T : 2);
  p[i++] = a.arr<unsigned long long>(cap * S);                  // 8 keys of all sets (S, cap)
  p[i++] = a.arr<int>(cap * S);                                 // 9 vals of all sets (S, cap)
  for (int s = 0; s < S; ++s) p[i++] = a.arr<int>(4 * T);       // 10 + s: coords of set s
  return fc_align(a.off, 256);
}

// level 0 from the points of the scenes: the collate fused with the hash insert, CH scenes per launch
int collate_insert(const int64_t* cfg, const int64_t* scenes, int4* coords_raw, float* feats_raw, unsigned long long* keys, int* vals, int* meta,
                   int* slot, bool probe, hipStream_t stream) {
  const int B = (int)cfg[C_B], nfeat = (int)cfg[C_NFEAT];
  const int64_t T = cfg[C_TOTAL];
  const float vs = (float)as_double(cfg[C_VS]), fdiv = (float)as_double(cfg[C_FEATDIV]);
  int64_t off = 0;
  for (int b0 = 0; b0 < B; b0 += CH) {
    SceneArgs sc;
    memset(&sc, 0, sizeof(sc));
    int maxn = 0;
    const int nb = B - b0 < CH ? B - b0 : CH;
    for (int j = 0; j < nb; ++j) {
      sc.p[j] = (const float*)scenes[3 * (b0 + j)];
      sc.n[j] = (int)scenes[3 * (b0 + j) + 1];
      if (sc.n[j] < 0 || (sc.n[j] > 0 && !sc.p[j]) || scenes[3 * (b0 + j) + 2] != cfg[C_PT_STRIDE]) return FC_EINVAL;
      sc.off[j] = (int)off;
      off += sc.n[j];
      if (sc.n[j] > maxn) maxn = sc.n[j];
    }
    if (off > T) return FC_EINVAL;
    sc.b0 = b0; sc.stride = (int)cfg[C_PT_STRIDE]; sc.nfeat = nfeat; sc.vs = vs; sc.feat_div = fdiv;
    if (sc.stride < 3 + nfeat) return FC_EINVAL;
    if (maxn > 0) {
      // points read, coords + features + slot written, one 12-byte table slot read and written per point
      Bracket br(probe, PK_VOXELIZE, (double)(off - sc.off[0]) * (4.0 * sc.stride + 16.0 + 4.0 * nfeat + 4.0 + 24.0), stream);
      dim3 grid((unsigned)fc_cdiv(maxn, 256), nb);
      k_plan_voxelize_insert<<<grid, 256, 0, stream>>>(sc, coords_raw, feats_raw, keys, vals, table_mask(T), meta, slot);
      FC_CHECK_LAUNCH();
    }
  }
  return off != T ? FC_EINVAL : FC_OK;
}

// the set records of the chain's sets, from the counts read back; -> the range flag of any set
int stage1_set_records(int64_t* out, const int* counts_host, void* const* coords, unsigned long long* keys_all, int* vals_all, int64_t cap0,
                       int64_t T, int S) {
  int bad = 0;
  for (int s = 0; s < S; ++s) {
    const int* m = counts_host + METAW * s;
    int64_t* o = out + HDR + SETW * s;
    o[S_COORDS] = (int64_t)coords[s];
    o[S_N] = m[META_ROWS];
    o[S_STRIDE] = 1 << s;
    o[S_KEYS] = (int64_t)(keys_all + cap0 * s);
    o[S_VALS] = (int64_t)(vals_all + cap0 * s);
    o[S_CAP] = (int64_t)table_mask(s ? counts_host[METAW * (s - 1) + META_ROWS] : T) + 1;
    o[S_PARENT] = -1;
    bad |= m[META_BAD];
  }
  return bad;
}

// ---- stage 2: which sets and maps exist ------------------------------------------------------------------------------------------
struct MapRec { int in, out, K; int64_t n_in, n_out; bool dense, self; };

struct Net {                        // what fc_plan_maps builds for: decided from cfg and the counts of stage 1, before any allocation
  int B, nl, S0, S, cs;             // S0 sets of the chain, S with the generated sets; cs: the coarsest backbone level
  bool backward, want_head, probe;
  int prune;                        // head level at which pts_threshold bites | -1
  int head_set[MAXLV];              // head level l (finest first) -> set index
  int64_t n_all;                    // head locations over all levels
  int nm;
  MapRec mr[MAPS_FIXED + MAPS_PER_LEVEL * MAXLV];
};

inline int64_t* set_rec(int64_t* out, int s) { return out + HDR + SETW * s; }
inline int64_t* map_rec(int64_t* out, int m) { return out + HDR + SETW * MAXSETS + MAPR * m; }
inline int64_t set_rows(int64_t* out, int s) { return set_rec(out, s)[S_N]; }
inline const int4* set_coords(int64_t* out, int s) { return (const int4*)set_rec(out, s)[S_COORDS]; }
// rows per scene of the coarsest level: rows of a scene in a generated set = these * 8^depth
inline const int* coarsest_scene_rows(const Net& n, const int* counts_host) { return counts_host + METAW * n.S0 + (int64_t)n.cs * n.B; }
// backbone level (0-based: set 3 + i) whose union rows live in generated set g
inline int union_level(const Net& n, int g) { return n.nl - 2 - (g - n.S0); }

// The neck's generated sets — g_i = children of the head level above it, i = nl-2 .. 0 (set index S0 + (nl-2-i)) — with the
// pts_threshold pruning rule, then the MapRec list; fills the header words and the generated sets' records (all but their buffers).
void decide_net(const int64_t* cfg, int64_t* out, const int* counts_host, Net& n) {
  n.B = (int)cfg[C_B]; n.nl = (int)cfg[C_NL];
  n.backward = cfg[C_BACKWARD] != 0;
  n.probe = cfg[C_PROBE] != 0;
  const bool neck = cfg[C_NECK] != 0;
  const int64_t pts_thr = cfg[C_PTS_THR];
  const int nl = n.nl;
  n.S0 = 3 + nl; n.S = n.S0; n.cs = n.S0 - 1;
  n.prune = -1;
  if (neck) {
    int x = n.cs;
    n.head_set[nl - 1] = x;
    for (int i = nl - 2; i >= 0; --i) {
      const int g = n.S++;
      const int depth = nl - 1 - i;
      int64_t* o = set_rec(out, g);
      o[S_N] = 8 * set_rows(out, x);
      o[S_STRIDE] = set_rec(out, x)[S_STRIDE] / 2;
      o[S_PARENT] = x;
      o[S_KEYS] = o[S_VALS] = o[S_CAP] = 0;
      n.head_set[i] = g;
      // pts_threshold (fcaf3d_neck_with_head.py:110-126): rows of a scene in g = its rows in the coarsest level * 8^depth
      if (pts_thr >= 0 && n.prune < 0) {
        const int* sc_cnt = coarsest_scene_rows(n, counts_host);
        for (int b = 0; b < n.B; ++b)
          if (((int64_t)sc_cnt[b] << (3 * depth)) > pts_thr) n.prune = i;
      }
      x = g;
      if (n.prune >= 0) break;                      // the sets below a pruned level depend on the network's scores
    }
  }
  out[H_S] = n.S;
  out[H_PRUNE] = n.prune;
  out[H_NHEAD] = neck ? nl : 0;
  auto SN = [&](int s) { return set_rows(out, s); };
  MapRec* mr = n.mr;
  int nm = 0;
  mr[nm++] = {0, 1, 27, SN(0), SN(1), false, false};           // stem conv k3 s2 (its own kernel: table only)
  mr[nm++] = {1, 2, 8, SN(1), SN(2), false, false};            // max-pool k2 s2
  for (int li = 1; li <= nl; ++li) {
    const int prev = 1 + li, mi = 2 + li;
    mr[nm++] = {prev, mi, 27, SN(prev), SN(mi), false, false}; // down  k3 s2
    mr[nm++] = {prev, mi, 1, SN(prev), SN(mi), false, false};  // ds    k1 s2 (row 13 of `down`)
    mr[nm++] = {mi, mi, 27, SN(mi), SN(mi), false, true};      // same  k3 s1
  }
  for (int g = n.S0; g < n.S; ++g) mr[nm++] = {g, g, 27, SN(g), SN(g), true, true};   // gsame (nl-2 .. ) k3 s1 on a generated set
  n.nm = nm;
  out[H_NMAPS] = nm;
  // the head's location arrays (training: what the target assignment and the loss read)
  n.n_all = 0;
  if (neck && n.prune < 0)
    for (int l = 0; l < nl; ++l) n.n_all += SN(n.head_set[l]);
  out[H_NALL] = n.n_all;
  n.want_head = cfg[C_TARGETS] != 0 && neck && n.prune < 0;
}

// Which derived tables a map gets and which route each pass of a convolution on it takes: THE statement of this rule on the native
// side — the layout (which tables are built) and the descriptors (which tables a route is pointed at) both read it.  In Python the
// same rule is sparse.KernelMap.prefetch (what is built) and sparse.KernelMap.desc (what the executor is told).
enum TableKind { T_NONE, T_PLAIN, T_SORTED, T_PAIRS };
struct MapTables {
  bool sort_rows, use_pairs;        // the map's own properties (MWF_*)
  TableKind fwd;                    // forward: per offset over the pair lists, or over the mask-sorted or the plain table | T_NONE: no convolution
  bool wgrad_pairs;                 // the weight gradient reduces over exact pair lists
  TableKind bwd;                    // backward-data: the same choice on the transposed table | T_NONE: no backward tables
};
MapTables map_tables(const MapRec& r, bool conv, const int64_t* cfg) {
  MapTables t;
  t.sort_rows = r.K == 27 && !r.dense && r.n_out >= cfg[C_SORT_MIN];
  t.use_pairs = r.K == 27 && !r.dense;
  const bool backward = conv && cfg[C_BACKWARD] != 0;
  const TableKind table = t.sort_rows ? T_SORTED : T_PLAIN;
  t.fwd = !conv ? T_NONE : t.use_pairs && r.n_out <= cfg[C_PAIR_ROWS] ? T_PAIRS : table;
  t.wgrad_pairs = backward && t.use_pairs;
  t.bwd = !backward ? T_NONE : t.use_pairs && r.n_in <= cfg[C_PAIR_ROWS] ? T_PAIRS : table;
  return t;
}
inline bool is_conv(int m) { return m >= MAPS_FIXED; }      // stem and pool run their own kernels on the plain table

// ---- stage 2: layout + job collection -----------------------------------------------------------------------------------------------
// Everything stage 2 builds, as one pass over a bump allocator, and the jobs that fill it — one batch per KIND of job.  With
// a.base == nullptr this is the sizing pass: the same walk, every address null, nothing to enqueue.
struct Jobs {
  Batch<GenJob> gen;
  Batch<KMapJob> kmaps;
  Batch<RowJob> fills, rows, prefills;              // fills (-1) run before the scatters; prefills: the tables of the strided maps, before k_plan_strided_maps
  Batch<SMapJob> smaps;
  Batch<SortJob> sorts;
  Batch<PairJob> pairs;
  Batch<GenRowsJob> grows;
  Child children[MAXLV];
  int nchildren = 0;
  int* cnt_dev = nullptr;                           // the pair-list counters of all maps in ONE block (read back together) + union hit counters
  float* pts = nullptr; int* scene = nullptr; int* level = nullptr; int* order = nullptr; int* seg = nullptr;
};

// the table of map m itself (and its transposed table): allocation + the job that fills it
int layout_table(const Net& n, int64_t* out, int m, Bump& a, Jobs& jb) {
  const MapRec& r = n.mr[m];
  int64_t* o = map_rec(out, m);
  const int64_t* din = set_rec(out, r.in);
  int* nbr = nullptr;
  int* nbr_t = nullptr;
  if (r.K == 1) {                                   // k1 s2: the centre row of the k3 s2 table of the same pair of sets
    const int64_t* od = map_rec(out, m - 1);
    if (a.base) {
      nbr = (int*)od[MW_NBR] + 13 * r.n_out;
      nbr_t = n.backward ? (int*)od[MW_NBRT] + 13 * r.n_in : nullptr;
    }
  } else {
    nbr = a.arr<int>((int64_t)r.K * r.n_out);
    if (r.dense) {                                  // generated set: from the parent's own k3 table (index arithmetic)
      const int par = (int)din[S_PARENT];
      const int64_t* op = nullptr;                  // the parent's k3 s1 map: `same` of the coarsest level, or the gsame above
      for (int mm = 0; mm < m; ++mm)
        if (n.mr[mm].self && n.mr[mm].in == par) op = map_rec(out, mm);
      if (!op) return FC_EINVAL;
      jb.children[jb.nchildren++] = {(const int*)op[MW_NBR], set_rows(out, par), nbr};
    } else {
      const int ks = r.K == 27 ? 3 : 2;
      const int nbx = (int)fc_cdiv(r.n_out, 256);
      const int64_t* dout = set_rec(out, r.out);
      if (r.in != r.out && dout[S_STRIDE] == 2 * din[S_STRIDE]) {      // stride s -> 2 s: from the input side (k_plan_strided_maps)
        jb.smaps.add({set_coords(out, r.in), (const unsigned long long*)dout[S_KEYS], (const int*)dout[S_VALS], (unsigned long long)(dout[S_CAP] - 1),
                      nbr, r.n_in, r.n_out, ks, (int)din[S_STRIDE], (int)fc_cdiv(8 * r.n_in, 256)}, fc_cdiv(8 * r.n_in, 256));
        jb.prefills.add({nullptr, nbr, r.n_out, r.n_out, r.K, 3, nbx}, fc_cdiv((int64_t)r.K * r.n_out, 1024));
      } else {
        jb.kmaps.add({set_coords(out, r.out), (const unsigned long long*)din[S_KEYS], (const int*)din[S_VALS], (unsigned long long)(din[S_CAP] - 1),
                      nbr, r.n_out, r.K, ks, (int)din[S_STRIDE], nbx}, (int64_t)r.K * nbx);
      }
    }
    if (is_conv(m) && n.backward) {
      nbr_t = a.arr<int>((int64_t)r.K * r.n_in);
      const int nbx = (int)fc_cdiv(r.n_in, 256);
      if (r.self) {
        jb.rows.add({nbr, nbr_t, r.n_in, r.n_in, r.K, 0, nbx}, (int64_t)r.K * ((nbx + 3) / 4));
      } else {
        jb.fills.add({nullptr, nbr_t, r.n_in, r.n_in, r.K, 3, nbx}, fc_cdiv((int64_t)r.K * r.n_in, 1024));
        const int nbo = (int)fc_cdiv(r.n_out, 256);
        jb.rows.add({nbr, nbr_t, r.n_out, r.n_in, r.K, 2, nbo}, (int64_t)r.K * ((nbo + 3) / 4));
      }
    }
  }
  o[MW_NBR] = (int64_t)nbr;
  o[MW_NBRT] = (int64_t)nbr_t;
  return FC_OK;
}

// pair lists of a (27, n) table into the PAIR_* group at `group` of a map record
void layout_pair_lists(int64_t* group, const int* tab, int64_t n, int* cnt, Bump& a, Jobs& jb) {
  PairJob j;
  j.tab = tab; j.n = n; j.cnt = cnt;
  j.pi = a.arr<int>(27 * n); j.po = a.arr<int>(27 * n); j.pos = a.arr<int>(27 * n);
  j.nblk = (int)fc_cdiv(n > 0 ? n : 1, PBLK);
  j.blk_cnt = a.arr<int>(27 * (int64_t)j.nblk);
  group[PAIR_IN] = (int64_t)j.pi; group[PAIR_OUT] = (int64_t)j.po; group[PAIR_POS] = (int64_t)j.pos; group[PAIR_CNT] = (int64_t)cnt;
  jb.pairs.add(j, n > 0 ? 27 * (int64_t)j.nblk : 0);
}

// a (27, n) table in mask order -> *w_tab, its row order -> *w_idx; a plain table stands for itself, with no order
void layout_route_table(TableKind kind, int64_t* w_tab, int64_t* w_idx, const int* tab, int64_t n, Bump& a, Jobs& jb) {
  if (kind == T_PLAIN) { *w_tab = (int64_t)tab; *w_idx = 0; }
  if (kind != T_SORTED) return;
  SortJob j;
  memset(&j, 0, sizeof(j));
  j.tab = tab; j.n = n;
  j.order = a.arr<int>(n);
  j.sorted = a.arr<int>(27 * n);
  j.masks = a.arr<int>(n);
  sort_job_ws(j, a.take(argsort27_ws_bytes(n)));
  *w_tab = (int64_t)j.sorted; *w_idx = (int64_t)j.order;
  jb.sorts.add(j, j.nbx);
}

// -> bytes of the arena (a.off), FC_* < 0 on error
int64_t layout(const int64_t* cfg, const Net& n, int64_t* out, Bump& a, Jobs& jb) {
  const int nl = n.nl;
  for (int g = n.S0; g < n.S; ++g) {                // generated sets, straight from the coarsest level
    int64_t* o = set_rec(out, g);
    o[S_COORDS] = (int64_t)a.arr<int>(4 * o[S_N]);
    o[S_ROWS] = (int64_t)a.arr<int>(set_rows(out, 3 + union_level(n, g)));
    jb.gen.add({set_coords(out, n.cs), (int4*)o[S_COORDS], o[S_N], g - n.S0 + 1, (int)o[S_STRIDE], 0}, fc_cdiv(o[S_N], 256));
  }
  jb.cnt_dev = a.arr<int>(cnt_words(n.nm));
  // -- pass A: the tables themselves, and what the records and descriptors say without a read-back --
  for (int m = 0; m < n.nm; ++m) {
    const MapRec& r = n.mr[m];
    int64_t* o = map_rec(out, m);
    o[MW_IN] = r.in; o[MW_OUT] = r.out; o[MW_K] = r.K; o[MW_NIN] = r.n_in; o[MW_NOUT] = r.n_out;
    if (int rc = layout_table(n, out, m, a, jb)) return rc;
    for (int64_t* d : {o + MW_DESC_F, o + MW_DESC_B}) { d[MAP_N_IN] = r.n_in; d[MAP_N_OUT] = r.n_out; d[MAP_K] = r.K; d[MAP_NBR] = o[MW_NBR]; }
    const MapTables t = map_tables(r, is_conv(m), cfg);
    o[MW_FLAGS] = (t.sort_rows ? MWF_SORT_ROWS : 0) | (t.use_pairs ? MWF_USE_PAIRS : 0) | (r.dense ? MWF_DENSE : 0);
  }
  // -- pass B: the derived tables of every convolution route --
  for (int m = MAPS_FIXED; m < n.nm; ++m) {
    const MapRec& r = n.mr[m];
    const MapTables t = map_tables(r, true, cfg);
    int64_t* o = map_rec(out, m);
    const int* nbr = (const int*)o[MW_NBR];
    const int* nbr_t = (const int*)o[MW_NBRT];
    int* cnt = at(jb.cnt_dev, CNT_MAP * m);
    if (t.fwd == T_PAIRS) layout_pair_lists(o + MW_PI, nbr, r.n_out, cnt, a, jb);
    layout_route_table(t.fwd, o + MW_SORT, o + MW_SORTI, nbr, r.n_out, a, jb);
    if (t.wgrad_pairs && t.fwd != T_PAIRS) layout_pair_lists(o + MW_PI, nbr, r.n_out, cnt, a, jb);
    if (t.bwd == T_PAIRS) layout_pair_lists(o + MW_TPI, nbr_t, r.n_in, at(cnt, CNT_T), a, jb);
    layout_route_table(t.bwd, o + MW_SORTT, o + MW_SORTTI, nbr_t, r.n_in, a, jb);
  }
  // -- union rows of the backbone levels inside the generated sets (fcaf3d_neck_with_head.py:101) --
  for (int g = n.S0; g < n.S; ++g) {
    const int s = 3 + union_level(n, g);
    jb.grows.add({set_coords(out, s), (int*)set_rec(out, g)[S_ROWS], at(jb.cnt_dev, CNT_MAP * n.nm + (g - n.S0)), set_rows(out, s),
                  (int)set_rec(out, s)[S_STRIDE], g - n.S0 + 1}, fc_cdiv(set_rows(out, s), 256));
  }
  if (n.want_head) {
    jb.pts = a.arr<float>(3 * n.n_all); jb.scene = a.arr<int>(n.n_all); jb.level = a.arr<int>(n.n_all); jb.order = a.arr<int>(n.n_all);
    jb.seg = a.arr<int>((int64_t)nl * n.B + 1);
    out[H_TGT_PTS] = (int64_t)jb.pts; out[H_TGT_SCENE] = (int64_t)jb.scene; out[H_TGT_LEVEL] = (int64_t)jb.level;
    out[H_TGT_ORDER] = (int64_t)jb.order; out[H_TGT_SEG] = (int64_t)jb.seg;
  }
  return fc_align(a.off, 256);
}

// ---- stage 2: the launches, in dependency order --------------------------------------------------------------------------------------
// the head's per-location arrays and the (level, scene) segment starts
int enqueue_head(const int64_t* cfg, const Net& n, int64_t* out, const Jobs& jb, const int* counts_host, int* cnt_host, hipStream_t stream) {
  const int nl = n.nl, B = n.B;
  HeadArgs h;
  memset(&h, 0, sizeof(h));
  h.nl = nl; h.vs = (float)as_double(cfg[C_VS_HEAD]);
  int64_t off = 0;
  for (int l = 0; l < nl; ++l) { h.coords[l] = set_coords(out, n.head_set[l]); h.off[l] = off; off += set_rows(out, n.head_set[l]); }
  h.off[nl] = off;
  if (n.n_all > 0) {
    Bracket br(n.probe, PK_HEAD, probe_bytes_head(n.n_all), stream);
    k_plan_head_arrays<<<(unsigned)fc_cdiv(n.n_all, 256), 256, 0, stream>>>(h, jb.pts, jb.scene, jb.level, jb.order);
    FC_CHECK_LAUNCH();
  }
  // (level, scene) segment starts: rows per scene of a generated set = 8^depth x those of the coarsest level — host arithmetic,
  // staged in the caller's pinned counter block behind the counters (it stays untouched until the read-back)
  int* stage = cnt_host + cnt_words(n.nm);
  const int* sc_cnt = coarsest_scene_rows(n, counts_host);
  int64_t run = 0;
  for (int l = 0; l < nl; ++l)
    for (int b = 0; b < B; ++b) {
      stage[l * B + b] = (int)run;
      run += (int64_t)sc_cnt[b] << (3 * (nl - 1 - l));
    }
  stage[nl * B] = (int)run;
  FC_HIP(hipMemcpyAsync(jb.seg, stage, sizeof(int) * ((size_t)nl * B + 1), hipMemcpyHostToDevice, stream));
  return FC_OK;
}

int enqueue(const int64_t* cfg, const Net& n, int64_t* out, const Jobs& jb, const int* counts_host, int* cnt_host, hipStream_t stream) {
  const bool probe = n.probe;
  FC_HIP(hipMemsetAsync(jb.cnt_dev, 0, sizeof(int) * cnt_words(n.nm), stream));
  int rc;
  { Bracket br(probe, PK_GEN, probe_bytes(jb.gen), stream); if ((rc = launch_batch(jb.gen, 256, stream, k_plan_gen_coords))) return rc; }
  {
    Bracket br(probe, PK_KMAPS, probe_bytes(jb.smaps, probe_bytes(jb.kmaps)), stream);
    if ((rc = launch_batch(jb.prefills, 256, stream, k_plan_rows))) return rc;
    if ((rc = launch_batch(jb.smaps, 256, stream, k_plan_strided_maps))) return rc;
    if ((rc = launch_batch(jb.kmaps, 256, stream, k_plan_kernel_maps))) return rc;
  }
  {
    Bracket br(probe, PK_CHILDREN, probe_bytes(jb.children, jb.nchildren), stream);
    for (int c = 0; c < jb.nchildren; ++c)          // a chain: each generated set's table from the one above it
      if ((rc = fc_kernel_map_children(jb.children[c].pnbr, jb.children[c].n_parent, jb.children[c].nbr, stream))) return rc;
  }
  { Bracket br(probe, PK_FILL, probe_bytes(jb.fills), stream); if ((rc = launch_batch(jb.fills, 256, stream, k_plan_rows))) return rc; }
  { Bracket br(probe, PK_TRANSPOSE, probe_bytes(jb.rows), stream); if ((rc = launch_batch(jb.rows, 256, stream, k_plan_rows))) return rc; }
  { Bracket br(probe, PK_MASKS, probe_bytes_masks(jb.sorts), stream); if ((rc = launch_batch(jb.sorts, 256, stream, k_plan_row_masks))) return rc; }
  { Bracket br(probe, PK_RADIX, probe_bytes_radix(jb.sorts), stream); if ((rc = argsort27_batch(jb.sorts, stream))) return rc; }
  {
    Batch<SortJob> perm;
    for (int i = 0; i < jb.sorts.count; ++i) perm.add(jb.sorts.j[i], 27 * (int64_t)jb.sorts.j[i].nbx);
    Bracket br(probe, PK_PERMUTE, probe_bytes_permute(jb.sorts), stream);
    if ((rc = launch_batch(perm, 256, stream, k_plan_permute))) return rc;
  }
  {
    Bracket br(probe, PK_PAIRS, probe_bytes(jb.pairs), stream);
    if ((rc = launch_batch(jb.pairs, PBLK, stream, k_plan_pairs_count))) return rc;
    if ((rc = launch_batch(jb.pairs, PBLK, stream, k_plan_pairs_fill))) return rc;
  }
  if (jb.grows.count && jb.grows.blocks()) {
    const int64_t* oc = set_rec(out, n.cs);
    Bracket br(probe, PK_GENROWS, probe_bytes(jb.grows), stream);
    k_plan_gen_rows<<<(unsigned)jb.grows.blocks(), 256, 0, stream>>>(jb.grows, (const unsigned long long*)oc[S_KEYS], (const int*)oc[S_VALS],
                                                                    (unsigned long long)(oc[S_CAP] - 1));
    FC_CHECK_LAUNCH();
  }
  if (n.want_head && (rc = enqueue_head(cfg, n, out, jb, counts_host, cnt_host, stream))) return rc;
  return FC_OK;
}

// ---- stage 2: after the read-back ------------------------------------------------------------------------------------------------
void put_pairs(int64_t* d, int group, const int64_t* lists, bool with_tiles) {
  for (int w = PAIR_IN; w <= PAIR_CNT; ++w) d[group + w] = lists[w];
  if (with_tiles) d[group + PAIR_TILES] = lists[PAIR_TILES];
}
// desc(conv, backward) of a map (sparse.KernelMap.desc) from its record o: the words that wait for the tables and the live-tile counts
void fill_descriptor(int64_t* d, const int64_t* o, const MapTables& t, bool backward) {
  int64_t flags = 0;
  if (t.fwd == T_PAIRS) {
    put_pairs(d, MAP_PAIRS, o + MW_PI, true);
    flags |= MAP_ROUTE_FWD_PAIRS;
  } else {
    d[MAP_FWD_TAB] = o[MW_SORT]; d[MAP_FWD_IDX] = o[MW_SORTI];
  }
  if (backward) {
    d[MAP_NBR_T] = o[MW_NBRT];
    if (t.wgrad_pairs) {
      put_pairs(d, MAP_PAIRS, o + MW_PI, false);
      flags |= MAP_ROUTE_WGRAD_PAIRS;
    }
    if (t.bwd == T_PAIRS) {
      put_pairs(d, MAP_PAIRS_T, o + MW_TPI, true);
      flags |= MAP_ROUTE_BWD_PAIRS;
    } else {
      d[MAP_BWD_TAB] = o[MW_SORTT]; d[MAP_BWD_IDX] = o[MW_SORTTI];
    }
  }
  d[MAP_FLAGS] = flags;
}
// the live-tile counts and both descriptors of every convolution map, and whether the unions are the generated sets
void finish_records(const int64_t* cfg, const Net& n, int64_t* out, const int* cnt_host) {
  int structured = 1;
  for (int g = n.S0; g < n.S; ++g)                  // a backbone voxel outside the generated set: per-operator path
    if (cnt_host[CNT_MAP * n.nm + (g - n.S0)] != set_rows(out, 3 + union_level(n, g))) structured = 0;
  out[H_STRUCT] = structured;
  for (int m = MAPS_FIXED; m < n.nm; ++m) {
    int64_t* o = map_rec(out, m);
    const MapTables t = map_tables(n.mr[m], true, cfg);
    if (t.fwd == T_PAIRS) o[MW_TILES] = live_tiles(cnt_host + CNT_MAP * m, 27);
    if (t.bwd == T_PAIRS) o[MW_TTILES] = live_tiles(cnt_host + CNT_MAP * m + CNT_T, 27);
    fill_descriptor(o + MW_DESC_F, o, t, false);
    fill_descriptor(o + MW_DESC_B, o, t, n.backward);      // (without backward tables: the forward half only)
  }
}

}  // namespace

extern "C" {

int fc_abi_version(void) { return FC_ABI_VERSION; }
int fc_plan_cfg_words(void) { return CFGW; }
int fc_plan_out_words(int B, int nl) { return HDR + SETW * MAXSETS + MAPR * max_maps(nl) + MAXSETS * (B > 0 ? B : 1) + PAD; }

int64_t fc_plan_stage1_bytes(int64_t total_points, int B, int nl, int nfeat) {
  if (total_points < 0 || B < 1 || nl < 1 || nl > MAXLV || nfeat < 0) return -1;
  void* p[10 + MAXSETS];
  return stage1_layout(total_points, B, nl, nfeat, nullptr, p, 3 + nl);
}

int fc_plan_levels(const int64_t* cfg, const int64_t* scenes, void* arena1, int64_t arena1_bytes, int64_t* out, int* counts_host,
                   hipStream_t stream) {
  const int B = (int)cfg[C_B], nl = (int)cfg[C_NL], nfeat = (int)cfg[C_NFEAT];
  const int64_t T = cfg[C_TOTAL];
  if (B < 1 || B > 32767 || nl < 1 || nl > MAXLV || nfeat < 0 || T < 0 || T > 0x7fffffffLL / 8 || !arena1 || !out || !counts_host) return FC_EINVAL;
  const int S = 3 + nl;
  void* p[10 + MAXSETS];
  if (arena1_bytes < stage1_layout(T, B, nl, nfeat, (char*)arena1, p, S)) return FC_EWS;
  int4* coords_raw = (int4*)p[0];
  float* feats_raw = (float*)p[1];
  int* slots[2] = {(int*)p[2], (int*)p[7]};
  unsigned char* flags = (unsigned char*)p[3];
  int* blocksums = (int*)p[4];
  int* coarse = blocksums + 4 * fc_cdiv(T > 0 ? T : 1, 1024) + 4;
  int* meta = (int*)p[5];
  float* F0 = (float*)p[6];
  const int64_t cap0 = next_pow2(T > 0 ? 2 * T : 2);
  unsigned long long* keys_all = (unsigned long long*)p[8];
  int* vals_all = (int*)p[9];
  const int64_t nmeta = (int64_t)METAW * S + (int64_t)S * B;
  FC_HIP(hipMemsetAsync(meta, 0, (size_t)nmeta * sizeof(int), stream));
  const bool probe = cfg[C_PROBE] != 0;
  size_t stage1_pp[MAXSETS] = {};
  if (!cfg[C_COORDS_IN] && !((float)as_double(cfg[C_VS]) > 0.f)) return FC_EINVAL;
  if (T > 0) {
    {
      Bracket br(probe, PK_TABLES, 12.0 * (double)(cap0 * S), stream);
      k_plan_tables_init<<<(unsigned)fc_cdiv(cap0 * S, 512), 256, 0, stream>>>(keys_all, vals_all, cap0 * S);
      FC_CHECK_LAUNCH();
    }
    // ---- level 0: the collate + insert ----
    const int4* src0 = coords_raw;
    if (!cfg[C_COORDS_IN]) {
      if (int rc = collate_insert(cfg, scenes, coords_raw, feats_raw, keys_all, vals_all, meta, slots[0], probe, stream)) return rc;
    } else {                                       // pre-voxelised input (an augmenting pipeline wrote coords / feats itself)
      src0 = (const int4*)cfg[C_COORDS_IN];
      feats_raw = (float*)cfg[C_FEATS_IN];
      if (!feats_raw && nfeat) return FC_EINVAL;
      Bracket br(probe, PK_VOXELIZE, (double)T * (16.0 + 4.0 + 24.0), stream);
      k_plan_insert<<<(unsigned)fc_cdiv(T, 256), 256, 0, stream>>>(src0, T, keys_all, vals_all, table_mask(T), meta, slots[0]);
      FC_CHECK_LAUNCH();
    }
    // ---- the chain: two launches per set ----
    const unsigned gB = (unsigned)fc_cdiv(T, 1024);  // both kernels: one block per 1 024 input rows
    for (int s = 0; s < S; ++s) {
      int* meta_s = meta + METAW * s;
      const int* n_in_dev = s ? meta + METAW * (s - 1) + META_ROWS : nullptr;
      const int4* src = s ? (const int4*)p[10 + s - 1] : src0;
      int* vals = vals_all + cap0 * s;
      const size_t pp0 = g_pp.size();
      {
        Bracket br(probe, PK_FLAGS, 0.0, stream);        // bytes are filled in after the read-back (they depend on the live counts)
        k_plan_flags<<<gB, 256, 0, stream>>>(slots[s & 1], vals, n_in_dev, T, flags, blocksums, coarse);
        FC_CHECK_LAUNCH();
      }
      if (probe) stage1_pp[s] = pp0;
      const bool more = s + 1 < S;
      Bracket br(probe, PK_FINALIZE, 0.0, stream);
      k_plan_finalize<<<gB, 1024, 0, stream>>>(src, n_in_dev, T, 1 << s, flags, blocksums, coarse, slots[s & 1], vals, (int4*)p[10 + s],
                                             s == 0 ? feats_raw : nullptr, s == 0 ? F0 : nullptr, nfeat,
                                             meta + METAW * S + (int64_t)s * B, B, meta_s, more ? keys_all + cap0 * (s + 1) : nullptr,
                                             more ? vals_all + cap0 * (s + 1) : nullptr, slots[(s + 1) & 1]);
      FC_CHECK_LAUNCH();
    }
  }
  int rc = sync_readback(counts_host, meta, nmeta * (int64_t)sizeof(int), stream);
  if (rc) return rc;
  if (probe && T > 0)
    for (int s = 0; s < S; ++s) {                   // compulsory bytes of the chain's launches, now that the counts are known
      const double n_in = s ? counts_host[METAW * (s - 1) + META_ROWS] : (double)T, n_out = counts_host[METAW * s + META_ROWS];
      g_pp[stage1_pp[s]].bytes = n_in * (4.0 + 4.0 + 1.0);                                     // slot, table value, flag
      g_pp[stage1_pp[s] + 1].bytes = n_in * (1.0 + 4.0) + n_out * (16.0 + 16.0 + 4.0 + (s == 0 ? 8.0 * nfeat : 0.0)) +
                                     (s + 1 < S ? n_out * (24.0 + 4.0) : 0.0);                 // ... + the next set's insert
    }
  // ---- host tables ----
  memset(out, 0, (size_t)fc_plan_out_words(B, nl) * sizeof(int64_t));
  out[H_S] = S;
  out[H_F0] = (int64_t)F0;
  out[H_PRUNE] = -1;
  out[H_BAD] = stage1_set_records(out, counts_host, p + 10, keys_all, vals_all, cap0, T, S);
  return FC_OK;
}

// the sizing pass: the layout without an arena, nothing enqueued
int64_t fc_plan_stage2_bytes(const int64_t* cfg, int64_t* out, const int* counts_host) {
  Net net;
  decide_net(cfg, out, counts_host, net);
  Bump a{nullptr, 0};
  Jobs jb;
  const int64_t need = layout(cfg, net, out, a, jb);
  return need < 0 ? -1 : need + 256;
}

int fc_plan_maps(const int64_t* cfg, int64_t* out, const int* counts_host, void* arena2, int64_t arena2_bytes, int* cnt_host,
                 hipStream_t stream) {
  if (!cfg || !out || !counts_host || !arena2 || !cnt_host) return FC_EINVAL;
  Net net;
  decide_net(cfg, out, counts_host, net);
  char* base = (char*)fc_align((int64_t)arena2, 256);
  Bump a{base, 0};
  Jobs jb;
  const int64_t need = layout(cfg, net, out, a, jb);
  if (need < 0) return (int)need;
  if (arena2_bytes - (base - (char*)arena2) < need) return FC_EWS;      // (nothing has touched the arena yet)
  int rc = enqueue(cfg, net, out, jb, counts_host, cnt_host, stream);
  if (rc) return rc;
  // ---- ONE read-back: pair-list counts of every map, union hit counters ----
  rc = sync_readback(cnt_host, jb.cnt_dev, sizeof(int) * cnt_words(net.nm), stream);
  if (rc) return rc;
  finish_records(cfg, net, out, cnt_host);
  return FC_OK;
}

// brackets of the plans run with cfg[C_PROBE] since the last read-out: ms (float), bytes (double), kind (int) per bracket; -> count
int64_t fc_plan_probe_read(float* ms, double* bytes, int* kind, int64_t cap) {
  int64_t n = 0;
  for (PlanProbe& p : g_pp) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, p.a, p.b) != hipSuccess) t = 0.f;
    if (n < cap) { ms[n] = t; bytes[n] = p.bytes; kind[n] = p.kind; ++n; }
    g_pp_pool.push_back(p.a);
    g_pp_pool.push_back(p.b);
  }
  g_pp.clear();
  return n;
}

// stable argsort of non-negative int32 keys below 2^27 (the occupancy masks of fc_nbr_row_masks) — what torch.argsort did for
// the mask-sorted tables of the per-operator path
int64_t fc_argsort27_ws_bytes(int64_t n) { return argsort27_ws_bytes(n); }
int fc_argsort27(const int* keys, int64_t n, int* order, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (n < 0) return FC_EINVAL;
  if (ws_bytes < argsort27_ws_bytes(n)) return FC_EWS;
  if (n == 0) return FC_OK;
  Batch<SortJob> bt;
  SortJob j;
  memset(&j, 0, sizeof(j));
  j.n = n; j.masks = const_cast<int*>(keys); j.order = order;
  sort_job_ws(j, ws);
  bt.add(j, j.nbx);
  return argsort27_batch(bt, stream);
}

}  // extern "C"
