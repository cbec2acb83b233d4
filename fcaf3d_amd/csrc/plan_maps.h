// Stage 2 of the native coordinate phase (fc_plan_maps): the kernels behind every kernel map and derived table, each over a Batch of
// jobs of its kind.  Beside every job struct: the compulsory bytes of a launch over a batch of it (the probe's roofline figure).
#ifndef FCAF3D_PLAN_MAPS_H
#define FCAF3D_PLAN_MAPS_H
#include "plan_batch.h"
#include "plan_radix.h"      // SortJob, sort_rows

namespace {

// ---- stage 2 kernels (batched) ---------------------------------------------------------------------------------------------------
// kernel maps with the offsets computed in the kernel (x fastest; centred for odd kernels, {0..k-1} for even — Appendix A.3):
// nbr[k][o] = row of out_coords[o] + offset_k * stride in the table, or -1.  job blocks = K * ceil(n_out / 256), k-major.
struct KMapJob { const int4* oc; const unsigned long long* keys; const int* vals; unsigned long long mask; int* nbr; int64_t n_out; int K, ks, stride, nbx; };
__global__ void k_plan_kernel_maps(Batch<KMapJob> bt) {
  int64_t lb;
  const KMapJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int k = (int)(lb / j.nbx);
  const int64_t o = (lb % j.nbx) * 256 + threadIdx.x;
  if (o >= j.n_out) return;
  const int ks = j.ks, c0 = (ks & 1) ? ks / 2 : 0;
  const int dx = (k % ks - c0) * j.stride, dy = ((k / ks) % ks - c0) * j.stride, dz = (k / (ks * ks) - c0) * j.stride;
  const int4 c = j.oc[o];
  j.nbr[(int64_t)k * j.n_out + o] = fc_lookup(j.keys, j.vals, j.mask, fc_pack(c.x, c.y + dx, c.z + dy, c.w + dz));
}
// compulsory bytes: coords, table entry written, slot probed
inline double probe_bytes(const Batch<KMapJob>& b, double by = 0) {
  for (int i = 0; i < b.count; ++i) by += (double)b.j[i].n_out * (16.0 + b.j[i].K * (4.0 + 12.0));
  return by;
}

// kernel maps from a set of stride s onto the set of stride 2 s (the stem's and the levels' k3 s2 convolutions, the k2 s2 max-pool),
// built from the INPUT side (r6, last take): row i of the input lies at offset k of output row o exactly when out = in - offset_k is a
// voxel of the output set — per axis ONE candidate output if the coordinate is a multiple of 2 s (offset 0), two if not (offsets
// +s / -s), one for the k2 kernel — so 1 ... 8 probes of the OUTPUT set's table per input row (3.4 on average) instead of 27 probes
// of the input table per output row, 14 % of which hit: the stem's map 18.9 M probes -> 2.7 M.  The table (pre-filled with -1 by the
// launch in front) gets nbr[k][o] = i; every entry has one writer (input rows are unique voxels).  Same tables bit for bit.
struct SMapJob { const int4* ic; const unsigned long long* okeys; const int* ovals; unsigned long long omask; int* nbr; int64_t n_in, n_out; int ks, stride, nbx; };
__global__ void k_plan_strided_maps(Batch<SMapJob> bt) {
  int64_t lb;
  const SMapJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  // eight threads per input row, one per candidate (a, b, c): the probes of a row are in flight together
  const int64_t t = lb * 256 + threadIdx.x;
  const int64_t i = t >> 3;
  if (i >= j.n_in) return;
  const int a = (int)t & 1, b = ((int)t >> 1) & 1, c = ((int)t >> 2) & 1;
  const int4 p = j.ic[i];
  const int s = j.stride, s2 = 2 * j.stride, ks = j.ks;
  const int pc[3] = {p.y, p.z, p.w};
  int nc[3], cc[3][2], ki[3][2];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int q = fc_floor_div(pc[d], s2) * s2, r = pc[d] - q;      // r = 0 or s
    cc[d][0] = q; cc[d][1] = q + s2;
    if (ks == 2) { nc[d] = 1; ki[d][0] = r / s; ki[d][1] = 0; }     // offsets {0, s}: out = q
    else if (r == 0) { nc[d] = 1; ki[d][0] = 1; ki[d][1] = 0; }     // offset 0
    else { nc[d] = 2; ki[d][0] = 2; ki[d][1] = 0; }                 // out = q: offset +s (index 2); out = q + 2 s: offset -s (index 0)
  }
  if (a >= nc[0] || b >= nc[1] || c >= nc[2]) return;
  const int o = fc_lookup(j.okeys, j.ovals, j.omask, fc_pack(p.x, cc[0][a], cc[1][b], cc[2][c]));
  if (o >= 0) j.nbr[(int64_t)(ki[0][a] + ks * ki[1][b] + ks * ks * ki[2][c]) * j.n_out + o] = (int)i;
}
// compulsory bytes: input coords, <= 8 probes of 12 B per input row (3.4 on average), the table filled and hit
inline double probe_bytes(const Batch<SMapJob>& b, double by = 0) {
  for (int i = 0; i < b.count; ++i)
    by += (double)b.j[i].n_in * (16.0 + 3.4 * 12.0 + 3.4 * 4.0) + (double)b.j[i].n_out * b.j[i].ks * b.j[i].ks * b.j[i].ks * 4.0;
  return by;
}

// row copies / fills of (K, n) tables.  mode 0: dst[k] = src[K - 1 - k] — the transposed table of a map of a set onto ITSELF with
// a centred odd kernel (offset k reversed is offset K - 1 - k: identical to fc_kernel_map_transpose); mode 1: dst = -1;
// mode 2: scatter dst[k][src[k][o]] = o (src (K, n), dst (K, n2)) — fc_kernel_map_transpose's second half; mode 3: dst = -1 as one flat
// run of K n entries, 16 bytes per thread
struct RowJob { const int* src; int* dst; int64_t n, n2; int K, mode, nbx; };
__global__ void k_plan_rows(Batch<RowJob> bt) {
  int64_t lb;
  const RowJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  if (j.mode == 3) {                                 // dst[0 .. K n) = -1, four entries per thread (dst is 16-byte aligned: bump allocator)
    const int64_t tot = (int64_t)j.K * j.n, e = (lb * 256 + threadIdx.x) * 4;
    if (e + 3 < tot) *reinterpret_cast<int4*>(j.dst + e) = make_int4(-1, -1, -1, -1);
    else for (int64_t q = e; q < tot; ++q) j.dst[q] = -1;
    return;
  }
  // four entries per thread, 256 apart (coalesced), their loads in flight together: at 4 bytes per thread a full chip holds ~2 MB in
  // flight — 1 TB/s at 2 us of latency (r6: the fills went 28 -> 10 us as 16-byte stores; the same for the copies and the scatters).
  // job blocks = K * ceil(nbx / 4)
  const int per = (j.nbx + 3) >> 2;
  const int k = (int)(lb / per);
  const int64_t i0 = (lb % per) * 1024 + threadIdx.x;
  int v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = i0 + 256 * u;
    v[u] = -1;
    if (i < j.n && j.mode != 1) v[u] = j.src[(int64_t)(j.mode == 0 ? j.K - 1 - k : k) * j.n + i];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = i0 + 256 * u;
    if (i >= j.n) continue;
    if (j.mode == 2) { if (v[u] >= 0) j.dst[(int64_t)k * j.n2 + v[u]] = (int)i; }
    else j.dst[(int64_t)k * j.n + i] = v[u];
  }
}
// compulsory bytes: a fill writes, a copy / scatter reads and writes
inline double probe_bytes(const Batch<RowJob>& b, double by = 0) {
  for (int i = 0; i < b.count; ++i) by += (double)b.j[i].K * b.j[i].n * ((b.j[i].mode == 1 || b.j[i].mode == 3) ? 4.0 : 8.0);
  return by;
}

// generated sets straight from the coarsest level (MinkowskiGenerativeConvolutionTranspose k2 s2 applied `depth` times, row 8i + k
// each time — Appendix A.4): row t = ((i * 8 + k_depth-1) * 8 + ...) + k_0 sits at coarse[i] + sum_d bits(k_d) * (stride << d)
struct GenJob { const int4* coarse; int4* out; int64_t n; int depth, stride, nbx; };
__global__ void k_plan_gen_coords(Batch<GenJob> bt) {
  int64_t lb;
  const GenJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int64_t t = lb * 256 + threadIdx.x;
  if (t >= j.n) return;
  int4 c = j.coarse[t >> (3 * j.depth)];
  for (int d = 0; d < j.depth; ++d) {
    const int k = (int)(t >> (3 * d)) & 7;
    const int h = j.stride << d;
    c.y += (k & 1) ? h : 0; c.z += (k & 2) ? h : 0; c.w += (k & 4) ? h : 0;
  }
  j.out[t] = c;
}
inline double probe_bytes(const Batch<GenJob>& b, double by = 0) {
  for (int i = 0; i < b.count; ++i) by += 16.0 * b.j[i].n;
  return by;
}

// row of each voxel of a backbone level (stride T) in the generated set `depth` levels below the coarsest level: the generated
// sets hold ALL descendants of the coarsest set (child k of row i at 8i + k), so the row follows from ONE probe of the coarsest
// table and `depth` child-bit triples — identical to fc_child_rows on the parent set's table.  *n_found counts the hits.
struct GenRowsJob { const int4* q; int* rows; int* n_found; int64_t n; int T, depth; };
__global__ void k_plan_gen_rows(Batch<GenRowsJob> bt, const unsigned long long* __restrict__ keys, const int* __restrict__ vals,
                                unsigned long long mask) {
  int64_t lb;
  const GenRowsJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int64_t i = lb * 256 + threadIdx.x;
  int hit = 0;
  if (i < j.n) {
    const int4 c = j.q[i];
    const int T = j.T, P = T << j.depth;           // stride of the coarsest set
    const int px = fc_floor_div(c.y, P) * P, py = fc_floor_div(c.z, P) * P, pz = fc_floor_div(c.w, P) * P;
    int r = fc_lookup(keys, vals, mask, fc_pack(c.x, px, py, pz));
    if (r >= 0) {
      const int rx = (c.y - px) / T, ry = (c.z - py) / T, rz = (c.w - pz) / T;       // in [0, 2^depth)
      for (int d = j.depth - 1; d >= 0; --d) r = 8 * r + (((rx >> d) & 1) | (((ry >> d) & 1) << 1) | (((rz >> d) & 1) << 2));
      hit = 1;
    }
    j.rows[i] = r;
  }
  const int hits = __syncthreads_count(hit);        // one atomic per block: all blocks of a job add to the same word
  if (threadIdx.x == 0 && hits) atomicAdd(j.n_found, hits);
}
// compulsory bytes: coords, row written, slot probed
inline double probe_bytes(const Batch<GenRowsJob>& b, double by = 0) {
  for (int i = 0; i < b.count; ++i) by += (double)b.j[i].n * (16.0 + 4.0 + 12.0);
  return by;
}

// the head's per-location arrays over all levels (finest first): location = voxel corner * voxel size
// (fcaf3d_neck_with_head.py:276-277), scene, level, identity order (rows of every set are grouped by scene)
struct HeadArgs { const int4* coords[MAXLV]; int64_t off[MAXLV + 1]; int nl; float vs; };
__global__ void k_plan_head_arrays(HeadArgs h, float* __restrict__ pts, int* __restrict__ scene, int* __restrict__ level, int* __restrict__ order) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= h.off[h.nl]) return;
  int l = 0;
  while (l + 1 < h.nl && t >= h.off[l + 1]) ++l;
  const int4 c = h.coords[l][t - h.off[l]];
  pts[3 * t] = (float)c.y * h.vs; pts[3 * t + 1] = (float)c.z * h.vs; pts[3 * t + 2] = (float)c.w * h.vs;
  scene[t] = c.x;
  level[t] = l;
  order[t] = (int)t;
}
inline double probe_bytes_head(int64_t n_all) { return (double)n_all * (16.0 + 12.0 + 12.0); }

// a generated set's k3 table from its parent's (fc_kernel_map_children: index arithmetic); a chain, one launch per set
struct Child { const int* pnbr; int64_t n_parent; int* nbr; };
inline double probe_bytes(const Child* c, int n) {
  double by = 0;
  for (int i = 0; i < n; ++i) by += 27.0 * 4.0 * (c[i].n_parent + 8.0 * c[i].n_parent);
  return by;
}

// occupancy masks of the rows of (27, n) tables (fc_nbr_row_masks), all tables that get a mask-sorted copy in one launch
__global__ void k_plan_row_masks(Batch<SortJob> bt) {
  int64_t lb;
  const SortJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int64_t o = lb * 256 + threadIdx.x;
  if (o >= j.n) return;
  unsigned int m = 0;
  for (int k = 0; k < 27; ++k)
    if (j.tab[(int64_t)k * j.n + o] >= 0) m |= 1u << k;
  j.masks[o] = (int)m;
}
inline double probe_bytes_masks(const Batch<SortJob>& b) { return sort_rows(b) * (27.0 * 4.0 + 4.0); }
// sorted[k][t] = tab[k][order[t]] (fc_permute_nbr); job blocks = 27 * ceil(n / 256)
__global__ void k_plan_permute(Batch<SortJob> bt) {
  int64_t lb;
  const SortJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int k = (int)(lb / j.nbx);
  const int64_t t = (lb % j.nbx) * 256 + threadIdx.x;
  if (t >= j.n) return;
  j.sorted[(int64_t)k * j.n + t] = j.tab[(int64_t)k * j.n + j.order[t]];      // (four rows per thread: no faster — a gather of 4-byte entries)
}
inline double probe_bytes_permute(const Batch<SortJob>& b) { return sort_rows(b) * (27.0 * 8.0 + 4.0); }

// ---- exact pair lists (fc_kernel_map_pairs) of many (27, n) tables per launch: count pass + fill pass ------------------------------
constexpr int PBLK = 1024;
struct PairJob { const int* tab; int* pi; int* po; int* pos; int* cnt; int* blk_cnt; int64_t n; int nblk; };
__global__ __launch_bounds__(PBLK) void k_plan_pairs_count(Batch<PairJob> bt) {
  int64_t lb;
  const PairJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int k = (int)(lb / j.nblk), blk = (int)(lb % j.nblk);
  const int64_t row = (int64_t)blk * PBLK + threadIdx.x;
  const int present = row < j.n && j.tab[(int64_t)k * j.n + row] >= 0;
  const int c = __syncthreads_count(present);
  if (threadIdx.x == 0) j.blk_cnt[k * j.nblk + blk] = c;
}
__global__ __launch_bounds__(PBLK) void k_plan_pairs_fill(Batch<PairJob> bt) {
  __shared__ int wave_cnt[PBLK / 64];
  __shared__ int base_s;
  int64_t lb;
  const PairJob& j = bt.j[batch_find(bt, blockIdx.x, &lb)];
  const int k = (int)(lb / j.nblk), blk = (int)(lb % j.nblk), nblk = j.nblk;
  const int64_t n = j.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave == 0) {                                   // pairs of offset k in the blocks before this one
    int a = 0;
    for (int b = lane; b < blk; b += 64) a += j.blk_cnt[k * nblk + b];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) base_s = a;
  }
  const int64_t row = (int64_t)blk * PBLK + tid;
  const int v = row < n ? j.tab[(int64_t)k * n + row] : -1;
  const unsigned long long bal = __ballot(v >= 0);
  if (lane == 0) wave_cnt[wave] = __popcll(bal);
  __syncthreads();
  int pre = base_s;
  for (int w = 0; w < wave; ++w) pre += wave_cnt[w];
  const int p = pre + __popcll(bal & ((1ull << lane) - 1ull));
  if (v >= 0) {
    j.pi[(int64_t)k * n + p] = v;
    j.po[(int64_t)k * n + p] = (int)row;
  }
  if (row < n) j.pos[(int64_t)k * n + row] = v >= 0 ? p : -1;
  if (blk == nblk - 1 && tid == PBLK - 1) j.cnt[k] = pre + __popcll(bal);
}
// compulsory bytes: table read twice, lists + positions written
inline double probe_bytes(const Batch<PairJob>& b, double by = 0) {
  for (int i = 0; i < b.count; ++i) by += 27.0 * (double)b.j[i].n * (4.0 + 4.0 + 12.0);
  return by;
}

int live_tiles(const int* cnt, int K) {
  int64_t t = 0;
  for (int k = 0; k < K; ++k) t += (cnt[k] + 127) / 128;
  return (int)t;
}

}  // namespace

#endif
