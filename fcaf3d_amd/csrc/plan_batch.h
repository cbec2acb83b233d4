// The plumbing of the native coordinate phase (plan.hip): the bump allocator of its arenas, the probe brackets around its launches,
// and the batched launch — one launch per KIND of job over the concatenated blocks of all jobs of that kind.
#ifndef FCAF3D_PLAN_BATCH_H
#define FCAF3D_PLAN_BATCH_H
#include "fc_common.h"
#include "plan_layout.h"
#include <vector>

namespace {

struct Bump {                       // bump allocation inside a caller-owned arena; base == nullptr: sizing pass
  char* base; int64_t off;
  void* take(int64_t bytes) {
    off = fc_align(off, 256);
    void* p = base ? base + off : nullptr;
    off += bytes > 0 ? bytes : 0;
    return p;
  }
  template <typename T> T* arr(int64_t n) { return (T*)take(n * (int64_t)sizeof(T)); }
};
// p + n elements where p may be the null block of the sizing pass: integer arithmetic (then simply the offset), no pointer arithmetic on nullptr
template <typename T> inline T* at(T* p, int64_t n) { return (T*)((intptr_t)p + n * (int64_t)sizeof(T)); }

// ---- probe: HIP-event brackets around every launch (group) of a plan, with its compulsory bytes — bench.py's `roofline.hbm_kernels`
// (cfg[C_PROBE] != 0; one thread at a time; read out by fc_plan_probe_read after the device has drained).  kind: PK_* ---------------
struct PlanProbe { int kind; double bytes; hipEvent_t a, b; };
std::vector<PlanProbe> g_pp;
std::vector<hipEvent_t> g_pp_pool;
hipEvent_t pp_event() {
  if (!g_pp_pool.empty()) { hipEvent_t e = g_pp_pool.back(); g_pp_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
struct Bracket {                     // RAII: records the closing event when the launch (group) has been enqueued
  hipStream_t s; bool on; size_t idx;
  Bracket(bool probe, int kind, double bytes, hipStream_t st) : s(st), on(probe), idx(0) {
    if (!on) return;
    PlanProbe p{kind, bytes, pp_event(), pp_event()};
    if (!p.a || !p.b) { on = false; return; }
    (void)hipEventRecord(p.a, s);
    idx = g_pp.size();
    g_pp.push_back(p);
  }
  ~Bracket() { if (on) (void)hipEventRecord(g_pp[idx].b, s); }
};

// ---- batched launches ------------------------------------------------------------------------------------------------------------
// Most of the phase is many small independent jobs of one kind (ten kernel maps, thirteen pair lists, five argsorts ...): each kind
// is ONE launch over the concatenated blocks of its jobs; a block finds its job by a scan of the (<= 24) first-block entries, which
// sit in the kernel arguments (scalar loads).
// (r6: a 2.1 KB argument block — 24 jobs of 80 bytes — made the launches misbehave on this stack, a 1.7 KB one did not: the
// batches stay below 1.5 KB, static_assert below; four pyramid levels need at most 16 jobs of a kind)
constexpr int MAXJ = 16;
template <typename J> struct Batch {
  J j[MAXJ];
  int64_t blk0[MAXJ + 1];
  int count;
  bool overflow;
  Batch() : count(0), overflow(false) { blk0[0] = 0; }
  void add(const J& job, int64_t blocks) {
    if (count >= MAXJ) { overflow = true; return; }
    j[count] = job;
    blk0[count + 1] = blk0[count] + (blocks > 0 ? blocks : 0);
    ++count;
  }
  int64_t blocks() const { return blk0[count]; }
};
template <typename J> __device__ __forceinline__ int batch_find(const Batch<J>& b, int64_t blk, int64_t* local) {
  int i = 0;
  while (i + 1 < b.count && blk >= b.blk0[i + 1]) ++i;
  *local = blk - b.blk0[i];
  return i;
}

template <typename J, typename F> int launch_batch(const Batch<J>& bt, int threads, hipStream_t s, F kernel) {
  static_assert(sizeof(Batch<J>) <= 1536, "batch descriptor too large for the kernel-argument block");
  if (bt.overflow) return FC_EINVAL;
  if (!bt.count || !bt.blocks()) return 0;
  kernel<<<(unsigned)bt.blocks(), threads, 0, s>>>(bt);
  FC_CHECK_LAUNCH();
  return 0;
}

}  // namespace

#endif
