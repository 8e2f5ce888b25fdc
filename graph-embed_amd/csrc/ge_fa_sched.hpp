// ge_fa_sched.hpp -- the single-level forceAtlas plan's schedule as pure host functions.
//
// fa_schedule decides which kernels a plan's step and repulsion pass launch and with
// what grid, lanes per row and row slots; fa_run_schedule decides how ge_force_atlas
// runs its iterations (one workgroup, the persistent kernel, graph replay).  None of it
// changes a bit of any result.  Host only, standard library only: the knobs are read
// from the environment in one place (fa_knobs_from_env) when a plan is created or
// ge_force_atlas is entered, never on a step; the plan (ge_fa.hip) passes in what it
// asked the device, and ge_fa_sched_query (include/ge.h) runs both with no device.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "ge.h"
#include "ge_dims.hpp"

namespace ge {

// What the kernels of ge_fa.hip fix.
constexpr int kRepThreads = 512;  // fa_repulse_strict's block
constexpr int kTileJ = 256;       // its LDS tile of partners
constexpr int kFastJBlocks = 16;  // j-range split
constexpr int kFastThreads = 256;
constexpr int kRowsPerThreadFast = 4;

constexpr int kSmallMax = 512;  // one row group per thread group below
// Above D = 4 (the wide schedule) the general kernel alone runs, with kSmallWideT
// threads: 512 threads leave 256 registers per lane, and the kernel holds xi, acc, F
// and fprev (D doubles each) beside a term.  Its rows are what the block's LDS leaves
// for records after the term buffer of kSmallWideT x D doubles, at most one row per
// thread: 256 at every D up to 16 (the LDS alone would allow 903 at D = 16).  Larger
// levels take the fused step.
constexpr int kSmallWideT = 256;
constexpr int small_cap(int D) {
  if (D <= kNarrowMaxDim) return kSmallMax;
  const size_t rows = (kLdsBlock - sizeof(double) * kSmallWideT * D) / (sizeof(double) * rec_width(D));
  return rows < (size_t)kSmallWideT ? (int)rows : kSmallWideT;
}
static_assert(small_cap(5) == 256 && small_cap(16) == 256, "one row per thread fits at every D");
constexpr int kSmallDefault = 64;
constexpr int kSmallNnz = 6144;
// CSR entries staged in LDS (the 4-D double-buffered term tile leaves less room)
constexpr int small_nnz_cap(int D) { return D == 4 ? 4096 : kSmallNnz; }
constexpr int kSmallFastT = 1024;  // domain-only kernel
constexpr int kSmallGenT = 512;    // general kernel
// The wide schedule's one-workgroup run: at most one row per thread of kSmallWideT.
constexpr int small_wide_cap(int D) { return small_cap(D) < kSmallWideT ? small_cap(D) : kSmallWideT; }

constexpr int kGrpT = 256;
// LDS of the fused step: the records (rec_width(D) doubles each), then the two term
// buffers of kGrpT x D doubles.  The records get what the block's LDS leaves after the
// term buffers, at most 96 KiB: 3072 records at D <= 3, 1536 at D = 4..7, 675 at D = 16.
constexpr size_t grouped_tb_bytes(int D) { return sizeof(double) * 2 * kGrpT * D; }
constexpr size_t grouped_rec_budget(int D) {
  return kLdsBlock - grouped_tb_bytes(D) < 96 * 1024 ? kLdsBlock - grouped_tb_bytes(D) : 96 * 1024;
}
constexpr int grouped_cap(int D) {
  return (int)(grouped_rec_budget(D) / (sizeof(double) * rec_width(D)));
}
static_assert(grouped_cap(3) == 3072 && grouped_cap(4) == 1536, "the D <= 4 caps are unchanged");

// The fused stream's bound (GE_STREAM_MAX overrides: tuning / tests).
constexpr int kStreamMax = 65536;

// GE_MODE_FARFIELD: the smallest level that runs the far field and the rows of a work
// item (64 R), both from measurement (fa_schedule; DESIGN.md, FARFIELD mode).
constexpr int kFarMinDefault = 131072;
constexpr int kFarItemRows = 64;

constexpr int kPersistMin = 128;  // fewer iterations: per-iteration launches
constexpr int kGraphSteps = 32;   // even: the buffers are back in place after a replay

// The single-level knobs, from the environment (fa_knobs_from_env): tuning and tests.
struct FaKnobs {
  int small_max = kSmallDefault;     // GE_SMALL_MAX, at most kSmallMax
  int small_g = 0;                   // GE_SMALL_G: 1, 2, 4, 8 or 16 (0: none)
  bool has_handover = false;         // GE_SMALL_HANDOVER: the domain-only kernel stops there
  int handover = 0;
  bool small_general_only = false;   // GE_SMALL_GENERAL_ONLY
  int stream_max = kStreamMax;       // GE_STREAM_MAX
  int grp_g = 0;                     // GE_GRP_G: a power of two up to 64 (0: none)
  bool grp_split = false;            // GE_GRP_SPLIT: no fused step
  int rep_blocks = 0;                // GE_REP_BLOCKS: caps fa_repulse_strict's blocks (0: none)
  int rep_r = 0;                     // GE_REP_R: 1, 2, 4 or 8 (0: none)
  bool sym_force = false, sym_off = false;  // GE_FA_SYM=1 / =0
  int far_min = kFarMinDefault;      // GE_FAR_MIN
  int far_item_rows = kFarItemRows;  // GE_FAR_R=1|4: 64 or 256 rows
  bool no_persist = false, no_graph = false;  // GE_NO_PERSIST, GE_NO_GRAPH
  bool packed = true;                // GE_FA_PACKED=0: no packed rows
  int pack_rows = 0;                 // GE_FA_PACK_ROWS=4|6 (0: by occupancy)
  bool persist_require = false;      // GE_PERSIST_REQUIRE=1: no fall-back from the persistent kernel
};

inline FaKnobs fa_knobs_from_env() {
  FaKnobs k;
  if (const char* e = std::getenv("GE_SMALL_MAX")) k.small_max = std::min(kSmallMax, std::atoi(e));
  if (const char* e = std::getenv("GE_SMALL_G")) {  // tuning override
    const int g = std::atoi(e);
    if (g == 1 || g == 2 || g == 4 || g == 8 || g == 16) k.small_g = g;
  }
  if (const char* e = std::getenv("GE_SMALL_HANDOVER")) {
    k.has_handover = true;
    k.handover = std::atoi(e);
  }
  k.small_general_only = std::getenv("GE_SMALL_GENERAL_ONLY") != nullptr;
  if (const char* e = std::getenv("GE_STREAM_MAX")) k.stream_max = std::atoi(e);
  if (const char* e = std::getenv("GE_GRP_G")) {  // tuning / test override
    const int g = std::atoi(e);
    if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) k.grp_g = g;
  }
  k.grp_split = std::getenv("GE_GRP_SPLIT") != nullptr;
  if (const char* e = std::getenv("GE_REP_BLOCKS")) k.rep_blocks = std::max(1, std::atoi(e));  // tests
  if (const char* e = std::getenv("GE_REP_R")) {  // tuning / test override
    const int r = std::atoi(e);
    if (r == 1 || r == 2 || r == 4 || r == 8) k.rep_r = r;
  }
  if (const char* e = std::getenv("GE_FA_SYM")) {
    k.sym_force = *e == '1';
    k.sym_off = *e == '0';
  }
  if (const char* e = std::getenv("GE_FAR_MIN")) k.far_min = std::atoi(e);
  if (const char* e = std::getenv("GE_FAR_R"))
    k.far_item_rows = std::atoi(e) == 1 ? 64 : std::atoi(e) == 4 ? 256 : k.far_item_rows;
  k.no_persist = std::getenv("GE_NO_PERSIST") != nullptr;
  k.no_graph = std::getenv("GE_NO_GRAPH") != nullptr;
  if (const char* e = std::getenv("GE_FA_PACKED")) k.packed = *e != '0';
  if (const char* e = std::getenv("GE_FA_PACK_ROWS")) k.pack_rows = std::atoi(e) == 6 ? 6 : 4;
  if (const char* e = std::getenv("GE_PERSIST_REQUIRE")) k.persist_require = *e == '1';
  return k;
}

struct FaSchedIn {
  int n = 0, rb = 0, re = 0, dim = 0;
  int mode = GE_MODE_STRICT;  // as requested (ge_fa_params.mode)
  bool repel_one = false;     // repel == 1
  bool linear = false;        // the linear attraction: !linlog && delta == 1
  bool wide = false;          // the wide schedule (wide_dim, ge_pair.hpp)
  int cus = 256;
  // every deg + 1 > 0 (far_masses_ok, ge_far.hpp).  A device answer: plan_init schedules
  // with true and, where FaSched::far_mass_check asks, again with what the device said.
  bool masses_ok = true;
  FaKnobs knobs;
};

// The kernels of a plan.  lanes, the ordered-pair grid and FAST's grid hold what their
// kernel would be launched with on these rows whether or not step / rep select it.
struct FaSched {
  int mode = GE_MODE_STRICT;  // effective: wide -> STRICT, a FARFIELD that does not run -> FAST
  int step = GE_FA_STEP_FUSED;  // ge_fa_plan_step: GE_FA_STEP_*
  int rep = GE_FA_REP_GROUPED;  // the repulsion pass (the split step, ge_fa_plan_repulse): GE_FA_REP_*
  bool wide = false;
  int lanes = 1;  // lanes per row of the fused step and the grouped repulsion; wide: 64 or 8
  bool repel_one = false, linear = false;  // the kernels' body flags (wide: the general bodies)
  int per = 0, nb = 0, R = 1;              // fa_repulse_strict: rows per block, blocks, row slots
  int fast_blocks = 0, fast_jb = 0;        // fa_repulse_fast's grid
  bool sym = false;                        // the plan holds the symmetric sweeps' tables
  int far_reason = GE_FAR_NOT_REQUESTED, far_item_rows = kFarItemRows;
  bool far_mass_check = false;  // the reason rests on masses_ok: ask the device
  bool fpart = false;           // FAST's partial sums are needed
};

namespace fa_sched {

// Lanes per row of the small-level kernels.
inline int grouped_lanes(int rows, const FaKnobs& k) {
  int G = 1;  // lanes per row: aim for >= 128 K lanes, at most one wave per row
  while (G < 64 && (long long)rows * G < 131072) G *= 2;  // n = 4373: G = 32 (175 us, G = 16: 211)
  return k.grp_g ? k.grp_g : G;
}

// fa_repulse_strict's grid: one block per CU, rows split evenly (rounded to whole
// 64-row wave slots).  GE_REP_BLOCKS caps the blocks (tests).  An empty shard launches
// nothing: no grid.
inline void rep_grid(int rows, int cus, const FaKnobs& k, int& per, int& nb) {
  per = nb = 0;
  if (rows <= 0) return;
  const int cap = k.rep_blocks ? k.rep_blocks : cus;
  const int blocks = std::max(1, std::min(cap, (rows + 63) / 64));
  per = (rows + blocks - 1) / blocks;
  per = (per + 63) / 64 * 64;
  nb = (rows + per - 1) / per;
}

// lanes per row for n rows in a T-thread workgroup
inline int small_group(int n, int T, const FaKnobs& k) {
  if (k.small_g && n * k.small_g <= T) return k.small_g;  // tuning override
  int G = 1;
  while (G < 16 && n * G * 2 <= T) G *= 2;
  return G;
}

}  // namespace fa_sched

inline FaSched fa_schedule(const FaSchedIn& in) {
  const FaKnobs& k = in.knobs;
  const int rows = std::max(in.re - in.rb, 0);
  const bool whole = in.rb == 0 && in.re == in.n;
  FaSched s;
  s.wide = in.wide || in.dim > kNarrowMaxDim;
  // FAST is a tolerance-only mode and has no wide kernels: the exact ones satisfy it
  s.mode = s.wide ? GE_MODE_STRICT : in.mode;
  // The far field runs for a whole narrow level with positive masses from far_min
  // vertices up; every other FARFIELD plan is a FAST plan (include/ge.h).  far_min: the
  // smallest power of two from 2^13 at which FARFIELD beat FAST at d = 3, theta = 0.5 on
  // an MI355X is 2^17 (ms per step, FAST / FARFIELD: 2^16 3.5 / 5.9, 2^17 13.9 / 12.0-12.5,
  // 2^18 50 / 25-27, 2^20 780 / 112-116; profiles/r13/farfield_crossover.jsonl);
  // GE_FAR_MIN overrides.  Items of 64 rows: 108-112 ms per C2 step against 231-268
  // for 256 rows (same log; GE_FAR_R=1|4 overrides, tests and tuning).
  s.far_item_rows = k.far_item_rows;
  if (in.mode == GE_MODE_FARFIELD) {
    s.far_mass_check = !s.wide && whole;
    s.far_reason = s.wide         ? GE_FAR_DIM
                   : !whole       ? GE_FAR_ROW_SHARD
                   : !in.masses_ok ? GE_FAR_MASS
                   : in.n < k.far_min ? GE_FAR_SMALL
                                      : GE_FAR_ACTIVE;
    if (s.far_reason != GE_FAR_ACTIVE && s.mode == GE_MODE_FARFIELD) s.mode = GE_MODE_FAST;
  }
  const bool far = s.far_reason == GE_FAR_ACTIVE;
  s.fpart = s.mode == GE_MODE_FAST || far;  // the far field's non-finite iterations run FAST
  // Symmetric repulsion: STRICT, every row on this plan (a row shard keeps the
  // ordered-pair kernel), and a level past the grouped / streamed kernels.
  // GE_FA_SYM=0 keeps fa_repulse_strict (comparisons), GE_FA_SYM=1 forces it: the plan
  // then holds the sweeps at any size, but up to stream_max its step is still the fused
  // one, and only ge_fa_plan_repulse (or GE_GRP_SPLIT) reaches them.
  s.sym = !k.sym_off && !s.wide && s.mode == GE_MODE_STRICT && whole &&
          (k.sym_force || in.n > k.stream_max);
  // Small levels (n <= grouped_cap: fa_grouped_step) and mid-size ones (n <=
  // stream_max: fa_grouped_stream): one launch per iteration.
  const int cap = grouped_cap(in.dim);
  s.step = s.mode != GE_MODE_STRICT || in.n > k.stream_max || k.grp_split ? GE_FA_STEP_SPLIT
           : in.n > cap                                                    ? GE_FA_STEP_STREAM
                                                                           : GE_FA_STEP_FUSED;
  // The repulsion launch of one iteration: the symmetric sweeps, the far field (FAST's
  // kernels in an iteration whose box is not finite) or the mode's ordered-pair kernels.
  // wide: the ordered-pair kernel at every size, one row slot per lane (ge_pair.hpp).
  s.rep = s.sym                      ? GE_FA_REP_SWEEPS
          : far                      ? GE_FA_REP_FARFIELD
          : s.wide                   ? GE_FA_REP_ORDERED_WIDE
          : s.mode == GE_MODE_FAST   ? GE_FA_REP_FAST
          : in.n <= cap              ? GE_FA_REP_GROUPED
                                     : GE_FA_REP_ORDERED;
  // wide (ge_pair.hpp): the general bodies (same bits as their specialisations) in two
  // group sizes, a wave per row below 8192 rows (grouped_lanes 32 or 64), else 8 lanes.
  s.lanes = fa_sched::grouped_lanes(rows, k);
  if (s.wide) s.lanes = s.lanes >= 32 ? 64 : 8;
  s.repel_one = in.repel_one && !s.wide;
  s.linear = in.linear && !s.wide;
  fa_sched::rep_grid(rows, in.cus, k, s.per, s.nb);
  // Row slots per lane.  Measured at C2 size (scripts/shard_tune.py, rows of
  // an N-GPU shard): with more than 1024 rows per block 8 slots x 1 partner is
  // fastest (500 K rows: 581 against 563 Gpairs/s for R = 1); at 1024 and below
  // 1 slot x 8 partners (250 K rows: R = 1 566, R = 8 551; 125 K rows: R = 1
  // 565 Gpairs/s).
  s.R = s.wide ? 1 : k.rep_r ? k.rep_r : s.per > 2 * kRepThreads ? 8 : 1;
  s.fast_blocks = (rows + kFastThreads * kRowsPerThreadFast - 1) / (kFastThreads * kRowsPerThreadFast);
  s.fast_jb = std::max(1, std::min(kFastJBlocks, (in.n + kTileJ - 1) / kTileJ));
  return s;
}

// How ge_force_atlas runs `iterations` of a whole level (plan.rb == 0, plan.re == n).
struct FaRunIn {
  FaSchedIn plan;
  int nnz = 0, iterations = 0;
};

struct FaRunSched {
  bool small = false;  // every iteration in one workgroup (fa_small_strict), no plan
  // lanes per row of its domain-only kernel (0: the general kernel from iteration 0)
  // and of its general kernel (wide: 8, 2 or 1)
  int small_g_domain = 0, small_g_general = 0;
  bool small_staged = false;  // the CSR entries fit the kernel's LDS
  int small_handover = 0;     // the iteration at which the domain-only kernel stops
  bool persist = false;       // fa_grouped_persistent is tried
  int persist_g = 0;          // from this many lanes per row down (launch_persistent)
  bool packed = false;        // at 64 lanes: the packed rows
  int pack_rows = 0;          // 4 or 6 (0: by occupancy)
  bool graph = false;         // the per-iteration path replays a graph of kGraphSteps
};

inline FaRunSched fa_run_schedule(const FaRunIn& in) {
  const FaSchedIn& p = in.plan;
  const FaKnobs& k = p.knobs;
  const FaSched plan = fa_schedule(p);
  FaRunSched r;
  // One workgroup wins only for tiny levels (n = 14: 3.7 against 12 us per
  // iteration); from n ~ 100 the multi-block grouped path does (n = 125: 17 us
  // against 26).  GE_SMALL_MAX moves the bound (tests use it up to kSmallMax).
  // The wide schedule runs the one-workgroup kernel in its general form up to
  // small_wide_cap(dim) rows (FAST runs the exact kernels there); it has no persistent
  // kernel: above the bound its long runs replay a graph of fused steps (below).
  const int small_max = plan.wide ? std::min(k.small_max, small_wide_cap(p.dim)) : k.small_max;
  r.small = p.n <= small_max && (p.mode == GE_MODE_STRICT || plan.wide);
  if (r.small) {
    if (plan.wide) {  // the general kernel from iteration 0, kSmallWideT threads, 1, 2 or 8 lanes
      const int G = fa_sched::small_group(p.n, kSmallWideT, k);  // n G <= kSmallWideT
      r.small_g_general = G >= 8 ? 8 : G >= 2 ? 2 : 1;
      r.small_handover = in.iterations;
    } else {
      r.small_staged = in.nnz <= small_nnz_cap(p.dim);
      // the domain-only kernel has the linear attraction only (linlog == 0, delta == 1)
      if (!k.small_general_only && p.linear)
        r.small_g_domain = fa_sched::small_group(p.n, kSmallFastT, k);
      r.small_g_general = fa_sched::small_group(p.n, kSmallGenT, k);
      r.small_handover = k.has_handover ? k.handover : in.iterations;  // test hook
    }
    return r;
  }
  // All iterations of a small level (n <= grouped_cap, every row) in one launch of
  // fa_grouped_persistent; 64 lanes per row: the packed rows unless GE_FA_PACKED=0.
  r.persist = p.mode == GE_MODE_STRICT && in.iterations >= kPersistMin && !plan.wide &&
              !k.no_persist && p.n <= grouped_cap(p.dim) && p.rb == 0 && p.re == p.n;
  if (r.persist) {
    r.persist_g = plan.lanes;
    r.packed = k.packed;
    r.pack_rows = k.packed ? k.pack_rows : 0;
  }
  // Long runs (the coarsest level's 1e5 iterations) replay a captured graph of
  // kGraphSteps iterations: host launch overhead would otherwise dominate the
  // microsecond-scale kernels of a small level.
  // (not with the far field: its pass synchronises once, include/ge.h)
  r.graph = in.iterations >= 4 * kGraphSteps && plan.rep != GE_FA_REP_FARFIELD && !k.no_graph;
  return r;
}

// ge_force_atlas_batch: many independent graphs in one call (ge_fa_batch.hip).  A graph of
// n rows and `entries` stored entries runs in one of three classes; none changes a bit:
//   wave    1 <= n <= kBatchWaveMax, STRICT or the wide schedule: one wave per graph,
//           kBatchWaves graphs per workgroup of one launch; lanes per row: the largest
//           power of two with n lanes <= 64 (GE_SMALL_G where it fits the wave);
//   block   up to small_cap(dim) rows, same modes: one workgroup per graph of one launch,
//           fa_small_strict's general form; lanes per row from small_group, at most
//           kBatchBlockLanes (more lanes would need n <= 64);
//   serial  everything else -- larger graphs, and every graph of a narrow dimension under
//           FAST / FARFIELD, where ge_force_atlas itself leaves the one-workgroup kernel:
//           fa_run_device, one graph after another.  An empty graph is serial and runs
//           nothing.
// Within a class the graphs launch by descending n + entries (fa_batch_order), so the
// waves of a workgroup finish together and the largest workgroups start first.
constexpr int kBatchWaveMax = 64;
constexpr int kBatchWaves = 4;
constexpr int kBatchBlockLanes = 4;

struct FaBatchIn {
  int dim = 0;
  int mode = GE_MODE_STRICT;  // as requested (ge_fa_params.mode)
  bool wide = false;          // the wide schedule (wide_dim, ge_pair.hpp)
  FaKnobs knobs;
};

// threads of the block class's workgroup: fa_small_strict's general kernel's
inline int fa_batch_block_threads(const FaBatchIn& in) {
  return in.wide || in.dim > kNarrowMaxDim ? kSmallWideT : kSmallGenT;
}

inline void fa_batch_class(const FaBatchIn& in, int n, int* cls, int* lanes) {
  const bool wide = in.wide || in.dim > kNarrowMaxDim;
  const bool one_workgroup = in.mode == GE_MODE_STRICT || wide;  // as FaRunSched::small
  const int cap = wide ? small_wide_cap(in.dim) : small_cap(in.dim);
  *cls = GE_FA_BATCH_SERIAL;
  *lanes = 0;
  if (!one_workgroup || n < 1 || n > cap) return;
  if (n <= kBatchWaveMax) {
    int G = 1;
    while (n * G * 2 <= 64) G *= 2;
    if (in.knobs.small_g && n * in.knobs.small_g <= 64) G = in.knobs.small_g;  // tuning override
    *cls = GE_FA_BATCH_WAVE;
    *lanes = G;
    return;
  }
  *cls = GE_FA_BATCH_BLOCK;
  *lanes = std::min(kBatchBlockLanes, fa_sched::small_group(n, fa_batch_block_threads(in), in.knobs));
}

// Classes and lanes per row of `count` graphs (cls, lanes: count ints each) and
// totals[GE_FA_BATCH_TOTALS] = {waves, blocks, serials, workgroups of the wave launch}.
inline void fa_batch_schedule(const FaBatchIn& in, int count, const int* sizes, int* cls,
                              int* lanes, int* totals) {
  int per[3] = {0, 0, 0};
  for (int g = 0; g < count; ++g) {
    fa_batch_class(in, sizes[g], &cls[g], &lanes[g]);
    ++per[cls[g]];
  }
  totals[0] = per[GE_FA_BATCH_WAVE];
  totals[1] = per[GE_FA_BATCH_BLOCK];
  totals[2] = per[GE_FA_BATCH_SERIAL];
  totals[3] = (per[GE_FA_BATCH_WAVE] + kBatchWaves - 1) / kBatchWaves;
}

// The graphs of class c in launch order: descending n + entries, ties by index.
inline void fa_batch_order(int count, const int* sizes, const int* entries, const int* cls, int c,
                           int* out) {
  int k = 0;
  for (int g = 0; g < count; ++g)
    if (cls[g] == c) out[k++] = g;
  std::stable_sort(out, out + k, [&](int a, int b) {
    return (long long)sizes[a] + entries[a] > (long long)sizes[b] + entries[b];
  });
}

// The scalars of ge_fa_sched_query / ge_fa_plan_schedule (GE_FA_SCHED_*).
inline void fa_sched_scalars(const FaSched& s, int* out) {
  out[GE_FA_SCHED_MODE] = s.mode;
  out[GE_FA_SCHED_STEP] = s.step;
  out[GE_FA_SCHED_REP] = s.rep;
  out[GE_FA_SCHED_WIDE] = s.wide;
  out[GE_FA_SCHED_LANES] = s.lanes;
  out[GE_FA_SCHED_REPEL_ONE] = s.repel_one;
  out[GE_FA_SCHED_LINEAR] = s.linear;
  out[GE_FA_SCHED_PER] = s.per;
  out[GE_FA_SCHED_NB] = s.nb;
  out[GE_FA_SCHED_R] = s.R;
  out[GE_FA_SCHED_FAST_BLOCKS] = s.fast_blocks;
  out[GE_FA_SCHED_FAST_JB] = s.fast_jb;
  out[GE_FA_SCHED_SYM] = s.sym;
  out[GE_FA_SCHED_FAR_REASON] = s.far_reason;
  out[GE_FA_SCHED_FAR_ITEM_ROWS] = s.far_item_rows;
  out[GE_FA_SCHED_FPART] = s.fpart;
}

inline void fa_run_scalars(const FaRunSched& r, int* out) {
  out[GE_FA_SCHED_SMALL] = r.small;
  out[GE_FA_SCHED_SMALL_G_DOMAIN] = r.small_g_domain;
  out[GE_FA_SCHED_SMALL_G_GENERAL] = r.small_g_general;
  out[GE_FA_SCHED_SMALL_STAGED] = r.small_staged;
  out[GE_FA_SCHED_SMALL_HANDOVER] = r.small_handover;
  out[GE_FA_SCHED_PERSIST] = r.persist;
  out[GE_FA_SCHED_PERSIST_G] = r.persist_g;
  out[GE_FA_SCHED_PACKED] = r.packed;
  out[GE_FA_SCHED_PACK_ROWS] = r.pack_rows;
  out[GE_FA_SCHED_GRAPH] = r.graph;
}

}  // namespace ge
