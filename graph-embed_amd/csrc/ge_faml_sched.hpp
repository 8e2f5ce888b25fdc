// ge_faml_sched.hpp -- the multilevel plan's schedule as a pure host function.
//
// faml_schedule decides everything about how a level runs that does not need the
// device: the size classes and resident packs, the rows of split aggregates a rank
// owns, the STRICT and FAST work items, which streamed aggregates run as symmetric
// sweeps and which as row blocks, and the queue position and priority level of
// every sweep unit.  None of it changes a bit of any result; the speed of the
// streamed path rests on it.  Host only, standard library only: the plan
// (ge_faml.hip, faml_plan_build) passes in what it asked the device and the
// environment, and ge_faml_sched_create (include/ge.h) runs it with no device at all.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "ge.h"

namespace ge {

// Layouts of int2 / int4 (asserted in ge_faml.hip): items, and units / FAST items.
struct SchedInt2 { int x, y; };
struct SchedInt4 { int x, y, z, w; };

// Streamed repulsion variants: row slots R x partners in flight U.
#define GE_BIG_VARIANTS(X) X(1, 1) X(1, 2) X(1, 4) X(2, 1) X(4, 1)
constexpr int big_code(int R, int U) { return R * 8 + U; }
constexpr int kBigDefaultR = 1, kBigDefaultU = 1;
// What the kernels fix (asserted equal to their constants in ge_faml.hip): 64-row
// tiles of one faml_fast_repulse item, waves of one faml_sym_repulse block, and the
// unit kinds of ge_sym.hpp.
constexpr int kSchedFastR = 4, kSchedSymWaves = 4, kSchedSweep = 0, kSchedRows = 1;
// GE_MODE_FARFIELD: the smallest streamed aggregate that takes the far field (ge_far.hip,
// the segmented engine): the smallest swept size from which FARFIELD's range lay wholly
// below FAST's on levels of equal aggregates, 4M rows, d = 3, theta = 0.5 (ms per step,
// FAST / FARFIELD: 2^12 13.21-13.29 / 12.99-13.05, 2^13 25.6 / 18.5-18.7, 2^14 50.5 /
// 26.7-26.9, 2^15 99.5 / 38.3-38.8, 2^16 197.5 / 51.1-51.5; profiles/r19/crossover.jsonl),
// and never below 4096.  A streamed aggregate has more than 256 members, so an override
// is held to 257 at least.
constexpr int kFarMinMlDefault = 4096;

// The schedule's knobs, from the environment (faml_knobs_from_env).
struct FamlKnobs {
  bool has_res_cap = false;
  int res_cap = 0;  // GE_FAML_RES_CAP: the cap itself (tests: the large-resident class on small inputs)
  int R = kBigDefaultR, U = kBigDefaultU;  // GE_FAML_R / GE_FAML_U
  bool sym = true;                         // GE_FAML_SYM (0: no symmetric sweeps)
  double chain_k = 2.5;                    // GE_FAML_SYM_CHAIN (0: all sweeps)
  int far_min_ml = kFarMinMlDefault;       // GE_FAR_MIN_ML
};

inline FamlKnobs faml_knobs_from_env() {
  FamlKnobs k;
  if (const char* e = std::getenv("GE_FAML_RES_CAP")) {
    k.has_res_cap = true;
    k.res_cap = std::atoi(e);
  }
  if (const char* e = std::getenv("GE_FAML_R")) k.R = std::atoi(e);
  if (const char* e = std::getenv("GE_FAML_U")) k.U = std::atoi(e);
  if (const char* e = std::getenv("GE_FAML_SYM")) k.sym = *e != '0';
  if (const char* e = std::getenv("GE_FAML_SYM_CHAIN")) k.chain_k = std::atof(e);  // 0: all sweeps
  if (const char* e = std::getenv("GE_FAR_MIN_ML")) k.far_min_ml = std::max(257, std::atoi(e));
  return k;
}

// aggs: the aggregates this plan runs (strictly increasing ids).
// split: aggregates whose row tiles are dealt over the ranks (the same list on
// every rank; tiles [T r / N, T (r + 1) / N) to rank r).
struct FamlSchedIn {
  const int* pt_ip = nullptr;  // P_T's indptr on the host
  const std::vector<int>* aggs = nullptr;
  const std::vector<int>* split = nullptr;
  int rank = 0, nranks = 1;
  int dim = 0, mode = GE_MODE_STRICT;  // mode as requested (ge_fa_params.mode)
  int large_cap = 0;                   // members the one-aggregate resident kernel holds
  bool wide = false;                   // the wide schedule (ge_pair.hpp)
  int cus = 256, sym_occ = 1;          // CUs; blocks per CU of faml_sym_repulse
  FamlKnobs knobs;
};

// Everything faml_plan_build uploads or stores.
struct FamlSched {
  int res_cap = 0, census[4] = {0, 0, 0, 0};  // aggregates: small, mid, large-resident, streamed
  std::vector<int> order, beg;  // resident packs; beg: small, mid (off_m), large (off_l)
  size_t off_m = 0, off_l = 0;
  int ns = 0, nm = 0, nl = 0;
  std::vector<int> rows, irows, huge;  // streamed rows of this rank; rows initialised; centred at the end
  std::vector<int> xr, xcounts;        // the split rows by rank, and how many per rank
  int R = kBigDefaultR, U = kBigDefaultU, code = 0;
  std::vector<SchedInt2> items;   // STRICT (aggregate, first row), descending work
  std::vector<SchedInt4> fitems;  // FAST (aggregate, first row, end row, 0), descending work
  std::vector<int> faraggs;       // FARFIELD: the whole streamed aggregates on the far field, larger first
  bool fast = false, sym = false, wide = false;
  std::vector<SchedInt4> units;  // (aggregate, row tile, progress offset or priority, kind)
  int ntiles = 0, swept = 0, rows_mode = 0, sym_blocks = 0;
  double streamed_pairs = 0.0;
};

namespace sched {

struct Tiles { int t0, t1; };

// The inputs with the streamed whole aggregates found by the classing.
struct Work {
  const FamlSchedIn& in;
  std::vector<int> big;
  int size_of(int a) const { return in.pt_ip[a + 1] - in.pt_ip[a]; }
  int ntiles_of(int a) const { return (size_of(a) + 63) / 64; }
  Tiles tiles_of(int a, int r) const {  // rank r's row tiles of split aggregate a
    const long long T = ntiles_of(a);
    return {(int)(T * r / in.nranks), (int)(T * (r + 1) / in.nranks)};
  }
  int row_end(int a, const Tiles& t) const { return std::min(size_of(a), 64 * t.t1); }
};

// Greedy packs over `ids` (already size-sorted) with total members <= cap.
inline void build_packs(const Work& w, const std::vector<int>& ids, int cap, int max_aggs,
                        std::vector<int>& order, std::vector<int>& beg) {
  beg.push_back((int)order.size());
  int tot = 0, cnt = 0;
  for (int a : ids) {
    const int s = w.size_of(a);
    if (cnt > 0 && (tot + s > cap || cnt >= max_aggs)) {
      beg.push_back((int)order.size());
      tot = 0;
      cnt = 0;
    }
    order.push_back(a);
    tot += s;
    ++cnt;
  }
  if (cnt > 0) beg.push_back((int)order.size());
}

// Size classes and the resident packs; w.big: the streamed whole aggregates by size.
inline void classes_and_packs(Work& w, FamlSched& s) {
  const FamlSchedIn& in = w.in;
  // Work of aggregate a per iteration ~ s^2.  Aggregates whose share would
  // keep one CU busy for more than a quarter of the per-CU average go to the
  // streamed path (many blocks per aggregate, one launch per iteration);
  // the rest stay resident in LDS for all iterations.
  double W = 0.0;
  for (int a : *in.aggs) {
    const double sz = w.size_of(a);
    W += sz * sz;
  }
  const double per_cu = W / std::max(in.cus, 1);
  int res_cap = (int)std::sqrt(per_cu / 4.0);  // largest aggregate kept resident
  if (in.knobs.has_res_cap) res_cap = in.knobs.res_cap;
  res_cap = std::max(256, std::min(res_cap, in.large_cap));
  s.res_cap = res_cap;

  std::vector<int> small, mid, large;
  for (int a : *in.aggs) {
    const int sz = w.size_of(a);
    if (sz <= 0) continue;
    if (sz <= 64) small.push_back(a);
    else if (sz <= 256) mid.push_back(a);
    else if (sz <= res_cap) large.push_back(a);
    else w.big.push_back(a);
  }
  s.census[0] = (int)small.size();
  s.census[1] = (int)mid.size();
  s.census[2] = (int)large.size();
  s.census[3] = (int)w.big.size() + (int)in.split->size();
  auto by_size = [&](int x, int y) {
    const int sx = w.size_of(x), sy = w.size_of(y);
    return sx != sy ? sx > sy : x < y;
  };
  std::sort(small.begin(), small.end(), by_size);
  std::sort(mid.begin(), mid.end(), by_size);
  std::sort(large.begin(), large.end(), by_size);
  std::sort(w.big.begin(), w.big.end(), by_size);

  std::vector<int> beg_m, beg_l;
  build_packs(w, small, 64, 64, s.order, s.beg);
  build_packs(w, mid, 256, 256, s.order, beg_m);
  build_packs(w, large, in.large_cap, 1, s.order, beg_l);
  s.ns = (int)s.beg.size() - 1;
  s.nm = (int)beg_m.size() - 1;
  s.nl = (int)beg_l.size() - 1;
  s.off_m = s.beg.size();
  s.beg.insert(s.beg.end(), beg_m.begin(), beg_m.end());
  s.off_l = s.beg.size();
  s.beg.insert(s.beg.end(), beg_l.begin(), beg_l.end());
}

// The streamed rows this rank computes, the rows it initialises, and the exchange
// tables of the split aggregates.
inline void owned_rows(const Work& w, FamlSched& s) {
  const FamlSchedIn& in = w.in;
  // streamed members and their repulsion work items (aggregate, first row):
  // R row slots of 64 per wave, taken in descending-work order
  for (int a : w.big)
    for (int li = 0; li < w.size_of(a); ++li) s.rows.push_back(in.pt_ip[a] + li);
  // split aggregates: this rank's row tiles are streamed rows like the others; every
  // member is initialised and given its internal degree (all are columns)
  s.irows = s.rows;
  s.xcounts.assign(in.nranks, 0);
  for (int r = 0; r < in.nranks; ++r)
    for (int a : *in.split) {
      const Tiles t = w.tiles_of(a, r);
      for (int li = 64 * t.t0; li < w.row_end(a, t); ++li) {
        const int c = in.pt_ip[a] + li;
        if (r == in.rank) s.rows.push_back(c);
        s.irows.push_back(c);
        s.xr.push_back(c);
        ++s.xcounts[r];
      }
    }
  s.huge = w.big;  // centred and scaled at the end: the split ones on every rank
  s.huge.insert(s.huge.end(), in.split->begin(), in.split->end());
  for (int a : w.big) {
    const double sa = w.size_of(a);
    s.streamed_pairs += sa * (sa - 1);
  }
  for (int a : *in.split) {  // this rank's rows against all members
    const Tiles t = w.tiles_of(a, in.rank);
    const double sa = w.size_of(a);
    s.streamed_pairs += (std::min(sa, 64.0 * t.t1) - std::min(sa, 64.0 * t.t0)) * (sa - 1);
  }
}

// The STRICT variant (R, U) and its work items.
inline void strict_items(const Work& w, FamlSched& s) {
  const FamlSchedIn& in = w.in;
  // row slots x partners in flight (GE_FAML_R / GE_FAML_U override; only the
  // compiled variants of GE_BIG_VARIANTS are accepted)
  int R = in.knobs.R, U = in.knobs.U;
  bool known = false;
#define GE_BIG_KNOWN(RR, UU) known = known || (R == RR && U == UU);
  GE_BIG_VARIANTS(GE_BIG_KNOWN)
#undef GE_BIG_KNOWN
  // the wide schedule (ge_pair.hpp) has the one variant, and no symmetric sweeps
  if (!known || in.wide) {
    R = kBigDefaultR;
    U = kBigDefaultU;
  }
  // split tiles are one-row-slot items (R = 1): settle R before any item is built,
  // so the whole-aggregate items step by the R the kernel is launched with
  for (int a : *in.split) {
    const Tiles t = w.tiles_of(a, in.rank);
    if (t.t1 > t.t0) R = 1;
  }
  struct Item { int a, r0; double work; };
  std::vector<Item> its;
  for (int a : w.big) {
    const int sz = w.size_of(a);
    for (int r0 = 0; r0 < sz; r0 += 64 * R)
      its.push_back({a, r0, (double)std::min(R, (sz - r0 + 63) / 64) * sz});
  }
  for (int a : *in.split) {  // this rank's tiles, one item each (R = 1 rows per slot)
    const int sz = w.size_of(a);
    const Tiles t = w.tiles_of(a, in.rank);
    for (int q = t.t0; q < t.t1; ++q) its.push_back({a, 64 * q, (double)sz});
  }
  std::stable_sort(its.begin(), its.end(),
                   [](const Item& x, const Item& y) { return x.work > y.work; });
  for (const Item& it : its) s.items.push_back({it.a, it.r0});
  s.R = R;
  s.U = U;
  s.code = big_code(R, U);
}

// FAST mode, and FARFIELD mode for the aggregates that do not take the far field: row
// items of up to kSchedFastR 64-row tiles, whole aggregates and this rank's
// tiles of the split ones alike (a row's sum does not depend on the item it is in);
// the STRICT schedule knobs (GE_FAML_SYM*, GE_FAML_R / U) do not apply
inline void fast_items(const Work& w, FamlSched& s) {
  const FamlSchedIn& in = w.in;
  const bool far = in.mode == GE_MODE_FARFIELD && !in.wide && in.dim <= 4;
  if (far)  // the size-qualified whole aggregates (w.big: larger first); the rest are FAST items
    for (int a : w.big)
      if (w.size_of(a) >= in.knobs.far_min_ml) s.faraggs.push_back(a);
  if ((in.mode == GE_MODE_FAST || in.mode == GE_MODE_FARFIELD) && !in.wide) {
    struct FItem { int a, r0, r1; double work; };
    std::vector<FItem> fi;
    auto cut = [&](int a, int b0, int b1) {  // rows [b0, b1) of aggregate a
      const int sz = w.size_of(a);
      for (int r0 = b0; r0 < b1; r0 += 64 * kSchedFastR) {
        const int r1 = std::min(b1, r0 + 64 * kSchedFastR);
        fi.push_back({a, r0, r1, (double)((r1 - r0 + 63) / 64) * sz});
      }
    };
    for (int a : w.big)
      if (!far || w.size_of(a) < in.knobs.far_min_ml) cut(a, 0, w.size_of(a));
    for (int a : *in.split) {
      const Tiles t = w.tiles_of(a, in.rank);
      cut(a, 64 * t.t0, w.row_end(a, t));
    }
    std::stable_sort(fi.begin(), fi.end(),
                     [](const FItem& x, const FItem& y) { return x.work > y.work; });
    for (const FItem& f : fi) s.fitems.push_back({f.a, f.r0, f.r1, 0});
  }
  s.fast = !s.fitems.empty();
}

// Per streamed whole aggregate (row tiles T, in w.big's order): 1 when it runs as
// whole row blocks, 0 as symmetric sweeps.
inline std::vector<char> sweeps_or_rows(const Work& w, const FamlSched& s,
                                        const std::vector<int>& T) {
  const FamlSchedIn& in = w.in;
  // The sweeps of an aggregate with T row tiles form a chain of ~2.5 T tile-times
  // (each sweep starts after its predecessor has passed its first two tiles); the
  // launch takes about (sum of T^2 / 2 sweep tiles) / (resident waves).  While the
  // longest chain exceeds that, the largest aggregate runs as plain row blocks
  // (every ordered pair, ~0.8 the step cost of a sweep, no chain).
  const bool any_big = !w.big.empty();
  const double waves = (double)s.sym_blocks * kSchedSymWaves;
  // Per streamed aggregate: symmetric sweeps or whole row blocks.  The launch lasts
  // about max(work / waves, the longest row block, the sweeps' start + the longest
  // sweep chain) tile-times, where
  //   sweeps:  work T^2 / 2 + T,  chain chain_k T (each sweep starts ~2 tiles behind
  //            the one before)
  //   rows:    work row_k T^2,    chain row_k T   (every ordered pair, no chain)
  // Whole row blocks are first in the queue, so when they hold more than the waves
  // the sweeps start late (start = their work / waves).  The k largest aggregates
  // run as row blocks, k minimising the prediction; no mix whose row blocks hold
  // more than half the waves (their raised waves delay and slow the sweeps: per-rank
  // shares of C4, N = 4: 20 of 24 aggregates as row blocks 70 ms per iteration, 7 of
  // 25 58 ms).  At N = 1 (C4) the launch is work-bound and every aggregate sweeps;
  // the shares of a multi-GPU run are chain-bound.
  // row_k: a row-block tile (64 x 64 ordered pairs) against a sweep tile (64 x 64
  // unordered), wave time at full load -- 0.6 measured on an N = 8 share of C4
  // (all row blocks: 17.9 us per row tile per wave, against 29.8 us per sweep tile
  // at N = 1; profiles/r04/sym_timeline_rows_n8.json)
  const double chain_k = in.knobs.chain_k;
  const double row_k = 0.6;
  std::vector<char> as_rows(w.big.size(), 0);
  if (chain_k > 0.0 && any_big) {
    std::vector<size_t> by_T(w.big.size());
    std::iota(by_T.begin(), by_T.end(), 0);
    std::stable_sort(by_T.begin(), by_T.end(), [&](size_t x, size_t y) { return T[x] > T[y]; });
    double work = 0.0, row_work = 0.0, row_units = 0.0, pbest = 1e300;
    size_t best_k = 0;
    for (size_t b = 0; b < w.big.size(); ++b) work += 0.5 * T[b] * (double)T[b] + T[b];
    for (size_t k = 0; k <= by_T.size(); ++k) {  // the k largest as row blocks
      const double start = row_units > waves ? row_work / waves : 0.0;
      const double sweep_chain = k < by_T.size() ? start + chain_k * T[by_T[k]] : 0.0;
      const double row_path = k > 0 ? row_k * T[by_T[0]] : 0.0;
      const double pred = std::max(work / waves, std::max(sweep_chain, row_path));
      const bool mixed_late = 2.0 * row_units > waves && k < by_T.size();
      if (!mixed_late && pred < pbest * 0.999) {
        pbest = pred;
        best_k = k;
      }
      if (k < by_T.size()) {
        const double t = T[by_T[k]];
        work += row_k * t * t - (0.5 * t * t + t);
        row_work += row_k * t * t;
        row_units += t;
      }
    }
    for (size_t k = 0; k < best_k; ++k) as_rows[by_T[k]] = 1;
  }
  return as_rows;
}

// symmetric sweeps: one unit per (aggregate, row tile), in the order of their
// earliest start (2A tile-times into the aggregate), larger aggregates first
inline void unit_order(const Work& w, FamlSched& s, const std::vector<int>& T,
                       const std::vector<char>& as_rows) {
  const FamlSchedIn& in = w.in;
  const std::vector<int>& big = w.big;
  struct Unit { int a, A, pb, T, kind; double est; };
  std::vector<Unit> us;
  int pb = 0;
  // Queue position of sweep A of an aggregate of T row tiles: 2A Tmax / T, i.e.
  // every aggregate's sweeps spread over the whole queue, so all aggregates reach
  // their last (chain-bound) sweeps together and the launch ends without a tail of
  // the largest aggregate's chain (C4: tail after the queue drained 8.7 -> 3.5 ms,
  // 148.1 -> 143.2 ms per launch; 2A alone, the sweep's earliest start, was the
  // round-2 order).  Every sweep comes after the sweeps it waits on (sweep A - 1
  // before A).
  const double est_k = 2.0;
  const int Tmax = big.empty() ? 1 : *std::max_element(T.begin(), T.end());
  // Big aggregates a little ahead: positions also scaled by 1 - g T / Tmax (g = 0.3),
  // so the largest chains finish before the queue's end and the small aggregates'
  // short chains fill it (C4, one box, 3 rounds interleaved: 136.2-136.4 against
  // 136.9-137.3 ms per step; g = 0.15 136.5-136.7, 0.5 and 0.7 slower;
  // profiles/r04/ab_big_first.log).  Positions stay increasing in A for g < 1, so
  // every unit still waits only on units before it.
  const double big_first = 0.3;
  auto scale_of = [&](int Tb) {
    return ((double)Tmax / Tb) * (1.0 - big_first * Tb / Tmax);
  };
  // row blocks' issue priority: one level per quarter of the longest row block's
  // column tiles (ge_sym.hpp rows_prio; one level per sixth or eighth: no different,
  // profiles/r05/scale_sim_c4_prio_divisor.log)
  int rows_q = 0;
  const int prio_div = 4;
  for (size_t b = 0; b < big.size(); ++b)
    if (as_rows[b]) rows_q = std::max(rows_q, T[b]);
  for (int a : *in.split) rows_q = std::max(rows_q, w.ntiles_of(a));
  rows_q = (rows_q + prio_div - 1) / prio_div;
  for (size_t b = 0; b < big.size(); ++b) {
    if (as_rows[b]) {
      // row blocks have no dependencies and each spans its aggregate's whole width:
      // first in the queue, longest first (measured on per-rank shares of C4: N = 4
      // 69 ms per iteration against 80 ms when spread among the sweeps).  Round 5
      // tried cutting the last-taken blocks into a head and a tail segment
      // (McNaughton's wrap-around, so the queue's last round is short): bit-exact,
      // no faster (N = 8 shares 26.6-28.0 against 27.0-27.3 ms per launch,
      // profiles/r05/scale_sim_c4_tailsplit.log) -- the share is bound by the row
      // blocks' instruction stream, not by the queue's last round.
      for (int A = 0; A < T[b]; ++A) us.push_back({big[b], A, rows_q, T[b], kSchedRows, -1.0});
      continue;
    }
    const double sc = scale_of(T[b]);
    // (round 6 measured sweep issue priorities by the followers a sweep holds up:
    // 115.8-116.0 against 115.3-115.4 ms per launch, profiles/r06/ab_sym_prio.log)
    for (int A = 0; A < T[b]; ++A) us.push_back({big[b], A, pb, T[b], kSchedSweep, est_k * A * sc});
    pb += T[b];
  }
  for (int a : *in.split) {  // this rank's row tiles of the split aggregates: row blocks
    const Tiles t = w.tiles_of(a, in.rank);
    const int Ta = w.ntiles_of(a);
    for (int A = t.t0; A < t.t1; ++A) us.push_back({a, A, rows_q, Ta, kSchedRows, -1.0});
  }
  std::stable_sort(us.begin(), us.end(), [](const Unit& x, const Unit& y) {
    return x.est != y.est ? x.est < y.est : x.T > y.T;
  });
  for (const Unit& x : us) s.units.push_back({x.a, x.A, x.pb, x.kind});
  s.ntiles = pb;
}

}  // namespace sched

inline FamlSched faml_schedule(const FamlSchedIn& in) {
  sched::Work w{in, {}};
  FamlSched s;
  s.wide = in.wide;
  sched::classes_and_packs(w, s);
  sched::owned_rows(w, s);
  sched::strict_items(w, s);
  sched::fast_items(w, s);
  s.sym = in.knobs.sym && !in.wide && !s.fast && s.faraggs.empty();
  if (s.sym && !s.huge.empty()) {
    std::vector<int> T(w.big.size());
    for (size_t b = 0; b < w.big.size(); ++b) T[b] = w.ntiles_of(w.big[b]);
    // three blocks (waves) per SIMD of the four that fit: fewer units in flight spin
    // less on hand-overs (C4 N = 1: 137.2 against 138.3 ms per launch; N = 8 shares
    // 30.0 against 32.7 ms; scripts/sym_timeline.py, profiles/r03/sym_timeline)
    const int bpc = std::min(std::max(in.sym_occ, 1), 3);
    s.sym_blocks = in.cus * bpc;
    const std::vector<char> as_rows = sched::sweeps_or_rows(w, s, T);
    for (size_t b = 0; b < w.big.size(); ++b) {
      if (as_rows[b]) ++s.rows_mode;
      else ++s.swept;
    }
    sched::unit_order(w, s, T, as_rows);
  }
  return s;
}

}  // namespace ge
