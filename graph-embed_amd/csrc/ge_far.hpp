// ge_far.hpp -- the far-field repulsion engines of GE_MODE_FARFIELD (ge_far.hip), as
// the single-level plan (ge_fa.hip) and the multilevel plan (ge_faml.hip) see them.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "ge_internal.hpp"

namespace ge {

constexpr int kFarLeaf = 64;   // sorted records per leaf
constexpr int kFarGroup = 16;  // cells per parent (G)
constexpr int kFarMaxLevels = GE_FAR_MAX_LEVELS;

struct FarEngine;

// Every buffer of the engine (nothing is allocated per pass).  item_rows: 64 R, R = 1 or 4.
FarEngine* far_create(hipStream_t s, int n, int dim, double theta, int item_rows, int cus);
void far_destroy(FarEngine* e);
// true when every dp1[j] > 0 (synchronises)
bool far_masses_ok(hipStream_t s, int n, const double* dp1);
// One repulsion pass: Frep (n * dim) at the original rows.  Synchronises once, after
// the bounding box; returns false, with nothing written, when the box is not finite.
bool far_repulse(FarEngine* e, hipStream_t s, const double* X, const double* dp1, double repel,
                 double* Frep);
// ge_fa_plan_far_info / ge_fa_plan_far_layout (include/ge.h)
void far_info(FarEngine* e, hipStream_t s, double* theta, int* item_rows, int* levels,
              int* level_cells, long long* level_points, int* fallback, long long* accepted,
              long long* exact_leaves, long long* pair_terms, double* prep_ms, double* item_ms);
void far_layout(FarEngine* e, hipStream_t s, int* perm, unsigned long long* keys, double* box,
                double* cells, double* items);

// ---- the segmented engine: one hierarchy per streamed aggregate of a multilevel level.
// Segment f holds the members at P_T positions [base[f], base[f] + size[f]); the
// segments are given larger first and are worked in that order.  One composite sort
// per pass: the segment's rank sits above the Morton bits, so the key has
// far_seg_key_bits(dim) bits per axis whatever the plan holds (kFarSegRankBits for the
// rank: a streamed aggregate has more than 256 members and a level fewer than 2^31).
constexpr int kFarSegRankBits = 23;
constexpr int far_seg_key_bits(int dim) { return (64 - kFarSegRankBits) / dim; }

struct FarSegEngine;

FarSegEngine* far_seg_create(hipStream_t s, int dim, double theta, int item_rows, int cus,
                             const std::vector<int>& base, const std::vector<int>& size);
void far_seg_destroy(FarSegEngine* e);
// true when dp[rows[q]] is finite and > 0 for every q (synchronises)
bool far_masses_ok_rows(hipStream_t s, int nrows, const int* rows, const double* dp);
// One pass over every segment on stream s, no host synchronisation: X and DP by P_T
// position, Frep written at the segments' P_T positions only.  A segment whose
// coordinates are not all finite gets all-zero keys and rejects every cell: its rows
// are one lane's chain over its members in P_T order, faml_fast_repulse's bits.
void far_seg_repulse(FarSegEngine* e, hipStream_t s, const double* X, const double* DP,
                     double repel, double* Frep);
bool far_seg_ran(const FarSegEngine* e);
// ge_faml_plan_far_info / ge_faml_plan_far_layout (include/ge.h); both synchronise
void far_seg_info(FarSegEngine* e, hipStream_t s, double* theta, int* item_rows, int* key_bits,
                  int* segments, long long* rows, int* bad_boxes, long long* accepted,
                  long long* exact_leaves, long long* pair_terms, double* prep_ms,
                  double* item_ms);
// sizes of segment f's layout: members, levels, cells per level (leaves first), items
void far_seg_shape(const FarSegEngine* e, int f, int* members, int* levels, int* level_cells,
                   int* items);
void far_seg_layout(FarSegEngine* e, hipStream_t s, int f, int* perm, unsigned long long* keys,
                    double* box, double* cells, double* items);

}  // namespace ge
