// ge_far.hpp -- the far-field repulsion engine of GE_MODE_FARFIELD (ge_far.hip),
// as the single-level plan (ge_fa.hip) sees it.
#pragma once

#include <hip/hip_runtime.h>

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

}  // namespace ge
