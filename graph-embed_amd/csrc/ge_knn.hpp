// ge_knn.hpp -- the shape of the exact k-nearest-neighbour pass (include/ge.h, "layout
// neighbours") and the entry points shared by its device code (ge_knn.hip) and its host
// path (ge_knn.cpp).
#pragma once

#include <algorithm>

#include "ge_dims.hpp"
#include "ge_internal.hpp"

namespace ge {

// One query row per lane; partners stream through LDS tiles of kKnnTileJ records of W
// doubles (W = d up to 4, kMaxDim above); a lane's sorted list of k entries {s, j} lies
// beside the tile, 12 bytes an entry.  A workgroup keeps to half of gfx950's 160 KiB of
// LDS, so that two fit on a CU: its rows are the largest of 256, 128, 64 whose lists fit
// beside the tile.  k = 64 in the run-time-d form fills the half exactly at 64 rows.
constexpr int kKnnTileJ = 256;
constexpr int kKnnMaxRows = 256;
constexpr int kKnnMinRows = 64;
constexpr int kKnnEntryBytes = 12;
constexpr size_t kKnnLdsBudget = 80 * 1024;
constexpr int kKnnMaxSplit = 16;      // j splits at most
constexpr int kKnnTargetBlocks = 512;  // workgroups wanted before the j range stays whole

inline int knn_record_width(int d) { return d <= kNarrowMaxDim ? d : kMaxDim; }
inline size_t knn_lds_bytes(int rows, int k, int d) {
  return (size_t)kKnnTileJ * knn_record_width(d) * sizeof(double) +
         (size_t)rows * k * kKnnEntryBytes;
}
inline int knn_rows_per_wg(int k, int d) {
  int rows = kKnnMaxRows;
  while (rows > kKnnMinRows && knn_lds_bytes(rows, k, d) > kKnnLdsBudget) rows /= 2;
  return rows;
}
// The j splits of a call without GE_KNN_JSPLIT: enough for kKnnTargetBlocks workgroups,
// at most kKnnMaxSplit and at most one per partner tile.
inline int knn_jsplit(int n, int n_rows, int rows_per_wg) {
  const int blocks = std::max(1, (n_rows + rows_per_wg - 1) / rows_per_wg);
  const int want = (kKnnTargetBlocks + blocks - 1) / blocks;
  const int tiles = (n + kKnnTileJ - 1) / kKnnTileJ;
  return std::max(1, std::min({want, kKnnMaxSplit, tiles}));
}

// The insertions of the last device call, from the context's scratch (KnnScratch,
// declared in ge_internal.hpp for ge_ctx); complete once that call's work is.
long long knn_device_insertions(const KnnScratch* s);

// Both paths: neighbours of the n_rows query rows (rows == nullptr: row q is vertex q)
// into idx (n_rows * k) and dist2 (may be nullptr), on validated arguments.
// knn_device takes device pointers, enqueues on the context's stream and does not
// synchronise; an id outside [0, n) in d_rows reads nothing and gets no neighbours.
void knn_device(ge_ctx* ctx, int n, int dim, const double* d_x, int k, int n_rows,
                const int* d_rows, int* d_idx, double* d_dist2);
long long knn_host(int n, int dim, const double* x, int k, int n_rows, const int* rows, int* idx,
                   double* dist2);

}  // namespace ge
