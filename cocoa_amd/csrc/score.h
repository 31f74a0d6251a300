// Scoring kernels (cocoa_score*): decision values f_r = sum_q val[q] * w[col[q]]
// of caller rows.  Columns and w are in ORIGINAL feature order; the pointers
// need only their natural alignment (int32 / double / int64), every entry
// offset is 64-bit.  score_strict.hip is built with -ffp-contract=off,
// score_fast.hip with -ffp-contract=fast.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cocoa {

// entries per workgroup tile of the fast sparse kernel
constexpr int kScoreTile = 2048;
inline int64_t score_tiles(int64_t nnz) { return nnz <= 0 ? 1 : (nnz + kScoreTile - 1) / kScoreTile; }

// strict: one thread per row, product then add in stored order (bitwise equal
// to the oracle's sp_dot and to a host loop compiled without contraction)
void launch_score_strict(const int64_t* row_ptr, const int32_t* col, const double* val, const double* w, int64_t n,
                         double* out, hipStream_t s);
void launch_score_strict_dense(const double* X, const double* w, int64_t n, int32_t d, double* out, hipStream_t s);

// fast sparse: entry tiles found on the device from row_ptr (binary search),
// one plain store per out[r], no atomics.  head / tail: double[score_tiles(nnz)]
// each, tail_row: int64[score_tiles(nnz)] (per-tile partials of the rows that
// cross a tile boundary, summed in tile order by a second kernel).
void launch_score_fast(const int64_t* row_ptr, const int32_t* col, const double* val, const double* w, int64_t n,
                       int64_t nnz, double* out, double* head, double* tail, int64_t* tail_row, hipStream_t s);
// fast dense: row-major X[n][d], any d >= 1
void launch_score_fast_dense(const double* X, const double* w, int64_t n, int32_t d, double* out, hipStream_t s);

// w_orig[j] = w_dev[perm[j]]: the context's device-order w in original order
void launch_score_gather_w(const double* w_dev, const int32_t* perm, int32_t d, double* w_orig, hipStream_t s);

}  // namespace cocoa
