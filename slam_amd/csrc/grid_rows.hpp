// grid_rows.hpp -- the occupancy grid's row ranges (grid.hip): which storage rows of the count planes hold counts, and which
// are due at the next finalize.  The transitions are plain functions on a value, host and device alike, so that they can be
// compiled alone (tests/cpp/grid_rows_check.cpp walks them); the one-thread kernels of grid.hip are wrappers around them.
//
// A range {lo, -hi} of storage rows, empty while lo > hi (both words kNoRow).  Counts are nonzero only in rows of the touched
// range (every update marks its rows; a merge over the GPUs marks the rows it summed: slam_grid_mark_rows), so a reset zeroes
// those rows only -- and remembers them as changed, because their evidence and occupancy are stale until the next finalize,
// which covers the touched and the changed rows and nothing else.  At 2000 x 2000 with a 40 x 30 m room the ranges are 30 % of
// the rows: reset 7 -> 2 us, finalize 12 -> 4 us per step.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define SLAM_ROWS_FN __host__ __device__ inline
#else
#define SLAM_ROWS_FN inline
#endif

namespace slam {

// "no row", in a register and in memory alike: slam_grid_clear sets the words with a memset of 0x7f bytes.  Above every row
// (a grid has at most 32767) and above every negated row, so a minimum with it is the other operand.
constexpr int kNoRow = 0x7f7f7f7f;

struct RowRanges {
    int touched_lo, touched_nhi; // rows touched since the counts were last reset (or folded): lowest, minus the highest
    int changed_lo, changed_nhi; // rows whose counts changed since the last finalize by something other than an update (a reset)
};
// slam_grid_dirty_rows_dev hands out a pointer to the touched pair as two int32 (slam_mi355x_rccl.h reads {lowest, -highest})
static_assert(sizeof(RowRanges) == 4 * sizeof(int) && offsetof(RowRanges, touched_lo) == 0 && offsetof(RowRanges, touched_nhi) == sizeof(int),
              "the touched pair is the first two words");

SLAM_ROWS_FN int rows_min(int a, int b) { return a < b ? a : b; }
SLAM_ROWS_FN int rows_max(int a, int b) { return a > b ? a : b; }

SLAM_ROWS_FN RowRanges rows_empty() { return {kNoRow, kNoRow, kNoRow, kNoRow}; }

// rows lo..hi were written (an update; from outside, a merge of those rows): they count as touched
SLAM_ROWS_FN RowRanges rows_mark(RowRanges r, int lo, int hi)
{
    return {rows_min(r.touched_lo, lo), rows_min(r.touched_nhi, -hi), r.changed_lo, r.changed_nhi};
}
// the touched rows become changed rows (hull), the touched range starts again
SLAM_ROWS_FN RowRanges rows_retire(RowRanges r)
{
    return {kNoRow, kNoRow, rows_min(r.changed_lo, r.touched_lo), rows_min(r.changed_nhi, r.touched_nhi)};
}
// slam_grid_fold of rows lo..hi: they and the touched rows are due for the next finalize; the touched range starts again
// if the fold covered it (rows it did not cover still hold counts: they stay touched)
SLAM_ROWS_FN RowRanges rows_fold(RowRanges r, int lo, int hi)
{
    const bool covered = r.touched_lo >= lo && -r.touched_nhi <= hi;
    return {covered ? kNoRow : r.touched_lo, covered ? kNoRow : r.touched_nhi, rows_min(rows_min(r.changed_lo, r.touched_lo), lo),
            rows_min(rows_min(r.changed_nhi, r.touched_nhi), -hi)};
}
// nothing changed any more (after a finalize)
SLAM_ROWS_FN RowRanges rows_finalized(RowRanges r) { return {r.touched_lo, r.touched_nhi, kNoRow, kNoRow}; }
// everything did (a roll, a merge of whole planes, a new threshold)
SLAM_ROWS_FN RowRanges rows_all_changed(RowRanges r, int sy) { return {r.touched_lo, r.touched_nhi, 0, -(sy - 1)}; }

// what a finalize covers: the hull of the touched and the changed rows, inside the grid (none: *hi < *lo)
SLAM_ROWS_FN void rows_due(const RowRanges &r, int sy, int *lo, int *hi)
{
    *lo = rows_max(rows_min(r.touched_lo, r.changed_lo), 0);
    *hi = rows_min(rows_max(-r.touched_nhi, -r.changed_nhi), sy - 1);
}
// what a reset covers: the touched rows, inside the grid (none: *hi < *lo)
SLAM_ROWS_FN void rows_touched(const RowRanges &r, int sy, int *lo, int *hi)
{
    *lo = rows_max(r.touched_lo, 0);
    *hi = rows_min(-r.touched_nhi, sy - 1);
}
// what slam_grid_dirty_rows reports: the touched rows, 0 and -1 for none
SLAM_ROWS_FN void rows_reported(const RowRanges &r, int *lo, int *hi)
{
    const bool none = r.touched_lo > -r.touched_nhi;
    *lo = none ? 0 : r.touched_lo;
    *hi = none ? -1 : -r.touched_nhi;
}

#ifdef __HIPCC__
// Widens the touched range by {lo, nhi} with the pair of atomics only where they would change it: thousands of wavefronts
// hitting one word cost 11 ns each (the lesson of the update counter, grid_view.hpp), so the caller looks first -- a stale look
// only costs a superfluous atomic, the atomic itself is what counts.  For ONE lane of whoever has reduced its rows.
__device__ inline void rows_widen_touched(RowRanges *r, int lo, int nhi)
{
    if (lo < __hip_atomic_load(&r->touched_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&r->touched_lo, lo);
    if (nhi < __hip_atomic_load(&r->touched_nhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&r->touched_nhi, nhi);
}

// Rows of the planes (storage order) that hold counts: a merge over the GPUs moves only these (slam_mi355x_rccl.h).  Wave
// minimum of every lane's {lo, -hi}, then rows_widen_touched by the first lane.  Every lane of the wavefront calls it.
__device__ inline void mark_dirty_rows(RowRanges *r, int row_lo, int row_hi /* -1: none */)
{
    int lo = row_hi >= 0 ? row_lo : kNoRow, nhi = row_hi >= 0 ? -row_hi : kNoRow;
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        nhi = min(nhi, __shfl_xor(nhi, off));
    }
    if ((threadIdx.x & 63) == 0 && lo != kNoRow) rows_widen_touched(r, lo, nhi);
}
#endif

} // namespace slam
