// grid_view.hpp -- what every kernel of the occupancy grid is handed (grid.hip and its raycast, grid_raycast.hpp): the
// window, its planes in toroidal storage order, and the two counters every update reports to.
#pragma once
#include <cstdint>

#include "grid_cell.hpp"
#include "grid_rows.hpp"

using namespace slam;

namespace {

struct GridView {
    int      sx, sy;       // window size in cells
    int      ox, oy;       // toroidal origin (Grid::origin_x/y, mls.h:69-70)
    double   res;
    double   max_range;
    double   pose_x, pose_y;
    int      rolling;
    int32_t *hits;         // [sx*sy] storage order
    int32_t *misses;       // [sx*sy] storage order
    unsigned long long *updates;
    RowRanges *dirty;      // storage rows touched / changed (grid_rows.hpp); the buffer in use: slam_grid::other_ranges
    const int32_t *acc_hits, *acc_misses; // nullable: counts folded away by slam_grid_fold (merged totals)
};

__device__ inline int storage_index(const GridView &g, int x, int y)
{
    int ix = x + g.ox, iy = y + g.oy; // mls.h:76-85
    if (ix >= g.sx) ix -= g.sx;
    if (iy >= g.sy) iy -= g.sy;
    return ix + g.sx * iy;
}

// mls.cpp:77-90: window cell of a point, or false when the range gate or the
// bounds test (with its `y >= size_x` quirk) drops it (grid_cell.hpp).
__device__ inline bool point_cell(const GridView &g, float px, float py, int *cx, int *cy)
{
    return point_cell_of(g.sx, g.sy, g.res, g.max_range, g.pose_x, g.pose_y, g.rolling, px, py, cx, cy);
}

constexpr int kUpdateSlots = 1024;

// Counter of cell updates: wave reduction, then one atomic per wavefront into
// one of kUpdateSlots slots (same-address device atomics retire at ~11 ns each,
// so thousands of wavefronts must not share one word); the reader sums the slots.
__device__ inline void block_add_updates(unsigned long long *slots, unsigned n)
{
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor((int)n, off);
    if ((threadIdx.x & 63) == 0 && n) {
        const unsigned wave = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) + blockIdx.y * 7919u;
        atomicAdd(&slots[wave & (kUpdateSlots - 1)], (unsigned long long)n);
    }
}

} // namespace
