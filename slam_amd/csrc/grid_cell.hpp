// grid_cell.hpp -- the binning of one point into a map cell (mls.cpp:77-90 and :371-381), shared by the
// occupancy grid (grid.hip) and the height-cluster map (mls.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace slam {

// (int)(v/res + size/2) of mls.cpp:77-78; false when an int cannot hold it
// (undefined in the reference; x86 gives INT_MIN there, i.e. "skip").
__device__ inline bool cell_coord(float v, double res, int half, int *out)
{
    const double f = __dadd_rn(__ddiv_rn((double)v, res), (double)half);
    if (!(f > -2147483648.0 && f < 2147483648.0)) return false;
    *out = (int)f; // truncation toward zero
    return true;
}

// mls.cpp:77-90: window cell of a point, or false when the range gate or the
// bounds test (with its `y >= size_x` quirk) drops it.  Also false for
// y >= size_y, where the reference would write out of bounds.
__device__ inline bool point_cell_of(int sx, int sy, double res, double max_range, double pose_x, double pose_y, int rolling,
                                     float px, float py, int *cx, int *cy)
{
    int x, y;
    if (!cell_coord(px, res, sx / 2, &x)) return false;
    if (!cell_coord(py, res, sy / 2, &y)) return false;
    double rng;
    if (rolling) {
        // mls.cpp:82: float expression, float sqrt, widened for the compare
        rng = (double)__fsqrt_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)));
    } else {
        const double rx = pose_x - (double)px, ry = pose_y - (double)py; // :84-86
        rng = __dsqrt_rn(__dadd_rn(__dmul_rn(rx, rx), __dmul_rn(ry, ry)));
    }
    if (x < 0 || y < 0 || x >= sx || y >= sx || rng > max_range) return false; // :90
    if (y >= sy) return false;
    *cx = x;
    *cy = y;
    return true;
}

} // namespace slam
