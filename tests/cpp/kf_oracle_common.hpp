// kf_oracle_common.hpp -- what the keyframe store's two restatements share (kf_edge_oracle.cpp: point-to-point ICP and the
// LUM block; kf_gicp_oracle.cpp: Generalized ICP): the gated search, the move in float and the stop tests' margin.
// tests/kf_edge_oracle.py and tests/kf_gicp_oracle.py name this file as a dependency, so an edit here rebuilds both.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace {

// ---------------------------------------------------------------- the gated search
// A lattice of edge `cell` >= gate: the nearest neighbour within the gate of a query is in the 27 cells around it.
struct Index {
    std::vector<float>  p;   // x y z per point, filtered-cloud order
    std::vector<double> cov; // Generalized ICP's: six doubles per point, empty otherwise
    int                 n = 0;
    double              inv = 0;
    std::unordered_map<uint64_t, std::vector<int>> cells;
};

const int64_t kHalf = 1 << 20; // 21 bits per axis

inline int64_t coord(float v, double inv)
{
    double c = std::floor((double)v * inv);
    if (!(c >= -(double)kHalf)) c = -(double)kHalf; // also NaN
    if (c > (double)(kHalf - 1)) c = (double)(kHalf - 1);
    return (int64_t)c + kHalf;
}
inline uint64_t key_of(int64_t cx, int64_t cy, int64_t cz) { return ((uint64_t)cz << 42) | ((uint64_t)cy << 21) | (uint64_t)cx; }

// f32, in this order, no FMA: dx*dx + dy*dy + dz*dz
inline float dist2(const float *a, const float *b)
{
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the nearest point among the 27 cells (lowest index on an exact tie), -1 when they are empty
inline int nearest(const Index &ix, const float *q, float *d2)
{
    const int64_t c[3] = {coord(q[0], ix.inv), coord(q[1], ix.inv), coord(q[2], ix.inv)};
    int   best = -1;
    float bd = 0;
    for (int64_t z = c[2] - 1; z <= c[2] + 1; ++z)
        for (int64_t y = c[1] - 1; y <= c[1] + 1; ++y)
            for (int64_t x = c[0] - 1; x <= c[0] + 1; ++x) {
                if (x < 0 || y < 0 || z < 0 || x >= 2 * kHalf || y >= 2 * kHalf || z >= 2 * kHalf) continue;
                auto it = ix.cells.find(key_of(x, y, z));
                if (it == ix.cells.end()) continue;
                for (int j : it->second) {
                    const float d = dist2(q, &ix.p[3 * (size_t)j]);
                    if (best < 0 || d < bd || (d == bd && j < best)) best = j, bd = d;
                }
            }
    *d2 = bd;
    return best;
}

// pcl::transformPointCloud with a Matrix4f, in float, left to right: m00 x + m01 y + m02 z + m03
inline void move_f32(const float M[16], const float *p, float *o)
{
    for (int r = 0; r < 3; ++r) o[r] = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
}

// the smallest relative distance of any stop test from its threshold
struct Margin {
    double m = DBL_MAX;
    void   see(double lhs, double rhs)
    {
        const double d = std::fabs(lhs - rhs) / (rhs != 0 ? std::fabs(rhs) : 1.0);
        if (d < m) m = d;
    }
};

} // namespace
