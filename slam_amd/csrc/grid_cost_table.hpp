// grid_cost_table.hpp -- the inflation byte table of the occupancy grid's costmap (docs/GRID_DIST.md section 1): the only
// floating point of the distance field, and it stays on the host.  Plain C++: no HIP, no device, no library state, so that it
// can be compiled alone (tests/cpp/grid_cost_table_check.cpp runs it under the host sanitizers).  Below it the likelihood-field
// table of a grid matcher (docs/GRID_MATCH.md), under the same terms (tests/cpp/grid_likelihood_table_check.cpp).
//
// The curve is the one of ROS costmap_2d's inflation layer, restated from its definition: a table T of R*R + 2 bytes indexed by
// the squared distance in cells,
//   T[0]       = 254                                          the obstacle cell itself (LETHAL)
//   T[k]       = 253                                          sqrt(k) * resolution <= inscribed_radius (INSCRIBED)
//              = 0                                            sqrt(k) * resolution >  inflation_radius
//              = (uint8_t)(252 * exp(-cost_scaling * (d - inscribed_radius)))   between the two, truncated
//   T[R*R + 1] = 0                                            what a cell beyond R cells (SLAM_GDIST_FAR) reads
#pragma once
#include <cmath>
#include <cstdint>

namespace slam {

constexpr int kGdistMaxCells = 254; // R <= 254: the row distance, capped at R + 1, fits a byte and R * R stays below 0xFFFF

// 0 and the table written, or -1, nothing written and *why naming the refusal
inline int grid_inflation_table(double resolution, double inscribed_radius, double inflation_radius, double cost_scaling, int max_cells,
                                uint8_t *table, int n, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!table) return *why = "null table", -1;
    if (max_cells < 1 || max_cells > kGdistMaxCells) return *why = "max_cells must be 1..254", -1;
    const int R = max_cells, far = R * R + 1;
    if (n != far + 1) return *why = "the table has max_cells * max_cells + 2 entries", -1;
    if (!std::isfinite(resolution) || !std::isfinite(inscribed_radius) || !std::isfinite(inflation_radius) || !std::isfinite(cost_scaling))
        return *why = "non-finite argument", -1;
    if (!(resolution > 0.0)) return *why = "resolution must be positive", -1;
    if (inscribed_radius < 0.0 || inflation_radius < 0.0 || cost_scaling < 0.0) return *why = "negative argument", -1;
    if (inscribed_radius > inflation_radius) return *why = "inscribed_radius exceeds inflation_radius", -1;
    if (inflation_radius > (double)R * resolution)
        return *why = "inflation_radius exceeds max_cells * resolution: the distance cap would cut the inflation short", -1;
    table[0] = 254;
    for (int k = 1; k < far; ++k) {
        const double d = std::sqrt((double)k) * resolution;
        uint8_t      c;
        if (d <= inscribed_radius)
            c = 253;
        else if (d > inflation_radius)
            c = 0;
        else
            c = (uint8_t)(252.0 * std::exp(-cost_scaling * (d - inscribed_radius))); // in [0, 252]: d > inscribed_radius here
        table[k] = c;
    }
    table[far] = 0;
    return 0;
}

// The likelihood-field table of a grid matcher (docs/GRID_MATCH.md section 2): the correlative matcher's Gaussian stamp
// (csm.hip, create_common) indexed by the squared distance in cells, so that entry i*i + j*j is stamp entry (i, j):
//   T[k]       = (uint8_t)rint(255 * exp(-(k * resolution^2) / (2 * sigma^2)))      k = 0 .. R*R
//   T[R*R + 1] = 0                                                                   what a cell beyond R cells reads
// Same answers as above.  resolution^2 and 2 sigma^2 must themselves be positive and finite doubles: where a square
// underflows to 0 or overflows, the quotient has no value.
inline int grid_likelihood_table(double resolution, double sigma, int max_cells, uint8_t *table, int n, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!table) return *why = "null table", -1;
    if (max_cells < 1 || max_cells > kGdistMaxCells) return *why = "max_cells must be 1..254", -1;
    const int R = max_cells, far = R * R + 1;
    if (n != far + 1) return *why = "the table has max_cells * max_cells + 2 entries", -1;
    if (!std::isfinite(resolution) || !std::isfinite(sigma)) return *why = "non-finite argument", -1;
    if (!(resolution > 0.0)) return *why = "resolution must be positive", -1;
    if (!(sigma > 0.0)) return *why = "sigma must be positive", -1;
    const double r2 = resolution * resolution, s2 = 2.0 * (sigma * sigma);
    if (!(r2 > 0.0) || !std::isfinite(r2) || !(s2 > 0.0) || !std::isfinite(s2))
        return *why = "resolution squared or sigma squared leaves the range of a double", -1;
    for (int k = 0; k < far; ++k) table[k] = (uint8_t)std::rint(255.0 * std::exp(-((double)k * r2) / s2)); // in [0, 255]
    table[far] = 0;
    return 0;
}

} // namespace slam
