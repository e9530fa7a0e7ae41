// grid_nav_table.hpp -- the step table of the navigation field (docs/GRID_NAV.md section 1): S[256] uint32, indexed by a cost
// byte; 0 closes the cell, otherwise 1 <= S[c] <= 2^20.  Plain C++: no HIP, no device, no library state, so that it can be
// compiled alone (tests/cpp/grid_nav_table_check.cpp runs it under the host sanitizers).  The maker answers 0 with the table
// written, or -1 with nothing written and *why naming the refusal.
#pragma once
#include <cstdint>

namespace slam {

constexpr int      kGnavTableLen = 256;
constexpr uint32_t kGnavMaxStep = 1u << 20;  // of a table entry
constexpr int      kGnavMaxNeutral = 1 << 19; // neutral + 252 stays below 2^20
constexpr int      kGnavMaxWeight = 255;      // orth_w, diag_w: a move is at most 255 * 2^21 < 2^29

// S[c] = neutral + c for c < lethal_from, 0 from there on; S[255] = unknown_step (0 keeps unknown cells closed)
inline int grid_step_table(int neutral, int lethal_from, int unknown_step, uint32_t *table, int n, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!table) return *why = "null table", -1;
    if (n != kGnavTableLen) return *why = "the table has 256 entries", -1;
    if (neutral < 1 || neutral > kGnavMaxNeutral) return *why = "neutral must be 1..2^19", -1;
    if (lethal_from < 1 || lethal_from > 256) return *why = "lethal_from must be 1..256", -1;
    if (unknown_step < 0 || (uint32_t)unknown_step > kGnavMaxStep) return *why = "unknown_step must be 0..2^20", -1;
    for (int c = 0; c < kGnavTableLen; ++c) table[c] = c < lethal_from ? (uint32_t)neutral + (uint32_t)c : 0u;
    table[255] = (uint32_t)unknown_step;
    return 0;
}

// what slam_gnav_set_table asks of a table given from outside
inline bool grid_step_table_ok(const uint32_t *table, int n)
{
    if (!table || n != kGnavTableLen) return false;
    for (int c = 0; c < n; ++c)
        if (table[c] > kGnavMaxStep) return false;
    return true;
}

} // namespace slam
