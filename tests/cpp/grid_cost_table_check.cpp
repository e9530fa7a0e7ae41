// grid_cost_table_check.cpp -- slam_amd/csrc/grid_cost_table.hpp alone, at the edges of its arguments, for a run under the host
// sanitizers (tests/test_grid_dist_cases.py compiles this with -fsanitize=address,undefined).  Every table is allocated at exactly
// the size the call is told, so a write past R * R + 2 bytes is a heap overflow the sanitizer reports.  One line per case:
//   <name> ok <T[0]> <T[1]> <T[R*R]> <T[R*R+1]> <sum of all bytes>      or      <name> invalid <reason>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "grid_cost_table.hpp"

static int failures = 0;

static void run(const char *name, double res, double inscribed, double inflation, double scaling, int R, int n, bool expect_ok)
{
    std::vector<uint8_t> t((size_t)(n > 0 ? n : 0), (uint8_t)0xAB);
    const char          *why = nullptr;
    const int            rc = slam::grid_inflation_table(res, inscribed, inflation, scaling, R, n > 0 ? t.data() : nullptr, n, &why);
    if (rc == 0) {
        unsigned long sum = 0;
        bool          monotone = true;
        for (size_t k = 0; k < t.size(); ++k) {
            sum += t[k];
            if (k > 0 && t[k] > t[k - 1]) monotone = false;
        }
        std::printf("%s ok %d %d %d %d %lu\n", name, t[0], t[1], t[(size_t)R * R], t[(size_t)R * R + 1], sum);
        if (!monotone || t[0] != 254 || t.back() != 0) {
            std::printf("%s BROKEN: not non-increasing from 254 to 0\n", name);
            ++failures;
        }
    } else {
        std::printf("%s invalid %s\n", name, why);
        for (uint8_t b : t)
            if (b != 0xAB) { // a refused call writes nothing
                std::printf("%s BROKEN: a refused call wrote the table\n", name);
                ++failures;
                break;
            }
        if (!why || !std::strlen(why)) ++failures;
    }
    if ((rc == 0) != expect_ok) {
        std::printf("%s BROKEN: expected %s\n", name, expect_ok ? "ok" : "invalid");
        ++failures;
    }
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tiny = std::numeric_limits<double>::denorm_min(), huge = std::numeric_limits<double>::max();
    const int    n1 = 1 * 1 + 2, n254 = 254 * 254 + 2;
    run("R1", 0.05, 0.02, 0.05, 3.0, 1, n1, true);
    run("R254", 0.05, 0.3, 12.7, 3.0, 254, n254, true);
    run("R254_zero_radii", 0.05, 0.0, 0.0, 0.0, 254, n254, true);
    run("R254_scaling_huge", 0.05, 0.3, 12.0, huge, 254, n254, true);
    run("R254_scaling_zero", 0.05, 0.3, 12.0, 0.0, 254, n254, true);
    run("tiny_resolution", tiny, 0.0, 0.0, 3.0, 254, n254, true);
    run("tiny_resolution_radii", tiny, tiny, 200 * tiny, huge, 254, n254, true);
    run("huge_resolution", huge, 1.0, huge, 3.0, 254, n254, true);      // sqrt(k) * resolution overflows to infinity beyond k = 1
    run("huge_everything", huge, huge, huge, huge, 1, n1, true);
    run("n_one_short", 0.05, 0.3, 1.0, 3.0, 254, n254 - 1, false);
    run("n_one_long", 0.05, 0.3, 1.0, 3.0, 254, n254 + 1, false);
    run("R1_n_one_short", 0.05, 0.01, 0.05, 3.0, 1, n1 - 1, false);
    run("R1_n_one_long", 0.05, 0.01, 0.05, 3.0, 1, n1 + 1, false);
    run("n_zero", 0.05, 0.3, 1.0, 3.0, 254, 0, false);
    run("n_negative", 0.05, 0.3, 1.0, 3.0, 254, -5, false);
    run("R0", 0.05, 0.0, 0.0, 3.0, 0, 2, false);
    run("R255", 0.05, 0.3, 1.0, 3.0, 255, 255 * 255 + 2, false);
    run("R_negative", 0.05, 0.3, 1.0, 3.0, -3, 11, false);
    run("R_int_max", 0.05, 0.3, 1.0, 3.0, std::numeric_limits<int>::max(), 3, false);
    run("nan_resolution", nan, 0.3, 1.0, 3.0, 32, 32 * 32 + 2, false);
    run("nan_inscribed", 0.05, nan, 1.0, 3.0, 32, 32 * 32 + 2, false);
    run("nan_inflation", 0.05, 0.3, nan, 3.0, 32, 32 * 32 + 2, false);
    run("nan_scaling", 0.05, 0.3, 1.0, nan, 32, 32 * 32 + 2, false);
    run("inf_resolution", inf, 0.3, 1.0, 3.0, 32, 32 * 32 + 2, false);
    run("inf_inflation", 0.05, 0.3, inf, 3.0, 32, 32 * 32 + 2, false);
    run("negative_resolution", -0.05, 0.3, 1.0, 3.0, 32, 32 * 32 + 2, false);
    run("zero_resolution", 0.0, 0.0, 0.0, 3.0, 32, 32 * 32 + 2, false);
    run("negative_inscribed", 0.05, -0.3, 1.0, 3.0, 32, 32 * 32 + 2, false);
    run("negative_scaling", 0.05, 0.3, 1.0, -3.0, 32, 32 * 32 + 2, false);
    run("inscribed_beyond_inflation", 0.05, 1.1, 1.0, 3.0, 32, 32 * 32 + 2, false);
    run("inflation_beyond_cap", 0.05, 0.3, 1.6001, 3.0, 32, 32 * 32 + 2, false);
    run("inflation_at_cap", 0.05, 0.3, 32 * 0.05, 3.0, 32, 32 * 32 + 2, true);
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
