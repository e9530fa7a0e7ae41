// grid_likelihood_table_check.cpp -- slam::grid_likelihood_table of slam_amd/csrc/grid_cost_table.hpp alone, at the edges of its
// arguments, for a run under the host sanitizers (tests/test_csm_plane_cases.py compiles this with -fsanitize=address,undefined).
// Every table is allocated at exactly the size the call is told, so a write past R * R + 2 bytes is a heap overflow the sanitizer
// reports, and a value that does not fit a byte is a float-cast overflow.  One line per case:
//   <name> ok <T[0]> <T[1]> <T[R*R]> <T[R*R+1]> <sum of all bytes>      or      <name> invalid <reason>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "grid_cost_table.hpp"

static int failures = 0;

static void run(const char *name, double res, double sigma, int R, int n, bool expect_ok)
{
    std::vector<uint8_t> t((size_t)(n > 0 ? n : 0), (uint8_t)0xAB);
    const char          *why = nullptr;
    const int            rc = slam::grid_likelihood_table(res, sigma, R, n > 0 ? t.data() : nullptr, n, &why);
    if (rc == 0) {
        unsigned long sum = 0;
        bool          monotone = true;
        for (size_t k = 0; k < t.size(); ++k) {
            sum += t[k];
            if (k > 0 && t[k] > t[k - 1]) monotone = false;
        }
        std::printf("%s ok %d %d %d %d %lu\n", name, t[0], t[1], t[(size_t)R * R], t[(size_t)R * R + 1], sum);
        if (!monotone || t[0] != 255 || t.back() != 0) {
            std::printf("%s BROKEN: not non-increasing from 255 to 0\n", name);
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
    const int    n1 = 1 * 1 + 2, n6 = 6 * 6 + 2, n254 = 254 * 254 + 2;
    run("R1", 0.1, 0.2, 1, n1, true);
    run("R6", 0.1, 0.2, 6, n6, true);
    run("R254", 0.05, 0.5, 254, n254, true);
    run("R254_wide", 0.05, 1e6, 254, n254, true);                       // every entry 255 but the last
    run("R254_narrow", 1e6, 0.05, 254, n254, true);                     // 255 at the obstacle, 0 everywhere else
    run("sqrt_huge", 1e154, 1e153, 254, n254, true);                    // the squares are finite, k times resolution^2 is not beyond k = 1
    // the squares themselves leave the double range: refused, whichever argument it is
    run("tiny_resolution", tiny, 0.2, 254, n254, false);
    run("tiny_sigma", 0.1, tiny, 254, n254, false);
    run("tiny_both", tiny, tiny, 1, n1, false);
    run("huge_resolution", huge, 0.2, 254, n254, false);
    run("huge_sigma", 0.1, huge, 254, n254, false);
    run("huge_both", huge, huge, 1, n1, false);
    run("n_one_short", 0.1, 0.2, 254, n254 - 1, false);
    run("n_one_long", 0.1, 0.2, 254, n254 + 1, false);
    run("R1_n_one_short", 0.1, 0.2, 1, n1 - 1, false);
    run("R1_n_one_long", 0.1, 0.2, 1, n1 + 1, false);
    run("n_zero", 0.1, 0.2, 254, 0, false);
    run("n_negative", 0.1, 0.2, 254, -5, false);
    run("R0", 0.1, 0.2, 0, 2, false);
    run("R255", 0.1, 0.2, 255, 255 * 255 + 2, false);
    run("R_negative", 0.1, 0.2, -3, 11, false);
    run("R_int_max", 0.1, 0.2, std::numeric_limits<int>::max(), 3, false);
    run("nan_resolution", nan, 0.2, 6, n6, false);
    run("nan_sigma", 0.1, nan, 6, n6, false);
    run("inf_resolution", inf, 0.2, 6, n6, false);
    run("inf_sigma", 0.1, inf, 6, n6, false);
    run("minus_inf_sigma", 0.1, -inf, 6, n6, false);
    run("negative_resolution", -0.1, 0.2, 6, n6, false);
    run("zero_resolution", 0.0, 0.2, 6, n6, false);
    run("negative_sigma", 0.1, -0.2, 6, n6, false);
    run("zero_sigma", 0.1, 0.0, 6, n6, false);
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
