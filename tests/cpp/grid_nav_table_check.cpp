// grid_nav_table_check.cpp -- slam_amd/csrc/grid_nav_table.hpp alone, as a program of its own: tests/test_grid_nav_cases.py builds
// it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  Every table is allocated at exactly 256 entries, so a
// write past either end is the sanitizer's to find; every refusal must leave its table untouched.  Prints "ok" and returns 0, or names the check that failed.
#include <cstdio>
#include <limits>
#include <memory>

#include "grid_nav_table.hpp"

static int failures = 0;

#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static bool untouched(const uint32_t *p, int n)
{
    for (int i = 0; i < n; ++i)
        if (p[i] != 7u) return false;
    return true;
}

static std::unique_ptr<uint32_t[]> marked(int n)
{
    std::unique_ptr<uint32_t[]> t(new uint32_t[n > 0 ? n : 1]);
    for (int i = 0; i < n; ++i) t[i] = 7u;
    return t;
}

int main()
{
    const int   imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    const char *why = nullptr;
    // ---- the formula at the defaults and at every edge of the ranges
    for (int neutral : {1, 50, 1 << 19})
        for (int lethal_from : {1, 2, 253, 255, 256})
            for (int unknown_step : {0, 1, 400, 1 << 20}) {
                auto t = marked(256);
                CHECK(slam::grid_step_table(neutral, lethal_from, unknown_step, t.get(), 256, &why) == 0 && why[0] == 0);
                for (int c = 0; c < 255; ++c) CHECK(t[c] == (c < lethal_from ? (uint32_t)neutral + (uint32_t)c : 0u));
                CHECK(t[255] == (uint32_t)unknown_step);
                CHECK(slam::grid_step_table_ok(t.get(), 256));
            }
    // ---- every refusal, the table allocated at 256 entries and left as it was
    for (int neutral : {0, -1, (1 << 19) + 1, imax, imin}) {
        auto t = marked(256);
        CHECK(slam::grid_step_table(neutral, 253, 0, t.get(), 256, &why) == -1 && why[0] != 0 && untouched(t.get(), 256));
    }
    for (int lethal_from : {0, -1, 257, imax, imin}) {
        auto t = marked(256);
        CHECK(slam::grid_step_table(50, lethal_from, 0, t.get(), 256, &why) == -1 && why[0] != 0 && untouched(t.get(), 256));
    }
    for (int unknown_step : {-1, (1 << 20) + 1, imax, imin}) {
        auto t = marked(256);
        CHECK(slam::grid_step_table(50, 253, unknown_step, t.get(), 256, &why) == -1 && why[0] != 0 && untouched(t.get(), 256));
    }
    for (int n : {255, 257, 0, 1, -256, imax, imin}) { // a wrong length claimed for a table of 256
        auto t = marked(256);
        CHECK(slam::grid_step_table(50, 253, 0, t.get(), n, &why) == -1 && why[0] != 0 && untouched(t.get(), 256));
    }
    CHECK(slam::grid_step_table(50, 253, 0, nullptr, 256, &why) == -1 && slam::grid_step_table(50, 253, 0, nullptr, 256, nullptr) == -1);
    {
        auto t = marked(256);
        CHECK(slam::grid_step_table(50, 253, 0, t.get(), 256, nullptr) == 0 && t[0] == 50u && t[252] == 302u && t[253] == 0u && t[255] == 0u);
    }
    // ---- a table from outside
    {
        auto t = marked(256);
        CHECK(slam::grid_step_table_ok(t.get(), 256) && !slam::grid_step_table_ok(t.get(), 255) && !slam::grid_step_table_ok(nullptr, 256));
        t[255] = (1u << 20) + 1u;
        CHECK(!slam::grid_step_table_ok(t.get(), 256));
        t[255] = 1u << 20;
        t[0] = 0u;
        CHECK(slam::grid_step_table_ok(t.get(), 256));
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
