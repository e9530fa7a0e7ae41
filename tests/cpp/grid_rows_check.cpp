// grid_rows_check.cpp -- the plain functions of slam_amd/csrc/grid_rows.hpp alone, as a program of its own (no HIP, no library):
// tests/test_grid_rows.py builds it with the host compiler and runs it.  A RowRanges value is walked through every transition of
// the occupancy grid's touched / changed rows, each state compared with the four words written out here.  Prints "ok" and returns
// 0, or names the check that failed.
#include <cstdio>
#include <cstring>

#include "grid_rows.hpp"

using namespace slam;

static int failures = 0;

#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static bool is(const RowRanges &r, int t_lo, int t_nhi, int c_lo, int c_nhi)
{
    return r.touched_lo == t_lo && r.touched_nhi == t_nhi && r.changed_lo == c_lo && r.changed_nhi == c_nhi;
}

// {lo, hi} of one of the three readers; none is hi < lo
struct Span {
    int lo, hi;
};
static Span due(const RowRanges &r, int sy)
{
    Span s;
    rows_due(r, sy, &s.lo, &s.hi);
    return s;
}
static Span touched(const RowRanges &r, int sy)
{
    Span s;
    rows_touched(r, sy, &s.lo, &s.hi);
    return s;
}
static Span reported(const RowRanges &r)
{
    Span s;
    rows_reported(r, &s.lo, &s.hi);
    return s;
}

int main()
{
    const int N = 0x7f7f7f7f, sy = 48;
    CHECK(kNoRow == N);
    // the sentinel is what a memset of its low byte leaves, in every word
    RowRanges m;
    std::memset(&m, kNoRow & 0xff, sizeof m);
    CHECK(is(m, N, N, N, N));

    RowRanges r = rows_empty();
    CHECK(is(r, N, N, N, N));
    CHECK(reported(r).lo == 0 && reported(r).hi == -1);
    CHECK(due(r, sy).hi < due(r, sy).lo && touched(r, sy).hi < touched(r, sy).lo);

    r = rows_mark(r, 5, 9);
    CHECK(is(r, 5, -9, N, N));
    CHECK(reported(r).lo == 5 && reported(r).hi == 9);
    r = rows_mark(r, 2, 3); // the hull
    CHECK(is(r, 2, -9, N, N));
    CHECK(touched(r, sy).lo == 2 && touched(r, sy).hi == 9 && due(r, sy).lo == 2 && due(r, sy).hi == 9);

    r = rows_retire(r); // touched becomes changed
    CHECK(is(r, N, N, 2, -9));
    CHECK(reported(r).lo == 0 && reported(r).hi == -1);
    CHECK(touched(r, sy).hi < touched(r, sy).lo && due(r, sy).lo == 2 && due(r, sy).hi == 9);

    r = rows_mark(r, 20, 21);
    CHECK(is(r, 20, -21, 2, -9));
    CHECK(due(r, sy).lo == 2 && due(r, sy).hi == 21);
    r = rows_fold(r, 20, 21); // covered: touched is empty again
    CHECK(is(r, N, N, 2, -21));

    r = rows_mark(r, 4, 30);
    CHECK(is(r, 4, -30, 2, -21));
    r = rows_fold(r, 10, 12); // not covered: touched stays, changed takes the fold and the touched rows
    CHECK(is(r, 4, -30, 2, -30));
    CHECK(reported(r).lo == 4 && reported(r).hi == 30);

    r = rows_all_changed(r, sy);
    CHECK(is(r, 4, -30, 0, -47));
    CHECK(due(r, sy).lo == 0 && due(r, sy).hi == 47);
    r = rows_finalized(r);
    CHECK(is(r, 4, -30, N, N));
    CHECK(due(r, sy).lo == 4 && due(r, sy).hi == 30);

    // what finalize_reset leaves in the other buffer: finalized, then retired
    CHECK(is(rows_retire(rows_finalized(r)), N, N, 4, -30));
    // a retire of nothing touched keeps what was changed
    CHECK(is(rows_retire(rows_retire(r)), N, N, 4, -30));

    // a range that reaches sy is clamped to the grid by both readers, and reported as it stands
    const RowRanges over = rows_mark(rows_empty(), 40, 48);
    CHECK(is(over, 40, -48, N, N));
    CHECK(touched(over, sy).lo == 40 && touched(over, sy).hi == 47 && due(over, sy).lo == 40 && due(over, sy).hi == 47);
    CHECK(reported(over).lo == 40 && reported(over).hi == 48);

    CHECK(reported(rows_empty()).lo == 0 && reported(rows_empty()).hi == -1);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
