// grid_clip_check.cpp -- the clip of one beam to one tile (slam_amd/csrc/grid_clip.hpp) alone, as a program of its own (no HIP, no
// library): tests/test_grid_clip.py builds it with the host compiler and runs it.  Every beam is walked with the plain integer
// Bresenham of oracle/slam_oracle.c (ogrid_raycast); for every tile the walk crosses, and for every neighbour of those that it
// misses, the clip must say what the walk did:
//   - the steps whose cell lies in the tile are one contiguous range,
//   - that range is exactly [i_lo, i_lo + rem) (i_lo = du - to_end),
//   - the cell and the error term at i_lo are the walk's, and stepping on from there as the kernel does (e += dv2, a wrap adds
//     step_v) gives the walk's cell at every step of the range,
//   - to_end is right: to_end < rem exactly where the end cell lies in the tile.
// Exhaustive: every beam with both ends in a 24 x 24 window against 5 x 5-cell tiles (the last ones partial).  Sampled, at the
// limits of a 32767-cell grid with its 128-cell tiles: the longest beams there are, where __mul24(den, k_hi + 1) comes within
// 2e5 of 2^31 and the float quotient of floor_div_small sits at its stated error bound.  The device's reciprocal is good to one
// ulp, so every beam is clipped with the correctly rounded reciprocals, with both one float above and with both one float below.
// Prints "ok" and what it covered and returns 0, or names the checks that failed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "grid_clip.hpp"

using namespace slam;

static long failures = 0, clips = 0, beams = 0;
static long long largest_product = 0; // of den * (k_hi + 1), over everything clipped

#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            if (failures < 20) {                                      \
                std::printf("FAILED line %d: %s  ", __LINE__, #cond); \
                std::printf(__VA_ARGS__);                             \
                std::printf("\n");                                    \
            }                                                         \
            ++failures;                                               \
        }                                                             \
    } while (0)

struct Seen { // what the walk did in one tile
    int first, last, count;
};

static std::vector<int>  xs, ys, es;     // the walk: cell and error term of step i
static std::vector<Seen> seen;           // per tile
static std::vector<int>  touched, near_; // tiles the walk crossed; their neighbours that it missed

// ulp: -1, 0, +1 floats off the correctly rounded reciprocal
static float recip(int d, int ulp)
{
    if (d == 0) return 0.0f; // (not looked at)
    const float r = 1.0f / (float)d;
    return ulp > 0 ? std::nextafterf(r, 2.0f) : ulp < 0 ? std::nextafterf(r, 0.0f) : r;
}

static void check_beam(int x0, int y0, int x1, int y1, int T, int sx, int sy, int ulp)
{
    const int tiles_x = (sx + T - 1) / T, tiles_y = (sy + T - 1) / T, pitch = T + 1;
    if ((int)seen.size() < tiles_x * tiles_y) seen.assign((size_t)tiles_x * tiles_y, Seen{0, 0, 0});
    ++beams;
    // the walk of ogrid_raycast, its error term kept beside the cell
    const int  dx = std::abs(x1 - x0), dy = std::abs(y1 - y0), stx = x1 > x0 ? 1 : -1, sty = y1 > y0 ? 1 : -1;
    const bool xm = dx >= dy;
    const int  du = xm ? dx : dy, dv = xm ? dy : dx;
    xs.resize(du + 1), ys.resize(du + 1), es.resize(du + 1);
    touched.clear();
    int x = x0, y = y0, e = du;
    for (int i = 0; i <= du; ++i) {
        xs[i] = x, ys[i] = y, es[i] = e;
        const int t = (y / T) * tiles_x + x / T;
        Seen     &s = seen[t];
        if (s.count == 0) s.first = i, touched.push_back(t);
        s.last = i, ++s.count;
        if (i == du) break;
        e += 2 * dv;
        const bool minor = e >= 2 * du;
        if (minor) e -= 2 * du;
        if (xm) x += stx, y += minor ? sty : 0;
        else    y += sty, x += minor ? stx : 0;
    }
    CHECK(x == x1 && y == y1, "walk (%d,%d)->(%d,%d) ended at (%d,%d)", x0, y0, x1, y1, x, y);

    const int   den = clip_den(x0, y0, x1, y1), dv2 = clip_dv2(x0, y0, x1, y1);
    const float rden = recip(den, ulp), rdv2 = recip(dv2, ulp);
    CHECK(den == (du ? 2 * du : 1) && dv2 == 2 * dv, "den %d dv2 %d", den, dv2);
    const auto tile_box = [&](int t, int *tx0, int *ty0, int *tx1, int *ty1) {
        *tx0 = (t % tiles_x) * T, *ty0 = (t / tiles_x) * T;
        *tx1 = clip_min(*tx0 + T, sx) - 1, *ty1 = clip_min(*ty0 + T, sy) - 1;
    };
    near_.clear();
    for (const int t : touched) {
        int tx0, ty0, tx1, ty1;
        tile_box(t, &tx0, &ty0, &tx1, &ty1);
        const Seen s = seen[t];
        {   // (what the clip multiplies: the issue's 65532 * 32767)
            const bool vp = (xm ? y1 > y0 : x1 > x0);
            const int  v0 = xm ? y0 : x0, tv0 = xm ? ty0 : tx0, tv1 = xm ? ty1 : tx1;
            const int  k_hi = clip_min(vp ? tv1 - v0 : v0 - tv0, dv);
            if (dv > 0 && (long long)den * (k_hi + 1) > largest_product) largest_product = (long long)den * (k_hi + 1);
        }
        const bool     live = clip_box_meets_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1);
        const TileClip c = clip_beam_to_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1, pitch, rden, rdv2, live);
        ++clips;
#define WHERE "beam (%d,%d)->(%d,%d) tile [%d..%d]x[%d..%d] ulp %d", x0, y0, x1, y1, tx0, tx1, ty0, ty1, ulp
        CHECK(live, WHERE);
        CHECK(s.count == s.last - s.first + 1, WHERE);                  // one contiguous range
        CHECK(c.rem == s.count && du - c.to_end == s.first, WHERE);     // and it is [i_lo, i_lo + rem)
        CHECK((c.to_end < c.rem) == (s.last == du), WHERE);             // the end cell's hit is added here or not
        CHECK(c.den == den && c.dv2 == dv2, WHERE);
        if (c.rem == s.count && du - c.to_end == s.first) {
            int  a = c.a, err = c.e;
            bool same = true;
            for (int i = s.first; i <= s.last; ++i) { // the kernel's walk from there (grid_raycast.hpp: advance)
                same = same && a == (ys[i] - ty0) * pitch + (xs[i] - tx0) && err == es[i];
                err += c.dv2;
                const bool carry = err >= c.den;
                a += c.step_u + (carry ? c.step_v : 0);
                err -= carry ? c.den : 0;
            }
            CHECK(same, WHERE);
        }
        for (int ny = -1; ny <= 1; ++ny)
            for (int nx = -1; nx <= 1; ++nx) {
                const int qx = t % tiles_x + nx, qy = t / tiles_x + ny;
                if (qx < 0 || qy < 0 || qx >= tiles_x || qy >= tiles_y || seen[qy * tiles_x + qx].count) continue;
                near_.push_back(qy * tiles_x + qx);
            }
    }
    for (const int t : near_) { // tiles the beam just misses: empty, whether the caller's box test says so or not
        int tx0, ty0, tx1, ty1;
        tile_box(t, &tx0, &ty0, &tx1, &ty1);
        const bool live = clip_box_meets_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1);
        CHECK(clip_beam_to_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1, pitch, rden, rdv2, live).rem == 0, WHERE);
        CHECK(clip_beam_to_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1, pitch, rden, rdv2, true).rem == 0, WHERE);
        CHECK(clip_beam_to_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1, pitch, rden, rdv2, false).rem == 0, WHERE);
        clips += 3;
    }
    for (const int t : touched) seen[t].count = 0;
}

int main()
{
    // the 24-bit product is the device's: low 32 bits of the signed 24-bit operands' product
    CHECK(clip_mul24(65532, 32767) == 2147287044 && clip_mul24(-3, 5) == -15 && clip_mul24(0x1000001, 7) == 7, "mul24");
    CHECK(clip_mul24(0x7fffff, 0x7fffff) == (int)(unsigned)(0x7fffffLL * 0x7fffffLL), "mul24 low word");

    // ---- exhaustive: 24 x 24 window, 5 x 5-cell tiles
    for (int ulp = -1; ulp <= 1; ++ulp)
        for (int a = 0; a < 24 * 24; ++a)
            for (int b = 0; b < 24 * 24; ++b) check_beam(a % 24, a / 24, b % 24, b / 24, 5, 24, 24, ulp);
    const long small_beams = beams, small_clips = clips;

    // ---- sampled, at the limits of a 32767 x 32767 grid with 128-cell tiles
    seen.clear();
    const int S = 32767, top = S - 1;
    const int dus[] = {32766, 32765, 23171, 23170, 16384};
    for (const int du : dus) {
        const int dvs[] = {0, 1, 2, du / 2 - 1, du / 2, du / 2 + 1, du - 1, du};
        for (const int dv : dvs)
            for (int su = -1; su <= 1; su += 2)
                for (int sv = -1; sv <= 1; sv += 2)
                    for (int high = 0; high <= 1; ++high)   // against the grid's low sides, or its high ones
                        for (int ymajor = 0; ymajor <= 1; ++ymajor)
                            for (int ulp = -1; ulp <= 1; ++ulp) {
                                const int ua = high ? top - du : 0, va = high ? top - dv : 0;
                                const int u0 = su > 0 ? ua : ua + du, u1 = su > 0 ? ua + du : ua;
                                const int v0 = sv > 0 ? va : va + dv, v1 = sv > 0 ? va + dv : va;
                                if (ymajor)
                                    check_beam(v0, u0, v1, u1, 128, S, S, ulp);
                                else
                                    check_beam(u0, v0, u1, v1, 128, S, S, ulp);
                            }
    }
    CHECK(largest_product == 65532LL * 32767LL, "largest den * (k_hi + 1) seen: %lld", largest_product);
    if (failures) {
        std::printf("%ld checks failed\n", failures);
        return 1;
    }
    std::printf("exhaustive: %ld beams, %ld clips; sampled: %ld beams, %ld clips; largest product %lld\nok\n", small_beams, small_clips,
                beams - small_beams, clips - small_clips, largest_product);
    return 0;
}
