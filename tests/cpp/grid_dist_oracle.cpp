// grid_dist_oracle.cpp -- the distance field of docs/GRID_DIST.md as a scalar two-pass restatement in C++, one thread: the CPU
// pass a consumer of the occupancy plane runs today, for tools/grid_dist_time.py to time beside the device (and to hold the
// device's plane to at sizes the numpy restatement is too slow for).
//   grid_dist_oracle <occ.i8> <size_x> <size_y> <R> <unknown_is_obstacle> <dist2.u16 out> [reps]
// prints one line: the milliseconds of each repetition (the two passes only, no file traffic).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static void distance_field(const int8_t *occ, int sx, int sy, int R, int unknown_is_obstacle, uint8_t *g, uint16_t *dist2)
{
    // rows: the distance to the nearest obstacle of the row, capped at R + 1, by a sweep from each side
    for (int y = 0; y < sy; ++y) {
        const int8_t *o = occ + (size_t)sx * y;
        uint8_t      *r = g + (size_t)sx * y;
        int           d = R + 1;
        for (int x = 0; x < sx; ++x) {
            d = (o[x] == 100 || (unknown_is_obstacle && o[x] == -1)) ? 0 : std::min(d + 1, R + 1);
            r[x] = (uint8_t)d;
        }
        d = R + 1;
        for (int x = sx - 1; x >= 0; --x) {
            d = (o[x] == 100 || (unknown_is_obstacle && o[x] == -1)) ? 0 : std::min(d + 1, R + 1);
            r[x] = (uint8_t)std::min<int>(r[x], d);
        }
    }
    // columns: min over dy of g(x, y + dy)^2 + dy^2, walking outwards until dy^2 >= best
    const unsigned far2 = (unsigned)(R * R + 1);
    for (int y = 0; y < sy; ++y)
        for (int x = 0; x < sx; ++x) {
            const unsigned g0 = g[(size_t)sx * y + x];
            unsigned       best = std::min(far2, g0 * g0);
            for (unsigned dy = 1; dy * dy < best; ++dy) {
                const int up = y - (int)dy, down = y + (int)dy;
                if (up >= 0) {
                    const unsigned a = g[(size_t)sx * up + x];
                    best = std::min(best, a * a + dy * dy);
                }
                if (down < sy) {
                    const unsigned b = g[(size_t)sx * down + x];
                    best = std::min(best, b * b + dy * dy);
                }
            }
            dist2[(size_t)sx * y + x] = best < far2 ? (uint16_t)best : (uint16_t)0xFFFF;
        }
}

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const int sx = std::atoi(argv[2]), sy = std::atoi(argv[3]), R = std::atoi(argv[4]), unk = std::atoi(argv[5]);
    const int reps = argc > 7 ? std::atoi(argv[7]) : 1;
    if (sx < 1 || sy < 1 || sx > 32767 || sy > 32767 || R < 1 || R > 254 || reps < 1) return 2;
    const size_t         cells = (size_t)sx * sy;
    std::vector<int8_t>  occ(cells);
    std::vector<uint8_t> g(cells);
    std::vector<uint16_t> dist2(cells);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(occ.data(), 1, cells, f) != cells) return 3;
    std::fclose(f);
    for (int k = 0; k < reps; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        distance_field(occ.data(), sx, sy, R, unk, g.data(), dist2.data());
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%s%.3f", k ? " " : "", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::printf("\n");
    f = std::fopen(argv[6], "wb");
    if (!f || std::fwrite(dist2.data(), sizeof(uint16_t), cells, f) != cells) return 4;
    return std::fclose(f) == 0 ? 0 : 4;
}
