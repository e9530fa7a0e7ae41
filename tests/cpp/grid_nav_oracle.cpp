// grid_nav_oracle.cpp -- the navigation field of docs/GRID_NAV.md as a scalar binary-heap Dijkstra in C++, one thread: the CPU
// pass a planner over the cost plane runs today, for tools/grid_nav_time.py to time beside the device (and to hold the device's
// field to at sizes the numpy restatement is too slow for).
//   grid_nav_oracle <cost.u8> <size_x> <size_y> <table.u32> <orth_w> <diag_w> <goals.i32> <pot.u32 out> [reps]
// prints one line: the milliseconds of each repetition (the search only, no file traffic).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

static const int kDx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, kDy[8] = {0, 1, 1, 1, 0, -1, -1, -1};

static void field(const uint8_t *cost, int sx, int sy, const uint32_t *S, uint64_t orth_w, uint64_t diag_w, const std::vector<int32_t> &goals,
                  std::vector<uint64_t> &dist, uint32_t *pot)
{
    const uint64_t inf = ~0ull;
    const size_t   cells = (size_t)sx * sy;
    dist.assign(cells, inf);
    typedef std::pair<uint64_t, uint32_t> Item; // (distance, cell)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (size_t i = 0; i + 1 < goals.size(); i += 2) {
        const int x = goals[i], y = goals[i + 1];
        if (x < 0 || y < 0 || x >= sx || y >= sy || S[cost[(size_t)y * sx + x]] == 0) continue;
        if (dist[(size_t)y * sx + x] != 0) heap.push(Item(0, (uint32_t)((size_t)y * sx + x)));
        dist[(size_t)y * sx + x] = 0;
    }
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        if (it.first != dist[it.second]) continue; // an entry a later, shorter one has replaced
        const int      x = (int)(it.second % (uint32_t)sx), y = (int)(it.second / (uint32_t)sx);
        const uint64_t su = S[cost[it.second]];
        for (int d = 0; d < 8; ++d) {
            const int vx = x + kDx[d], vy = y + kDy[d];
            if (vx < 0 || vy < 0 || vx >= sx || vy >= sy) continue;
            const size_t   v = (size_t)vy * sx + vx;
            const uint64_t sv = S[cost[v]];
            if (!sv) continue;
            const bool diagonal = kDx[d] != 0 && kDy[d] != 0;
            if (diagonal && (S[cost[(size_t)y * sx + vx]] == 0 || S[cost[(size_t)vy * sx + x]] == 0)) continue; // no corner cutting
            const uint64_t cand = it.first + (diagonal ? diag_w : orth_w) * (su + sv);
            if (cand < dist[v]) {
                dist[v] = cand;
                heap.push(Item(cand, (uint32_t)v));
            }
        }
    }
    for (size_t i = 0; i < cells; ++i) pot[i] = dist[i] < 0xFFFFFFFFull ? (uint32_t)dist[i] : 0xFFFFFFFFu; // clamped at the end
}

template <class T>
static bool load(const char *path, std::vector<T> &v, size_t n)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    if (n == 0) {
        std::fseek(f, 0, SEEK_END);
        n = (size_t)std::ftell(f) / sizeof(T);
        std::fseek(f, 0, SEEK_SET);
    }
    v.resize(n);
    const bool ok = std::fread(v.data(), sizeof(T), n, f) == n;
    std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    const int sx = std::atoi(argv[2]), sy = std::atoi(argv[3]), orth_w = std::atoi(argv[5]), diag_w = std::atoi(argv[6]);
    const int reps = argc > 9 ? std::atoi(argv[9]) : 1;
    if (sx < 1 || sy < 1 || sx > 32767 || sy > 32767 || orth_w < 1 || orth_w > 255 || diag_w < 1 || diag_w > 255 || reps < 1) return 2;
    const size_t          cells = (size_t)sx * sy;
    std::vector<uint8_t>  cost;
    std::vector<uint32_t> S, pot(cells);
    std::vector<int32_t>  goals;
    std::vector<uint64_t> dist;
    if (!load(argv[1], cost, cells) || !load(argv[4], S, 256) || !load(argv[7], goals, 0)) return 3;
    for (int k = 0; k < reps; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        field(cost.data(), sx, sy, S.data(), (uint64_t)orth_w, (uint64_t)diag_w, goals, dist, pot.data());
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%s%.3f", k ? " " : "", std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::printf("\n");
    FILE *f = std::fopen(argv[8], "wb");
    if (!f || std::fwrite(pot.data(), sizeof(uint32_t), cells, f) != cells) return 4;
    return std::fclose(f) == 0 ? 0 : 4;
}
