// slam_amd::MapLocalizer::search and relocalize (include/slam_amd/global_match.hpp, docs/VOXEL_MAP.md section 13.4) on a saved
// map and a scan from plain binary files:
//   map_relocalize_test DIR LEVELS CX CY CZ RADIUS
// loads DIR/map.vmap, reads DIR/scan.f32 (x y z per point) and relocalises around (CX, CY, CZ) within RADIUS (the four as C
// hexadecimal floats), twice.  On stdout: one line per hit (score, k, dx, dy, dz, n_with_cell, the sixteen floats of init), one
// line per (level, hit) that ran, and the verdict, as map_localizer_test prints them, everything that is a number in
// hexadecimal.  tests/test_gpu_map_relocalize.py compares all of it with slam_amd.api.MapLocalizer.relocalize bit for bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/global_match.hpp"

static std::vector<float> read_all(const std::string &path)
{
    std::vector<float> v;
    FILE              *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(float));
    if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) std::exit(2);
    std::fclose(f);
    return v;
}

static void print_all(slam_amd::MapLocalizer &loc, const slam_amd::MapLocalizerResult &out, int levels)
{
    for (size_t h = 0; h < loc.hits.size(); ++h) {
        const slam_vmap_search_hit &s = loc.hits[h];
        std::printf("hit %d %d %d %d %d %d %d", (int)h, s.score, s.k, s.dx, s.dy, s.dz, s.n_with_cell);
        for (int c = 0; c < 16; ++c) std::printf(" %a", (double)s.init[c]);
        std::printf("\n");
    }
    for (int k = levels - 1; k >= 0; --k)
        for (size_t i = 0; i < loc.ran[(size_t)k].size(); ++i) {
            if (!loc.ran[(size_t)k][i]) continue;
            const slam_vmap_gicp_result &r = loc.last[(size_t)k][i];
            std::printf("result %d %d %d %d %d %d %d %a", k, (int)i, r.iterations, r.state, r.converged, r.pairs, r.fitness_pairs, r.fitness);
            for (int c = 0; c < 16; ++c) std::printf(" %a", (double)r.transform[c]);
            for (int c = 0; c < 16; ++c) std::printf(" %a", r.transform64[c]);
            std::printf("\n");
        }
    std::printf("verdict %d %d %d %a %a %a", (int)out.found, out.index, out.n_source, out.x, out.y, out.theta);
    for (int c = 0; c < 16; ++c) std::printf(" %a", (double)out.transform[c]);
    for (int c = 0; c < 16; ++c) std::printf(" %a", out.transform64[c]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const std::string dir = argv[1];
    const int         levels = std::atoi(argv[2]);
    const float       cx = (float)std::strtod(argv[3], nullptr), cy = (float)std::strtod(argv[4], nullptr), cz = (float)std::strtod(argv[5], nullptr);
    const double      radius = std::strtod(argv[6], nullptr);

    slam_amd::MapLocalizer loc(levels);
    if (!loc.ok()) return 3;
    slam_amd::MapLocalizerResult out;
    const std::vector<float>     scan = read_all(dir + "/scan.f32");
    const int                    n = (int)(scan.size() / 3);
    if (loc.relocalize(scan.data(), n, 3, cx, cy, cz, radius, &out)) return 4; // no map yet: refused
    if (!loc.load((dir + "/map.vmap").c_str())) return 5;
    for (int round = 0; round < 2; ++round) { // twice: the same bits
        if (!loc.relocalize(scan.data(), n, 3, cx, cy, cz, radius, &out)) return 6;
        std::printf("round %d\n", round);
        print_all(loc, out, levels);
    }
    // a window that sees nothing of the map: no hit, not found, and no error
    if (!loc.relocalize(scan.data(), n, 3, cx + 5000.0f, cy + 5000.0f, cz, 4.0, &out) || out.found || !loc.hits.empty()) return 7;
    // the scan keyframes are gone: a removed id is refused by every call that names it
    int n_points = 0;
    for (int id = 0; id < slam_kf_count(loc.store()); ++id)
        if (slam_kf_keyframe_info(loc.store(), id, &n_points, 0, 0, 0, 0) == SLAM_OK) return 8;
    std::printf("keyframes %d issued, none live\n", slam_kf_count(loc.store()));
    return 0;
}
