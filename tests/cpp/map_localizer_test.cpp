// slam_amd::MapLocalizer (include/slam_amd/global_match.hpp, docs/VOXEL_MAP.md section 11.3) on a saved map and a scan from
// plain binary files:
//   map_localizer_test DIR LEVELS X Y YAW N
// loads DIR/map.vmap, reads DIR/scan.f32 (x y z per point), draws yawFan(X, Y, YAW, N) (the three as C hexadecimal floats) and
// localises.  On stdout: one line per start of the fan (its sixteen floats), one line per (level, start) that ran (iterations,
// state, converged, pairs, fitness pairs, fitness, the f32 and the f64 transform), and the verdict, everything that is a
// number in hexadecimal.  tests/test_gpu_map_localizer.py compares all of it with slam_amd.api.MapLocalizer bit for bit.
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

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const std::string dir = argv[1];
    const int         levels = std::atoi(argv[2]), n = std::atoi(argv[6]);
    const float       x = (float)std::strtod(argv[3], nullptr), y = (float)std::strtod(argv[4], nullptr), yaw = (float)std::strtod(argv[5], nullptr);

    slam_amd::MapLocalizer loc(levels);
    if (!loc.ok()) return 3;
    slam_amd::MapLocalizerResult out;
    const std::vector<float>     scan = read_all(dir + "/scan.f32");
    const std::vector<float>     starts = slam_amd::MapLocalizer::yawFan(x, y, yaw, n);
    if (loc.localize(scan.data(), (int)(scan.size() / 3), 3, starts, &out)) return 4; // no map yet: refused
    if (loc.load((dir + "/absent.vmap").c_str())) return 4;
    if (!loc.load((dir + "/map.vmap").c_str())) return 5;
    for (int i = 0; i < n; ++i) {
        std::printf("start %d", i);
        for (int k = 0; k < 16; ++k) std::printf(" %a", (double)starts[16 * (size_t)i + k]);
        std::printf("\n");
    }
    if (!loc.localize(scan.data(), (int)(scan.size() / 3), 3, starts, &out)) return 6;
    for (int k = levels - 1; k >= 0; --k)
        for (int i = 0; i < n; ++i) {
            if (!loc.ran[(size_t)k][(size_t)i]) continue;
            const slam_vmap_gicp_result &r = loc.last[(size_t)k][(size_t)i];
            std::printf("result %d %d %d %d %d %d %d %a", k, i, r.iterations, r.state, r.converged, r.pairs, r.fitness_pairs, r.fitness);
            for (int c = 0; c < 16; ++c) std::printf(" %a", (double)r.transform[c]);
            for (int c = 0; c < 16; ++c) std::printf(" %a", r.transform64[c]);
            std::printf("\n");
        }
    std::printf("verdict %d %d %d %a %a %a", (int)out.found, out.index, out.n_source, out.x, out.y, out.theta);
    for (int c = 0; c < 16; ++c) std::printf(" %a", (double)out.transform[c]);
    for (int c = 0; c < 16; ++c) std::printf(" %a", out.transform64[c]);
    std::printf("\n");
    // the scan keyframes are gone: a removed id is refused by every call that names it
    int n_points = 0;
    for (int id = 0; id < slam_kf_count(loc.store()); ++id)
        if (slam_kf_keyframe_info(loc.store(), id, &n_points, 0, 0, 0, 0) == SLAM_OK) return 7;
    std::printf("keyframes %d issued, none live\n", slam_kf_count(loc.store()));
    return 0;
}
