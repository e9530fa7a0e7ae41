// slam_amd::GlobalMapBuilder with `carve` on (include/slam_amd/map_builder.hpp, docs/VOXEL_MAP.md section 8) on a sequence of
// clouds from plain binary files:
//   map_builder_carve_test DIR N
// reads DIR/cloud_<i>.f32 (x y z per point), i = 0 .. N - 1, and calls addCloud on each.  One line per cloud on stdout
// (accepted, whether a request was made, iterations, state, pairs, the fitness and the sixteen floats of trans_full in
// hexadecimal, then the six counters of the cloud's carve), then DIR/map.key, DIR/map.seen and DIR/map.miss as
// slam_vmap_read_carve gives them and DIR/map.carved, the builder's map().  tests/test_gpu_map_builder_carve.py compares all
// of it with slam_amd.api.GlobalMapBuilder(carve=True) bit for bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/map_builder.hpp"

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

static void write_all(const std::string &path, const void *p, size_t bytes)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int         n_clouds = std::atoi(argv[2]);

    slam_amd::GlobalMapBuilder b(0.30, 2.0, true);
    if (!b.ok() || !b.carve) return 3;
    for (int i = 0; i < n_clouds; ++i) {
        const std::vector<float> cloud = read_all(dir + "/cloud_" + std::to_string(i) + ".f32");
        const bool               accepted = b.addCloud(cloud.data(), (int)(cloud.size() / 3), 3);
        const slam_kf_gicp_result &r = b.last;
        std::printf("cloud %d %d %d %d %d %a", (int)accepted, (int)b.last_valid, b.last_valid ? r.edge.iterations : 0, b.last_valid ? r.edge.state : 0,
                    b.last_valid ? r.fitness_pairs : 0, b.last_valid ? r.fitness : 0.0);
        for (int k = 0; k < 16; ++k) std::printf(" %a", (double)b.pose()[k]);
        const slam_vmap_carve_result &c = b.last_carve;
        std::printf(" %lld %lld %lld %lld %lld %lld\n", (long long)c.n_rays, (long long)c.n_dropped, (long long)c.n_skipped, (long long)c.n_steps,
                    (long long)c.n_seen, (long long)c.n_missed);
    }
    int64_t n_voxels = 0, n_points = 0;
    if (slam_vmap_info(b.vmap(), &n_voxels, nullptr, &n_points, nullptr) != SLAM_OK) return 4;
    std::vector<uint32_t> seen((size_t)n_voxels), miss((size_t)n_voxels);
    std::vector<uint64_t> key((size_t)n_voxels);
    int                   n = 0;
    if (slam_vmap_read_carve(b.vmap(), seen.data(), miss.data(), key.data(), (int)n_voxels, &n) != SLAM_OK || n != (int)n_voxels) return 4;
    const std::vector<float> carved = b.map();
    write_all(dir + "/map.key", key.data(), key.size() * sizeof(uint64_t));
    write_all(dir + "/map.seen", seen.data(), seen.size() * sizeof(uint32_t));
    write_all(dir + "/map.miss", miss.data(), miss.size() * sizeof(uint32_t));
    write_all(dir + "/map.carved", carved.data(), carved.size() * sizeof(float));
    std::printf("map %lld %lld %lld\n", (long long)n_voxels, (long long)n_points, (long long)(carved.size() / 4));
    return 0;
}
