// slam_amd::GlobalMapBuilder with `direct` on (include/slam_amd/map_builder.hpp, docs/VOXEL_MAP.md section 9) on a sequence of
// clouds from plain binary files:
//   map_builder_direct_test DIR N TIGHT_FROM TIGHT_SCORE
// reads DIR/cloud_<i>.f32 (x y z per point), i = 0 .. N - 1, and calls addCloud on each; from cloud TIGHT_FROM on MAX_SCORE is
// TIGHT_SCORE.  One line per cloud on stdout (accepted, whether a request was made, iterations, state, pairs, fitness pairs,
// the fitness and the sixteen floats of trans_full in hexadecimal), then DIR/map.xyz4 (the builder's map()) and, of the
// DIST_LEAF map, DIR/dist.key, DIR/dist.E, DIR/dist.M and DIR/dist.flag.  tests/test_gpu_map_builder_direct.py compares all of
// it with slam_amd.api.GlobalMapBuilder(direct=True) bit for bit.
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
    if (argc < 5) return 2;
    const std::string dir = argv[1];
    const int         n_clouds = std::atoi(argv[2]), tight_from = std::atoi(argv[3]);
    const double      tight = std::atof(argv[4]);

    slam_amd::GlobalMapBuilder b(0.30, 2.0, false, true);
    if (!b.ok() || !b.direct || !b.distMap()) return 3;
    for (int i = 0; i < n_clouds; ++i) {
        if (i >= tight_from) b.MAX_SCORE = tight;
        const std::vector<float>     cloud = read_all(dir + "/cloud_" + std::to_string(i) + ".f32");
        const bool                   accepted = b.addCloud(cloud.data(), (int)(cloud.size() / 3), 3);
        const slam_vmap_gicp_result &r = b.last_direct;
        const bool                   v = b.last_valid;
        std::printf("cloud %d %d %d %d %d %d %a", (int)accepted, (int)v, v ? r.iterations : 0, v ? r.state : 0, v ? r.pairs : 0, v ? r.fitness_pairs : 0,
                    v ? r.fitness : 0.0);
        for (int k = 0; k < 16; ++k) std::printf(" %a", (double)b.pose()[k]);
        std::printf("\n");
    }
    if (b.mapKeyframe() != -1) return 5; // no map keyframe in direct mode
    const std::vector<float> map = b.map();
    write_all(dir + "/map.xyz4", map.data(), map.size() * sizeof(float));
    int64_t n_voxels = 0, n_points = 0;
    if (slam_vmap_info(b.distMap(), &n_voxels, nullptr, &n_points, nullptr) != SLAM_OK) return 4;
    std::vector<int64_t>  E(3 * (size_t)n_voxels), M(6 * (size_t)n_voxels);
    std::vector<uint64_t> key((size_t)n_voxels);
    std::vector<uint8_t>  flag((size_t)n_voxels);
    int                   n = 0;
    if (slam_vmap_read_moments(b.distMap(), E.data(), M.data(), key.data(), (int)n_voxels, &n) != SLAM_OK || n != (int)n_voxels) return 4;
    if (slam_vmap_read_distributions(b.distMap(), nullptr, nullptr, nullptr, nullptr, flag.data(), nullptr, (int)n_voxels, &n) != SLAM_OK) return 4;
    write_all(dir + "/dist.key", key.data(), key.size() * sizeof(uint64_t));
    write_all(dir + "/dist.E", E.data(), E.size() * sizeof(int64_t));
    write_all(dir + "/dist.M", M.data(), M.size() * sizeof(int64_t));
    write_all(dir + "/dist.flag", flag.data(), flag.size());
    std::printf("map %lld %lld %lld %d\n", (long long)(map.size() / 4), (long long)n_voxels, (long long)n_points, slam_kf_count(b.store()));
    return 0;
}
