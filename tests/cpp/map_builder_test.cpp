// slam_amd::GlobalMapBuilder (include/slam_amd/map_builder.hpp) on a sequence of clouds from plain binary files:
//   map_builder_test DIR N MAX_SCORE_FROM MAX_SCORE
// reads DIR/cloud_<i>.f32 (x y z per point), i = 0 .. N - 1, and calls addCloud on each; from cloud MAX_SCORE_FROM on,
// MAX_SCORE is set to the fourth argument.  One line per cloud on stdout (accepted, whether a request was made, iterations,
// state, pairs, the fitness and the sixteen floats of trans_full in hexadecimal), then the map: DIR/map.xyz4, DIR/map.count
// and DIR/map.key as slam_vmap_read gives them.  tests/test_gpu_map_builder_adapter.py compares all of it with
// slam_amd.api.GlobalMapBuilder bit for bit.
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
    const int         n_clouds = std::atoi(argv[2]), score_from = std::atoi(argv[3]);
    const double      max_score = std::atof(argv[4]);

    slam_amd::GlobalMapBuilder b;
    if (!b.ok()) return 3;
    for (int i = 0; i < n_clouds; ++i) {
        const std::vector<float> cloud = read_all(dir + "/cloud_" + std::to_string(i) + ".f32");
        if (i >= score_from) b.MAX_SCORE = max_score;
        const bool accepted = b.addCloud(cloud.data(), (int)(cloud.size() / 3), 3);
        const slam_kf_gicp_result &r = b.last;
        std::printf("cloud %d %d %d %d %d %a", (int)accepted, (int)b.last_valid, b.last_valid ? r.edge.iterations : 0, b.last_valid ? r.edge.state : 0,
                    b.last_valid ? r.fitness_pairs : 0, b.last_valid ? r.fitness : 0.0);
        for (int k = 0; k < 16; ++k) std::printf(" %a", (double)b.pose()[k]);
        std::printf("\n");
    }
    int64_t n_voxels = 0, n_points = 0;
    if (slam_vmap_info(b.vmap(), &n_voxels, nullptr, &n_points, nullptr) != SLAM_OK) return 4;
    std::vector<float>    xyz4(4 * (size_t)n_voxels);
    std::vector<uint32_t> count((size_t)n_voxels);
    std::vector<uint64_t> key((size_t)n_voxels);
    int                   n = 0;
    if (slam_vmap_read(b.vmap(), nullptr, nullptr, 0, xyz4.data(), count.data(), key.data(), (int)n_voxels, &n) != SLAM_OK || n != (int)n_voxels) return 4;
    if (b.map() != xyz4) return 5; // map() is the same extraction
    write_all(dir + "/map.xyz4", xyz4.data(), xyz4.size() * sizeof(float));
    write_all(dir + "/map.count", count.data(), count.size() * sizeof(uint32_t));
    write_all(dir + "/map.key", key.data(), key.size() * sizeof(uint64_t));
    // ids issued: the map keyframe and one per cloud after the first that reached the store; only the map's still answers
    int live = 0;
    for (int id = 0; id < slam_kf_count(b.store()); ++id) live += slam_kf_keyframe_info(b.store(), id, nullptr, nullptr, nullptr, nullptr, nullptr) == SLAM_OK;
    std::printf("store %d %d %d %lld %lld\n", slam_kf_count(b.store()), live, b.mapKeyframe(), (long long)n_voxels, (long long)n_points);
    return 0;
}
