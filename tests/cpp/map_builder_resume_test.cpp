// slam_amd::GlobalMapBuilder's save and resume (include/slam_amd/map_builder.hpp, docs/VOXEL_MAP.md section 10.5) against the
// Python twin's:
//   map_builder_resume_test DIR CARVE DIRECT
// reads DIR/cloud_<i>.f32 (x y z per point), i = 0 .. 5.  One builder adds clouds 0 .. 2 and saves to DIR/cpp_half; a second
// one resumes from DIR/py_half (written by slam_amd.api.GlobalMapBuilder after the same three clouds), adds clouds 3 .. 5 and
// saves to DIR/cpp_full.  A resume on the builder that has added clouds, and one into a builder of another leaf, must be
// refused.  One line per step on stdout; tests/test_gpu_map_builder_resume.py compares the files byte for byte.
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

static bool add(slam_amd::GlobalMapBuilder &b, const std::string &dir, int i)
{
    const std::vector<float> cloud = read_all(dir + "/cloud_" + std::to_string(i) + ".f32");
    const bool               ok = b.addCloud(cloud.data(), (int)(cloud.size() / 3), 3);
    std::printf("cloud %d %d\n", i, (int)ok);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string dir = argv[1];
    const bool        carve = std::atoi(argv[2]) != 0, direct = std::atoi(argv[3]) != 0;
    {
        slam_amd::GlobalMapBuilder a(0.30, 2.0, carve, direct);
        if (!a.ok()) return 3;
        for (int i = 0; i < 3; ++i)
            if (!add(a, dir, i)) return 4;
        if (!a.save(dir + "/cpp_half")) return 5;
        if (a.resume(dir + "/py_half")) return 6; // it has added clouds
        std::printf("refused after clouds\n");
    }
    {
        slam_amd::GlobalMapBuilder other(0.25, 2.0, carve, direct);
        if (!other.ok()) return 3;
        if (other.resume(dir + "/py_half") || other.n_clouds != 0) return 7; // another leaf
        std::printf("refused another leaf\n");
    }
    slam_amd::GlobalMapBuilder b(0.30, 2.0, carve, direct);
    if (!b.ok()) return 3;
    if (!b.resume(dir + "/py_half")) return 8;
    std::printf("resumed %d %d\n", b.n_clouds, b.n_accepted);
    for (int i = 3; i < 6; ++i)
        if (!add(b, dir, i)) return 4;
    if (!b.save(dir + "/cpp_full")) return 9;
    std::printf("saved %d %d\n", b.n_clouds, b.n_accepted);
    return 0;
}
