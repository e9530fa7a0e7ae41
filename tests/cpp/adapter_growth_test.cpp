// Growth in the middle of a sequence changes nothing: every adapter that grows device or pinned blocks (MLS, MLSMap, CCICP,
// GlobalMapBuilder) is run twice over the same two clouds, a small one and then one several times as large.
//   object A  gets the two clouds and nothing else: every block it sizes by a cloud grows between the two calls;
//   object B  is first given a cloud larger than both and then emptied (clearMap, a fresh target, a scan the builder rejects),
//             so none of its blocks grows after that.
//   adapter_growth_test <dir> <out>
// reads <dir>/{small,big,huge,base}.f32 (x y z per point; base: the CCICP target and the builder's first cloud) and writes what
// A and B report to <out>.<adapter>.A and <out>.<adapter>.B; tests/test_gpu_adapter_growth.py compares the pairs byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "slam_amd/ccicp.hpp"
#include "slam_amd/map_builder.hpp"
#include "slam_amd/mls.hpp"
#include "slam_amd/mls_map.hpp"

using slam_amd::Pose;
typedef std::vector<float> Cloud;

static Cloud read_all(const std::string &path)
{
    Cloud v;
    FILE *f = std::fopen(path.c_str(), "rb");
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

struct Blob { // what one object reports, appended field by field
    std::vector<unsigned char> bytes;
    void add(const void *p, size_t n) { bytes.insert(bytes.end(), (const unsigned char *)p, (const unsigned char *)p + n); }
    template <class T>
    void add(const std::vector<T> &v)
    {
        const uint64_t n = v.size();
        add(&n, sizeof n);
        add(v.data(), v.size() * sizeof(T));
    }
    void write(const std::string &path) const
    {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f || (bytes.size() && std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size())) {
            std::perror(path.c_str());
            std::exit(2);
        }
        std::fclose(f);
    }
};

static int npts(const Cloud &c) { return (int)(c.size() / 3); }

static Pose pose_of(int k) // the poses the two clouds are added with (yaw about z)
{
    Pose         p;
    const double yaw = 0.02 * k;
    p.x = 0.13 * k, p.y = -0.21 * k, p.qz = std::sin(0.5 * yaw), p.qw = std::cos(0.5 * yaw);
    return p;
}

// local_mapper's calls (local_mapper.cpp:107-120) behind every cloud: add_cloud's four blocks, the pinned block and the filter's two
static Blob run_mls(const Cloud &small, const Cloud &big, const Cloud *huge)
{
    slam_amd::MLS m(100, 100, 0.2, true);
    m.setMinClusterPoints(5);
    m.clearMap();
    if (huge) {
        m.addToMap(huge->data(), npts(*huge), 3, pose_of(1)); // (at the first cloud's pose: the window does not move again)
        m.filterPointCloud(0.1, 0.1);
        m.clearMap();
    }
    Blob b;
    int  k = 1;
    for (const Cloud *c : {&small, &big}) {
        m.addToMap(c->data(), npts(*c), 3, pose_of(k++));
        m.filterPointCloud(0.1, 0.1);
        b.add(m.lastSegmentCounts(), 2 * sizeof(int));
        b.add(m.getGlobalCloud());
        b.add(m.getDrivability().data);
    }
    std::printf("mls %s: drv %d gnd %d global %zu\n", huge ? "B" : "A", m.lastSegmentCounts()[0], m.lastSegmentCounts()[1], m.getGlobalCloud().size() / 3);
    return b;
}

// graph_slam's calls (graph_slam.cpp:268-275): the keyframe, transformed and global-cloud blocks, and the filter's
static Blob run_mls_map(const Cloud &small, const Cloud &big, const Cloud *huge)
{
    slam_amd::MLSMap m(100, 100, 0.5, false);
    if (!m.ok()) std::exit(3);
    if (huge) {
        m.addKeyframe(huge->data(), npts(*huge), 3, pose_of(1));
        m.filterPointCloud(0.1, 0.1);
    }
    m.clearMap(); // A and B alike: a cleared map is not a new one (clearMap does not put the start pad back, mls.cpp:18-31)
    Blob b;
    int  k = 1;
    for (const Cloud *c : {&small, &big}) {
        m.addKeyframe(c->data(), npts(*c), 3, pose_of(k++));
        m.filterPointCloud(0.1, 0.1);
        Cloud obstacle, ground;
        m.getSegmentedClouds(obstacle, ground);
        b.add(m.getDrivability().data);
        b.add(obstacle);
        b.add(ground);
        b.add(m.getGlobalCloud());
        if (c == &big) std::printf("mls_map %s: obstacle %zu ground %zu global %zu\n", huge ? "B" : "A", obstacle.size() / 3, ground.size() / 3, m.getGlobalCloud().size() / 3);
    }
    return b;
}

// scan_registration's calls (scan_registration.cpp:139-159) against one target: the scene's blocks
static Blob run_ccicp(const Cloud &base, const Cloud &small, const Cloud &big, const Cloud *huge)
{
    slam_amd::CCICP icp(slam_amd::SCAN_TO_SCAN);
    Pose            init;
    init.x = 0.15, init.y = -0.1, init.z = 0.05, init.qz = std::sin(0.015), init.qw = std::cos(0.015);
    icp.setTargetCloud(base.data(), npts(base), 3, init);
    if (huge) {
        icp.setSceneCloud(huge->data(), npts(*huge), 3);
        (void)icp.doICPMatch(init);
        Cloud a, b, c, d;
        icp.getSegmentedClouds(a, b, c, d);
        icp.setTargetCloud(base.data(), npts(base), 3, init); // a fresh target: the crop box and the index start over
    }
    Blob b;
    for (const Cloud *c : {&small, &big}) {
        icp.setSceneCloud(c->data(), npts(*c), 3);
        const Pose   r = icp.doICPMatch(init);
        const double pose[7] = {r.x, r.y, r.z, r.qx, r.qy, r.qz, r.qw};
        const int    counts[8] = {icp.getNumberCorrespondences(), icp.lastIterations(), icp.sceneCounts()[0], icp.sceneCounts()[1],
                                  icp.modelCounts()[0], icp.modelCounts()[1], icp.sceneSize(), icp.groundSceneSize()};
        b.add(pose, sizeof pose);
        b.add(counts, sizeof counts);
        Cloud target, scene, g_target, g_scene;
        icp.getSegmentedClouds(target, scene, g_target, g_scene);
        b.add(scene);
        b.add(g_scene);
        std::printf("ccicp %s: pose %.6f %.6f %.6f qw %.6f corr %d iters %d scene %d+%d model %d+%d\n", huge ? "B" : "A", r.x, r.y, r.z, r.qw, counts[0],
                    counts[1], counts[2], counts[3], counts[4], counts[5]);
    }
    return b;
}

// global_generate's loop (global_generate.cpp:122-232): the scan's block, and the cropped map's as the map grows.  The builder
// cannot be emptied: B's oversized scan is one it rejects (MAX_SCORE below any fitness), which leaves map and pose as they were.
static Blob run_builder(const Cloud &base, const Cloud &small, const Cloud &big, const Cloud *huge)
{
    slam_amd::GlobalMapBuilder g;
    if (!g.ok()) std::exit(3);
    if (!g.addCloud(base.data(), npts(base), 3)) std::exit(4); // the first cloud is the map
    if (huge) {
        g.MAX_SCORE = -1.0;
        if (g.addCloud(huge->data(), npts(*huge), 3)) std::exit(4);
        g.MAX_SCORE = 1.0;
    }
    Blob b;
    for (const Cloud *c : {&small, &big}) {
        const int accepted = g.addCloud(c->data(), npts(*c), 3), valid = g.last_valid;
        b.add(&accepted, sizeof accepted);
        b.add(&valid, sizeof valid);
        b.add(&g.last, sizeof g.last);
        b.add(g.pose(), 16 * sizeof(float));
        b.add(g.map());
        std::printf("builder %s: accepted %d valid %d iterations %d pairs %d fitness %g voxels %zu\n", huge ? "B" : "A", accepted, valid, g.last.edge.iterations,
                    g.last.fitness_pairs, g.last.fitness, g.map().size() / 4);
    }
    return b;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1], out = argv[2];
    const Cloud       small = read_all(dir + "/small.f32"), big = read_all(dir + "/big.f32"), huge = read_all(dir + "/huge.f32"),
                base = read_all(dir + "/base.f32");
    run_mls(small, big, nullptr).write(out + ".mls.A");
    run_mls(small, big, &huge).write(out + ".mls.B");
    run_mls_map(small, big, nullptr).write(out + ".mls_map.A");
    run_mls_map(small, big, &huge).write(out + ".mls_map.B");
    run_ccicp(base, small, big, nullptr).write(out + ".ccicp.A");
    run_ccicp(base, small, big, &huge).write(out + ".ccicp.B");
    run_builder(base, small, big, nullptr).write(out + ".builder.A");
    run_builder(base, small, big, &huge).write(out + ".builder.B");
    return 0;
}
