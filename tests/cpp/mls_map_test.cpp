// graph_slam's global map over the adapter include/slam_amd/mls_map.hpp, written like graph_slam.cpp:
//   the first keyframe as it arrives (:306-316: setMinClusterPoints(5), addToMap, setMinClusterPoints(10)),
//   regenerateGlobalMap (:260-280: clearMap, every keyframe transformed by its pose and added, filterPointCloud(0.1, 0.1)),
//   getSegmentedClouds (:456) handed to scan_registration's CCICP(SCAN_TO_MAP) (scan_registration.cpp:73-104, 139-159),
//   offsetMap.
//   mls_map_test <dir> <out> <K>
// dir: kf<k>.f32 (keyframes in the sensor frame, PointXYZ: 4 floats per point), poses.f64 (K x 7: x y z qx qy qz qw),
// scene.f32 (n x 3), init.f64 (7), oracle_obstacle.f32 / oracle_ground.f32 (the restatement's segmented clouds).
// Exit 5 when CCICP on the map's clouds and CCICP on the restatement's clouds give different poses.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/ccicp.hpp"
#include "slam_amd/mls_map.hpp"

template <class T>
static std::vector<T> read_all(const std::string &path)
{
    std::vector<T> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) std::exit(2);
    std::fclose(f);
    return v;
}

template <class T>
static void write_all(const std::string &path, const std::vector<T> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(2);
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
}

static slam_amd::Pose pose_of(const double *q)
{
    slam_amd::Pose p;
    p.x = q[0], p.y = q[1], p.z = q[2], p.qx = q[3], p.qy = q[4], p.qz = q[5], p.qw = q[6];
    return p;
}

static slam_amd::Pose match(const std::vector<float> &obstacle, const std::vector<float> &ground, const std::vector<float> &scene,
                            const slam_amd::Pose &init, int *n_corr)
{
    slam_amd::CCICP icp(slam_amd::SCAN_TO_MAP);                            // scan_registration.cpp:57
    icp.setTargetCloud(obstacle.data(), (int)obstacle.size() / 3, 3, init); // :97
    icp.setTargetGndCloud(ground.data(), (int)ground.size() / 3, 3);       // :98
    icp.setSceneCloud(scene.data(), (int)scene.size() / 3, 3);             // :139
    const slam_amd::Pose r = icp.doICPMatch(init);                         // :159
    *n_corr = icp.getNumberCorrespondences();
    return r;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string dir = argv[1], out = argv[2];
    const int         K = std::atoi(argv[3]);
    const auto        poses = read_all<double>(dir + "/poses.f64");
    std::vector<std::vector<float>> kf(K);
    for (int k = 0; k < K; ++k) kf[k] = read_all<float>(dir + "/kf" + std::to_string(k) + ".f32");

    slam_amd::MLSMap globalMap(1000, 1000, 0.5, false, 1.45); // graph_slam.cpp:71
    if (!globalMap.ok()) return 3;
    {
        slam_amd::MLSMap rolling(100, 100, 0.5, true); // rolling maps are slam_amd::MLS: no handle
        if (rolling.ok()) return 3;
    }
    // the first keyframe (graph_slam.cpp:306-316)
    globalMap.setMinClusterPoints(5);
    globalMap.addKeyframe(kf[0].data(), (int)kf[0].size() / 4, 4, pose_of(&poses[0]));
    globalMap.setMinClusterPoints(10);
    std::vector<float> obstacle, ground;
    globalMap.getSegmentedClouds(obstacle, ground);
    write_all(out + ".first_obstacle", obstacle);
    write_all(out + ".first_ground", ground);
    // a refused setter leaves the parameters as they were, and the next setter still takes effect
    globalMap.setMaxClusters(1000);
    globalMap.setMinClusterPoints(10);
    if (globalMap.params().max_clusters != 50 || globalMap.params().min_cluster_points != 10) return 4;

    // regenerateGlobalMap (graph_slam.cpp:260-280)
    globalMap.clearMap();
    for (int k = 0; k < K; ++k) globalMap.addKeyframe(kf[k].data(), (int)kf[k].size() / 4, 4, pose_of(&poses[7 * (size_t)k]));
    std::vector<float> unfiltered = globalMap.getGlobalCloud();
    globalMap.filterPointCloud(0.1, 0.1);
    const std::vector<float> filtered = globalMap.getGlobalCloud();
    slam_amd::voxel_filter_host(unfiltered, 0.1, 0.1); // the host fallback's filter on the same cloud
    write_all(out + ".global", filtered);
    write_all(out + ".global_host", unfiltered);

    globalMap.getSegmentedClouds(obstacle, ground); // graph_slam.cpp:456
    write_all(out + ".obstacle", obstacle);
    write_all(out + ".ground", ground);
    write_all(out + ".drivability", globalMap.getDrivability().data);

    // scan_registration's CCICP(SCAN_TO_MAP) on the map's clouds and on the restatement's
    const auto init = read_all<double>(dir + "/init.f64");
    const auto scene = read_all<float>(dir + "/scene.f32");
    int        nc_map = 0, nc_ora = 0;
    const slam_amd::Pose r = match(obstacle, ground, scene, pose_of(init.data()), &nc_map);
    const slam_amd::Pose q = match(read_all<float>(dir + "/oracle_obstacle.f32"), read_all<float>(dir + "/oracle_ground.f32"), scene,
                                   pose_of(init.data()), &nc_ora);
    write_all(out + ".pose", std::vector<double>{r.x, r.y, r.z, r.qx, r.qy, r.qz, r.qw, (double)nc_map});

    // offsetMap (mls.cpp:481-505)
    slam_amd::Pose off;
    off.z = 0.25;
    globalMap.offsetMap(off);
    globalMap.getSegmentedClouds(obstacle, ground);
    write_all(out + ".offset_obstacle", obstacle);
    write_all(out + ".offset_global", globalMap.getGlobalCloud());

    if (r.x != q.x || r.y != q.y || r.z != q.z || r.qx != q.qx || r.qy != q.qy || r.qz != q.qz || r.qw != q.qw || nc_map != nc_ora) {
        std::fprintf(stderr, "map clouds: %.9f %.9f %.9f, restatement's clouds: %.9f %.9f %.9f\n", r.x, r.y, r.z, q.x, q.y, q.z);
        return 5;
    }
    return 0;
}
