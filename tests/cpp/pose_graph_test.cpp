// graph_slam's back-end loop (graph_slam.cpp:479-560) over the adapters: every keyframe goes through
// slam_amd::KeyframeGraph (the node, its edges), slam_amd::PoseGraphOptimizer (addVertex, addEdge, optimizeGraph) and
// slam_amd::MLSMap (regenerateGlobalMap with the optimised poses).
//   pose_graph_test <dir> <out> <K> [min cluster points of the map replay, 10]
// dir: kf<k>.f32 (keyframes in the sensor frame, 3 floats per point), poses.f64 (K x 7: curPose when keyframe k arrives).
// out.edges: 45 doubles per pushed edge (from, to, the edge pose, edgeInf); out.steps: per keyframe k >= 1 the number of edges
// so far, iterations, stop reason, trials, w, chi2 before and after, the pose offset (7), then the k + 1 node poses (7 each);
// out.drivability: the global map after the last regenerateGlobalMap.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/mls_map.hpp"
#include "slam_amd/pose_graph.hpp"

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

static void push_pose(std::vector<double> &v, const slam_amd::Pose &p)
{
    const double q[7] = {p.x, p.y, p.z, p.qx, p.qy, p.qz, p.qw};
    v.insert(v.end(), q, q + 7);
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string dir = argv[1], out = argv[2];
    const int         K = std::atoi(argv[3]);
    const int         minClusterPoints = argc > 4 ? std::atoi(argv[4]) : 10;
    const auto        poses = read_all<double>(dir + "/poses.f64");
    if ((int)poses.size() < 7 * K) return 2;
    std::vector<std::vector<float>> kf(K);
    for (int k = 0; k < K; ++k) kf[k] = read_all<float>(dir + "/kf" + std::to_string(k) + ".f32");

    slam_amd::KeyframeGraph      pG;
    slam_amd::PoseGraphOptimizer optimizer;
    slam_amd::MLSMap             globalMap(1000, 1000, 0.5, false, 1.45); // graph_slam.cpp:71
    if (!pG.ok() || !optimizer.ok() || !globalMap.ok()) return 3;

    // initOptimizer (:286-317): the fixed first vertex, the first node, the first cloud into the map
    slam_amd::Pose curPose = pose_of(&poses[0]), first;
    if (!optimizer.initOptimizer(curPose, &first)) return 4;
    if (pG.addNode(kf[0].data(), (int)kf[0].size() / 3, 3, first) != 0) return 4;
    globalMap.setMinClusterPoints(5);
    globalMap.addKeyframe(kf[0].data(), (int)kf[0].size() / 3, 3, pG.nodes[0].pose);
    globalMap.setMinClusterPoints(minClusterPoints); // 10 in graph_slam.cpp:316; sparse test clouds ask for fewer

    std::vector<double> steps, edges;
    for (int k = 1; k < K; ++k) {
        curPose = pose_of(&poses[7 * (size_t)k]);
        // :485-505 (every keyframe of the run is far enough from the others)
        if (pG.addNode(kf[k].data(), (int)kf[k].size() / 3, 3, curPose) != k) return 4;
        if (!optimizer.addVertex(pG.nodes.back())) return 4;
        // :508-519: the KNN edges and the edge to the previous keyframe; every edge pushed goes to the optimiser
        const size_t had = pG.edges.size();
        pG.addEdgesForNewNode();
        for (size_t e = had; e < pG.edges.size(); ++e) {
            const slam_amd::GraphEdge &gE = pG.edges[e];
            if (!optimizer.addEdge(gE)) return 4;
            edges.push_back(gE.from), edges.push_back(gE.to);
            push_pose(edges, gE.edge);
            edges.insert(edges.end(), gE.edgeInf, gE.edgeInf + 36);
        }
        // :550-551
        slam_amd::Pose newPose;
        if (!optimizer.optimizeGraph(pG, curPose, &newPose)) return 5;
        const slam_pgo_result &r = optimizer.result();
        std::fprintf(stderr, "keyframe %d: %zu edges, %d iterations, %d trials, stop %d, w %d, chi2 %.6g -> %.6g, offset %.4f %.4f %.4f\n", k,
                     pG.edges.size(), r.iterations, r.n_trials, r.stop_reason, r.half_bandwidth, r.chi2_initial, r.chi2_final, newPose.x,
                     newPose.y, newPose.z);
        const double head[7] = {(double)pG.edges.size(), (double)r.iterations, (double)r.stop_reason, (double)r.n_trials,
                                (double)r.half_bandwidth, r.chi2_initial, r.chi2_final};
        steps.insert(steps.end(), head, head + 7);
        push_pose(steps, newPose);
        for (const slam_amd::GraphNode &n : pG.nodes) push_pose(steps, n.pose);
        // regenerateGlobalMap (:260-280)
        globalMap.clearMap();
        for (size_t i = 0; i < pG.nodes.size(); ++i) globalMap.addKeyframe(kf[i].data(), (int)kf[i].size() / 3, 3, pG.nodes[i].pose);
        globalMap.filterPointCloud(0.1, 0.1);
    }
    write_all(out + ".edges", edges);
    write_all(out + ".steps", steps);
    write_all(out + ".drivability", globalMap.getDrivability().data);
    return 0;
}
