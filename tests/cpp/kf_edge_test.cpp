// graph_slam's keyframe loop over the adapter include/slam_amd/graph_edges.hpp, written like graph_slam.cpp:497-518:
// every keyframe is added with its pose, then its edges -- the KNN and the previous keyframe -- are registered.
//   kf_edge_test <dir> <out> <K> [ROT_MOVE_THRESH]
// dir: kf<k>.f32 (keyframes in the sensor frame, 3 floats per point), poses.f64 (K x 7: x y z qx qy qz qw).
// out: one line per edge tried: to from accepted pushed-so-far iterations state converged pairs numCorr singular, the edge
// pose (7), x_diff y_diff theta_diff, init (16), transform (16), edgeInf (36), %.17g / %.9g: enough for every bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/graph_edges.hpp"

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

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const std::string dir = argv[1];
    const int         K = std::atoi(argv[3]);
    slam_amd::KeyframeGraph g;
    if (!g.ok()) return 3;
    if (argc > 4) g.ROT_MOVE_THRESH = std::atof(argv[4]);
    const std::vector<double> poses = read_all<double>(dir + "/poses.f64");
    if ((int)poses.size() < 7 * K) return 2;
    FILE *out = std::fopen(argv[2], "w");
    if (!out) return 2;
    for (int k = 0; k < K; ++k) {
        const std::vector<float> cloud = read_all<float>(dir + "/kf" + std::to_string(k) + ".f32");
        slam_amd::Pose           p;
        const double            *q = &poses[7 * (size_t)k];
        p.x = q[0], p.y = q[1], p.z = q[2], p.qx = q[3], p.qy = q[4], p.qz = q[5], p.qw = q[6];
        // graph_slam.cpp:494-499 asks getNearestKF before it adds; here every keyframe is added, the distance is printed
        const double nearest = g.getNearestKF(p, (int)g.nodes.size());
        if (g.addNode(cloud.data(), (int)cloud.size() / 3, 3, p) != k) return 4;
        std::vector<slam_amd::GraphEdge> tried;
        const int                        pushed = g.addEdgesForNewNode(&tried);
        std::fprintf(stderr, "keyframe %d: nearest %.3f m, %zu edges tried, %d pushed\n", k, nearest, tried.size(), pushed);
        for (const slam_amd::GraphEdge &e : tried) {
            std::fprintf(out, "%d %d %d %zu %d %d %d %d %d %d", e.to, e.from, e.accepted ? 1 : 0, g.edges.size(), e.iterations, e.state, e.converged,
                         e.pairs, e.numCorr, e.singular);
            std::fprintf(out, " %.17g %.17g %.17g %.17g %.17g %.17g %.17g", e.edge.x, e.edge.y, e.edge.z, e.edge.qx, e.edge.qy, e.edge.qz, e.edge.qw);
            std::fprintf(out, " %.17g %.17g %.17g", e.x_diff, e.y_diff, e.theta_diff);
            for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)e.init[i]);
            for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)e.transform[i]);
            for (int i = 0; i < 36; ++i) std::fprintf(out, " %.17g", e.edgeInf[i]);
            std::fprintf(out, "\n");
        }
    }
    std::fclose(out);
    // calcEdgeIcp alone gives what the batch gave
    if (K >= 2) {
        slam_amd::GraphEdge one;
        const bool          ok = g.calcEdgeIcp(0, 1, one);
        std::fprintf(stderr, "calcEdgeIcp(0, 1): %s, %d iterations\n", ok ? "accepted" : "rejected", one.iterations);
    }
    return 0;
}
