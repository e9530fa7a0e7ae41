// slam_amd::GlobalMatcher (include/slam_amd/global_match.hpp) run the way global_match.cpp runs: the prior map once, then a
// scan with its current pose; and slam_amd::KeyframeGraph with registration = GICP on the keyframe loop of kf_edge_test.cpp.
//   global_match_test match <dir> <out> <seed> <cur_x> <cur_y> <cur_yaw>
//     dir: map.f32, scan.f32 (3 floats per point).  out: line 1: published matched start try_count norm_score x y theta,
//     coarse (16), refined (16); then one line per start: dx dy dth, state iterations converged pairs fitness_pairs, fitness,
//     transform (16).  %.9g / %.17g: enough for every bit.
//   global_match_test graph <dir> <out> <K>
//     dir: kf<k>.f32, poses.f64 (K x 7).  out: one line per edge tried: to from accepted iterations state converged pairs
//     numCorr singular, init (16), transform (16).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "slam_amd/global_match.hpp"
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

static int run_match(int argc, char **argv)
{
    if (argc < 8) return 2;
    const std::string dir = argv[2];
    slam_amd::GlobalMatcher gm(1.5, 10.0, 0.25, 1.0, (uint32_t)std::atoi(argv[4]));
    if (!gm.ok()) return 3;
    const std::vector<float> map = read_all<float>(dir + "/map.f32"), scan = read_all<float>(dir + "/scan.f32");
    if (!gm.setMap(map.data(), (int)map.size() / 3, 3)) return 4;
    slam_amd::GlobalMatchEdge e;
    const bool published = gm.match(scan.data(), (int)scan.size() / 3, 3, (float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]), 1, &e);
    FILE *out = std::fopen(argv[3], "w");
    if (!out) return 2;
    std::fprintf(out, "%d %d %d %d %.17g %.17g %.17g %.17g", published ? 1 : 0, e.matched ? 1 : 0, e.start, gm.try_count, e.norm_score, e.x, e.y, e.theta);
    for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)e.coarse[i]);
    for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)e.refined[i]);
    std::fprintf(out, "\n");
    for (size_t s = 0; s < gm.last.size(); ++s) {
        const slam_kf_gicp_result &r = gm.last[s];
        std::fprintf(out, "%.9g %.9g %.9g %d %d %d %d %d %.17g", (double)gm.last_starts[3 * s], (double)gm.last_starts[3 * s + 1], (double)gm.last_starts[3 * s + 2],
                     r.edge.state, r.edge.iterations, r.edge.converged, r.edge.pairs, r.fitness_pairs, r.fitness);
        for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)r.edge.transform[i]);
        std::fprintf(out, "\n");
    }
    std::fclose(out);
    std::fprintf(stderr, "match: %s, start %d, score %.6g, refined in %d iterations\n", e.matched ? "found" : "none", e.start, e.norm_score, e.refine_iterations);
    return 0;
}

static int run_graph(int argc, char **argv)
{
    if (argc < 5) return 2;
    const std::string dir = argv[2];
    const int         K = std::atoi(argv[4]);
    slam_amd::KeyframeGraph g;
    if (!g.ok()) return 3;
    g.registration = slam_amd::KeyframeGraph::GICP;
    const std::vector<double> poses = read_all<double>(dir + "/poses.f64");
    if ((int)poses.size() < 7 * K) return 2;
    FILE *out = std::fopen(argv[3], "w");
    if (!out) return 2;
    for (int k = 0; k < K; ++k) {
        const std::vector<float> cloud = read_all<float>(dir + "/kf" + std::to_string(k) + ".f32");
        slam_amd::Pose           p;
        const double            *q = &poses[7 * (size_t)k];
        p.x = q[0], p.y = q[1], p.z = q[2], p.qx = q[3], p.qy = q[4], p.qz = q[5], p.qw = q[6];
        if (g.addNode(cloud.data(), (int)cloud.size() / 3, 3, p) != k) return 4;
        std::vector<slam_amd::GraphEdge> tried;
        const int                        pushed = g.addEdgesForNewNode(&tried);
        std::fprintf(stderr, "keyframe %d: %zu edges tried, %d pushed\n", k, tried.size(), pushed);
        for (const slam_amd::GraphEdge &e : tried) {
            std::fprintf(out, "%d %d %d %d %d %d %d %d %d", e.to, e.from, e.accepted ? 1 : 0, e.iterations, e.state, e.converged, e.pairs, e.numCorr, e.singular);
            for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)e.init[i]);
            for (int i = 0; i < 16; ++i) std::fprintf(out, " %.9g", (double)e.transform[i]);
            std::fprintf(out, "\n");
        }
    }
    std::fclose(out);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "match")) return run_match(argc, argv);
    if (!std::strcmp(argv[1], "graph")) return run_graph(argc, argv);
    return 2;
}
