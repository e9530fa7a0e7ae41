// Loop closure by appearance through the adapters: keyframes of two laps go through slam_amd::KeyframeGraph; each gets the
// reference's pose-based edges (addEdgesForNewNode) and, from the second lap on, loop edges by descriptor
// (addLoopEdgesForNewNode).  Beside them the best any candidate search could do: the true neighbours of the first lap as
// pairs and the true relative yaw as start, through the same calcEdgesFrom.  Two slam_amd::PoseGraphOptimizer hold the
// pose-based edges plus the one or the other kind, and are optimised once at the end.
//   loop_closure_test <dir> <out> <K> <first keyframe of lap two> <descriptor max_range> <SC_MAX_DISTANCE> <GSLAM_KNN> [registration: 0 ICP, 1 GICP]
// dir: kf<k>.f32 (sensor frame, 3 floats per point), poses.f64 (K x 7: the drifting pose estimate when keyframe k arrives),
// truth.f64 (K x 3: x y yaw).  out.edges: 19 doubles per tried edge -- kind (0 pose-based, 1 loop, 2 ground truth), from, to,
// accepted, pairs, numCorr, converged, x_diff, y_diff, theta_diff, the edge pose (7), the yaw it started from, the descriptor
// distance (loop edges).  out.poses: 2 K x 7, the nodes after optimising with the loop edges, then with the ground-truth edges.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

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

static void write_all(const std::string &path, const std::vector<double> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(2);
    if (!v.empty()) std::fwrite(v.data(), sizeof(double), v.size(), f);
    std::fclose(f);
}

static slam_amd::Pose pose_of(const double *q)
{
    slam_amd::Pose p;
    p.x = q[0], p.y = q[1], p.z = q[2], p.qx = q[3], p.qy = q[4], p.qz = q[5], p.qw = q[6];
    return p;
}

static void push_edge(std::vector<double> &v, int kind, const slam_amd::GraphEdge &e, double distance)
{
    const double row[19] = {(double)kind, (double)e.from, (double)e.to, e.accepted ? 1.0 : 0.0, (double)e.pairs, (double)e.numCorr, (double)e.converged,
                            e.x_diff, e.y_diff, e.theta_diff, e.edge.x, e.edge.y, e.edge.z, e.edge.qx, e.edge.qy, e.edge.qz, e.edge.qw,
                            std::atan2((double)e.init[4], (double)e.init[0]), distance};
    v.insert(v.end(), row, row + 19);
}

int main(int argc, char **argv)
{
    if (argc < 8) return 2;
    const std::string dir = argv[1], out = argv[2];
    const int         K = std::atoi(argv[3]), lapTwo = std::atoi(argv[4]);
    const auto        poses = read_all<double>(dir + "/poses.f64"), truth = read_all<double>(dir + "/truth.f64");
    if ((int)poses.size() < 7 * K || (int)truth.size() < 3 * K) return 2;

    slam_amd::KeyframeGraph      pG;
    slam_amd::PoseGraphOptimizer withLoop, withTruth;
    if (!pG.ok() || !withLoop.ok() || !withTruth.ok()) return 3;
    slam_kf_sc_params sp;
    slam_kf_sc_default_params(&sp);
    sp.max_range = std::atof(argv[5]);
    if (slam_kf_set_sc_params(pG.handle(), &sp) != SLAM_OK) return 3;
    pG.SC_MAX_DISTANCE = std::atoi(argv[6]);
    if (argc > 8 && std::atoi(argv[8]) == 1) pG.registration = slam_amd::KeyframeGraph::GICP;
    pG.GSLAM_KNN = std::atoi(argv[7]); // 3: the reference's; 0: the pose-based edges are the one to the predecessor alone
    withLoop.iterations = withTruth.iterations = 30;

    slam_amd::Pose first;
    if (!withLoop.initOptimizer(pose_of(&poses[0]), &first) || !withTruth.initOptimizer(pose_of(&poses[0]))) return 4;
    std::vector<double> rows;
    for (int k = 0; k < K; ++k) {
        const auto cloud = read_all<float>(dir + "/kf" + std::to_string(k) + ".f32");
        if (pG.addNode(cloud.data(), (int)cloud.size() / 3, 3, k ? pose_of(&poses[7 * (size_t)k]) : first) != k) return 4;
        if (k == 0) continue;
        if (!withLoop.addVertex(pG.nodes.back()) || !withTruth.addVertex(pG.nodes.back())) return 4;
        std::vector<slam_amd::GraphEdge> tried;
        // the reference's edges: the neighbours by estimated pose and the predecessor
        pG.addEdgesForNewNode(&tried);
        for (const slam_amd::GraphEdge &e : tried) {
            push_edge(rows, 0, e, 0.0);
            if (e.accepted && (!withLoop.addEdge(e) || !withTruth.addEdge(e))) return 4;
        }
        if (k < lapTwo) continue;
        // by appearance
        const std::vector<slam_amd::LoopCandidate> cands = pG.getLoopCandidates(pG.nodes.back(), pG.SC_CANDIDATES);
        pG.addLoopEdgesForNewNode(&tried);
        for (size_t e = 0; e < tried.size(); ++e) {
            if (tried[e].ctype != slam_amd::CTYPE_LOOP || e >= cands.size() || cands[e].id != tried[e].from) return 6;
            push_edge(rows, 1, tried[e], (double)cands[e].distance);
            if (tried[e].accepted && !withLoop.addEdge(tried[e])) return 4;
        }
        // by ground truth: the keyframes of lap one within 1.5 m, nearest first, at most SC_CANDIDATES; the true relative yaw
        std::vector<std::pair<double, int>> near;
        for (int i = 0; i < lapTwo; ++i) {
            const double dx = truth[3 * i] - truth[3 * k], dy = truth[3 * i + 1] - truth[3 * k + 1], d = std::sqrt(dx * dx + dy * dy);
            if (d <= 1.5) near.push_back(std::make_pair(d, i));
        }
        std::stable_sort(near.begin(), near.end());
        if ((int)near.size() > pG.SC_CANDIDATES) near.resize((size_t)pG.SC_CANDIDATES);
        std::vector<std::pair<int, int>>   pairs;
        std::vector<std::array<float, 16>> inits;
        for (const auto &c : near) {
            pairs.push_back(std::make_pair(c.second, k));
            inits.push_back(slam_amd::KeyframeGraph::yawInit(truth[3 * k + 2] - truth[3 * c.second + 2]));
        }
        if (!pG.calcEdgesFrom(pairs, inits, tried)) return 4;
        for (const slam_amd::GraphEdge &e : tried) {
            push_edge(rows, 2, e, 0.0);
            if (e.accepted && !withTruth.addEdge(e)) return 4;
        }
    }
    // optimise either graph from the same drifting estimates
    const std::vector<slam_amd::GraphNode> estimates = pG.nodes;
    std::vector<double>                    result;
    for (slam_amd::PoseGraphOptimizer *o : {&withLoop, &withTruth}) {
        pG.nodes = estimates;
        slam_amd::Pose newPose;
        if (!o->optimizeGraph(pG, pG.nodes.back().pose, &newPose)) return 5;
        const slam_pgo_result &r = o->result();
        std::fprintf(stderr, "%s: %d iterations, %d trials, stop %d, chi2 %.6g -> %.6g\n", o == &withLoop ? "loop edges" : "ground-truth edges", r.iterations,
                     r.n_trials, r.stop_reason, r.chi2_initial, r.chi2_final);
        for (const slam_amd::GraphNode &n : pG.nodes) {
            const double q[7] = {n.pose.x, n.pose.y, n.pose.z, n.pose.qx, n.pose.qy, n.pose.qz, n.pose.qw};
            result.insert(result.end(), q, q + 7);
        }
    }
    write_all(out + ".edges", rows);
    write_all(out + ".poses", result);
    return 0;
}
