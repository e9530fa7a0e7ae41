// slam_amd/graph_edges.hpp -- header-only adapter with the shape of graph_slam's keyframe tools
// (graph_slam/include/graph_slam/graphSlamTools.h, src/graphSlamTools.cpp) over the C-ABI (slam_mi355x.h, slam_kf_*):
//   graphSlamGetNearestKF   :43-65     getNearestKF
//   graphSlamGetKNN         :72-106    getKNN
//   calcEdgeIcp             :218-364   calcEdgeIcp / calcEdges (a batch in one device call)
//   graph_slam.cpp:508-518             addEdgesForNewNode: the KNN edges and the edge to the previous keyframe, one call
// getKNN picks by estimated pose ("FIXME: only based on distance", :70), which finds nothing once drift exceeds the distance
// between revisits.  getLoopCandidates / calcEdgesFrom / addLoopEdgesForNewNode pick by appearance instead (slam_kf_sc_*,
// docs/SCAN_CONTEXT.md) and have no counterpart in the reference.
// A keyframe is filtered (pcl::VoxelGrid 0.5) and indexed once, when it is added; the reference filters both clouds again at
// every edge, which gives the same clouds.  The device does the ICP and computeEdgeInformationLUM; what is left of
// calcEdgeIcp runs here: the initial transform from the two poses, the edge pose and quaternion, the acceptance gate.
// addVertex / addEdge / optimizeGraph are slam_amd/pose_graph.hpp.
//
// Two places where this differs from the reference's host arithmetic by rounding, neither pinned (docs/KF_EDGE.md):
// Mfrom.inverse() is taken as the rigid inverse (R', -R't) instead of Eigen's general 4 x 4 inverse, and the initial pose's
// quaternion comes from the linear part of the f32 matrix instead of Affine3d::rotation()'s polar factor.
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "slam_amd/buffer.hpp" // detail::warn
#include "slam_amd/pose.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

// graphSlamTools.h:27-34
enum { CTYPE_HOME = 0, CTYPE_ODOM = 1, CTYPE_NN = 2 };
enum { CTYPE_LOOP = 3 }; // an edge found by appearance (addLoopEdgesForNewNode); not the reference's

struct GraphNode { // graph_slam.h Node: idx, pose (the keyframe cloud lives in the store)
    int  idx = 0;
    Pose pose;
};

struct GraphEdge { // graph_slam/Edge: from, to, ctype, edge (pose), edgeInf
    int    from = 0, to = 0, ctype = CTYPE_NN;
    Pose   edge;
    double edgeInf[36] = {0};
    // what the reference computes and drops: the Matrix4f handed to align and the one it returned, hasConverged() & co.
    float  init[16] = {0}, transform[16] = {0};
    int    iterations = 0, state = 0, converged = 0, pairs = 0, numCorr = 0, singular = 0;
    double x_diff = 0, y_diff = 0, theta_diff = 0;
    bool   accepted = false;
};

struct LoopCandidate {
    int    id = 0, distance = 0, shift = 0; // slam_kf_sc_match_t's: the candidate rolled by +shift sectors lies on the query
    double yaw = 0.0;                       // -shift 2 pi / n_sectors in (-pi, pi]: Rz(yaw) takes the query's points into the candidate's frame
};

class KeyframeGraph {
public:
    // graphSlamTools.h:23-24, 32-33: macros there, members here
    double KNN_DIST_THRESH = 5.0;
    int    GSLAM_KNN = 3;
    double DIST_MOVE_THRESH = 10.0;
    double ROT_MOVE_THRESH = 0.2;

    // The solver behind calcEdgeIcp / calcEdges / addEdgesForNewNode.  ICP: pcl::IterativeClosestPoint, what graph_slam runs.
    // GICP: slam_kf_register_gicp (docs/KF_GICP.md), the solver graphSlamTools.cpp names its matcher after (:10,17,37); the
    // information is still computeEdgeInformationLUM's block and the acceptance gate is the same.
    enum Registration { ICP = 0, GICP = 1 };
    Registration registration = ICP;

    // Loop-closure candidates by appearance (docs/SCAN_CONTEXT.md)
    int SC_MAX_DISTANCE = INT_MAX; // a candidate's descriptor distance is at most this; the scale depends on the scene, so no limit by default
    int SC_MIN_GAP = 10;           // a query never matches itself or the SC_MIN_GAP keyframes before it
    int SC_CANDIDATES = 3;         // candidates registered per new node

    std::vector<GraphNode> nodes; // PoseGraph
    std::vector<GraphEdge> edges;

    explicit KeyframeGraph(const slam_kf_params *params = nullptr) // null: setup_gicp's values
    {
        if (slam_kf_create(params, &h_) != SLAM_OK) {
            warn();
            h_ = nullptr;
        }
    }
    ~KeyframeGraph() { slam_kf_destroy(h_); }
    KeyframeGraph(const KeyframeGraph &) = delete;
    KeyframeGraph &operator=(const KeyframeGraph &) = delete;
    bool       ok() const { return h_ != nullptr; }
    slam_kf_t *handle() { return h_; }

    // graph_slam.cpp:501-504: *gN.keyframe = *current_cloud; pG.nodes.push_back(gN).  Returns the node's idx, -1 on failure.
    int addNode(const float *xyz, int n, int stride, const Pose &pose)
    {
        int id = -1;
        if (!h_ || slam_kf_add_keyframe(h_, xyz, n, stride, &id) != SLAM_OK) {
            warn();
            return -1;
        }
        GraphNode g;
        g.idx = id, g.pose = pose;
        nodes.push_back(g);
        return id;
    }

    // graphSlamGetNearestKF (:43-65): the distance from a node (idx = nodes.size() for one not added yet) to its nearest other
    double getNearestKF(const Pose &pose, int idx) const
    {
        double smallestDist = 1e20;
        for (size_t i = 0; i < nodes.size(); ++i) {
            const double dx = nodes[i].pose.x - pose.x, dy = nodes[i].pose.y - pose.y;
            const double currDist = std::sqrt(dx * dx + dy * dy);
            if (currDist < smallestDist && idx != nodes[i].idx) smallestDist = currDist;
        }
        return smallestDist;
    }

    // graphSlamGetKNN (:72-106), the loop bound numKF - 2 and K = min(numKF - 1, K) as written there
    std::vector<int> getKNN(const GraphNode &gN, int K) const
    {
        std::vector<int>                    toReturn;
        std::vector<std::pair<double, int>> sC;
        const int                           numKF = (int)nodes.size();
        K = std::min(numKF - 1, K);
        for (int i = 0; i < numKF - 2; ++i) {
            const double dx = nodes[i].pose.x - gN.pose.x, dy = nodes[i].pose.y - gN.pose.y;
            sC.push_back(std::make_pair(std::sqrt(dx * dx + dy * dy), i));
        }
        // the reference's std::sort on the distance alone leaves the order of equal distances open; stable here
        std::stable_sort(sC.begin(), sC.end(), [](const std::pair<double, int> &a, const std::pair<double, int> &b) { return a.first < b.first; });
        for (int i = 0; i < K; ++i)
            if (i < (int)sC.size() && gN.idx != sC[i].second) toReturn.push_back(sC[i].second);
        return toReturn;
    }

    // calcEdgeIcp for a batch: every (from, to) registered in one device call.  out[e].accepted is calcEdgeIcp's return value.
    bool calcEdges(const std::vector<std::pair<int, int>> &pairs, std::vector<GraphEdge> &out)
    {
        out.clear();
        if (!h_ || pairs.empty()) return h_ != nullptr;
        std::vector<slam_kf_edge_req>    req(pairs.size());
        std::vector<slam_kf_edge_result> res(pairs.size());
        for (size_t e = 0; e < pairs.size(); ++e) {
            const int from = pairs[e].first, to = pairs[e].second;
            if (from < 0 || to < 0 || from >= (int)nodes.size() || to >= (int)nodes.size()) return false;
            req[e].from = from, req[e].to = to;
            detail::relative_f32(nodes[from].pose, nodes[to].pose, req[e].init); // :258
        }
        int rc;
        if (registration == GICP) {
            std::vector<slam_kf_gicp_result> gres(pairs.size());
            rc = slam_kf_register_gicp(h_, req.data(), (int)req.size(), gres.data(), nullptr);
            for (size_t e = 0; e < pairs.size(); ++e) res[e] = gres[e].edge;
        } else
            rc = slam_kf_register_edges(h_, req.data(), (int)req.size(), res.data(), nullptr);
        if (rc != SLAM_OK) {
            warn();
            return false;
        }
        out.resize(pairs.size());
        for (size_t e = 0; e < pairs.size(); ++e) finish(req[e], res[e], &out[e]);
        return true;
    }

    // calcEdgeIcp (:218-364): true = a good match
    bool calcEdgeIcp(int from, int to, GraphEdge &gE)
    {
        std::vector<GraphEdge> one;
        if (!calcEdges({std::make_pair(from, to)}, one) || one.empty()) return false;
        gE = one[0];
        return gE.accepted;
    }

    // graph_slam.cpp:508-518 for the node added last: graphSlamAddEdgeToX for its KNN, then for its predecessor -- registered
    // together, pushed in that order.  Returns the edges pushed; `tried` (optional) gets every edge, rejected ones too.
    int addEdgesForNewNode(std::vector<GraphEdge> *tried = nullptr)
    {
        if (tried) tried->clear();
        if (nodes.size() < 2) return 0; // graphSlamAddEdgeToX :409
        const GraphNode                 &gN = nodes.back();
        std::vector<std::pair<int, int>> pairs;
        for (int k : getKNN(gN, GSLAM_KNN)) pairs.push_back(std::make_pair(k, gN.idx));
        pairs.push_back(std::make_pair(gN.idx - 1, gN.idx));
        std::vector<GraphEdge> got;
        if (!calcEdges(pairs, got)) return 0;
        int pushed = 0;
        for (const GraphEdge &e : got)
            if (e.accepted) edges.push_back(e), ++pushed;
        if (tried) *tried = got;
        return pushed;
    }

    // The K keyframes nearest to gN by descriptor among those more than SC_MIN_GAP before it, nearest first (equal
    // distances by id).  One search on the device against every keyframe; missing descriptors are computed by it.
    std::vector<LoopCandidate> getLoopCandidates(const GraphNode &gN, int K)
    {
        std::vector<LoopCandidate> out;
        const int                  count = h_ ? slam_kf_count(h_) : 0, q = gN.idx;
        if (q < 0 || q >= count || K <= 0) return out;
        std::vector<slam_kf_sc_match_t> m((size_t)count);
        int                             n_rings = 0, n_sectors = 0;
        if (slam_kf_sc_match(h_, &q, 1, m.data(), nullptr) != SLAM_OK || slam_kf_sc_read(h_, q, nullptr, 0, &n_rings, &n_sectors) != SLAM_OK) {
            warn();
            return out;
        }
        for (int i = 0; i < q - SC_MIN_GAP; ++i) {
            if (m[i].distance < 0 || m[i].distance > SC_MAX_DISTANCE) continue;
            LoopCandidate c;
            c.id = i, c.distance = m[i].distance, c.shift = m[i].shift;
            c.yaw = -(double)c.shift * (2.0 * M_PI / n_sectors);
            if (c.yaw <= -M_PI) c.yaw += 2.0 * M_PI;
            out.push_back(c);
        }
        std::stable_sort(out.begin(), out.end(), [](const LoopCandidate &a, const LoopCandidate &b) { return a.distance < b.distance; });
        if ((int)out.size() > K) out.resize((size_t)K);
        return out;
    }

    // calcEdges with the initial transforms given (row-major 4 x 4, source `to` into target `from`) and not taken from the poses
    bool calcEdgesFrom(const std::vector<std::pair<int, int>> &pairs, const std::vector<std::array<float, 16>> &inits, std::vector<GraphEdge> &out)
    {
        out.clear();
        if (!h_ || pairs.size() != inits.size()) return false;
        if (pairs.empty()) return true;
        std::vector<slam_kf_edge_req>    req(pairs.size());
        std::vector<slam_kf_edge_result> res(pairs.size());
        for (size_t e = 0; e < pairs.size(); ++e) {
            const int from = pairs[e].first, to = pairs[e].second;
            if (from < 0 || to < 0 || from >= (int)nodes.size() || to >= (int)nodes.size()) return false;
            req[e].from = from, req[e].to = to;
            std::copy(inits[e].begin(), inits[e].end(), req[e].init);
        }
        int rc;
        if (registration == GICP) {
            std::vector<slam_kf_gicp_result> gres(pairs.size());
            rc = slam_kf_register_gicp(h_, req.data(), (int)req.size(), gres.data(), nullptr);
            for (size_t e = 0; e < pairs.size(); ++e) res[e] = gres[e].edge;
        } else
            rc = slam_kf_register_edges(h_, req.data(), (int)req.size(), res.data(), nullptr);
        if (rc != SLAM_OK) {
            warn();
            return false;
        }
        out.resize(pairs.size());
        for (size_t e = 0; e < pairs.size(); ++e) finish(req[e], res[e], &out[e]);
        return true;
    }

    // Rz(yaw), zero translation: the transform a loop candidate's registration starts from
    static std::array<float, 16> yawInit(double yaw)
    {
        const float           c = (float)std::cos(yaw), s = (float)std::sin(yaw);
        std::array<float, 16> m = {c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        return m;
    }

    // For the node added last: its SC_CANDIDATES loop candidates registered in one device call, target = candidate (from),
    // source = the node (to), from Rz(-shift 2 pi / n_sectors) with zero translation; the acceptance gate is calcEdgeIcp's,
    // against that start.  Accepted edges are pushed with CTYPE_LOOP.  Returns the edges pushed; `tried` as addEdgesForNewNode.
    int addLoopEdgesForNewNode(std::vector<GraphEdge> *tried = nullptr)
    {
        if (tried) tried->clear();
        if (nodes.empty()) return 0;
        const GraphNode                   &gN = nodes.back();
        std::vector<std::pair<int, int>>   pairs;
        std::vector<std::array<float, 16>> inits;
        for (const LoopCandidate &c : getLoopCandidates(gN, SC_CANDIDATES)) {
            pairs.push_back(std::make_pair(c.id, gN.idx));
            inits.push_back(yawInit(c.yaw));
        }
        std::vector<GraphEdge> got;
        if (pairs.empty() || !calcEdgesFrom(pairs, inits, got)) return 0;
        int pushed = 0;
        for (GraphEdge &e : got) {
            e.ctype = CTYPE_LOOP;
            if (e.accepted) edges.push_back(e), ++pushed;
        }
        if (tried) *tried = got;
        return pushed;
    }

private:
    void finish(const slam_kf_edge_req &req, const slam_kf_edge_result &res, GraphEdge *gE) const
    {
        using namespace detail;
        gE->from = req.from, gE->to = req.to, gE->ctype = CTYPE_NN;
        for (int k = 0; k < 16; ++k) gE->init[k] = req.init[k], gE->transform[k] = res.transform[k];
        for (int k = 0; k < 36; ++k) gE->edgeInf[k] = res.information[k];
        gE->iterations = res.iterations, gE->state = res.state, gE->converged = res.converged, gE->pairs = res.pairs;
        gE->numCorr = res.num_corr, gE->singular = res.singular;
        // :259-260 initialization_pose(transformation.cast<double>()) -> initPose
        Pose   initPose;
        double m[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m[3 * r + c] = (double)req.init[4 * r + c];
        initPose.x = (double)req.init[3], initPose.y = (double)req.init[7], initPose.z = (double)req.init[11];
        eigen_quaternion(m, &initPose);
        // :318-331 the edge pose from the f32 result
        const float *T = res.transform;
        gE->edge.x = static_cast<double>(T[3]), gE->edge.y = static_cast<double>(T[7]), gE->edge.z = static_cast<double>(T[11]);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m[3 * r + c] = static_cast<double>(T[4 * r + c]);
        tf_quaternion(m, &gE->edge);
        // :335-342 (abs on doubles: fabs)
        gE->x_diff = std::fabs(initPose.x - gE->edge.x);
        gE->y_diff = std::fabs(initPose.y - gE->edge.y);
        double theta_diff = std::fabs(tf_yaw(initPose) - tf_yaw(gE->edge));
        if (theta_diff > 2 * M_PI)
            theta_diff = theta_diff - 2 * M_PI;
        else if (theta_diff > M_PI)
            theta_diff = 2 * M_PI - theta_diff;
        gE->theta_diff = theta_diff;
        // :355-360
        gE->accepted = !((gE->x_diff > DIST_MOVE_THRESH) || (gE->y_diff > DIST_MOVE_THRESH) || (theta_diff > ROT_MOVE_THRESH));
    }
    static void warn() { detail::warn("KeyframeGraph"); }

    slam_kf_t *h_ = nullptr;
};

} // namespace slam_amd
