// slam_amd/pose_graph.hpp -- header-only adapter with the shape of graph_slam's optimiser globals (graph_slam/src/graph_slam.cpp)
// over the C-ABI (slam_mi355x.h, slam_pgo_*; the contract is docs/PGO.md):
//   initOptimizer   :286-306   vertex 0 at the origin with the current orientation, fixed
//   addVertex       :179-186   VertexSE3::setEstimateDataImpl(x y z qx qy qz qw)
//   addEdge         :188-202   EdgeSE3 with the edge pose as measurement and edgeInf as information
//   optimizeGraph   :322-390   optimize(10), the estimates written back into the pose graph, the pose offset
// The pose offset is computed AS WRITTEN at :356-384.  It is not a rigid transform: y takes vpy cos + vpx sin (a rotation would
// subtract in x), and a yaw difference past +-pi is wrapped and then negated.  The reference publishes it with the remark
// that it "seems to be breaking everything" (:555); nothing here consumes it, and it is kept so that a node built on this
// header publishes what the reference publishes.
#pragma once
#include <cmath>
#include <cstdio>

#include "slam_amd/graph_edges.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

class PoseGraphOptimizer {
public:
    int iterations = 10; // optimizer.optimize(10), :332

    explicit PoseGraphOptimizer(const slam_pgo_params *params = nullptr)
    {
        if (slam_pgo_create(params, &h_) != SLAM_OK) {
            warn();
            h_ = nullptr;
        }
    }
    ~PoseGraphOptimizer() { slam_pgo_destroy(h_); }
    PoseGraphOptimizer(const PoseGraphOptimizer &) = delete;
    PoseGraphOptimizer &operator=(const PoseGraphOptimizer &) = delete;
    bool                   ok() const { return h_ != nullptr; }
    slam_pgo_t            *handle() { return h_; }
    const slam_pgo_result &result() const { return last_; } // of the last optimizeGraph

    // :294-303: the first vertex, fixed at (0, 0, 0) with curPose's orientation.  The node the reference pushes for it (idx 0,
    // x = y = 0, that orientation) is returned through `first`; its keyframe goes to KeyframeGraph::addNode with this pose.
    bool initOptimizer(const Pose &curPose, Pose *first = nullptr)
    {
        Pose origin = curPose;
        origin.x = origin.y = origin.z = 0.0;
        if (first) *first = origin;
        const double p[7] = {0, 0, 0, curPose.qx, curPose.qy, curPose.qz, curPose.qw};
        return h_ && check(slam_pgo_clear(h_)) && check(slam_pgo_add_vertex(h_, 0, p, 1));
    }

    bool addVertex(const GraphNode &node) // :179-186
    {
        const Pose  &q = node.pose;
        const double p[7] = {q.x, q.y, q.z, q.qx, q.qy, q.qz, q.qw};
        return h_ && check(slam_pgo_add_vertex(h_, node.idx, p, 0));
    }

    bool addEdge(const GraphEdge &gE) // :188-202
    {
        const Pose  &q = gE.edge;
        const double z[7] = {q.x, q.y, q.z, q.qx, q.qy, q.qz, q.qw};
        return h_ && check(slam_pgo_add_edge(h_, gE.from, gE.to, z, gE.edgeInf));
    }

    // :322-390.  false (pG untouched, *newPose untouched) where the optimiser fails.
    bool optimizeGraph(KeyframeGraph &pG, const Pose &curPose, Pose *newPose)
    {
        if (!h_ || pG.nodes.empty()) return false;
        if (!check(slam_pgo_optimize(h_, iterations, &last_, nullptr))) return false;
        int n = 0;
        if (!check(slam_pgo_read_vertices(h_, nullptr, 0, &n))) return false;
        std::vector<double> est(7 * (size_t)n);
        if (!check(slam_pgo_read_vertices(h_, est.data(), n, &n))) return false;
        const GraphNode preNode = pG.nodes.back(); // :334
        for (size_t i = 0; i < pG.nodes.size() && i < (size_t)n; ++i) { // :335-354
            Pose &p = pG.nodes[i].pose;
            p.x = est[7 * i], p.y = est[7 * i + 1], p.z = est[7 * i + 2];
            p.qx = est[7 * i + 3], p.qy = est[7 * i + 4], p.qz = est[7 * i + 5], p.qw = est[7 * i + 6];
        }
        if (newPose) *newPose = poseOffset(preNode.pose, pG.nodes.back().pose, curPose);
        return true;
    }

    // :356-384, as written
    static Pose poseOffset(const Pose &pre, const Pose &post, const Pose &curPose)
    {
        using detail::tf_yaw;
        const double vnx = post.x - pre.x, vny = post.y - pre.y, vnz = post.z - pre.z;
        double       vntheta = tf_yaw(post) - tf_yaw(pre);
        if (vntheta > M_PI)
            vntheta = -(vntheta - 2 * M_PI);
        else if (vntheta < -M_PI)
            vntheta = -(vntheta + 2 * M_PI);
        const double vpx = curPose.x - pre.x, vpy = curPose.y - pre.y;
        double       vptheta = tf_yaw(curPose) - tf_yaw(pre);
        if (vptheta > M_PI)
            vptheta = -(vptheta - 2 * M_PI);
        else if (vptheta < -M_PI)
            vptheta = -(vptheta + 2 * M_PI);
        Pose out;
        out.x = (vpx * std::cos(vntheta) + vpy * std::sin(vntheta) + vnx) - vpx;
        out.y = (vpy * std::cos(vntheta) + vpx * std::sin(vntheta) + vny) - vpy;
        out.z = vnz;
        const double half = (vntheta + vptheta) * 0.5; // tf::createQuaternionMsgFromYaw
        out.qx = 0.0, out.qy = 0.0, out.qz = std::sin(half), out.qw = std::cos(half);
        return out;
    }

private:
    static bool check(int rc)
    {
        if (rc != SLAM_OK) warn();
        return rc == SLAM_OK;
    }
    static void warn() { detail::warn("PoseGraphOptimizer"); }

    slam_pgo_t     *h_ = nullptr;
    slam_pgo_result last_ = {};
};

} // namespace slam_amd
