// slam_amd/global_match.hpp -- header-only adapter with the shape of global_matching's matcher
// (global_matching/src/global_match.cpp:72-235) over the C-ABI (slam_mi355x.h, slam_kf_register_gicp):
//   setup_gicp        :225-235   gate 10, 10 iterations
//   laser_callback    :72-223    match(): up to ITERATIONS = 20 starts of the scan against the voxel-filtered prior map, the
//                                first whose normalised score passes is refined against the finer map and becomes an edge
// The reference tries its starts one after another and stops at the first that passes.  Here all of them are one batch of
// requests -- one launch, one workgroup each, one wait -- and the lowest-index start that passes is taken, which is the same
// start.  ROS, the publishers and the .pcd loader stay with the caller.
//
// Stated deviations (docs/KF_GICP.md section 4):
//   * the solver is the store's Generalized ICP, a restated contract, not PCL's;
//   * getFitnessScore() is ungated in PCL and gated by the store, so a start counts only if it converged and kept pairs;
//   * the random starts come from the generator the caller passes (default: the LCG below), not rand(), so that a run can be
//     repeated and C++ and Python draw the same starts;
//   * the store always filters: the refinement's target is the map at `refine_leaf` (0.25 m), not the unfiltered map, with a
//     gate of `refine_gate` (1 m) instead of 10 m, which the coarse match is well inside;
//   * scans stay in the stores: one filtered scan per match() and store, which a test reads back afterwards; a caller that
//     minds frees them with slam_kf_remove_keyframe (docs/VOXEL_MAP.md section 4).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "slam_amd/buffer.hpp" // detail::warn
#include "slam_mi355x.h"

namespace slam_amd {

// x <- 1664525 x + 1013904223 mod 2^32 (Numerical Recipes' constants); next() is the top 24 bits as a float in [0, 1).
// slam_amd.api.Lcg is the same generator.
struct Lcg {
    uint32_t state;
    explicit Lcg(uint32_t seed = 1) : state(seed) {}
    float next()
    {
        state = state * 1664525u + 1013904223u;
        return (float)(state >> 8) * (1.0f / 16777216.0f);
    }
};

struct GlobalMatchEdge { // graph_slam/Edge as laser_callback fills it (:181-195)
    int    from = 0, to = 0;
    double x = 0, y = 0, theta = 0;
    double covariance[9] = {0};
    // what the reference computes and drops
    bool   matched = false;  // false: the fallback edge of :204-221 (the current pose)
    int    start = -1;       // index of the start that passed
    float  coarse[16] = {0}, refined[16] = {0};
    double norm_score = 0;   // fitness / n_source of that start
    int    coarse_iterations = 0, coarse_state = 0, refine_iterations = 0, refine_state = 0;
};

class GlobalMatcher {
public:
    // global_match.cpp:30-41: macros there, members here
    double MAX_SCORE = 0.002;
    int    MAX_TRIES = 50;
    int    ITERATIONS = 20;
    double GUESS_DIST_RNG = 10.0;
    double GUESS_ANGLE_RNG = 2 * M_PI;
    double COV_YAW = 100, COV_XY = 1000;

    std::function<float()> random; // uniform in [0, 1); the default is an Lcg seeded with 1
    int                    try_count = 0;
    std::vector<slam_kf_gicp_result> last; // every start of the last match()
    std::vector<float>               last_starts; // dx dy dth per start

    // LEAF_SIZE 1.5 and setMaxCorrespondenceDistance(10) (:33, :227) for the coarse store
    explicit GlobalMatcher(double leaf = 1.5, double gate = 10.0, double refine_leaf = 0.25, double refine_gate = 1.0, uint32_t seed = 1)
    {
        Lcg g(seed);
        random = [g]() mutable { return g.next(); };
        slam_kf_params p;
        slam_kf_default_params(&p);
        p.leaf_size = leaf, p.gate = gate;
        if (slam_kf_create(&p, &coarse_) != SLAM_OK) warn(), coarse_ = nullptr;
        p.leaf_size = refine_leaf, p.gate = refine_gate;
        if (slam_kf_create(&p, &refine_) != SLAM_OK) warn(), refine_ = nullptr;
    }
    ~GlobalMatcher()
    {
        slam_kf_destroy(coarse_);
        slam_kf_destroy(refine_);
    }
    GlobalMatcher(const GlobalMatcher &) = delete;
    GlobalMatcher &operator=(const GlobalMatcher &) = delete;
    bool       ok() const { return coarse_ && refine_; }
    slam_kf_t *coarse() { return coarse_; }
    slam_kf_t *refine() { return refine_; }

    // main() of global_match.cpp: the prior map, filtered once per store
    bool setMap(const float *xyz, int n, int stride)
    {
        if (!ok()) return false;
        if (slam_kf_add_keyframe(coarse_, xyz, n, stride, &map_coarse_) != SLAM_OK || slam_kf_add_keyframe(refine_, xyz, n, stride, &map_refine_) != SLAM_OK) {
            warn();
            return false;
        }
        return true;
    }

    // laser_callback (:72-223).  True when an edge was filled: a match, or after MAX_TRIES failures the current pose.
    bool match(const float *cloud, int n, int stride, float cur_x, float cur_y, float cur_yaw, int id, GlobalMatchEdge *out)
    {
        if (!ok() || map_coarse_ < 0) return false;
        int scan = -1, n_scan = 0;
        if (slam_kf_add_keyframe(coarse_, cloud, n, stride, &scan) != SLAM_OK || slam_kf_keyframe_info(coarse_, scan, &n_scan, 0, 0, 0, 0) != SLAM_OK) {
            warn();
            return false;
        }
        // :105-122: start 0 is the current pose, the others are drawn around it
        std::vector<slam_kf_edge_req> req((size_t)ITERATIONS);
        last_starts.assign(3 * (size_t)ITERATIONS, 0.0f);
        for (int i = 0; i < ITERATIONS; ++i) {
            float dx = cur_x, dy = cur_y, dth = cur_yaw;
            if (i > 0) {
                dx = (float)((double)random() * 2.0 * GUESS_DIST_RNG - GUESS_DIST_RNG + (double)cur_x);
                dy = (float)((double)random() * 2.0 * GUESS_DIST_RNG - GUESS_DIST_RNG + (double)cur_y);
                dth = (float)((double)random() * GUESS_ANGLE_RNG);
            }
            last_starts[3 * i] = dx, last_starts[3 * i + 1] = dy, last_starts[3 * i + 2] = dth;
            req[i].from = map_coarse_, req[i].to = scan;
            planar(dx, dy, dth, req[i].init);
        }
        last.assign((size_t)ITERATIONS, slam_kf_gicp_result());
        if (slam_kf_register_gicp(coarse_, req.data(), ITERATIONS, last.data(), nullptr) != SLAM_OK) { // all starts, one call
            warn();
            return false;
        }
        bool match_found = false;
        for (int i = 0; i < ITERATIONS && !match_found; ++i) {
            const slam_kf_gicp_result &r = last[i];
            const double normScore = r.fitness / (double)n_scan; // :131-132, the double normalisation as written
            if (!(r.edge.converged && r.fitness_pairs > 0 && normScore < MAX_SCORE)) continue; // :151
            // :155-162 refine from the coarse result
            int fine = -1;
            slam_kf_edge_req    rq;
            slam_kf_gicp_result rr;
            rq.from = map_refine_;
            for (int k = 0; k < 16; ++k) rq.init[k] = r.edge.transform[k];
            if (slam_kf_add_keyframe(refine_, cloud, n, stride, &fine) != SLAM_OK || (rq.to = fine, slam_kf_register_gicp(refine_, &rq, 1, &rr, nullptr)) != SLAM_OK) {
                warn();
                return false;
            }
            match_found = true;
            *out = GlobalMatchEdge();
            out->matched = true, out->start = i, out->norm_score = normScore;
            for (int k = 0; k < 16; ++k) out->coarse[k] = r.edge.transform[k], out->refined[k] = rr.edge.transform[k];
            out->coarse_iterations = r.edge.iterations, out->coarse_state = r.edge.state;
            out->refine_iterations = rr.edge.iterations, out->refine_state = rr.edge.state;
            const float *T = rr.edge.transform;
            fill(out, id, (double)T[3], (double)T[7], std::atan2((double)T[4], (double)T[0])); // :182-190: getEulerYPR's yaw
        }
        if (match_found) {
            try_count = 0;
            return true;
        }
        ++try_count; // :199-221
        if (try_count >= MAX_TRIES) {
            *out = GlobalMatchEdge();
            fill(out, id, (double)cur_x, (double)cur_y, (double)cur_yaw);
            return true;
        }
        return false;
    }

    // the Matrix4f of :119-122, row-major: cos and sin in double of the float angle, rounded to float
    static void planar(float dx, float dy, float dth, float M[16])
    {
        const float c = (float)std::cos((double)dth), s = (float)std::sin((double)dth);
        const float m[16] = {c, -s, 0, dx, s, c, 0, dy, 0, 0, 1, 0, 0, 0, 0, 1};
        for (int k = 0; k < 16; ++k) M[k] = m[k];
    }

private:
    void fill(GlobalMatchEdge *e, int id, double x, double y, double theta) const
    {
        e->from = 0, e->to = id, e->x = x, e->y = y, e->theta = theta;
        for (int k = 0; k < 9; ++k) e->covariance[k] = 0;
        e->covariance[0] = e->covariance[4] = COV_XY, e->covariance[8] = COV_YAW;
    }
    static void warn() { detail::warn("GlobalMatcher"); }

    slam_kf_t *coarse_ = nullptr, *refine_ = nullptr;
    int        map_coarse_ = -1, map_refine_ = -1;
};

} // namespace slam_amd
