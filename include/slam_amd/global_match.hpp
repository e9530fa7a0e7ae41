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
//
// MapLocalizer, below GlobalMatcher, relocalises a scan in a saved voxel map (docs/VOXEL_MAP.md section 11.3): the consumer
// slam_vmap_save / slam_vmap_load were written for.  It stands where GlobalMatcher stands, on the map's own plane voxels:
//   setMap / load   the fine map (borrowed / owned, through slam_vmap_load); it must have distributions.  Level k is an owned
//                   map of leaf ldexp(leaf, k) with the fine map's distribution parameters, filled by slam_vmap_coarsen from
//                   level k - 1: the bits of a map integrated at that leaf, derived after load, nothing of it in the file
//   yawFan          n planar starts at one position, yaws 2 pi / n apart
//   localize        the scan becomes a keyframe of the store; from the coarsest level down ONE slam_vmap_register_gicp call
//                   carries every live start, gated at GATE_RATIO times the level's leaf, from the level above's f32
//                   transform; a start that ends a level without pairs or degenerate is out; the winner is chosen at level 0
//   search          the scan becomes a keyframe and slam_vmap_search_keyframe scores it against one derived level: every pose
//                   of a lattice of rotations and whole-cell offsets, no prior (docs/VOXEL_MAP.md section 13)
//   relocalize      the cold start: SEARCH_YAWS rotations and every offset within `radius` at level SEARCH_LEVEL, the
//                   SEARCH_STARTS best hits' init are the starts, and localize descends from that level
// A 1 m map can be entered by the direct registration only from about a leaf away (its candidates are the 27 cells around the
// moved point); at an 8 m leaf the same rule reaches 8 m.  No random numbers: the same call gives the same bits.
// slam_amd.api.MapLocalizer is the same thing with Python's names and habits:
//   setMap -> set_map, yawFan -> yaw_fan, localize(cloud, n, stride, starts) -> localize(cloud, starts) returning a dict where
//   search(cloud, n, stride, params, level) -> search(cloud, params, level) returning the list of hits, relocalize alike, where
//   this fills a MapLocalizerResult; ok() has no twin (the constructor raises); an error of the library and a map that cannot
//   be taken are printed here and return false, there they raise SlamError.  The scan keyframe is removed on every way out.
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

// ---- MapLocalizer (the head of this file; docs/VOXEL_MAP.md section 11.3)
struct MapLocalizerResult {
    bool   found = false;
    int    index = -1; // of the winning start
    float  transform[16] = {0};
    double transform64[16] = {0};
    double x = 0, y = 0, theta = 0; // of the f32 transform, as GlobalMatcher fills its edge
    int    n_source = 0;            // points of the filtered scan
};

class MapLocalizer {
public:
    // fixed at construction
    const int    LEVELS;
    const double LEAF_SIZE; // of the store's filter
    const int    MAX_ITERATIONS = 100;
    const double TRANSFORMATION_EPSILON = 1e-6, FITNESS_EPSILON = 1e-6;
    // read at every call
    double GATE_RATIO = 2.0;
    int    N_YAW = 8;
    double MIN_PAIR_SHARE = 0.5;
    double MAX_SCORE = 0.03; // between the two level-0 fitness populations of section 11.3: sqrt(0.00745 * 0.0964)
    // relocalize's (section 13.4): the level searched and descended from, the rotations scored, the hits taken as starts
    int SEARCH_LEVEL = 1, SEARCH_YAWS = 64, SEARCH_STARTS = 4;

    std::vector<slam_vmap_search_hit> hits; // of the last search() or relocalize(), best first
    // every start's result per level of the last localize(): last[level][start], valid where ran[level][start]
    std::vector<std::vector<slam_vmap_gicp_result>> last;
    std::vector<std::vector<char>>                  ran;

    explicit MapLocalizer(int levels = 4, double leaf = 0.30) : LEVELS(levels), LEAF_SIZE(leaf)
    {
        slam_kf_params p;
        slam_kf_default_params(&p);
        p.leaf_size = leaf, p.gate = 2.0, p.transformation_epsilon = TRANSFORMATION_EPSILON, p.fitness_epsilon = FITNESS_EPSILON;
        slam_kf_gicp_params gp;
        slam_kf_gicp_default_params(&gp);
        gp.max_iterations = MAX_ITERATIONS, gp.transformation_epsilon = TRANSFORMATION_EPSILON;
        if (levels < 1 || slam_kf_create(&p, &store_) != SLAM_OK || slam_kf_set_gicp_params(store_, &gp) != SLAM_OK) {
            if (levels >= 1) warn();
            slam_kf_destroy(store_);
            store_ = nullptr;
        }
    }
    ~MapLocalizer()
    {
        dropMap();
        slam_kf_destroy(store_);
    }
    MapLocalizer(const MapLocalizer &) = delete;
    MapLocalizer &operator=(const MapLocalizer &) = delete;
    bool         ok() const { return store_ != nullptr; }
    slam_kf_t   *store() { return store_; }
    slam_vmap_t *level(int k) { return k == 0 ? fine_ : coarse_[(size_t)k - 1]; } // 0: the fine map; k >= 1: the derived ones

    // the fine map, borrowed: the caller keeps and destroys it
    bool setMap(slam_vmap_t *fine) { return take(fine, false); }
    // the fine map from a file of slam_vmap_save, owned
    bool load(const char *path)
    {
        slam_vmap_t *fine = nullptr;
        if (!ok() || slam_vmap_load(path, &fine) != SLAM_OK) return warn(), false;
        if (take(fine, true)) return true;
        slam_vmap_destroy(fine);
        return false;
    }
    // clears and refills the derived levels, after the fine map has grown
    bool rebuild()
    {
        if (!ok() || !fine_) return false;
        slam_vmap_t *below = fine_;
        for (slam_vmap_t *m : coarse_) {
            if (slam_vmap_clear(m, nullptr) != SLAM_OK || slam_vmap_coarsen(m, below, nullptr) != SLAM_OK) return warn(), false;
            below = m;
        }
        return true;
    }

    // n planar starts (16 floats each, row-major) at (x, y) with yaws (float)((double) yaw + 2 pi k / n)
    static std::vector<float> yawFan(float x, float y, float yaw, int n)
    {
        std::vector<float> out(16 * (size_t)(n > 0 ? n : 0));
        for (int k = 0; k < n; ++k) GlobalMatcher::planar(x, y, (float)((double)yaw + 2.0 * M_PI * (double)k / (double)n), &out[16 * (size_t)k]);
        return out;
    }

    // One scan (sensor frame, `stride` >= 3 floats per point) from `starts` (16 floats each).  False on an error of the library
    // or without a map; otherwise *out says whether a start won.  The winner among the level-0 results that converged with
    // fitness <= MAX_SCORE and fitness_pairs >= MIN_PAIR_SHARE n_source has the most fitness_pairs, then the lowest index.
    // from_level: the level the descent begins at (the levels above it are not run); -1, the default, is the coarsest.
    bool localize(const float *cloud, int n, int stride, const std::vector<float> &starts, MapLocalizerResult *out, int from_level = -1)
    {
        if (!ok() || !fine_ || !out || !cloud || n <= 0 || stride < 3 || from_level >= LEVELS) return false;
        *out = MapLocalizerResult();
        const int n_starts = (int)(starts.size() / 16);
        last.assign((size_t)LEVELS, std::vector<slam_vmap_gicp_result>((size_t)n_starts, slam_vmap_gicp_result()));
        ran.assign((size_t)LEVELS, std::vector<char>((size_t)n_starts, 0));
        int scan = -1;
        if (slam_kf_add_keyframe(store_, cloud, n, stride, &scan) != SLAM_OK) return warn(), false;
        std::vector<char> alive((size_t)n_starts, 1);
        const bool        done = slam_kf_keyframe_info(store_, scan, &out->n_source, 0, 0, 0, 0) == SLAM_OK &&
                                 descend(scan, starts, alive, from_level < 0 ? LEVELS - 1 : from_level);
        if (!done) warn();
        if (slam_kf_remove_keyframe(store_, scan) != SLAM_OK) warn();
        if (!done) return false;
        int best = -1;
        for (int i = 0; i < n_starts; ++i) {
            const slam_vmap_gicp_result &r = last[0][(size_t)i];
            if (!ran[0][(size_t)i] || !alive[(size_t)i] || !r.converged || !(r.fitness <= MAX_SCORE)) continue;
            if (!((double)r.fitness_pairs >= MIN_PAIR_SHARE * (double)out->n_source)) continue;
            if (best < 0 || r.fitness_pairs > last[0][(size_t)best].fitness_pairs) best = i;
        }
        if (best >= 0) {
            const slam_vmap_gicp_result &w = last[0][(size_t)best];
            out->found = true, out->index = best;
            for (int k = 0; k < 16; ++k) out->transform[k] = w.transform[k], out->transform64[k] = w.transform64[k];
            const float *T = w.transform;
            out->x = (double)T[3], out->y = (double)T[7], out->theta = std::atan2((double)T[4], (double)T[0]);
        }
        return true;
    }

    // The scan becomes a keyframe, as in localize, and slam_vmap_search_keyframe scores it against level `level` (-1:
    // SEARCH_LEVEL) with `params`: `hits` holds what was found, best first.  False on an error of the library or without a map.
    bool search(const float *cloud, int n, int stride, const slam_vmap_search_params &params, int level = -1)
    {
        hits.clear();
        if (level < 0) level = SEARCH_LEVEL;
        if (!ok() || !fine_ || !cloud || n <= 0 || stride < 3 || level >= LEVELS || params.top_m < 0) return false;
        int scan = -1, found = 0;
        if (slam_kf_add_keyframe(store_, cloud, n, stride, &scan) != SLAM_OK) return warn(), false;
        hits.resize((size_t)params.top_m);
        const bool done = slam_vmap_search_keyframe(this->level(level), store_, scan, &params, hits.data(), &found, nullptr, nullptr) == SLAM_OK;
        if (!done) warn();
        if (slam_kf_remove_keyframe(store_, scan) != SLAM_OK) warn();
        hits.resize(done ? (size_t)found : 0);
        return done;
    }

    // The cold start: no yaw, and no position closer than `radius` metres around (cx, cy), is asked for.  The window is
    // ceil(radius / leaf) cells of level SEARCH_LEVEL in x and y and none in z.  False on an error; otherwise *out says
    // whether a hit's descent won (found is false when there is no hit), and out->index is the hit's.
    bool relocalize(const float *cloud, int n, int stride, float cx, float cy, float cz, double radius, MapLocalizerResult *out)
    {
        if (!ok() || !fine_ || !out || SEARCH_LEVEL < 0 || SEARCH_LEVEL >= LEVELS) return false;
        *out = MapLocalizerResult();
        double leaf = 0;
        if (slam_vmap_layout(level(SEARCH_LEVEL), &leaf, nullptr, nullptr, nullptr) != SLAM_OK) return warn(), false;
        slam_vmap_search_params p;
        slam_vmap_default_search_params(&p);
        p.n_yaw = SEARCH_YAWS, p.top_m = SEARCH_STARTS, p.cx = cx, p.cy = cy, p.cz = cz;
        p.wx = p.wy = (int)std::ceil(radius / leaf), p.wz = 0;
        if (!search(cloud, n, stride, p, SEARCH_LEVEL)) return false;
        if (hits.empty()) {
            last.assign((size_t)LEVELS, std::vector<slam_vmap_gicp_result>());
            ran.assign((size_t)LEVELS, std::vector<char>());
            return true;
        }
        std::vector<float> starts;
        for (const slam_vmap_search_hit &h : hits) starts.insert(starts.end(), h.init, h.init + 16);
        return localize(cloud, n, stride, starts, out, SEARCH_LEVEL);
    }

private:
    void dropMap()
    {
        for (slam_vmap_t *m : coarse_) slam_vmap_destroy(m);
        coarse_.clear();
        if (owned_) slam_vmap_destroy(fine_);
        fine_ = nullptr, owned_ = false;
    }
    bool take(slam_vmap_t *fine, bool owned)
    {
        if (!ok() || !fine) return false;
        double                leaf = 0;
        int                   dist = 0;
        slam_vmap_dist_params dp;
        if (slam_vmap_layout(fine, &leaf, nullptr, &dist, &dp) != SLAM_OK) return warn(), false;
        if (!dist) return refuse("the map has no distributions");
        if (!(std::ldexp(leaf, LEVELS - 1) <= 8.0)) return refuse("the coarsest level's leaf is more than the 8 m a map with distributions may have");
        std::vector<slam_vmap_t *> coarse;
        slam_vmap_t               *below = fine;
        bool                       good = true;
        for (int k = 1; k < LEVELS && good; ++k) {
            slam_vmap_params vp;
            slam_vmap_default_params(&vp);
            vp.leaf = std::ldexp(leaf, k);
            slam_vmap_t *m = nullptr;
            good = slam_vmap_create(&vp, &m) == SLAM_OK;
            if (m) coarse.push_back(m);
            good = good && slam_vmap_enable_distributions(m, &dp) == SLAM_OK && slam_vmap_coarsen(m, below, nullptr) == SLAM_OK;
            below = m;
        }
        if (!good) {
            warn();
            for (slam_vmap_t *m : coarse) slam_vmap_destroy(m);
            return false;
        }
        dropMap();
        fine_ = fine, owned_ = owned, coarse_ = coarse;
        return true;
    }
    // the levels from the coarsest down: one call per level carries every live start
    bool descend(int scan, const std::vector<float> &starts, std::vector<char> &alive, int top)
    {
        const int          n_starts = (int)alive.size();
        std::vector<float> T(starts.begin(), starts.begin() + 16 * (size_t)n_starts);
        for (int k = top; k >= 0; --k) {
            std::vector<int>                ids;
            std::vector<slam_vmap_gicp_req> req;
            for (int i = 0; i < n_starts; ++i) {
                if (!alive[(size_t)i]) continue;
                slam_vmap_gicp_req rq;
                rq.src = scan;
                for (int c = 0; c < 16; ++c) rq.init[c] = T[16 * (size_t)i + c];
                ids.push_back(i), req.push_back(rq);
            }
            if (ids.empty()) break;
            double leaf = 0;
            if (slam_vmap_layout(level(k), &leaf, nullptr, nullptr, nullptr) != SLAM_OK) return false;
            slam_vmap_gicp_params gp;
            slam_vmap_default_gicp_params(&gp);
            gp.gate = GATE_RATIO * leaf, gp.max_iterations = MAX_ITERATIONS, gp.transformation_epsilon = TRANSFORMATION_EPSILON;
            std::vector<slam_vmap_gicp_result> res(ids.size());
            if (slam_vmap_register_gicp(level(k), store_, req.data(), (int)req.size(), &gp, res.data(), nullptr) != SLAM_OK) return false;
            for (size_t e = 0; e < ids.size(); ++e) {
                const size_t i = (size_t)ids[e];
                last[(size_t)k][i] = res[e], ran[(size_t)k][i] = 1;
                if (res[e].state == SLAM_KF_NO_CORRESPONDENCES || res[e].state == SLAM_KF_DEGENERATE) alive[i] = 0;
                else
                    for (int c = 0; c < 16; ++c) T[16 * i + c] = res[e].transform[c];
            }
        }
        return true;
    }
    static bool refuse(const char *why)
    {
        std::fprintf(stderr, "MapLocalizer: %s\n", why);
        return false;
    }
    static void warn() { detail::warn("MapLocalizer"); }

    slam_kf_t                 *store_ = nullptr;
    slam_vmap_t               *fine_ = nullptr;
    bool                       owned_ = false;
    std::vector<slam_vmap_t *> coarse_;
};

} // namespace slam_amd
