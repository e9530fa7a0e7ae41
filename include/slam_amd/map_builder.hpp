// slam_amd/map_builder.hpp -- header-only adapter with the shape of global_matching's map builder
// (global_matching/src/global_generate.cpp:122-232) over the C-ABI (slam_mi355x.h: slam_vmap_*, slam_kf_*):
//   laser_callback   :59-80     the first cloud is the map
//   setup_gicp       :82-92     100 iterations, epsilons 1e-6
//   the loop         :122-232   addCloud(): filter scan and map, crop the map around the pose, Generalized ICP of the scan
//                               onto the map, drop the scan on a bad score, otherwise move it and append it to the map
// The map is a slam_vmap_t (exact mean per voxel of everything integrated); the store holds the scan and the cropped map
// for the length of one call.  ROS, the publishers and the .csv stay with the caller.
// slam_amd.api.GlobalMapBuilder is the same thing with Python's names and habits:
//   addCloud -> add_cloud, returning (accepted, result or None) where this sets `last` and `last_valid`;
//   mapKeyframe() -> map_id, cropBox() -> crop_box(), pose() and map() alike, ok() has no twin (the constructor raises);
//   an error of the library is printed here and counts as a rejection, there it raises SlamError (the scan keyframe is
//   removed on both ways out).
// `carve` (default false, fixed at construction; docs/VOXEL_MAP.md section 8): every accepted cloud, the first included, is
// carved with trans_full right after it is integrated, and map() and the cropped map a scan registers against are the carved
// extraction at CARVE_NUM / CARVE_DEN.  While it is false nothing here calls a carve entry point.
// `direct` (default false, fixed at construction; docs/VOXEL_MAP.md section 9): the builder owns a second map of leaf DIST_LEAF
// with plane distributions; every accepted cloud goes into both maps with the same transform, and a later scan is registered
// with slam_vmap_register_gicp straight against the second map's plane voxels from init = trans_full: no extraction, no map
// keyframe (mapKeyframe() stays -1), `last_direct` instead of `last`, and the fitness that is held against MAX_SCORE is the
// point-to-plane score.  map() stays the LEAF_SIZE map.  With carve on as well the second map is carved too and the carved
// rule at CARVE_NUM / CARVE_DEN (as they stand at construction) is part of its plane rule.  While it is false nothing here
// calls an entry point of section 9.
// save(prefix) / resume(prefix) (docs/VOXEL_MAP.md section 10.5): the builder's state as prefix.vmap (slam_vmap_save of the
// map), prefix.dmap (the second map, with `direct`) and prefix.pose (trans_full as 16 little-endian floats, then n_clouds and
// n_accepted as int32).  resume is legal only before the first addCloud and only when the files' leaves, carve state and
// distribution parameters are this builder's; it loads with slam_vmap_load and the loaded handles take the place of the
// builder's own empty ones.  A refusal is printed and returns false with nothing changed (Python raises SlamError).  While
// neither is called nothing of section 10 is called.
//
// Stated deviations (docs/VOXEL_MAP.md section 5):
//   * the start is passed to the solver as `init` instead of moving the source first (:144), so the solver's result is
//     trans_full itself and not a factor of it (:188);
//   * the map is the exact mean per voxel of every point integrated; the reference filters the previous round's centroids
//     again together with the new scan (:135-137, :223), which weights old points by their voxel, not by their number;
//   * the gate is `gate` = 2 m, not 10 (:84): docs/KF_GICP.md section 4's reasoning for refine_gate;
//   * the fitness is gated at the store's gate, not at MAX_DIST (:178); MAX_DIST is kept as a member and unused;
//   * the source is not cropped (:160-168): a scan reaches 100 m at most, so the crop around the pose keeps all of it.
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "slam_amd/buffer.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

class GlobalMapBuilder {
public:
    // global_generate.cpp:21-29, :84-90: macros and setup_gicp's arguments there, members here.  The store and the map are made
    // with them, so all but the two below are fixed at construction (const here, read-only properties in Python).
    const double LEAF_SIZE;
    const double gate;
    const int    MAX_ITERATIONS = 100;
    const double TRANSFORMATION_EPSILON = 1e-6, FITNESS_EPSILON = 1e-6;
    const double MAX_DIST = 4.0; // of getFitnessScore(MAX_DIST), :178: kept for the name, without effect (the store's gate rules)
    // read at every addCloud: may be changed between calls
    double MAX_SCORE = 1.0;
    double CROP_DIST = 100.0;
    // free-space carving: the switch is fixed at construction, the ratio and the parameters are read at every call
    const bool             carve;
    int                    CARVE_NUM = 1, CARVE_DEN = 1; // a voxel stays while miss * CARVE_DEN <= max(seen, 1) * CARVE_NUM
    slam_vmap_carve_params carve_params;
    slam_vmap_carve_result last_carve; // of the last accepted cloud when carve is on
    // registration straight against a second map's plane voxels: fixed at construction
    const bool                direct;
    static constexpr double   DIST_LEAF = 1.0;
    slam_vmap_gicp_result     last_direct; // the last request's result when direct is on (last_valid as for `last`)

    float               trans_full[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int                 n_clouds = 0, n_accepted = 0;
    slam_kf_gicp_result last;            // the last request's result
    bool                last_valid = false; // false for the first cloud and when nothing of the map was near the pose

    explicit GlobalMapBuilder(double leaf = 0.30, double gate_ = 2.0, bool carve_ = false, bool direct_ = false)
        : LEAF_SIZE(leaf), gate(gate_), carve(carve_), last_carve(), direct(direct_), last_direct(), last()
    {
        slam_vmap_default_carve_params(&carve_params);
        slam_vmap_params vp;
        slam_vmap_default_params(&vp);
        vp.leaf = leaf;
        if (slam_vmap_create(&vp, &vmap_) != SLAM_OK) warn(), vmap_ = nullptr;
        slam_kf_params p;
        slam_kf_default_params(&p);
        p.leaf_size = leaf, p.gate = gate_, p.transformation_epsilon = TRANSFORMATION_EPSILON, p.fitness_epsilon = FITNESS_EPSILON;
        slam_kf_gicp_params gp;
        slam_kf_gicp_default_params(&gp);
        gp.max_iterations = MAX_ITERATIONS, gp.transformation_epsilon = TRANSFORMATION_EPSILON;
        if (slam_kf_create(&p, &store_) != SLAM_OK || slam_kf_set_gicp_params(store_, &gp) != SLAM_OK) {
            warn();
            slam_kf_destroy(store_);
            store_ = nullptr;
        }
        if (direct) {
            slam_vmap_dist_params dp;
            slam_vmap_default_dist_params(&dp);
            if (carve) dp.max_miss_num = CARVE_NUM, dp.max_miss_den = CARVE_DEN;
            vp.leaf = DIST_LEAF;
            if (slam_vmap_create(&vp, &dmap_) != SLAM_OK || slam_vmap_enable_distributions(dmap_, &dp) != SLAM_OK) {
                warn();
                slam_vmap_destroy(dmap_);
                dmap_ = nullptr;
            }
        }
    }
    ~GlobalMapBuilder()
    {
        slam_kf_destroy(store_);
        slam_vmap_destroy(dmap_);
        slam_vmap_destroy(vmap_);
    }
    GlobalMapBuilder(const GlobalMapBuilder &) = delete;
    GlobalMapBuilder &operator=(const GlobalMapBuilder &) = delete;
    bool         ok() const { return vmap_ && store_ && (dmap_ || !direct); }
    slam_vmap_t *vmap() { return vmap_; }
    slam_vmap_t *distMap() { return dmap_; } // the DIST_LEAF map of direct mode, NULL otherwise
    slam_kf_t   *store() { return store_; }
    int          mapKeyframe() const { return map_id_; }
    const float *pose() const { return trans_full; }
    // :149-157: -+CROP_DIST around the pose, the limits in double rounded to float once
    void cropBox(float lo[2], float hi[2]) const
    {
        for (int k = 0; k < 2; ++k) {
            lo[k] = (float)(-CROP_DIST + (double)trans_full[4 * k + 3]);
            hi[k] = (float)(CROP_DIST + (double)trans_full[4 * k + 3]);
        }
    }

    // One scan (sensor frame, `stride` >= 3 floats per point).  True when it was integrated into the map; `last` holds the
    // request's result when last_valid.  An error of the library is printed and counts as a rejection.
    bool addCloud(const float *xyz, int n, int stride)
    {
        if (!ok() || n <= 0 || stride < 3 || !xyz) return false;
        ++n_clouds;
        last_valid = false;
        int64_t n_points = 0, n_voxels = 0;
        if (slam_vmap_info(vmap_, &n_voxels, nullptr, &n_points, nullptr) != SLAM_OK) return warn(), false;
        if (n_points == 0) { // :63-70: the first cloud is the map
            if (slam_vmap_integrate(vmap_, xyz, n, stride, nullptr, nullptr, nullptr) != SLAM_OK) return warn(), false;
            if (carve && slam_vmap_carve(vmap_, xyz, n, stride, nullptr, nullptr, nullptr, &carve_params, &last_carve) != SLAM_OK) return warn(), false;
            if (direct) {
                if (slam_vmap_integrate(dmap_, xyz, n, stride, nullptr, nullptr, nullptr) != SLAM_OK) return warn(), false;
                if (carve && slam_vmap_carve(dmap_, xyz, n, stride, nullptr, nullptr, nullptr, &carve_params, nullptr) != SLAM_OK) return warn(), false;
            }
            ++n_accepted;
            return true;
        }
        const size_t scan_bytes = sizeof(float) * (size_t)n * stride;
        if (!detail::reserve_quarter(d_scan_, scan_bytes) || slam_memcpy_h2d(d_scan_.p, xyz, scan_bytes, nullptr) != SLAM_OK) return warn(), false;
        int scan = -1;
        if (slam_kf_add_keyframe_dev(store_, d_scan_.as<float>(), n, stride, &scan, nullptr) != SLAM_OK) return warn(), false;
        const bool accepted = registerAndIntegrate(scan, n, stride, (int)n_voxels);
        if (slam_kf_remove_keyframe(store_, scan) != SLAM_OK) warn(); // the store holds two keyframes at most
        if (accepted) ++n_accepted;
        return accepted;
    }

    // the whole map as GlobalMatcher::setMap takes it: (x, y, z, 0) per voxel in key order, stride 4
    std::vector<float> map()
    {
        std::vector<float> out;
        int64_t            n_voxels = 0;
        if (!ok() || slam_vmap_info(vmap_, &n_voxels, nullptr, nullptr, nullptr) != SLAM_OK || n_voxels == 0) return out;
        out.resize(4 * (size_t)n_voxels);
        int n = 0;
        const int rc = carve ? slam_vmap_read_carved(vmap_, nullptr, nullptr, 0, CARVE_NUM, CARVE_DEN, out.data(), nullptr, nullptr, (int)n_voxels, &n)
                             : slam_vmap_read(vmap_, nullptr, nullptr, 0, out.data(), nullptr, nullptr, (int)n_voxels, &n);
        if (rc != SLAM_OK) warn(), n = 0;
        out.resize(4 * (size_t)n);
        return out;
    }

    // prefix.vmap, prefix.dmap with `direct`, prefix.pose: the same bytes as the Python twin writes
    bool save(const std::string &prefix)
    {
        if (!ok()) return false;
        if (slam_vmap_save(vmap_, (prefix + ".vmap").c_str()) != SLAM_OK) return warn(), false;
        if (direct && slam_vmap_save(dmap_, (prefix + ".dmap").c_str()) != SLAM_OK) return warn(), false;
        unsigned char pose[72]; // little-endian hosts only, as the library
        const int32_t n[2] = {n_clouds, n_accepted};
        std::memcpy(pose, trans_full, 64), std::memcpy(pose + 64, n, 8);
        std::FILE *f = std::fopen((prefix + ".pose").c_str(), "wb");
        const bool written = f && std::fwrite(pose, 1, sizeof pose, f) == sizeof pose;
        if ((f && std::fclose(f) != 0) || !written) return refuse(prefix, ".pose cannot be written");
        return true;
    }
    bool resume(const std::string &prefix)
    {
        if (!ok()) return false;
        if (n_clouds != 0) return refuse(prefix, ": resume is legal only on a builder that has added no cloud");
        if (!direct) {
            if (std::FILE *f = std::fopen((prefix + ".dmap").c_str(), "rb")) {
                std::fclose(f);
                return refuse(prefix, ".dmap exists: saved by a direct builder, this one is not");
            }
        }
        unsigned char pose[73];
        std::FILE    *f = std::fopen((prefix + ".pose").c_str(), "rb");
        const size_t  got = f ? std::fread(pose, 1, sizeof pose, f) : 0;
        if (f) std::fclose(f);
        if (got != 72) return refuse(prefix, ".pose cannot be read or does not hold 72 bytes");
        slam_vmap_t *loaded[2] = {nullptr, nullptr};
        bool         good = slam_vmap_load((prefix + ".vmap").c_str(), &loaded[0]) == SLAM_OK && sameLayout(loaded[0], vmap_);
        if (good && direct) good = slam_vmap_load((prefix + ".dmap").c_str(), &loaded[1]) == SLAM_OK && sameLayout(loaded[1], dmap_);
        if (!good) {
            slam_vmap_destroy(loaded[0]);
            slam_vmap_destroy(loaded[1]);
            return refuse(prefix, ": a file cannot be loaded, or was saved with another leaf, carve state or distribution parameters");
        }
        slam_vmap_destroy(vmap_);
        vmap_ = loaded[0];
        if (direct) slam_vmap_destroy(dmap_), dmap_ = loaded[1];
        int32_t n[2];
        std::memcpy(trans_full, pose, 64), std::memcpy(n, pose + 64, 8);
        n_clouds = n[0], n_accepted = n[1];
        return true;
    }

private:
    // a loaded map against the builder's own empty one: the leaf's bits, the carve state of construction, the distributions
    bool sameLayout(slam_vmap_t *file, slam_vmap_t *own) const
    {
        double                leaf[2];
        int                   carved[2], dist[2];
        slam_vmap_dist_params a, b;
        if (slam_vmap_layout(file, &leaf[0], &carved[0], &dist[0], &a) != SLAM_OK || slam_vmap_layout(own, &leaf[1], &carved[1], &dist[1], &b) != SLAM_OK)
            return warn(), false;
        const bool same_dp = a.min_points == b.min_points && a.flat_ratio == b.flat_ratio && a.line_ratio == b.line_ratio && a.epsilon == b.epsilon &&
                             a.max_miss_num == b.max_miss_num && a.max_miss_den == b.max_miss_den;
        return std::memcmp(&leaf[0], &leaf[1], sizeof(double)) == 0 && (carved[0] != 0) == carve && dist[0] == dist[1] && same_dp;
    }
    static bool refuse(const std::string &prefix, const char *why)
    {
        std::fprintf(stderr, "GlobalMapBuilder: %s%s\n", prefix.c_str(), why);
        return false;
    }
    // direct mode: the scan against the plane voxels of the DIST_LEAF map; fills last_direct and the verdict of :182
    bool registerDirect(int scan)
    {
        slam_vmap_gicp_req rq;
        rq.src = scan;
        for (int k = 0; k < 16; ++k) rq.init[k] = trans_full[k];
        slam_vmap_gicp_params gp;
        slam_vmap_default_gicp_params(&gp);
        gp.gate = gate, gp.max_iterations = MAX_ITERATIONS, gp.transformation_epsilon = TRANSFORMATION_EPSILON;
        if (slam_vmap_register_gicp(dmap_, store_, &rq, 1, &gp, &last_direct, nullptr) != SLAM_OK) return warn(), false;
        last_valid = true;
        if (last_direct.fitness_pairs <= 0 || !last_direct.converged || last_direct.fitness > MAX_SCORE) return false;
        for (int k = 0; k < 16; ++k) trans_full[k] = last_direct.transform[k];
        return true;
    }
    // the accepted scan, moved by trans_full, into the map (and the second one of direct mode), carved when carve is on
    bool integrateAccepted(int n, int stride)
    {
        double R[9], t[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)trans_full[4 * r + c];
            t[r] = (double)trans_full[4 * r + 3];
        }
        if (slam_vmap_integrate_dev(vmap_, d_scan_.as<float>(), n, stride, R, t, nullptr, nullptr) != SLAM_OK) return warn(), false;
        if (direct && slam_vmap_integrate_dev(dmap_, d_scan_.as<float>(), n, stride, R, t, nullptr, nullptr) != SLAM_OK) return warn(), false;
        if (carve && slam_vmap_carve_dev(vmap_, d_scan_.as<float>(), n, stride, R, t, nullptr, &carve_params, &last_carve, nullptr) != SLAM_OK)
            return warn(), false;
        if (carve && direct && slam_vmap_carve_dev(dmap_, d_scan_.as<float>(), n, stride, R, t, nullptr, &carve_params, nullptr, nullptr) != SLAM_OK)
            return warn(), false;
        return true;
    }
    bool registerAndIntegrate(int scan, int n, int stride, int n_voxels)
    {
        if (direct) return registerDirect(scan) && integrateAccepted(n, stride);
        float lo[2], hi[2]; // the map inside the crop box
        cropBox(lo, hi);
        const int   cap = n_voxels > 0 ? n_voxels : 1;
        int         n_map = 0;
        if (!detail::reserve_quarter(d_map_, sizeof(float) * 4 * (size_t)cap)) return warn(), false;
        const int rx = carve ? slam_vmap_extract_carved_dev(vmap_, lo, hi, 0, CARVE_NUM, CARVE_DEN, d_map_.as<float>(), nullptr, nullptr, cap, &n_map, nullptr)
                             : slam_vmap_extract_dev(vmap_, lo, hi, 0, d_map_.as<float>(), nullptr, nullptr, cap, &n_map, nullptr);
        if (rx != SLAM_OK) return warn(), false;
        if (slam_device_synchronize() != SLAM_OK) return warn(), false;
        if (n_map == 0) return false; // nothing of the map near the pose: nothing to register against
        const int rc = map_id_ < 0 ? slam_kf_add_keyframe_dev(store_, d_map_.as<float>(), n_map, 4, &map_id_, nullptr)
                                   : slam_kf_replace_keyframe_dev(store_, map_id_, d_map_.as<float>(), n_map, 4, nullptr);
        if (rc != SLAM_OK) return warn(), false;
        slam_kf_edge_req rq;
        rq.from = map_id_, rq.to = scan;
        for (int k = 0; k < 16; ++k) rq.init[k] = trans_full[k];
        if (slam_kf_register_gicp(store_, &rq, 1, &last, nullptr) != SLAM_OK) return warn(), false;
        last_valid = true;
        if (last.fitness_pairs <= 0 || !last.edge.converged || last.fitness > MAX_SCORE) return false; // :182
        for (int k = 0; k < 16; ++k) trans_full[k] = last.edge.transform[k];
        return integrateAccepted(n, stride);
    }
    static void warn() { detail::warn("GlobalMapBuilder"); }

    slam_vmap_t         *vmap_ = nullptr, *dmap_ = nullptr;
    slam_kf_t           *store_ = nullptr;
    detail::DeviceBuffer d_scan_, d_map_;
    int                  map_id_ = -1;
};

} // namespace slam_amd
