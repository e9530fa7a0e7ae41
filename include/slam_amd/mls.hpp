// slam_amd/mls.hpp -- header-only adapter with the shape of class MLS
// (mls/include/mls/mls.h:104-242) in the rolling / occupancy mode local_mapper
// uses (local_mapper.cpp:29,86,107), over the C-ABI (slam_mi355x.h).
//
// The reference takes PCL clouds and geometry_msgs poses and runs the ground
// segmentation inside addToOccupancy (mls.cpp:59-67).  Both levels are here:
//   addToOccupancy(cloud_xyz, n, stride)            the one-cloud form: segmentGround on the device
//                                                   (slam_gseg_*), split into drv / ground clouds, the two
//                                                   point loops of mls.cpp:73-142 in their order, and the
//                                                   drv cloud appended to global_cloud (:144-149);
//   addToOccupancy(obstacle, n, ground, n, stride)  below the segmentation, for callers that have the
//                                                   segmented clouds already (PointXYZGD = 8 floats).
// Clouds are float arrays (x, y, z first, `stride` floats per point), poses the Pose struct of slam_amd/pose.hpp
// (the pose part of geometry_msgs::PoseStamped).  getDrivability() fills a struct laid out like
// nav_msgs/OccupancyGrid (mls.h:167-175): data[x + size_x*y] in {-1, 0, 100}, origin -res*size/2.
// global_cloud lives on the host, as the reference's PCL cloud does.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

#include "slam_amd/buffer.hpp"
#include "slam_amd/pose.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

// pcl::VoxelGrid(xy, xy, z) on a host cloud (x, y, z per point): one centroid per occupied voxel, in increasing voxel index
// (x fastest), the lattice anchored at the cloud's minimum as PCL anchors it -- what filterPointCloud (here and in
// mls_map.hpp) falls back to for a lattice beyond the device filter's accumulator
inline void voxel_filter_host(std::vector<float> &cloud, double xy, double z)
{
    const size_t n = cloud.size() / 3;
    if (!n) return;
    float mn[3] = {cloud[0], cloud[1], cloud[2]}, mx[3] = {mn[0], mn[1], mn[2]};
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            mn[k] = std::min(mn[k], cloud[3 * i + k]);
            mx[k] = std::max(mx[k], cloud[3 * i + k]);
        }
    const float inv[3] = {(float)(1.0 / xy), (float)(1.0 / xy), (float)(1.0 / z)};
    long        lo[3], div[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = (long)std::floor(mn[k] * inv[k]);
        div[k] = (long)std::floor(mx[k] * inv[k]) - lo[k] + 1;
    }
    struct Acc {
        double s[3] = {0, 0, 0};
        long   n = 0;
    };
    std::map<long, Acc> vox;
    for (size_t i = 0; i < n; ++i) {
        long idx = 0, mul = 1;
        for (int k = 0; k < 3; ++k) {
            idx += ((long)std::floor(cloud[3 * i + k] * inv[k]) - lo[k]) * mul;
            mul *= div[k];
        }
        Acc &a = vox[idx];
        for (int k = 0; k < 3; ++k) a.s[k] += cloud[3 * i + k];
        ++a.n;
    }
    cloud.clear();
    for (const auto &kv : vox)
        for (int k = 0; k < 3; ++k) cloud.push_back((float)(kv.second.s[k] / (double)kv.second.n));
}

struct GridInfo { // nav_msgs::MapMetaData, what MLS fills of it
    double   resolution = 0;
    uint32_t width = 0, height = 0;
    double   origin_x = 0, origin_y = 0;
};

struct OccupancyGrid { // the fields of nav_msgs::OccupancyGrid that MLS fills
    GridInfo            info;
    std::vector<int8_t> data;
};

// The costmap of a drivability plane (slam_gdist_*, docs/GRID_DIST.md; the reference has none): per cell, data[x + width*y], the
// squared distance in cells to the nearest obstacle cell (SLAM_GDIST_FAR beyond max_cells) and the inflated cost byte
// (costmap_2d's scale: 254 lethal, 253 inscribed, 255 unknown, 0 free).
struct Costmap {
    GridInfo              info;
    std::vector<uint8_t>  cost;
    std::vector<uint16_t> dist2;
};

// RAII over slam_gdist_t.  A failed construction logs and leaves an unusable object (ok() == false), as the other adapters do.
class DistanceField {
public:
    DistanceField(int size_x, int size_y, const slam_gdist_params *params = nullptr)
    {
        if (slam_gdist_create(size_x, size_y, params, &h_) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            h_ = nullptr;
            return;
        }
        slam_gdist_default_params(&prm_);
        if (params) prm_ = *params;
        cells_ = (size_t)size_x * size_y;
    }
    ~DistanceField() { slam_gdist_destroy(h_); }
    DistanceField(const DistanceField &) = delete;
    DistanceField &operator=(const DistanceField &) = delete;

    bool ok() const { return h_ != nullptr; }
    bool setTable(const std::vector<uint8_t> &table) { return h_ && good(slam_gdist_set_table(h_, table.data(), (int)table.size())); }
    // costmap_2d's inflation curve for this handle's max_cells (slam_grid_inflation_table)
    bool setInflation(double resolution, double inscribed_radius, double inflation_radius, double cost_scaling)
    {
        if (!h_) return false;
        std::vector<uint8_t> t((size_t)prm_.max_cells * prm_.max_cells + 2);
        return good(slam_grid_inflation_table(resolution, inscribed_radius, inflation_radius, cost_scaling, prm_.max_cells, t.data(), (int)t.size())) &&
               setTable(t);
    }
    bool compute(const int8_t *occ) { return h_ && good(slam_gdist_compute(h_, occ)); }
    bool computeDev(const int8_t *d_occ, slam_stream_t stream) { return h_ && good(slam_gdist_compute_dev(h_, d_occ, stream)); }
    bool computeFromGrid(slam_grid_t *grid, slam_stream_t stream = nullptr) { return h_ && grid && good(slam_grid_distance_field(grid, h_, stream)); }
    // either vector may be null; they are sized here
    bool read(std::vector<uint16_t> *dist2, std::vector<uint8_t> *cost)
    {
        if (!h_) return false;
        if (dist2) dist2->resize(cells_);
        if (cost) cost->resize(cells_);
        return good(slam_gdist_read(h_, dist2 ? dist2->data() : nullptr, cost ? cost->data() : nullptr));
    }
    const slam_gdist_params &params() const { return prm_; }
    slam_gdist_t            *handle() { return h_; }

private:
    static bool good(int rc)
    {
        if (rc != SLAM_OK) std::fprintf(stderr, "%s\n", slam_last_error());
        return rc == SLAM_OK;
    }
    slam_gdist_t     *h_ = nullptr;
    slam_gdist_params prm_ = {};
    size_t            cells_ = 0;
};

// A path down a navigation field (slam_gnav_*, docs/GRID_NAV.md; the reference has no planner): window cells (x, y) from the
// start to the goal, the same cells as world points at their centres, and one of slam_mi355x.h's SLAM_GNAV_PATH_* statuses.
struct NavPath {
    int                  status = SLAM_GNAV_PATH_NOT_CONVERGED;
    std::vector<int32_t> cells;  // 2 per cell
    std::vector<double>  points; // 2 per cell
};

// slam_gnav_params at the library's defaults, or with other move weights
struct NavParams : slam_gnav_params {
    NavParams() { slam_gnav_default_params(this); }
    NavParams(int orth, int diag) : NavParams() { orth_w = orth, diag_w = diag; }
};

// RAII over slam_gnav_t.  A failed construction logs and leaves an unusable object (ok() == false), as the other adapters do.
class NavField {
public:
    NavField(int size_x, int size_y, int orth_w, int diag_w) : NavField(size_x, size_y, NavParams(orth_w, diag_w)) {}
    NavField(int size_x, int size_y, const NavParams &p = NavParams())
    {
        if (slam_gnav_create(size_x, size_y, &p, &h_) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            h_ = nullptr;
            return;
        }
        cells_ = (size_t)size_x * size_y;
    }
    ~NavField()
    {
        slam_device_synchronize(); // (the goal block goes with its member, behind this wait)
        slam_gnav_destroy(h_);
    }
    NavField(const NavField &) = delete;
    NavField &operator=(const NavField &) = delete;

    bool ok() const { return h_ != nullptr; }
    bool setTable(const std::vector<uint32_t> &table) { return h_ && good(slam_gnav_set_table(h_, table.data(), (int)table.size())); }
    // the default curve: neutral + cost below lethal_from, closed from there on, unknown cells (255) at unknown_step (0: closed)
    bool setSteps(int neutral, int lethal_from, int unknown_step)
    {
        std::vector<uint32_t> t(256);
        return h_ && good(slam_grid_step_table(neutral, lethal_from, unknown_step, t.data(), (int)t.size())) && setTable(t);
    }
    // host plane and host goals (x, y pairs), to convergence
    bool compute(const uint8_t *cost, const std::vector<int32_t> &goals, int max_rounds = 0)
    {
        return h_ && good(slam_gnav_compute(h_, cost, goals.data(), (int)(goals.size() / 2), max_rounds));
    }
    bool computeDev(const uint8_t *d_cost, const int32_t *d_goals, int n_goals, int rounds, bool restart, slam_stream_t stream)
    {
        return h_ && good(slam_gnav_compute_dev(h_, d_cost, d_goals, n_goals, rounds, restart ? 1 : 0, stream));
    }
    // over the cost plane of a distance field computed on `grid`, to convergence: rounds in batches, the state read per batch
    bool computeFromGrid(slam_grid_t *grid, DistanceField &df, const std::vector<int32_t> &goals)
    {
        const int n = (int)(goals.size() / 2), batch = 16;
        if (!h_ || !grid || !df.ok() || n < 1 || !d_goals_.reserve(sizeof(int32_t) * goals.size())) return false;
        if (!good(slam_memcpy_h2d(d_goals_.p, goals.data(), sizeof(int32_t) * 2 * (size_t)n, nullptr))) return false;
        if (!good(slam_grid_nav_field(grid, df.handle(), h_, d_goals_.as<int32_t>(), n, batch, nullptr))) return false;
        for (size_t done = batch;; done += batch) {
            slam_gnav_state st;
            if (!state(st)) return false;
            if (st.converged) return true;
            if (done > cells_) return false; // (cells + 1 rounds always suffice)
            uint8_t *d_cost = nullptr;
            if (!good(slam_gdist_planes_dev(df.handle(), nullptr, &d_cost)) || !d_cost) return false;
            if (!computeDev(d_cost, d_goals_.as<int32_t>(), n, batch, false, nullptr)) return false;
        }
    }
    bool read(std::vector<uint32_t> *pot)
    {
        if (!h_ || !pot) return false;
        pot->resize(cells_);
        return good(slam_gnav_read(h_, pot->data()));
    }
    // window cells from (sx, sy) down the field; max_len 0: the plane's cell count, which no path exceeds
    bool path(int sx, int sy, std::vector<int32_t> *cells, int *status, int max_len = 0)
    {
        if (!h_ || !cells || !status) return false;
        const size_t room = max_len > 0 ? (size_t)max_len : cells_;
        cells->resize(2 * room);
        int len = 0;
        if (!good(slam_gnav_path(h_, sx, sy, (int)room, cells->data(), &len, status))) return false;
        cells->resize(2 * (size_t)len);
        return true;
    }
    bool state(slam_gnav_state &s) { return h_ && good(slam_gnav_read_state(h_, &s)); }
    slam_gnav_t *handle() { return h_; }

private:
    static bool good(int rc)
    {
        if (rc != SLAM_OK) std::fprintf(stderr, "%s\n", slam_last_error());
        return rc == SLAM_OK;
    }
    slam_gnav_t         *h_ = nullptr;
    size_t               cells_ = 0;
    detail::DeviceBuffer d_goals_;
};

class MLS {
public:
    // mls.h:154: MLS(int size_x_, int size_y_, double res, bool roll, double robot_size = 1.45)
    MLS(int size_x_, int size_y_, double res, bool roll, double /*robot_size*/ = 1.45)
    {
        slam_grid_params p;
        slam_grid_default_params(&p);
        p.rolling = roll ? 1 : 0;
        rolling_ = roll;
        if (slam_grid_create(size_x_, size_y_, res, &p, &h_) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            h_ = nullptr;
        }
        grid_.info.resolution = res;
        grid_.info.width = (uint32_t)size_x_;
        grid_.info.height = (uint32_t)size_y_;
        grid_.info.origin_x = -(res * size_x_ / 2); // mls.h:171-172
        grid_.info.origin_y = -(res * size_y_ / 2);
        grid_.data.assign((size_t)size_x_ * size_y_, (int8_t)-1);
    }
    ~MLS()
    {
        slam_device_synchronize(); // (the buffers go with their members, behind this wait)
        slam_ccicp_destroy(cc_);
        slam_gseg_destroy(gseg_);
        slam_grid_destroy(h_);
    }
    MLS(const MLS &) = delete;
    MLS &operator=(const MLS &) = delete;

    void clearMap()                                                                           // mls.cpp:18-31
    {
        if (h_) slam_grid_clear(h_, nullptr);
        global_cloud_.clear();
    }
    void setPose(double x, double y)                                                          // mls.cpp:408-479
    {
        if (!h_) return;
        double x0 = 0, y0 = 0;
        slam_grid_get_pose(h_, &x0, &y0);
        slam_grid_set_pose(h_, x, y, nullptr);
        double x1 = 0, y1 = 0;
        slam_grid_get_pose(h_, &x1, &y1);
        if (rolling_ && !disable_pointcloud_ && (x1 != x0 || y1 != y0)) {
            // global_cloud follows the window (:433-454): shift by -dx*res, -dy*res, then PassThrough x, y within
            // +-min(size)*res/2 (float limits, closed interval)
            const float sx = (float)-(x1 - x0), sy = (float)-(y1 - y0);
            const float crop = (float)(std::min(grid_.info.width, grid_.info.height) * grid_.info.resolution / 2);
            size_t      k = 0;
            for (size_t i = 0; i + 2 < global_cloud_.size(); i += 3) {
                const float px = global_cloud_[i] + sx, py = global_cloud_[i + 1] + sy, pz = global_cloud_[i + 2];
                if (px >= -crop && px <= crop && py >= -crop && py <= crop) {
                    global_cloud_[k] = px, global_cloud_[k + 1] = py, global_cloud_[k + 2] = pz;
                    k += 3;
                }
            }
            global_cloud_.resize(k);
        }
    }
    void setPose(const Pose &p) { setPose(p.x, p.y); }
    // mls.cpp:59-150, the one-cloud form: segmentGround (groundSegmentation.cpp:91-468) on the device, the drv
    // (obstacle below robot height) and ground clouds, then the two point loops in the reference's order
    void addToOccupancy(const float *cloud_xyz, int n, int stride = 3) { add_cloud(cloud_xyz, n, stride, nullptr, nullptr); }
    // ... of the cloud as it is (R null) or turned by R (row-major) and offset by t first
    void add_cloud(const float *cloud_xyz, int n, int stride, const double *R, const double *t)
    {
        if (!h_ || n <= 0) return;
        if (!gseg_ && slam_gseg_create(nullptr, &gseg_) != SLAM_OK) return warn();
        if (n > cap_) { // one capacity, in points, for four blocks: they grow together or not at all
            const int c = n + n / 4;
            cap_ = 0;
            if (!(d_cloud_.reserve(sizeof(float) * (size_t)c * 8) && d_labels_.reserve((size_t)c) && d_gnd_.reserve(16 * (size_t)c) &&
                  d_obs_.reserve(16 * (size_t)c))) {
                for (detail::DeviceBuffer *b : {&d_cloud_, &d_labels_, &d_gnd_, &d_obs_}) b->release();
                return warn();
            }
            cap_ = c;
        }
        if (!d_counts_.reserve(16)) return warn();
        if (stride > 8) return (void)std::fprintf(stderr, "MLS::addToOccupancy: stride %d > 8 floats\n", stride);
        // the cloud as it came, behind the place the segmentation reads (d_cloud_ holds 8 floats per point: a turned copy of at
        // most 3 in front, the upload of at most 5 ... 8 behind it when a transform is asked for)
        const bool turn = R != nullptr;
        float     *d_up = turn ? d_cloud_.as<float>() + 3 * (size_t)cap_ : d_cloud_.as<float>();
        if (turn && stride > 5) return (void)std::fprintf(stderr, "MLS::addToMap: stride %d > 5 floats\n", stride);
        if (slam_memcpy_h2d(d_up, cloud_xyz, sizeof(float) * (size_t)n * stride, nullptr) != SLAM_OK) return warn();
        if (turn) { // mls.cpp:34-53 on the device (round 6: the host loop was 0.15 of a cloud's 0.35 ms)
            if (slam_grid_transform_cloud_dev(d_up, n, stride, R, t, d_cloud_.as<float>(), nullptr) != SLAM_OK) return warn();
            stride = 3;
        }
        if (slam_gseg_segment_dev(gseg_, d_cloud_.as<float>(), n, stride, d_labels_.as<uint8_t>(), nullptr) != SLAM_OK) return warn();
        if (slam_gseg_split_dev(gseg_, d_cloud_.as<float>(), n, stride, d_labels_.as<uint8_t>(), d_gnd_.as<float>(), d_obs_.as<float>(),
                                d_counts_.as<int32_t>(), nullptr) != SLAM_OK)
            return warn();
        // the two counts, and the drv cloud where global_cloud is kept, come back into PINNED memory (a read-back into pageable
        // memory is staged by the runtime: 0.1 ms for the cloud's 300 KB)
        if (!detail::reserve_half(h_pin_, 64)) return warn();
        int32_t *counts = h_pin_.as<int32_t>(); // ground, obstacle
        if (slam_memcpy_d2h(counts, d_counts_.p, 2 * sizeof(int32_t), nullptr) != SLAM_OK) return warn();
        const int32_t n_gnd = counts[0], n_drv = counts[1];
        const float  *drv_ = nullptr;
        if (!disable_pointcloud_ && n_drv > 0) { // *global_cloud += drv_cloud (:144-149): read back BEFORE the grid update is
            if (!detail::reserve_half(h_pin_, 64 + 16 * (size_t)n_drv)) return warn(); // enqueued (it runs while the host appends)
            drv_ = reinterpret_cast<const float *>(h_pin_.as<unsigned char>() + 64);
            if (slam_memcpy_d2h(h_pin_.as<unsigned char>() + 64, d_obs_.p, 16 * (size_t)n_drv, nullptr) != SLAM_OK) return warn();
        }
        counts = nullptr; // (the reserve may have moved the block)
        if (slam_grid_add_scan_inorder_dev(h_, d_obs_.as<float>(), n_drv, d_gnd_.as<float>(), n_gnd, 4, nullptr) != SLAM_OK)
            return warn();
        if (drv_) {
            const size_t at = global_cloud_.size();
            global_cloud_.resize(at + 3 * (size_t)n_drv);
            float *dst = global_cloud_.data() + at;
            for (int i = 0; i < n_drv; ++i) {
                dst[3 * (size_t)i] = drv_[4 * (size_t)i];
                dst[3 * (size_t)i + 1] = drv_[4 * (size_t)i + 1];
                dst[3 * (size_t)i + 2] = drv_[4 * (size_t)i + 2];
            }
        }
        last_counts_[0] = n_drv;
        last_counts_[1] = n_gnd;
    }
    // mls.cpp:34-53: setPose, then (rolling) the cloud turned into the global orientation and offset by the
    // sub-cell residual curPose - pose (tf::poseMsgToEigen + pcl::transformPointCloud: computed in double, stored
    // as float), then addToOccupancy of that cloud
    void addToMap(const float *cloud_xyz, int n, int stride, const Pose &pose)
    {
        setPose(pose);
        if (!h_ || n <= 0) return;
        if (!rolling_) return addToOccupancy(cloud_xyz, n, stride);
        double cx = 0, cy = 0;
        slam_grid_get_pose(h_, &cx, &cy);
        const double tx = cx - pose.x, ty = cy - pose.y, tz = pose.z;
        double       r[9];
        detail::tf_matrix(pose, r);
        // (float)(r0 x + r1 y + r2 z + t) per coordinate, in double: slam_grid_transform_cloud_dev, the same floats as the host loop
        // this was until round 6 (tests/test_gpu_cpp_adapters.py holds the map against the oracle's, which transforms on the host)
        const double t3[3] = {tx, ty, tz};
        if (stride <= 5) return add_cloud(cloud_xyz, n, stride, r, t3);
        trans_.resize(3 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            const double px = cloud_xyz[(size_t)i * stride], py = cloud_xyz[(size_t)i * stride + 1], pz = cloud_xyz[(size_t)i * stride + 2];
            trans_[3 * (size_t)i] = (float)(r[0] * px + r[1] * py + r[2] * pz + tx);
            trans_[3 * (size_t)i + 1] = (float)(r[3] * px + r[4] * py + r[5] * pz + ty);
            trans_[3 * (size_t)i + 2] = (float)(r[6] * px + r[7] * py + r[8] * pz + tz);
        }
        addToOccupancy(trans_.data(), n, 3);
    }
    // mls.cpp:481-505: the z offset from graph_slam; the occupancy mode keeps no heights, global_cloud moves
    void offsetMap(const Pose &pose)
    {
        if (disable_pointcloud_) return;
        for (size_t i = 2; i < global_cloud_.size(); i += 3) global_cloud_[i] += (float)pose.z;
    }
    // mls.cpp:508-518: pcl::VoxelGrid(xy, xy, z) over global_cloud: one centroid per occupied voxel, in increasing
    // voxel index (x fastest), the voxel lattice anchored at the cloud's minimum as PCL anchors it
    void filterPointCloud(double xy, double z)
    {
        const size_t n = global_cloud_.size() / 3;
        if (!n) return;
        // On the device (round 6): local_mapper filters its global cloud behind EVERY cloud (local_mapper.cpp:111), and the host
        // filter below -- an ordered map over 90 000 points -- was 4.3 of a cloud's 4.6 ms.  The library's pcl::VoxelGrid
        // (slam_ccicp_voxel_downsample_dev: the same lattice and order, centroids from exact 64-bit sums) takes the cloud as it
        // lies; a lattice beyond its accumulator (a stray point far off) falls back to the host.
        if (filter_on_device(xy, z)) return;
        filter_on_host(xy, z);
    }
    bool filter_on_device(double xy, double z)
    {
        const size_t n = global_cloud_.size() / 3;
        if (n > (size_t)1 << 30) return false;
        if (!cc_ && slam_ccicp_create(&cc_) != SLAM_OK) return false;
        if (!detail::reserve_half(d_gc_in_, 12 * n) || !detail::reserve_half(d_gc_out_, 16 * n)) return false;
        if (!detail::reserve_half(h_pin_, 64 + 16 * n)) return false;
        if (slam_memcpy_h2d(d_gc_in_.p, global_cloud_.data(), 12 * n, nullptr) != SLAM_OK) return false;
        int n_out = 0;
        if (slam_ccicp_voxel_downsample_dev(cc_, d_gc_in_.as<float>(), nullptr, (int)n, 3, (float)xy, (float)xy, (float)z, d_gc_out_.as<float>(),
                                            (int)n, &n_out, nullptr) != SLAM_OK)
            return false;
        float *rec = reinterpret_cast<float *>(h_pin_.as<unsigned char>() + 64);
        if (n_out > 0 && slam_memcpy_d2h(rec, d_gc_out_.p, 16 * (size_t)n_out, nullptr) != SLAM_OK) return false;
        global_cloud_.resize(3 * (size_t)n_out);
        for (int i = 0; i < n_out; ++i)
            for (int k = 0; k < 3; ++k) global_cloud_[3 * (size_t)i + k] = rec[4 * (size_t)i + k];
        return true;
    }
    void filter_on_host(double xy, double z) { voxel_filter_host(global_cloud_, xy, z); }
    const std::vector<float> &getGlobalCloud() const { return global_cloud_; }                // mls.h:216 (x, y, z per point)
    void setDisablePointCloud(bool v) { disable_pointcloud_ = v; }                            // mls.h:223
    const int *lastSegmentCounts() const { return last_counts_; }                             // drv, ground points of the last cloud
    // mls.cpp:59-150 below the segmentation: obstacle points +1.0, ground points -0.3, in that order
    void addToOccupancy(const float *obstacle, int n_obstacle, const float *ground, int n_ground, int stride = 8)
    {
        if (h_ && slam_grid_add_scan_inorder(h_, obstacle, n_obstacle, ground, n_ground, stride) != SLAM_OK)
            std::fprintf(stderr, "%s\n", slam_last_error());
    }
    // mls.cpp:34-53 (rolling branch): setPose, then the points (already rotated into the
    // global orientation and offset by the sub-cell residual, as mls.cpp:41-47 does with PCL)
    void addToMap(const float *obstacle, int n_obstacle, const float *ground, int n_ground, double pose_x,
                  double pose_y, int stride = 8)
    {
        setPose(pose_x, pose_y);
        addToOccupancy(obstacle, n_obstacle, ground, n_ground, stride);
    }
    const OccupancyGrid &getDrivability()                                                    // mls.h:215
    {
        if (h_) slam_grid_read_occupancy(h_, grid_.data.data());
        return grid_;
    }
    // Opt-in costmap (not in the reference, where robot_size only sets a height): from here on getCostmap() inflates the
    // drivability plane by costmap_2d's curve, radii in metres, distances capped at max_cells cells.  Nothing is allocated and
    // nothing changes without this call; false (logged) when the arguments or the device refuse.
    bool enableCostmap(double inscribed_radius, double inflation_radius, double cost_scaling, int max_cells = 32)
    {
        if (!h_) return false;
        slam_gdist_params p;
        slam_gdist_default_params(&p);
        p.max_cells = max_cells;
        std::unique_ptr<DistanceField> df(new DistanceField((int)grid_.info.width, (int)grid_.info.height, &p));
        if (!df->ok() || !df->setInflation(grid_.info.resolution, inscribed_radius, inflation_radius, cost_scaling)) return false;
        df_ = std::move(df);
        costmap_.info = grid_.info;
        return true;
    }
    // getDrivability()'s state -> slam_grid_distance_field -> slam_gdist_read; empty planes before enableCostmap
    const Costmap &getCostmap()
    {
        if (!(h_ && df_ && df_->computeFromGrid(h_) && df_->read(&costmap_.dist2, &costmap_.cost))) {
            costmap_.dist2.clear();
            costmap_.cost.clear();
        }
        return costmap_;
    }
    // Opt-in planner over the costmap (not in the reference): needs enableCostmap first.  Moves cost orth_w / diag_w times the
    // sum of the two cells' steps; a cell's step is neutral + its cost byte, cells from lethal_from on are closed, unknown cells
    // (255) take unknown_step (0: closed).  false (logged) when the parameters or the device refuse.
    bool enablePlanner(const NavParams &p = NavParams())
    {
        if (!h_ || !df_) return false;
        std::unique_ptr<NavField> nav(new NavField((int)grid_.info.width, (int)grid_.info.height, p));
        if (!nav->ok()) return false;
        nav_ = std::move(nav);
        return true;
    }
    // The window cell of a world point, by the grid's own binning (mls.cpp:77-78, grid_cell.hpp): with p the point in the window's
    // frame -- the world point minus the grid's pose when the map rolls, the world point itself otherwise -- stored as a float
    // as the clouds are, cell = (int)(p / resolution + size / 2), truncated toward zero, size / 2 the integer half.  false when
    // the cell lies outside the plane.  cellCentre is its inverse on the cell centres.
    bool worldToCell(double wx, double wy, int *cx, int *cy) const
    {
        double px = 0, py = 0;
        if (h_ && rolling_) slam_grid_get_pose(h_, &px, &py);
        const int    sx = (int)grid_.info.width, sy = (int)grid_.info.height;
        const double fx = (double)(float)(wx - px) / grid_.info.resolution + (double)(sx / 2);
        const double fy = (double)(float)(wy - py) / grid_.info.resolution + (double)(sy / 2);
        if (!(fx > -2147483648.0 && fx < 2147483648.0 && fy > -2147483648.0 && fy < 2147483648.0)) return false;
        *cx = (int)fx, *cy = (int)fy;
        return *cx >= 0 && *cy >= 0 && *cx < sx && *cy < sy;
    }
    void cellCentre(int cx, int cy, double *wx, double *wy) const
    {
        double px = 0, py = 0;
        if (h_ && rolling_) slam_grid_get_pose(h_, &px, &py);
        *wx = ((double)(cx - (int)grid_.info.width / 2) + 0.5) * grid_.info.resolution + px;
        *wy = ((double)(cy - (int)grid_.info.height / 2) + 0.5) * grid_.info.resolution + py;
    }
    // getCostmap()'s plane -> slam_grid_nav_field from the goal's cell, to convergence -> slam_gnav_path from the start's
    // cell.  World points in, world points at cell centres out; NO_START with no cells when either point lies outside the
    // window, NOT_CONVERGED before enablePlanner or when the device refuses.
    NavPath planPath(double from_x, double from_y, double to_x, double to_y)
    {
        NavPath out;
        if (!(h_ && df_ && nav_)) return out;
        int sx, sy, gx, gy;
        if (!worldToCell(from_x, from_y, &sx, &sy) || !worldToCell(to_x, to_y, &gx, &gy)) {
            out.status = SLAM_GNAV_PATH_NO_START;
            return out;
        }
        if (!(df_->computeFromGrid(h_) && nav_->computeFromGrid(h_, *df_, {gx, gy}) && nav_->path(sx, sy, &out.cells, &out.status))) {
            out.status = SLAM_GNAV_PATH_NOT_CONVERGED;
            out.cells.clear();
            return out;
        }
        out.points.resize(out.cells.size());
        for (size_t i = 0; i + 1 < out.cells.size(); i += 2) cellCentre(out.cells[i], out.cells[i + 1], &out.points[i], &out.points[i + 1]);
        return out;
    }
    NavField *planner() { return nav_.get(); }
    void setMinClusterPoints(double v) { if (h_) slam_grid_set_min_cluster_points(h_, (int)v); } // mls.h:235
    void setMaxRange(double v) { if (h_) slam_grid_set_max_range(h_, v); }                     // mls.h:237
    slam_grid_t *handle() { return h_; }
    bool         rolling() const { return rolling_; }

private:
    static void warn() { detail::warn("MLS"); }
    slam_grid_t  *h_ = nullptr;
    slam_gseg_t  *gseg_ = nullptr;
    OccupancyGrid grid_;
    std::unique_ptr<DistanceField> df_; // enableCostmap
    std::unique_ptr<NavField>      nav_; // enablePlanner
    Costmap       costmap_;
    bool          rolling_ = false, disable_pointcloud_ = false;
    detail::DeviceBuffer d_cloud_, d_labels_, d_gnd_, d_obs_, d_counts_; // the first four hold cap_ points each
    int                  cap_ = 0, last_counts_[2] = {0, 0};
    std::vector<float>   global_cloud_, trans_;
    detail::PinnedBuffer h_pin_;       // [counts | drv cloud, or the filtered global cloud]
    slam_ccicp_t        *cc_ = nullptr; // filterPointCloud's voxel grid
    detail::DeviceBuffer d_gc_in_, d_gc_out_;
};

} // namespace slam_amd
