// slam_amd/mls_map.hpp -- header-only adapter with the shape of class MLS (mls/include/mls/mls.h:154-237) in its
// non-rolling, height-cluster mode: graph_slam's global map (graph_slam.cpp:71), over the C-ABI (slam_mi355x.h,
// slam_mls_*).  The rolling / occupancy mode stays slam_amd::MLS (mls.hpp).
//
// Clouds are float arrays (x, y, z first, `stride` floats per point), poses the Pose struct of pose.hpp.  The clouds
// come from host memory: addToMap and addKeyframe upload them with a copy that waits for the map's stream, so each
// call waits for the previous call's device work before it enqueues its own (no pipelining across keyframes here;
// slam_mls_add_cloud_dev with device-resident clouds enqueues without a wait).  global_cloud is kept on the device
// and read back by getGlobalCloud.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "slam_amd/buffer.hpp"
#include "slam_amd/mls.hpp" // OccupancyGrid, voxel_filter_host
#include "slam_amd/pose.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

class MLSMap {
public:
    // mls.h:154: MLS(int size_x_, int size_y_, double res, bool roll, double robot_size = 1.45)
    MLSMap(int size_x_, int size_y_, double res, bool roll, double robot_size = 1.45)
    {
        grid_.info.resolution = res;
        grid_.info.width = (uint32_t)(size_x_ > 0 ? size_x_ : 0);
        grid_.info.height = (uint32_t)(size_y_ > 0 ? size_y_ : 0);
        grid_.info.origin_x = -(res * size_x_ / 2); // mls.h:171-172
        grid_.info.origin_y = -(res * size_y_ / 2);
        if (roll) {
            std::fprintf(stderr, "MLSMap: rolling maps are slam_amd::MLS (include/slam_amd/mls.hpp)\n");
            return;
        }
        slam_mls_params p;
        slam_mls_default_params(&p);
        p.robot_height = robot_size;
        if (slam_mls_create(size_x_, size_y_, res, &p, &h_) != SLAM_OK) {
            warn();
            h_ = nullptr;
            return;
        }
        slam_mls_info(h_, nullptr, nullptr, nullptr, nullptr, &p_, nullptr);
        if (slam_stream_create(&st_) != SLAM_OK) st_ = nullptr;
    }
    ~MLSMap()
    {
        if (st_) slam_stream_synchronize(st_); // (the one stream that uses the buffers, which go with their members)
        slam_ccicp_destroy(cc_);
        slam_mls_destroy(h_);
        if (st_) slam_stream_destroy(st_);
    }
    MLSMap(const MLSMap &) = delete;
    MLSMap &operator=(const MLSMap &) = delete;
    bool        ok() const { return h_ != nullptr; }
    slam_mls_t *handle() { return h_; }

    void clearMap() // mls.cpp:18-31
    {
        if (!h_) return;
        if (slam_mls_clear(h_, st_) != SLAM_OK) warn();
        n_gc_ = 0;
    }
    void setPose(const Pose &p) { setPose(p.x, p.y); } // mls.cpp:408-414
    void setPose(double x, double y)
    {
        if (h_) slam_mls_set_pose(h_, x, y);
    }
    // mls.cpp:34-53: setPose, then the non-rolling addToMap of the cloud as it is (already in the map frame)
    void addToMap(const float *xyz, int n, int stride, const Pose &pose)
    {
        setPose(pose);
        addToMap(xyz, n, stride);
    }
    void addToMap(const float *xyz, int n, int stride) // mls.cpp:345-402
    {
        if (!h_ || n <= 0) return;
        float *d = stage(xyz, n, stride, d_cloud_);
        if (!d || slam_mls_add_cloud_dev(h_, d, n, stride, st_) != SLAM_OK) return warn();
        append_global(d, n, stride);
    }
    // graph_slam.cpp:268-275: the keyframe transformed by its pose (tf::poseMsgToEigen + pcl::transformPointCloud,
    // on the device) and added with that pose
    void addKeyframe(const float *xyz, int n, int stride, const Pose &pose)
    {
        setPose(pose);
        if (!h_ || n <= 0) return;
        float *d_in = stage(xyz, n, stride, d_kf_);
        if (!d_in) return warn();
        if (!detail::reserve_half(d_cloud_, sizeof(float) * 3 * (size_t)n)) return warn();
        double r[9], t[3] = {pose.x, pose.y, pose.z};
        detail::tf_matrix(pose, r); // tf::poseMsgToEigen: the quaternion's matrix (as MLS::addToMap)
        if (slam_grid_transform_cloud_dev(d_in, n, stride, r, t, d_cloud_.as<float>(), st_) != SLAM_OK) return warn();
        if (slam_mls_add_cloud_dev(h_, d_cloud_.as<float>(), n, 3, st_) != SLAM_OK) return warn();
        append_global(d_cloud_.as<float>(), n, 3);
    }
    // mls.cpp:481-505: clusters' mean z (device), global_cloud's z (+ (float)pose.z, float arithmetic)
    void offsetMap(const Pose &pose)
    {
        if (!h_) return;
        if (slam_mls_offset_z(h_, pose.z, st_) != SLAM_OK) return warn();
        if (disable_pointcloud_ || !n_gc_) return;
        std::vector<float> gc = getGlobalCloud();
        const float        dz = (float)pose.z;
        for (size_t i = 2; i < gc.size(); i += 3) gc[i] = gc[i] + dz;
        slam_memcpy_h2d(d_gc_.p, gc.data(), gc.size() * sizeof(float), st_);
    }
    std::vector<float> getGlobalCloud() // mls.h:214 (x, y, z per point)
    {
        std::vector<float> out(3 * n_gc_);
        if (h_ && n_gc_) {
            slam_stream_synchronize(st_);
            slam_memcpy_d2h(out.data(), d_gc_.p, out.size() * sizeof(float), st_);
        }
        return out;
    }
    // mls.cpp:508-518: pcl::VoxelGrid(xy, xy, z) over global_cloud: the library's voxel filter on the device (the same
    // lattice and order as slam_amd::MLS::filterPointCloud); a lattice beyond its accumulator (more than 2^26 voxels: a
    // large map at a fine leaf) is filtered on the host instead, as slam_amd::MLS does
    void filterPointCloud(double xy, double z)
    {
        if (!h_ || !n_gc_) return;
        if (!filter_on_device(xy, z)) filter_on_host(xy, z);
    }
    bool filter_on_device(double xy, double z)
    {
        if (n_gc_ > ((size_t)1 << 30)) return false;
        if (!cc_ && slam_ccicp_create(&cc_) != SLAM_OK) return false;
        if (!detail::reserve_half(d_filt_, 16 * n_gc_)) return false;
        int n_out = 0;
        if (slam_ccicp_voxel_downsample_dev(cc_, d_gc_.as<float>(), nullptr, (int)n_gc_, 3, (float)xy, (float)xy, (float)z, d_filt_.as<float>(),
                                            (int)n_gc_, &n_out, st_) != SLAM_OK)
            return false;
        slam_stream_synchronize(st_);
        std::vector<float> rec(4 * (size_t)n_out), gc(3 * (size_t)n_out);
        if (n_out) slam_memcpy_d2h(rec.data(), d_filt_.p, rec.size() * sizeof(float), st_);
        for (int i = 0; i < n_out; ++i)
            for (int k = 0; k < 3; ++k) gc[3 * (size_t)i + k] = rec[4 * (size_t)i + k];
        if (n_out) slam_memcpy_h2d(d_gc_.p, gc.data(), gc.size() * sizeof(float), st_);
        n_gc_ = (size_t)n_out;
        return true;
    }
    const OccupancyGrid &getDrivability() // mls.h:215
    {
        grid_.data.resize((size_t)grid_.info.width * grid_.info.height);
        if (h_) {
            slam_stream_synchronize(st_);
            slam_mls_read_drivability(h_, grid_.data.data());
        }
        return grid_;
    }
    // mls.cpp:520-556: cluster means (x, y, z floats per point) in the reference's order
    void getSegmentedClouds(std::vector<float> &obstacle, std::vector<float> &ground)
    {
        obstacle.clear(), ground.clear();
        if (!h_) return;
        slam_stream_synchronize(st_);
        int no = 0, ng = 0;
        const int rc = slam_mls_segmented_clouds(h_, nullptr, 0, &no, nullptr, 0, &ng);
        if (rc != SLAM_OK && rc != SLAM_E_NOMEM) return warn();
        obstacle.resize(3 * (size_t)no), ground.resize(3 * (size_t)ng);
        if (slam_mls_segmented_clouds(h_, obstacle.data(), no, &no, ground.data(), ng, &ng) != SLAM_OK) {
            obstacle.clear(), ground.clear();
            warn();
        }
    }

    // the setters of mls.h:223-237 (a value the library refuses -- max_clusters above the capacity fixed at create -- is
    // reported and not kept)
    void setNormalTheshold(double v) { with([&](slam_mls_params &p) { p.normal_threshold = v; }); }
    void setHeightTheshold(double v) { with([&](slam_mls_params &p) { p.height_threshold = v; }); }
    void setClusterDistTheshold(double v) { with([&](slam_mls_params &p) { p.cluster_dist_threshold = v; }); }
    void setClusterCombineDist(double v) { with([&](slam_mls_params &p) { p.cluster_combine_dist = v; }); }
    void setClusterSigmaFactor(double v) { with([&](slam_mls_params &p) { p.cluster_sigma_factor = v; }); }
    void setDriveDistTheshold(double v) { with([&](slam_mls_params &p) { p.drive_dist_threshold = v; }); }
    void setMaxClusters(double v) { with([&](slam_mls_params &p) { p.max_clusters = (int)v; }); }
    void setMaxClusterPoints(double v) { with([&](slam_mls_params &p) { p.max_cluster_points = (int)v; }); }
    void setMinClusterPoints(double v) { with([&](slam_mls_params &p) { p.min_cluster_points = (int)v; }); }
    void setMaxRange(double v) { with([&](slam_mls_params &p) { p.max_range = v; }); } // update_dist stays (mls.h:236)
    void setUpdateDistMeters(double m) { with([&](slam_mls_params &p) { p.update_dist = (int)(m / grid_.info.resolution); }); }
    void setDisablePointCloud(bool v) { disable_pointcloud_ = v; }
    const slam_mls_params &params() const { return p_; }

    // pcl::VoxelGrid on the host (the form slam_amd::MLS::filterPointCloud falls back to): for a lattice beyond the
    // device filter's accumulator
    void filter_on_host(double xy, double z)
    {
        std::vector<float> gc = getGlobalCloud();
        voxel_filter_host(gc, xy, z);
        n_gc_ = gc.size() / 3;
        if (n_gc_) slam_memcpy_h2d(d_gc_.p, gc.data(), gc.size() * sizeof(float), st_);
    }

private:
    static void warn() { detail::warn("MLSMap"); }
    template <class F>
    void with(F set)
    {
        // the parameters are read when a call is enqueued: the stream's earlier calls keep theirs
        slam_mls_params p = p_;
        set(p);
        if (!h_) return;
        if (slam_mls_set_params(h_, &p) != SLAM_OK) return warn();
        slam_mls_info(h_, nullptr, nullptr, nullptr, nullptr, &p_, nullptr);
    }
    // the host cloud uploaded into a device buffer (the copy waits for the stream's earlier use of the buffer)
    float *stage(const float *xyz, int n, int stride, detail::DeviceBuffer &d)
    {
        const size_t bytes = sizeof(float) * (size_t)n * stride;
        if (!detail::reserve_half(d, bytes)) return nullptr;
        if (slam_memcpy_h2d(d.p, xyz, bytes, st_) != SLAM_OK) return nullptr;
        return d.as<float>();
    }
    // *global_cloud += *input_cloud (mls.cpp:397-400), on the device
    void append_global(const float *d, int n, int stride)
    {
        if (disable_pointcloud_) return;
        if (3 * sizeof(float) * (n_gc_ + n) > d_gc_.cap) {
            std::vector<float> keep = getGlobalCloud();
            if (!detail::reserve_half(d_gc_, 3 * sizeof(float) * 2 * (n_gc_ + n))) return warn(); // (twice what is there, on top of the half)
            if (!keep.empty()) slam_memcpy_h2d(d_gc_.p, keep.data(), keep.size() * sizeof(float), st_);
        }
        float *dst = d_gc_.as<float>() + 3 * n_gc_;
        if (stride == 3) {
            slam_memcpy_d2d(dst, d, 3 * sizeof(float) * (size_t)n, st_);
        } else { // the x, y, z of each point: the identity transform (exact in double) packs them
            const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
            slam_grid_transform_cloud_dev(d, n, stride, I, z, dst, st_);
        }
        n_gc_ += (size_t)n;
    }

    slam_mls_t     *h_ = nullptr;
    slam_stream_t   st_ = nullptr;
    slam_mls_params p_{};
    OccupancyGrid   grid_;
    bool            disable_pointcloud_ = false;
    detail::DeviceBuffer d_cloud_, d_kf_, d_gc_, d_filt_;
    size_t          n_gc_ = 0;
    slam_ccicp_t   *cc_ = nullptr;
};

} // namespace slam_amd
