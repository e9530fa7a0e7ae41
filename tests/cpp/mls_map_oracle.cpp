// mls_map_oracle.cpp -- scalar restatement of class MLS in its non-rolling, height-cluster mode
// (mls/include/mls/mls.h:20-51, 154-237; mls/src/mls.cpp:18-53, 152-402, 481-556), the yardstick of
// slam_mls_* (slam_amd/csrc/mls.hip).  Serial and recursive, exactly as the reference runs: one
// std::vector<Cluster> and one std::deque of points per cell.  mls.cpp needs PCL, Eigen and tf and
// cannot be compiled here, so parity is against this restatement (docs/MLS_MAP.md).
//
// Built by the tests with g++ -O2 -ffp-contract=off (the reference is x86-64 without FMA) and loaded
// with ctypes (tests/mls_map_oracle.py).  Not part of the product.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <vector>

#include "slam_mi355x.h" // slam_mls_params only

using namespace std; // mls.cpp:16: abs and max below are std::abs(double), std::max

namespace {

struct Cluster { // mls.h:20-33: only mean and cov(2,2) are ever read
    double mean[3] = {0, 0, 0};
    double cov = 0;
    double num_pts = 0;
};
struct Pt {
    float x, y, z;
};
struct Cell { // mls.h:37-51
    vector<Cluster> clusters;
    deque<Pt>       cloud;
    int             drivable = -1;
    bool            updated = false;
};

struct Map {
    int             sx, sy;
    double          res;
    slam_mls_params p;
    vector<Cell>    grid;
    vector<int8_t>  bytes;
    double          pose_x = 0, pose_y = 0;
    long            updates = 0, outside = 0; // updateCell calls, and those of cells outside the window (through the recursion)
    int             wx0 = 0, wx1 = 0, wy0 = 0, wy1 = 0;
    Cell &cell(int x, int y) { return grid[(size_t)x + (size_t)sx * y]; }

    // libstdc++ std::sort on at most 16 elements is an insertion sort: stable.  Above 16 it is an introsort,
    // which orders equal keys differently; both sides here use the stable form (docs/MLS_MAP.md).
    static void sort_clusters(vector<Cluster> &c)
    {
        for (size_t i = 1; i < c.size(); ++i) {
            Cluster v = c[i];
            size_t  j = i;
            while (j > 0 && v.mean[2] < c[j - 1].mean[2]) {
                c[j] = c[j - 1];
                --j;
            }
            c[j] = v;
        }
    }

    void updateCell(int x, int y) // mls.cpp:152-342
    {
        ++updates;
        if (x < wx0 || x >= wx1 || y < wy0 || y >= wy1) ++outside;
        Cell *cell = &this->cell(x, y);
        cell->updated = false; // :155
        for (size_t jp = 0; jp < cell->cloud.size(); jp++) {
            const Pt &pt = cell->cloud[jp];
            int    cluster_idx = -1; // :162-180 choose a cluster
            double uninit_dist = 100000;
            int    uninit_idx = -1;
            for (int c = 0; c < (int)cell->clusters.size(); c++) {
                const double cur_dist = abs(cell->clusters[c].mean[2] - (double)pt.z);
                if (cell->clusters[c].num_pts < p.min_cluster_points) {
                    if (cur_dist < uninit_dist) {
                        uninit_dist = cur_dist;
                        uninit_idx = c;
                    }
                } else if (cur_dist < (sqrt(cell->clusters[c].cov) * p.cluster_sigma_factor + p.cluster_dist_threshold)) {
                    cluster_idx = c;
                    break;
                }
            }
            if (cell->clusters.empty() || cluster_idx == -1) { // :182-198
                if (uninit_idx == -1 || uninit_dist > p.robot_height) {
                    if (cell->clusters.size() < (size_t)p.max_clusters) {
                        cell->clusters.push_back(Cluster());
                        cluster_idx = (int)cell->clusters.size() - 1;
                    } else {
                        continue; // :194 too many clusters: the point is dropped
                    }
                } else {
                    cluster_idx = uninit_idx;
                }
            }
            // :200 the reference takes a Cluster* here; the erases below shift other clusters under it
            if (cell->clusters[cluster_idx].num_pts == p.max_cluster_points) { // :202-213
                for (int k = 1; k < (int)cell->clusters.size(); k++) {
                    if (cluster_idx != k) {
                        cell->clusters[k].num_pts--;
                        if (cell->clusters[k].num_pts <= 0) cell->clusters.erase(cell->clusters.begin() + k); // the next one is skipped
                    }
                }
            } else {
                cell->clusters[cluster_idx].num_pts++; // :215
            }
            if (cluster_idx >= (int)cell->clusters.size()) continue; // the stale slot lies past the end: the update is lost
            Cluster     *cluster = &cell->clusters[cluster_idx];
            const double n = cluster->num_pts;
            cluster->mean[0] = ((n - 1) / n) * cluster->mean[0] + 1 / n * pt.x; // :218-223
            cluster->mean[1] = ((n - 1) / n) * cluster->mean[1] + 1 / n * pt.y;
            cluster->mean[2] = ((n - 1) / n) * cluster->mean[2] + 1 / n * pt.z;
            if (n > 1) { // :232-234
                cluster->cov = ((n - 1) / n) * cluster->cov + 1.0 / (n - 1) * (pt.z - cluster->mean[2]) * (pt.z - cluster->mean[2]);
                cluster->cov = max(cluster->cov, 0.001);
            } else {
                sort_clusters(cell->clusters); // :236
            }
        }
        int ground_idx = -1; // :240-250
        for (int c = 0; c < (int)cell->clusters.size(); c++)
            if (cell->clusters[c].num_pts > p.min_cluster_points) {
                ground_idx = c;
                break;
            }
        if (ground_idx == -1) return; // :247: the points stay pending
        cell->cloud.clear();          // :252
        vector<Cluster> &cl = cell->clusters;
        if (ground_idx + 1 < (int)cl.size() && cl[ground_idx + 1].num_pts > p.min_cluster_points) { // :282-304
            const double clearance = cl[ground_idx + 1].mean[2] - sqrt(cl[ground_idx + 1].cov) * 2 - cl[ground_idx].mean[2];
            if (clearance < p.cluster_combine_dist) {
                const double n0 = cl[ground_idx].num_pts, n1 = cl[ground_idx + 1].num_pts;
                const double r0 = n0 / (n0 + n1), r1 = n1 / (n0 + n1);
                for (int a = 0; a < 3; ++a) cl[ground_idx].mean[a] = r0 * cl[ground_idx].mean[a] + r1 * cl[ground_idx + 1].mean[a];
                cl[ground_idx].cov = (r0 * cl[ground_idx].cov + r1 * cl[ground_idx + 1].cov);
                cl.erase(cl.begin() + ground_idx + 1);
            } else if (clearance < p.drive_dist_threshold) {
                cell->drivable = 0;
                bytes[(size_t)x + (size_t)sx * y] = 100;
                return;
            }
        }
        for (int i = -1; i <= 1; i++) // :308-329
            for (int j = -1; j <= 1; j++) {
                if ((i == 0 && j == 0) || i + x < 0 || i + x >= sx || j + y < 0 || j + y >= sy) continue;
                if (this->cell(x + i, y + j).updated) updateCell(x + i, y + j); // :312 the recursion
                cell = &this->cell(x, y);
                const Cell &nb = this->cell(x + i, y + j);
                if (!nb.clusters.empty() && nb.clusters[0].num_pts > p.min_cluster_points) {
                    const double ndiff = cell->clusters[0].mean[2] - nb.clusters[0].mean[2];
                    if (ndiff > p.height_threshold) {
                        cell->drivable = 0;
                        bytes[(size_t)x + (size_t)sx * y] = 100;
                        return;
                    }
                }
            }
        if (abs(cell->clusters[ground_idx].cov) > p.normal_threshold) { // :333-337
            cell->drivable = 0;
            bytes[(size_t)x + (size_t)sx * y] = 100;
            return;
        }
        cell->drivable = 1; // :340-341
        bytes[(size_t)x + (size_t)sx * y] = 0;
    }

    void addToMap(const float *xyz, int n, int stride) // mls.cpp:345-402, non-rolling
    {
        const int offset_x = sx / 2, offset_y = sy / 2;
        for (int i = 0; i < n; i++) {
            const Pt pt = {xyz[(size_t)i * stride], xyz[(size_t)i * stride + 1], xyz[(size_t)i * stride + 2]};
            const double fx = pt.x / res + offset_x, fy = pt.y / res + offset_y;
            if (!(fx > -2147483648.0 && fx < 2147483648.0) || !(fy > -2147483648.0 && fy < 2147483648.0)) continue;
            const int    x = (int)fx, y = (int)fy;
            const double rx = pose_x - pt.x, ry = pose_y - pt.y;
            const double rng = sqrt(rx * rx + ry * ry);
            if (x < 0 || y < 0 || x >= sx || y >= sx || rng > p.max_range) continue; // :381 (sic: y >= size_x)
            if (y >= sy) continue;                                                     // where the reference writes out of bounds
            cell(x, y).cloud.push_back(pt);
            cell(x, y).updated = true;
        }
        const int curX = (int)(pose_x / res + offset_x), curY = (int)(pose_y / res + offset_y);
        const int u = p.update_dist;
        wx0 = curX - u, wx1 = curX + u, wy0 = curY - u, wy1 = curY + u;
        for (int i = -u; i < u; i++)
            for (int j = -u; j < u; j++) {
                const int x = i + curX, y = j + curY;
                if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
                if (cell(x, y).updated) updateCell(x, y);
            }
    }
};

} // namespace

extern "C" {

// null when the start pad does not fit in the grid (slam_mls_create refuses such a grid too: docs/MLS_MAP.md)
Map *mlso_create(int sx, int sy, double res, const slam_mls_params *p) // mls.h:154-205
{
    if (!(2.0 * std::floor(1.0 / res) + 1.0 <= (double)std::min(sx, sy))) return nullptr;
    Map *m = new Map;
    m->sx = sx, m->sy = sy, m->res = res, m->p = *p;
    if (m->p.update_dist < 0) m->p.update_dist = (int)fmin((int)m->p.max_range / res, sx / 2);
    m->grid.resize((size_t)sx * sy);
    m->bytes.assign((size_t)sx * sy, 0); // data.resize zero-fills (mls.h:175)
    const int set_size = (int)(1.0 / res);
    Cluster   c;
    c.mean[2] = -p->robot_height;
    c.num_pts = p->min_cluster_points;
    c.cov = 0.01;
    for (int i = -set_size; i <= set_size; i++)
        for (int j = -set_size; j <= set_size; j++) {
            c.mean[0] = i * res;
            c.mean[1] = j * res;
            m->cell(i + sx / 2, j + sy / 2).clusters.push_back(c);
        }
    return m;
}
void mlso_destroy(Map *m) { delete m; }
void mlso_set_params(Map *m, const slam_mls_params *p)
{
    const int u = m->p.update_dist;
    m->p = *p;
    if (p->update_dist < 0) m->p.update_dist = u;
}
void mlso_clear(Map *m) // mls.cpp:18-31
{
    for (Cell &c : m->grid) {
        c.cloud.clear();
        c.clusters.clear();
        c.drivable = -1;
        c.updated = false;
    }
    std::fill(m->bytes.begin(), m->bytes.end(), (int8_t)-1);
}
void mlso_set_pose(Map *m, double x, double y) { m->pose_x = x, m->pose_y = y; }
// returns the wall time of the call in seconds
double mlso_add_cloud(Map *m, const float *xyz, int n, int stride)
{
    const auto t0 = std::chrono::steady_clock::now();
    m->addToMap(xyz, n, stride);
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
void mlso_offset_z(Map *m, double dz) // mls.cpp:481-491
{
    for (Cell &c : m->grid)
        for (Cluster &k : c.clusters) k.mean[2] += dz;
}
void mlso_read_drivability(Map *m, int8_t *out) { std::memcpy(out, m->bytes.data(), m->bytes.size()); }
// mls.cpp:520-556; returns the counts, fills up to the capacities
void mlso_segmented(Map *m, float *obs, int obs_cap, int *n_obs, float *gnd, int gnd_cap, int *n_gnd)
{
    int       no = 0, ng = 0;
    const int curX = (int)(m->pose_x / m->res + m->sx / 2), curY = (int)(m->pose_y / m->res + m->sy / 2);
    const int u = m->p.update_dist;
    for (int i = -u + curX; i < u + curX; i++)
        for (int j = -u + curY; j < u + curY; j++) {
            if (i < 0 || i >= m->sx || j >= m->sy || j < 0) continue;
            const Cell &cell = m->cell(i, j);
            for (int c = 0; c < (int)cell.clusters.size(); c++) {
                if (!(cell.clusters[c].num_pts >= m->p.min_cluster_points)) continue;
                const float pt[3] = {(float)cell.clusters[c].mean[0], (float)cell.clusters[c].mean[1], (float)cell.clusters[c].mean[2]};
                if (cell.drivable == 0 || c > 0) {
                    if (no < obs_cap) std::memcpy(obs + 3 * (size_t)no, pt, sizeof pt);
                    ++no;
                } else {
                    if (ng < gnd_cap) std::memcpy(gnd + 3 * (size_t)ng, pt, sizeof pt);
                    ++ng;
                }
            }
        }
    *n_obs = no, *n_gnd = ng;
}
// the layout of slam_mls_read_cells, clusters[i*cap + c]
void mlso_read_cells(Map *m, const int32_t *cells, int n, int cap, int32_t *n_clusters, double *clusters, int8_t *drivable,
                     int8_t *bytes, uint8_t *updated, int32_t *pending)
{
    for (int i = 0; i < n; ++i) {
        const Cell &c = m->grid[cells[i]];
        n_clusters[i] = (int32_t)c.clusters.size();
        for (int k = 0; clusters && k < cap; ++k) {
            double *o = clusters + ((size_t)i * cap + k) * 5;
            if (k < (int)c.clusters.size()) {
                const Cluster &q = c.clusters[k];
                o[0] = q.mean[0], o[1] = q.mean[1], o[2] = q.mean[2], o[3] = q.cov, o[4] = q.num_pts;
            } else {
                for (int a = 0; a < 5; ++a) o[a] = 0;
            }
        }
        drivable[i] = (int8_t)c.drivable;
        bytes[i] = m->bytes[cells[i]];
        updated[i] = c.updated ? 1 : 0;
        pending[i] = (int32_t)c.cloud.size();
    }
}
// cells with any state: clusters, pending points or a raised flag (what the tests compare)
int mlso_touched(Map *m, int32_t *out, int cap)
{
    int k = 0;
    for (size_t i = 0; i < m->grid.size(); ++i) {
        const Cell &c = m->grid[i];
        if (c.clusters.empty() && c.cloud.empty() && !c.updated && c.drivable == -1) continue;
        if (k < cap) out[k] = (int32_t)i;
        ++k;
    }
    return k;
}
int  mlso_update_dist(Map *m) { return m->p.update_dist; }
long mlso_updates(Map *m) { return m->updates; }
long mlso_outside_updates(Map *m) { return m->outside; }

} // extern "C"
