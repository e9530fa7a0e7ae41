// vmap_carve_oracle.cpp -- the scalar restatement of the voxel map with free-space carving (docs/VOXEL_MAP.md sections 1
// and 8): a std::map over the key, one point, one ray and one step at a time, the ray walked with the error-term iteration
// of the driving-axis 3-D Bresenham.  slam_vmap_* (slam_amd/csrc/voxmap.hip) must equal it bit for bit.  Compiled by
// tests/oracle_build.py with -ffp-contract=off.  Uses nothing of the library but the header's structs.
//
// `mutation` plants one wrong rule, for the tests that have to catch it (tests/test_vmap_carve_oracle.py):
//   1  the end cell is visited (the margin and the tail count from one step further out)
//   2  `e >= 0` for `e > 0` in the walk (the closed form's + n for + n - 1)
//   3  within-cloud hit protection off: a voxel crossed by a ray is charged a miss although the cloud ends in it
//   4  per-ray for per-scan units: every endpoint and every crossing counts
//   5  truncation instead of floor for the cell (the origin's and the endpoints')
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "slam_mi355x.h"

namespace {

struct Voxel {
    uint32_t count = 0;
    int64_t  sum[3] = {0, 0, 0};
    uint32_t seen = 0, miss = 0;
};

struct Map {
    double                    leaf;
    int                       mutation = 0;
    std::map<uint64_t, Voxel> vox;
    int64_t                   n_points = 0;
};

float centroid(int64_t s, uint32_t count) { return (float)(((double)s / (double)count) * (1.0 / 1048576.0)); }

// the point as the map takes it; false when it is dropped
bool moved_cell(const Map *m, const double p[3], const double *R, const double *t, float q[3], int32_t c[3])
{
    for (int k = 0; k < 3; ++k) {
        if (R && t) {
            const double a = R[3 * k] * p[0], b = R[3 * k + 1] * p[1], cc = R[3 * k + 2] * p[2];
            q[k] = (float)(((a + b) + cc) + t[k]);
        } else {
            q[k] = (float)p[k];
        }
    }
    for (int k = 0; k < 3; ++k) {
        const float v = q[k];
        if (!std::isfinite(v) || std::fabs(v) >= 4194304.0f) return false;
        const double d = (double)v / m->leaf;
        const double f = m->mutation == 5 ? std::trunc(d) : std::floor(d);
        if (!(std::fabs(f) < 1048576.0)) return false;
        c[k] = (int32_t)f;
    }
    return true;
}

uint64_t key_of(const int32_t c[3])
{
    return (uint64_t)(c[2] + (1 << 20)) << 42 | (uint64_t)(c[1] + (1 << 20)) << 21 | (uint64_t)(c[0] + (1 << 20));
}

// The cells one ray visits, in order: nothing when it is longer than max_ray_cells (*skipped set).
void walk(const int32_t c0[3], const int32_t c1[3], const slam_vmap_carve_params &P, int mutation, std::vector<uint64_t> *cells, bool *skipped)
{
    int64_t a[3], s[3], n = 0;
    for (int k = 0; k < 3; ++k) {
        const int64_t d = (int64_t)c1[k] - c0[k];
        a[k] = d < 0 ? -d : d;
        s[k] = d < 0 ? -1 : (d > 0 ? 1 : 0);
        if (a[k] > n) n = a[k];
    }
    *skipped = n > P.max_ray_cells;
    if (*skipped) return;
    int64_t T = (n * P.tail_num + P.tail_den - 1) / P.tail_den;
    if (T < P.end_margin) T = P.end_margin;
    int64_t last = n - T - 1; // the last step visited
    if (mutation == 1) last += 1;
    int m = 0; // the driving axis: the first with a = n
    while (a[m] != n) ++m;
    int64_t e[3], c[3] = {c0[0], c0[1], c0[2]};
    for (int k = 0; k < 3; ++k) e[k] = 2 * a[k] - n;
    for (int64_t i = 0; i <= last && i <= n; ++i) {
        const int32_t cc[3] = {(int32_t)c[0], (int32_t)c[1], (int32_t)c[2]};
        cells->push_back(key_of(cc));
        c[m] += s[m];
        for (int k = 0; k < 3; ++k) {
            if (k == m) continue;
            if (mutation == 2 ? e[k] >= 0 : e[k] > 0) {
                c[k] += s[k];
                e[k] -= 2 * n;
            }
            e[k] += 2 * a[k];
        }
    }
}

} // namespace

extern "C" {

void *vco_create(double leaf)
{
    Map *m = new Map();
    m->leaf = leaf;
    return m;
}
void vco_destroy(void *h) { delete static_cast<Map *>(h); }
void vco_set_mutation(void *h, int mutation) { static_cast<Map *>(h)->mutation = mutation; }
void vco_clear(void *h)
{
    Map *m = static_cast<Map *>(h);
    m->vox.clear();
    m->n_points = 0;
}
long long vco_n_voxels(void *h) { return (long long)static_cast<Map *>(h)->vox.size(); }
long long vco_n_points(void *h) { return (long long)static_cast<Map *>(h)->n_points; }

// returns the number of points dropped
int vco_integrate(void *h, const float *xyz, int n, int stride, const double *R, const double *t)
{
    Map *m = static_cast<Map *>(h);
    int  dropped = 0;
    for (int i = 0; i < n; ++i) {
        const float *p = xyz + (size_t)i * stride;
        const double pd[3] = {p[0], p[1], p[2]};
        float        q[3];
        int32_t      c[3];
        if (!moved_cell(m, pd, R, t, q, c)) {
            ++dropped;
            continue;
        }
        Voxel &v = m->vox[key_of(c)];
        ++v.count;
        for (int k = 0; k < 3; ++k) v.sum[k] += (int64_t)std::rint((double)q[k] * 1048576.0); // to nearest even
        ++m->n_points;
    }
    return dropped;
}

// One carve call.  -1 when the origin has no cell (nothing changed), 0 otherwise.
int vco_carve(void *h, const float *xyz, int n, int stride, const double *R, const double *t, const double *origin,
              const slam_vmap_carve_params *params, slam_vmap_carve_result *res)
{
    Map                   *m = static_cast<Map *>(h);
    slam_vmap_carve_params P = *params;
    slam_vmap_carve_result r = {};
    const double           o[3] = {origin ? origin[0] : 0.0, origin ? origin[1] : 0.0, origin ? origin[2] : 0.0};
    float                  qo[3];
    int32_t                c0[3];
    if (!moved_cell(m, o, R, t, qo, c0)) return -1;
    std::vector<uint64_t> ends;
    std::vector<uint64_t> visited; // every cell of every ray, in order
    for (int i = 0; i < n; ++i) {
        const float *p = xyz + (size_t)i * stride;
        const double pd[3] = {p[0], p[1], p[2]};
        float        q[3];
        int32_t      c1[3];
        if (!moved_cell(m, pd, R, t, q, c1)) {
            ++r.n_dropped;
            continue;
        }
        ++r.n_rays;
        ends.push_back(key_of(c1));
        bool skipped = false;
        walk(c0, c1, P, m->mutation, &visited, &skipped);
        if (skipped) ++r.n_skipped;
    }
    r.n_steps = (int64_t)visited.size();
    // phase 1: every existing voxel that holds an endpoint, once
    std::set<uint64_t> hit;
    for (uint64_t k : ends) {
        auto it = m->vox.find(k);
        if (it == m->vox.end()) continue;
        if (m->mutation == 4) {
            ++it->second.seen;
            if (hit.insert(k).second) ++r.n_seen;
        } else if (hit.insert(k).second) {
            ++it->second.seen;
            ++r.n_seen;
        }
    }
    // phase 2: every other existing voxel that a ray visited, once
    std::set<uint64_t> crossed;
    for (uint64_t k : visited) {
        auto it = m->vox.find(k);
        if (it == m->vox.end()) continue;
        if (m->mutation != 3 && m->mutation != 4 && hit.count(k)) continue;
        if (m->mutation == 4) {
            ++it->second.miss;
            if (crossed.insert(k).second) ++r.n_missed;
        } else if (crossed.insert(k).second) {
            ++it->second.miss;
            ++r.n_missed;
        }
    }
    if (res) *res = r;
    return 0;
}

// The cells (keys) one ray from cell c0 to cell c1 visits, by the iteration: returns their number, -1 when the ray is skipped;
// writes the first `cap`.
int vco_ray_cells(const int32_t *c0, const int32_t *c1, const slam_vmap_carve_params *params, int mutation, uint64_t *out, int cap)
{
    std::vector<uint64_t> cells;
    bool                  skipped = false;
    walk(c0, c1, *params, mutation, &cells, &skipped);
    if (skipped) return -1;
    for (size_t i = 0; i < cells.size() && (int)i < cap; ++i) out[i] = cells[i];
    return (int)cells.size();
}

// Returns the number of qualifying voxels; writes the first `cap` of them (every array nullable).  den <= 0: no carved rule.
int vco_extract(void *h, const float *lo, const float *hi, int min_count, int num, int den, float *xyz4, uint32_t *count, uint64_t *key,
                int64_t *sums, uint32_t *seen, uint32_t *miss, int cap)
{
    Map *m = static_cast<Map *>(h);
    int  n = 0;
    for (const auto &kv : m->vox) {
        const Voxel &v = kv.second;
        if (v.count < (uint32_t)(min_count < 0 ? 0 : min_count)) continue;
        if (den > 0 && !((uint64_t)v.miss * (uint64_t)den <= (uint64_t)(v.seen > 1 ? v.seen : 1) * (uint64_t)num)) continue;
        const float c[3] = {centroid(v.sum[0], v.count), centroid(v.sum[1], v.count), centroid(v.sum[2], v.count)};
        if (lo && hi && !(lo[0] <= c[0] && c[0] <= hi[0] && lo[1] <= c[1] && c[1] <= hi[1])) continue;
        if (n < cap) {
            if (xyz4) xyz4[4 * n] = c[0], xyz4[4 * n + 1] = c[1], xyz4[4 * n + 2] = c[2], xyz4[4 * n + 3] = 0.0f;
            if (count) count[n] = v.count;
            if (key) key[n] = kv.first;
            if (sums) sums[3 * n] = v.sum[0], sums[3 * n + 1] = v.sum[1], sums[3 * n + 2] = v.sum[2];
            if (seen) seen[n] = v.seen;
            if (miss) miss[n] = v.miss;
        }
        ++n;
    }
    return n;
}

// sizeof and offsets of the two structs, for the Python mirrors
void vco_layout(int *out)
{
    out[0] = (int)sizeof(slam_vmap_carve_params);
    out[1] = (int)offsetof(slam_vmap_carve_params, end_margin);
    out[2] = (int)offsetof(slam_vmap_carve_params, tail_num);
    out[3] = (int)offsetof(slam_vmap_carve_params, tail_den);
    out[4] = (int)offsetof(slam_vmap_carve_params, max_ray_cells);
    out[5] = (int)sizeof(slam_vmap_carve_result);
    out[6] = (int)offsetof(slam_vmap_carve_result, n_rays);
    out[7] = (int)offsetof(slam_vmap_carve_result, n_dropped);
    out[8] = (int)offsetof(slam_vmap_carve_result, n_skipped);
    out[9] = (int)offsetof(slam_vmap_carve_result, n_steps);
    out[10] = (int)offsetof(slam_vmap_carve_result, n_seen);
    out[11] = (int)offsetof(slam_vmap_carve_result, n_missed);
}

} // extern "C"
