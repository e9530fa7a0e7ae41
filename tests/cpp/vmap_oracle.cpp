// vmap_oracle.cpp -- the scalar restatement of the voxel map's contract (docs/VOXEL_MAP.md section 1): a std::map over the
// key, one point at a time.  slam_vmap_* (slam_amd/csrc/voxmap.hip) must equal it bit for bit.  Compiled by
// tests/oracle_build.py with -ffp-contract=off.  Uses nothing of the library but the header's parameter struct.
//
// `mutation` plants one wrong rule, for the tests that have to catch it (tests/test_vmap_oracle.py):
//   1  truncation instead of floor for the cell
//   2  '<' instead of '<=' at the box
//   3  arrival order instead of key order in the extraction
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "slam_mi355x.h"

namespace {

struct Voxel {
    uint32_t count = 0;
    int64_t  sum[3] = {0, 0, 0};
};

struct Map {
    double                   leaf;
    int                      mutation = 0;
    std::map<uint64_t, Voxel> vox;
    std::vector<uint64_t>    arrival; // keys in the order they first appeared (mutation 3 only)
    int64_t                  n_points = 0;
};

float centroid(int64_t s, uint32_t count) { return (float)(((double)s / (double)count) * (1.0 / 1048576.0)); }

} // namespace

extern "C" {

void *vmo_create(double leaf)
{
    Map *m = new Map();
    m->leaf = leaf;
    return m;
}
void vmo_destroy(void *h) { delete static_cast<Map *>(h); }
void vmo_set_mutation(void *h, int mutation) { static_cast<Map *>(h)->mutation = mutation; }
void vmo_clear(void *h)
{
    Map *m = static_cast<Map *>(h);
    m->vox.clear();
    m->arrival.clear();
    m->n_points = 0;
}
long long vmo_n_voxels(void *h) { return (long long)static_cast<Map *>(h)->vox.size(); }
long long vmo_n_points(void *h) { return (long long)static_cast<Map *>(h)->n_points; }

// returns the number of points dropped
int vmo_integrate(void *h, const float *xyz, int n, int stride, const double *R, const double *t)
{
    Map *m = static_cast<Map *>(h);
    int  dropped = 0;
    for (int i = 0; i < n; ++i) {
        const float *p = xyz + (size_t)i * stride;
        float        q[3] = {p[0], p[1], p[2]};
        if (R && t) {
            const double px = p[0], py = p[1], pz = p[2];
            for (int k = 0; k < 3; ++k) {
                const double a = R[3 * k] * px, b = R[3 * k + 1] * py, c = R[3 * k + 2] * pz;
                q[k] = (float)(((a + b) + c) + t[k]);
            }
        }
        uint64_t key = 0;
        int64_t  f[3];
        bool     keep = true;
        for (int k = 0; k < 3 && keep; ++k) {
            const float v = q[k];
            if (!std::isfinite(v) || std::fabs(v) >= 4194304.0f) {
                keep = false;
                break;
            }
            const double d = (double)v / m->leaf;
            const double c = m->mutation == 1 ? std::trunc(d) : std::floor(d);
            if (!(std::fabs(c) < 1048576.0)) {
                keep = false;
                break;
            }
            key |= (uint64_t)((int32_t)c + (1 << 20)) << (21 * k);
            f[k] = (int64_t)std::rint((double)v * 1048576.0); // the default rounding mode: to nearest even
        }
        if (!keep) {
            ++dropped;
            continue;
        }
        auto it = m->vox.find(key);
        if (it == m->vox.end()) {
            it = m->vox.emplace(key, Voxel()).first;
            m->arrival.push_back(key);
        }
        Voxel &v = it->second;
        ++v.count;
        for (int k = 0; k < 3; ++k) v.sum[k] += f[k];
        ++m->n_points;
    }
    return dropped;
}

// Returns the number of qualifying voxels; writes the first `cap` of them (every array nullable).
int vmo_extract(void *h, const float *lo, const float *hi, int min_count, float *xyz4, uint32_t *count, uint64_t *key, int64_t *sums, int cap)
{
    Map                  *m = static_cast<Map *>(h);
    std::vector<uint64_t> order;
    if (m->mutation == 3)
        order = m->arrival;
    else
        for (const auto &kv : m->vox) order.push_back(kv.first);
    int n = 0;
    for (uint64_t k : order) {
        const Voxel &v = m->vox[k];
        if (v.count < (uint32_t)(min_count < 0 ? 0 : min_count)) continue;
        const float c[3] = {centroid(v.sum[0], v.count), centroid(v.sum[1], v.count), centroid(v.sum[2], v.count)};
        if (lo && hi) {
            const bool in = m->mutation == 2 ? (lo[0] < c[0] && c[0] < hi[0] && lo[1] < c[1] && c[1] < hi[1])
                                             : (lo[0] <= c[0] && c[0] <= hi[0] && lo[1] <= c[1] && c[1] <= hi[1]);
            if (!in) continue;
        }
        if (n < cap) {
            if (xyz4) xyz4[4 * n] = c[0], xyz4[4 * n + 1] = c[1], xyz4[4 * n + 2] = c[2], xyz4[4 * n + 3] = 0.0f;
            if (count) count[n] = v.count;
            if (key) key[n] = k;
            if (sums) sums[3 * n] = v.sum[0], sums[3 * n + 1] = v.sum[1], sums[3 * n + 2] = v.sum[2];
        }
        ++n;
    }
    return n;
}

// sizeof and offsets of the parameter struct, for the Python mirror
void vmo_params_layout(int *out)
{
    out[0] = (int)sizeof(slam_vmap_params);
    out[1] = (int)offsetof(slam_vmap_params, leaf);
    out[2] = (int)offsetof(slam_vmap_params, initial_capacity);
}

} // extern "C"
