// vmap_gicp_oracle.cpp -- the scalar restatement of the voxel map's moments, plane distributions and the Generalized ICP
// against them (docs/VOXEL_MAP.md section 9): a std::map over the key, one point at a time.  slam_vmap_read_moments and
// slam_vmap_read_distributions must equal it bit for bit; slam_vmap_register_gicp is held to it as docs/KF_GICP.md holds the
// store's solver (the device sums a block's pairs in another order).  plane_covariance, gicp_pair, gicp_step, move_f32 and
// the stop margin are those of kf_gicp_oracle.cpp, included as text.  Compiled by tests/oracle_build.py with
// -ffp-contract=off.
//
// `mutation` plants one wrong rule, for the tests that have to catch it (tests/test_vmap_gicp_oracle.py):
//   1  truncation instead of floor for e = d / 16
//   2  '<=' instead of '<' at the gate
//   3  voxels that are no plane voxels are paired too (with C' = I)
//   4  the lowest-key rule of an exact tie in d^2 dropped (the highest key wins)
#include <cstddef>
#include <cstdlib>
#include <map>

#include "kf_gicp_oracle.cpp"

namespace {

struct VVoxel {
    uint32_t count = 0, seen = 0, miss = 0;
    int64_t  sum[3] = {0, 0, 0}, E[3] = {0, 0, 0}, M[6] = {0, 0, 0, 0, 0, 0};
    // the distribution
    float  cen[3] = {0, 0, 0};
    double nrm[3] = {0, 0, 0}, cov[6] = {0, 0, 0, 0, 0, 0}, eig[3] = {0, 0, 0};
    int    flag = 0;
};

struct VMap {
    double                     leaf;
    slam_vmap_dist_params      P;
    int                        mutation = 0;
    std::map<uint64_t, VVoxel> vox;
};

// plane_covariance's decomposition with its results laid open: the same text as slam_amd/csrc/kf_gicp_math.hpp
inline void plane_eigen(const double C[6], double lam[3], double nrm[3])
{
    double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#define KF_JACOBI(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                                                  \
    if (apq != 0.0) {                                                                                                                     \
        const double th = (aqq - app) / (2.0 * apq);                                                                                      \
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));                                           \
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;                                                                         \
        app = app - t * apq, aqq = aqq + t * apq, apq = 0.0;                                                                              \
        const double rp = arp, rq = arq, x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;                                      \
        arp = c * rp - s * rq, arq = s * rp + c * rq;                                                                                     \
        v0p = c * x0 - s * y0, v0q = s * x0 + c * y0;                                                                                     \
        v1p = c * x1 - s * y1, v1q = s * x1 + c * y1;                                                                                     \
        v2p = c * x2 - s * y2, v2q = s * x2 + c * y2;                                                                                     \
    }
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        KF_JACOBI(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        KF_JACOBI(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        KF_JACOBI(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    }
#undef KF_JACOBI
    int    n = 0;
    double mn = a00;
    if (a11 <= mn) n = 1, mn = a11;
    if (a22 <= mn) n = 2;
    nrm[0] = n == 0 ? v00 : n == 1 ? v01 : v02, nrm[1] = n == 0 ? v10 : n == 1 ? v11 : v12, nrm[2] = n == 0 ? v20 : n == 1 ? v21 : v22;
    const double p = n == 0 ? a11 : a00, q = n == 2 ? a11 : a22; // the other two, by index
    lam[0] = p >= q ? p : q, lam[1] = p >= q ? q : p, lam[2] = n == 0 ? a00 : n == 1 ? a11 : a22;
}

inline void plane_from_normal(const double nrm[3], double eps, double out[6])
{
    const double nx = nrm[0], ny = nrm[1], nz = nrm[2];
    const double xx = nx * nx, xy = nx * ny, xz = nx * nz, yy = ny * ny, yz = ny * nz, zz = nz * nz;
    out[0] = (1.0 - xx) + eps * xx, out[1] = (0.0 - xy) + eps * xy, out[2] = (0.0 - xz) + eps * xz;
    out[3] = (1.0 - yy) + eps * yy, out[4] = (0.0 - yz) + eps * yz, out[5] = (1.0 - zz) + eps * zz;
}

// the cell of one coordinate by the map's rule; false when it has none
inline bool cell_of(float v, double leaf, int32_t *c)
{
    if (!std::isfinite(v) || std::fabs(v) >= 4194304.0f) return false;
    const double f = std::floor((double)v / leaf);
    if (!(std::fabs(f) < 1048576.0)) return false;
    *c = (int32_t)f;
    return true;
}
inline uint64_t vkey(int64_t x, int64_t y, int64_t z) { return ((uint64_t)(z + (1 << 20)) << 42) | ((uint64_t)(y + (1 << 20)) << 21) | (uint64_t)(x + (1 << 20)); }

void distributions(VMap *m)
{
    for (auto &kv : m->vox) {
        VVoxel &v = kv.second;
        for (int k = 0; k < 3; ++k) v.cen[k] = (float)(((double)v.sum[k] / (double)v.count) * (1.0 / 1048576.0));
        const double n = (double)v.count;
        double       mu[3], s[6];
        for (int k = 0; k < 3; ++k) mu[k] = (double)v.E[k] / n;
        for (int k = 0; k < 6; ++k) s[k] = (double)v.M[k] / n;
        const double scale = 1.0 / 4294967296.0;
        const double c6[6] = {(s[0] - mu[0] * mu[0]) * scale, (s[1] - mu[0] * mu[1]) * scale, (s[2] - mu[0] * mu[2]) * scale,
                              (s[3] - mu[1] * mu[1]) * scale, (s[4] - mu[1] * mu[2]) * scale, (s[5] - mu[2] * mu[2]) * scale};
        double       nn[3];
        plane_eigen(c6, v.eig, nn);
        bool plane = v.count >= (uint32_t)m->P.min_points && v.eig[1] >= m->P.flat_ratio * v.eig[2] && v.eig[1] >= m->P.line_ratio * v.eig[0];
        if (plane && m->P.max_miss_den > 0)
            plane = (uint64_t)v.miss * (uint32_t)m->P.max_miss_den <= (uint64_t)(v.seen > 1u ? v.seen : 1u) * (uint32_t)m->P.max_miss_num;
        v.flag = plane ? 1 : 0;
        for (int k = 0; k < 3; ++k) v.nrm[k] = plane ? nn[k] : 0.0;
        for (int k = 0; k < 6; ++k) v.cov[k] = 0.0;
        if (plane) plane_from_normal(nn, m->P.epsilon, v.cov);
    }
}

// the pair of the moved point x: the plane voxel among the 27 cells around cell(x) with the smallest (d^2, key), or null
const VVoxel *pair_of(const VMap *m, const float x[3], float *d2)
{
    int32_t c[3];
    for (int k = 0; k < 3; ++k)
        if (!cell_of(x[k], m->leaf, &c[k])) return nullptr;
    const VVoxel *best = nullptr;
    float         bd = 0;
    for (int oz = -1; oz <= 1; ++oz)
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) { // ascending key order
                const int64_t X = (int64_t)c[0] + ox, Y = (int64_t)c[1] + oy, Z = (int64_t)c[2] + oz;
                if (std::llabs(X) >= (1 << 20) || std::llabs(Y) >= (1 << 20) || std::llabs(Z) >= (1 << 20)) continue;
                auto it = m->vox.find(vkey(X, Y, Z));
                if (it == m->vox.end()) continue;
                const VVoxel &v = it->second;
                if (!v.flag && m->mutation != 3) continue;
                const float d = dist2(x, v.cen);
                if (!best || d < bd || (m->mutation == 4 && d == bd)) best = &v, bd = d;
            }
    *d2 = bd;
    return best;
}

inline bool inside(const VMap *m, float d2, double gate2) { return m->mutation == 2 ? (double)d2 <= gate2 : (double)d2 < gate2; }

const double kIdentity6[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};

void vregister(VMap *m, const float *src, int ns, int stride, const double *src_cov, const float init[16], const slam_vmap_gicp_params &P,
               slam_vmap_gicp_result *out, int32_t *trace, int trace_cap, double *margin, double *fitness_abs)
{
    distributions(m);
    const double gate2 = P.gate * P.gate;
    double       T[12];
    for (int i = 0; i < 12; ++i) T[i] = init[i];
    int    iterations = 0, state = 0, pairs = 0;
    double mse = 0, cost = 0, H[36];
    Margin mg;
    std::memset(H, 0, sizeof H);
    for (int i = 0; i < trace_cap; ++i) trace[i] = -1;
    for (;;) {
        double h[21], g[6], c = 0, sum = 0;
        std::memset(h, 0, sizeof h), std::memset(g, 0, sizeof g);
        pairs = 0;
        for (int i = 0; i < ns; ++i) {
            const float *p = src + (size_t)i * stride;
            float        x[3], d2;
            for (int r = 0; r < 3; ++r) x[r] = (float)(((T[4 * r] * (double)p[0] + T[4 * r + 1] * (double)p[1]) + T[4 * r + 2] * (double)p[2]) + T[4 * r + 3]);
            const VVoxel *v = pair_of(m, x, &d2);
            if (!(v && inside(m, d2, gate2))) continue;
            double ph[21], pg[6], pc = 0; // the pair's terms are summed on their own and then added, as a lane of the device adds them
            std::memset(ph, 0, sizeof ph), std::memset(pg, 0, sizeof pg);
            gicp_pair(T, p, v->cen, src_cov + 6 * (size_t)i, v->flag ? v->cov : kIdentity6, ph, pg, &pc);
            for (int e = 0; e < 21; ++e) h[e] += ph[e];
            for (int e = 0; e < 6; ++e) g[e] += pg[e];
            c += pc, sum += (double)d2, ++pairs;
        }
        mse = pairs ? sum / (double)pairs : 0.0;
        cost = pairs ? c / (double)pairs : 0.0;
        if (iterations < trace_cap) trace[iterations] = pairs;
        int at = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b, ++at) H[6 * a + b] = H[6 * b + a] = h[at];
        if (pairs < 3) {
            state = SLAM_KF_NO_CORRESPONDENCES;
            break;
        }
        double N[12];
        if (!gicp_step(H, g, T, N)) {
            state = SLAM_KF_DEGENERATE;
            break;
        }
        double dr = 0, dt = 0;
        for (int k = 0; k < 12; ++k) {
            const double d = std::fabs(N[k] - T[k]);
            if (k % 4 == 3)
                dt = d > dt ? d : dt;
            else
                dr = d > dr ? d : dr;
        }
        std::memcpy(T, N, sizeof T);
        ++iterations;
        if (iterations >= P.max_iterations) {
            state = SLAM_KF_ITERATIONS;
            break;
        }
        mg.see(dr, P.rotation_epsilon);
        if (dr <= P.rotation_epsilon) mg.see(dt, P.transformation_epsilon);
        if (dr <= P.rotation_epsilon && dt <= P.transformation_epsilon) {
            state = SLAM_KF_TRANSFORM;
            break;
        }
    }
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < 12; ++i) out->transform64[i] = T[i], out->transform[i] = (float)T[i];
    out->transform64[15] = 1.0, out->transform[15] = 1.0f;
    out->iterations = iterations, out->state = state, out->converged = state == SLAM_KF_ITERATIONS || state == SLAM_KF_TRANSFORM;
    out->pairs = pairs, out->mse = mse, out->cost = cost;
    std::memcpy(out->hessian, H, sizeof H);
    if (margin) *margin = mg.m;
    // the fitness: the f32 transform, points moved in f32, the same pairing, (n . (q - x))^2 in f64
    double fsum = 0;
    int    fn = 0;
    for (int i = 0; i < ns; ++i) {
        float s[3], d2;
        move_f32(out->transform, src + (size_t)i * stride, s);
        const VVoxel *v = pair_of(m, s, &d2);
        if (!(v && inside(m, d2, gate2))) continue;
        const double r0 = (double)v->cen[0] - (double)s[0], r1 = (double)v->cen[1] - (double)s[1], r2 = (double)v->cen[2] - (double)s[2];
        const double dot = (v->nrm[0] * r0 + v->nrm[1] * r1) + v->nrm[2] * r2;
        fsum += dot * dot, ++fn;
    }
    out->fitness_pairs = fn, out->fitness = fn ? fsum / (double)fn : 0.0;
    if (fitness_abs) *fitness_abs = fsum;
}

} // namespace

extern "C" {

void vgo_default_dist_params(slam_vmap_dist_params *p)
{
    p->min_points = 6, p->flat_ratio = 4.0, p->line_ratio = 0.01, p->epsilon = 1e-3, p->max_miss_num = 0, p->max_miss_den = 0;
}
void vgo_default_gicp_params(slam_vmap_gicp_params *p)
{
    p->gate = 2.0, p->max_iterations = 100, p->transformation_epsilon = 1e-6, p->rotation_epsilon = 2e-3;
}
void *vgo_create(double leaf)
{
    VMap *m = new VMap();
    m->leaf = leaf;
    vgo_default_dist_params(&m->P);
    return m;
}
// slam_vmap_enable_distributions' refusals: a map that holds voxels, leaf > 8; 0 or SLAM_E_INVALID
int vgo_enable(void *h, const slam_vmap_dist_params *p)
{
    VMap *m = static_cast<VMap *>(h);
    if (!m->vox.empty() || m->leaf > 8.0) return SLAM_E_INVALID;
    if (p) m->P = *p;
    return SLAM_OK;
}
void vgo_destroy(void *h) { delete static_cast<VMap *>(h); }
void vgo_set_mutation(void *h, int mutation) { static_cast<VMap *>(h)->mutation = mutation; }
void vgo_clear(void *h) { static_cast<VMap *>(h)->vox.clear(); }
long long vgo_n_voxels(void *h) { return (long long)static_cast<VMap *>(h)->vox.size(); }

// returns the number of points dropped
int vgo_integrate(void *h, const float *xyz, int n, int stride, const double *R, const double *t)
{
    VMap         *m = static_cast<VMap *>(h);
    const int64_t L = (int64_t)std::rint(m->leaf * 1048576.0);
    int           dropped = 0;
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
        int32_t c[3];
        int64_t f[3], e[3];
        bool    keep = true;
        for (int k = 0; k < 3 && keep; ++k) {
            keep = cell_of(q[k], m->leaf, &c[k]);
            if (!keep) break;
            f[k] = (int64_t)std::rint((double)q[k] * 1048576.0);
            const int64_t d = f[k] - (int64_t)c[k] * L;
            e[k] = m->mutation == 1 ? d / 16 : (d - ((d % 16 + 16) % 16)) / 16; // floor, without relying on the shift of a negative
        }
        if (!keep) {
            ++dropped;
            continue;
        }
        VVoxel &v = m->vox[vkey(c[0], c[1], c[2])];
        ++v.count;
        for (int k = 0; k < 3; ++k) v.sum[k] += f[k], v.E[k] += e[k];
        v.M[0] += e[0] * e[0], v.M[1] += e[0] * e[1], v.M[2] += e[0] * e[2];
        v.M[3] += e[1] * e[1], v.M[4] += e[1] * e[2], v.M[5] += e[2] * e[2];
    }
    return dropped;
}

// carve evidence from outside (tests/vmap_carve_oracle.py or the device's planes): seen and miss of the voxels named by key
void vgo_set_carve(void *h, const uint64_t *key, const uint32_t *seen, const uint32_t *miss, int n)
{
    VMap *m = static_cast<VMap *>(h);
    for (int i = 0; i < n; ++i) {
        auto it = m->vox.find(key[i]);
        if (it != m->vox.end()) it->second.seen = seen[i], it->second.miss = miss[i];
    }
}

// every voxel in key order, the distributions computed first; returns their number and writes the first `cap`
int vgo_read(void *h, int cap, uint64_t *key, uint32_t *count, int64_t *sums, int64_t *E3, int64_t *M6, float *cen3, double *nrm3, double *cov6,
             double *eig3, uint8_t *flag)
{
    VMap *m = static_cast<VMap *>(h);
    distributions(m);
    int n = 0;
    for (const auto &kv : m->vox) {
        const VVoxel &v = kv.second;
        if (n < cap) {
            if (key) key[n] = kv.first;
            if (count) count[n] = v.count;
            for (int k = 0; k < 3; ++k) {
                if (sums) sums[3 * n + k] = v.sum[k];
                if (E3) E3[3 * n + k] = v.E[k];
                if (cen3) cen3[3 * n + k] = v.cen[k];
                if (nrm3) nrm3[3 * n + k] = v.nrm[k];
                if (eig3) eig3[3 * n + k] = v.eig[k];
            }
            for (int k = 0; k < 6; ++k) {
                if (M6) M6[6 * n + k] = v.M[k];
                if (cov6) cov6[6 * n + k] = v.cov[k];
            }
            if (flag) flag[n] = (uint8_t)v.flag;
        }
        ++n;
    }
    return n;
}

void vgo_register(void *h, const float *src, int ns, int stride, const double *src_cov, const float *init, const slam_vmap_gicp_params *P,
                  slam_vmap_gicp_result *out, int32_t *trace, int trace_cap, double *margin, double *fitness_abs)
{
    vregister(static_cast<VMap *>(h), src, ns, stride, src_cov, init, *P, out, trace, trace_cap, margin, fitness_abs);
}

// sizeof and offsets of the new structs, for the Python mirrors
void vgo_layout(int *o)
{
    int at = 0;
    o[at++] = (int)sizeof(slam_vmap_dist_params);
    o[at++] = (int)offsetof(slam_vmap_dist_params, min_points), o[at++] = (int)offsetof(slam_vmap_dist_params, flat_ratio);
    o[at++] = (int)offsetof(slam_vmap_dist_params, line_ratio), o[at++] = (int)offsetof(slam_vmap_dist_params, epsilon);
    o[at++] = (int)offsetof(slam_vmap_dist_params, max_miss_num), o[at++] = (int)offsetof(slam_vmap_dist_params, max_miss_den);
    o[at++] = (int)sizeof(slam_vmap_gicp_req);
    o[at++] = (int)offsetof(slam_vmap_gicp_req, src), o[at++] = (int)offsetof(slam_vmap_gicp_req, init);
    o[at++] = (int)sizeof(slam_vmap_gicp_params);
    o[at++] = (int)offsetof(slam_vmap_gicp_params, gate), o[at++] = (int)offsetof(slam_vmap_gicp_params, max_iterations);
    o[at++] = (int)offsetof(slam_vmap_gicp_params, transformation_epsilon), o[at++] = (int)offsetof(slam_vmap_gicp_params, rotation_epsilon);
    o[at++] = (int)sizeof(slam_vmap_gicp_result);
    o[at++] = (int)offsetof(slam_vmap_gicp_result, transform), o[at++] = (int)offsetof(slam_vmap_gicp_result, transform64);
    o[at++] = (int)offsetof(slam_vmap_gicp_result, iterations), o[at++] = (int)offsetof(slam_vmap_gicp_result, state);
    o[at++] = (int)offsetof(slam_vmap_gicp_result, converged), o[at++] = (int)offsetof(slam_vmap_gicp_result, pairs);
    o[at++] = (int)offsetof(slam_vmap_gicp_result, mse), o[at++] = (int)offsetof(slam_vmap_gicp_result, cost);
    o[at++] = (int)offsetof(slam_vmap_gicp_result, hessian), o[at++] = (int)offsetof(slam_vmap_gicp_result, fitness);
    o[at++] = (int)offsetof(slam_vmap_gicp_result, fitness_pairs), o[at++] = (int)offsetof(slam_vmap_gicp_result, reserved);
}

} // extern "C"
