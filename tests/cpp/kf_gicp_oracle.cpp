// kf_gicp_oracle.cpp -- scalar restatement of the store's Generalized ICP (docs/KF_GICP.md), the yardstick
// slam_kf_compute_covariances and slam_kf_register_gicp are held against.  pcl::GeneralizedIterativeClosestPoint cannot be
// built here, so this is a stated contract ("restated, unpinned" as docs/KF_EDGE.md section 2 has it), and it deviates
// from PCL on purpose: one Gauss-Newton step per outer iteration where PCL runs BFGS, f64 sums, covariances centred on
// the query point, neighbours from within a radius, a gated fitness.
//   neighbours     brute force over the whole cloud, ordered by (f32 d^2, index)
//   covariance     C' = V diag(1, 1, eps) V' from the sums in list order; plane_covariance below is the device's text
//   gicp           pairs by a gated 1-NN (strict), gicp_pair / gicp_step below are the device's text; sums in source order
//   fitness        mean f32 d^2 of the source points, moved in f32, whose 1-NN lies strictly inside the gate
// Built by tests/kf_gicp_oracle.py with g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "kf_oracle_common.hpp"
#include "slam_mi355x.h"

namespace {

constexpr int kJacobiSweeps = 8;

inline void plane_covariance(const double C[6], double eps, double out[6])
{
    double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#define KF_JACOBI(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                                                  \
    if (apq != 0.0) {                                                                                                                     \
        const double th = (aqq - app) / (2.0 * apq);                                                                                      \
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));                                                     \
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;                                                                              \
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
    const double nx = n == 0 ? v00 : n == 1 ? v01 : v02, ny = n == 0 ? v10 : n == 1 ? v11 : v12, nz = n == 0 ? v20 : n == 1 ? v21 : v22;
    const double xx = nx * nx, xy = nx * ny, xz = nx * nz, yy = ny * ny, yz = ny * nz, zz = nz * nz;
    out[0] = (1.0 - xx) + eps * xx, out[1] = (0.0 - xy) + eps * xy, out[2] = (0.0 - xz) + eps * xz;
    out[3] = (1.0 - yy) + eps * yy, out[4] = (0.0 - yz) + eps * yz, out[5] = (1.0 - zz) + eps * zz;
}

inline void gicp_pair(const double T[12], const float p[3], const float q[3], const double Cp[6], const double Cq[6], double h[21],
                                 double g[6], double *cost)
{
    double x[3], r[3];
    for (int k = 0; k < 3; ++k) {
        x[k] = ((T[4 * k] * (double)p[0] + T[4 * k + 1] * (double)p[1]) + T[4 * k + 2] * (double)p[2]) + T[4 * k + 3];
        r[k] = (double)q[k] - x[k];
    }
    const double cp[9] = {Cp[0], Cp[1], Cp[2], Cp[1], Cp[3], Cp[4], Cp[2], Cp[4], Cp[5]};
    double       B[9], A[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) B[3 * a + b] = (T[4 * a] * cp[b] + T[4 * a + 1] * cp[3 + b]) + T[4 * a + 2] * cp[6 + b];
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) A[3 * a + b] = (B[3 * a] * T[4 * b] + B[3 * a + 1] * T[4 * b + 1]) + B[3 * a + 2] * T[4 * b + 2];
    const double s00 = Cq[0] + A[0], s01 = Cq[1] + A[1], s02 = Cq[2] + A[2], s11 = Cq[3] + A[4], s12 = Cq[4] + A[5], s22 = Cq[5] + A[8];
    const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    const double M[9] = {c00 / det, c01 / det, c02 / det, c01 / det, c11 / det, c12 / det, c02 / det, c12 / det, c22 / det};
    const double J[18] = {0.0, -x[2], x[1], -1.0, 0.0, 0.0, x[2], 0.0, -x[0], 0.0, -1.0, 0.0, -x[1], x[0], 0.0, 0.0, 0.0, -1.0};
    double       Mr[3], MJ[18];
    for (int a = 0; a < 3; ++a) {
        Mr[a] = (M[3 * a] * r[0] + M[3 * a + 1] * r[1]) + M[3 * a + 2] * r[2];
        for (int b = 0; b < 6; ++b) MJ[6 * a + b] = (M[3 * a] * J[b] + M[3 * a + 1] * J[6 + b]) + M[3 * a + 2] * J[12 + b];
    }
    int at = 0;
    for (int a = 0; a < 6; ++a) {
        g[a] += (J[a] * Mr[0] + J[6 + a] * Mr[1]) + J[12 + a] * Mr[2];
        for (int b = a; b < 6; ++b, ++at) h[at] += (J[a] * MJ[b] + J[6 + a] * MJ[6 + b]) + J[12 + a] * MJ[12 + b];
    }
    *cost += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
}

inline bool gicp_step(const double H[36], const double g[6], const double T[12], double N[12])
{
    double L[36], y[6], xi[6];
    bool   ok = true;
    for (int k = 0; k < 6; ++k) {
        double d = H[6 * k + k];
        for (int j = 0; j < k; ++j) d -= L[6 * k + j] * L[6 * k + j];
        if (!(d > 0.0) || !(d <= DBL_MAX)) ok = false;
        L[6 * k + k] = std::sqrt(d);
        for (int i = k + 1; i < 6; ++i) {
            double s = H[6 * i + k];
            for (int j = 0; j < k; ++j) s -= L[6 * i + j] * L[6 * k + j];
            L[6 * i + k] = s / L[6 * k + k];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
        for (int j = 0; j < i; ++j) s -= L[6 * i + j] * y[j];
        y[i] = s / L[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int j = i + 1; j < 6; ++j) s -= L[6 * j + i] * xi[j];
        xi[i] = s / L[6 * i + i];
    }
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double       a, b;
    if (th2 < 1e-16) {
        a = 1.0 - th2 / 6.0, b = 0.5 - th2 / 24.0;
    } else {
        const double th = std::sqrt(th2);
        a = std::sin(th) / th, b = (1.0 - std::cos(th)) / th2;
    }
    // I + a [w]x + b [w]x^2, [w]x^2 = w w' - theta^2 I
    const double Rs[9] = {1.0 + b * (wx * wx - th2), b * (wx * wy) - a * wz,     b * (wx * wz) + a * wy,
                          b * (wx * wy) + a * wz,     1.0 + b * (wy * wy - th2), b * (wy * wz) - a * wx,
                          b * (wx * wz) - a * wy,     b * (wy * wz) + a * wx,     1.0 + b * (wz * wz - th2)};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) N[4 * r + c] = (Rs[3 * r] * T[c] + Rs[3 * r + 1] * T[4 + c]) + Rs[3 * r + 2] * T[8 + c];
        N[4 * r + 3] = ((Rs[3 * r] * T[3] + Rs[3 * r + 1] * T[7]) + Rs[3 * r + 2] * T[11]) + xi[3 + r];
    }
    return ok;
}


// ---------------------------------------------------------------- neighbour lists and covariances
// idx / d2: k per point (-1 / 0 behind the last), cnt: the list's length.  Every point of the cloud is a candidate.
void neighbours(const float *xyz, int n, int stride, int k, double radius, int32_t *idx, float *d2, int32_t *cnt)
{
    const double r2 = radius * radius;
    std::vector<std::pair<float, int>> cand;
    for (int i = 0; i < n; ++i) {
        cand.clear();
        for (int j = 0; j < n; ++j) {
            const float d = dist2(xyz + (size_t)i * stride, xyz + (size_t)j * stride);
            if ((double)d <= r2) cand.emplace_back(d, j);
        }
        std::sort(cand.begin(), cand.end()); // by d^2, then by index
        const int m = std::min((int)cand.size(), k);
        for (int e = 0; e < k; ++e) idx[(size_t)i * k + e] = e < m ? cand[e].second : -1, d2[(size_t)i * k + e] = e < m ? cand[e].first : 0.0f;
        cnt[i] = m;
    }
}

void covariances(const float *xyz, int n, int stride, int k, const int32_t *idx, const int32_t *cnt, double eps, int min_nbr, double *cov6)
{
    for (int i = 0; i < n; ++i) {
        double      *C = cov6 + 6 * (size_t)i;
        const int    m = cnt[i];
        const float *p = xyz + (size_t)i * stride;
        C[0] = C[3] = C[5] = 1.0, C[1] = C[2] = C[4] = 0.0;
        if (m < min_nbr) continue;
        double s1x = 0, s1y = 0, s1z = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
        for (int e = 0; e < m; ++e) {
            const float *q = xyz + (size_t)idx[(size_t)i * k + e] * stride;
            const double dx = (double)q[0] - (double)p[0], dy = (double)q[1] - (double)p[1], dz = (double)q[2] - (double)p[2];
            s1x += dx, s1y += dy, s1z += dz;
            sxx += dx * dx, sxy += dx * dy, sxz += dx * dz, syy += dy * dy, syz += dy * dz, szz += dz * dz;
        }
        const double dm = (double)m, mx = s1x / dm, my = s1y / dm, mz = s1z / dm;
        const double raw[6] = {sxx / dm - mx * mx, sxy / dm - mx * my, sxz / dm - mx * mz, syy / dm - my * my, syz / dm - my * mz, szz / dm - mz * mz};
        plane_covariance(raw, eps, C);
    }
}

// ---------------------------------------------------------------- the iteration
void gicp(const Index &tgt, const float *src, int ns, int stride, const double *src_cov, const float init[16], double gate,
          const slam_kf_gicp_params &P, slam_kf_gicp_result *out, int32_t *trace, int trace_cap, double *margin)
{
    const double gate2 = gate * gate;
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
            float        m[3], d2;
            for (int r = 0; r < 3; ++r) m[r] = (float)(((T[4 * r] * (double)p[0] + T[4 * r + 1] * (double)p[1]) + T[4 * r + 2] * (double)p[2]) + T[4 * r + 3]);
            const int j = nearest(tgt, m, &d2);
            if (!(j >= 0 && (double)d2 < gate2)) continue; // strict
            // the pair's terms are summed on their own and then added, as a lane of the device adds them
            double ph[21], pg[6], pc = 0;
            std::memset(ph, 0, sizeof ph), std::memset(pg, 0, sizeof pg);
            gicp_pair(T, p, &tgt.p[3 * (size_t)j], src_cov + 6 * (size_t)i, &tgt.cov[6 * (size_t)j], ph, pg, &pc);
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
    slam_kf_edge_result *e = &out->edge;
    for (int i = 0; i < 12; ++i) e->transform64[i] = T[i], e->transform[i] = (float)T[i];
    e->transform64[15] = 1.0, e->transform[15] = 1.0f;
    e->iterations = iterations, e->state = state, e->converged = state == SLAM_KF_ITERATIONS || state == SLAM_KF_TRANSFORM;
    e->pairs = pairs, e->mse = mse;
    out->cost = cost;
    std::memcpy(out->hessian, H, sizeof H);
    if (margin) *margin = mg.m;
}

} // namespace

extern "C" {

int kgo_covariances(const float *xyz, int n, int stride, int k, double radius, double eps, int min_nbr, double *cov6, int32_t *idx, float *d2,
                    int32_t *cnt)
{
    if (n < k) return SLAM_E_INVALID; // as PCL refuses a cloud of fewer than k points
    neighbours(xyz, n, stride, k, radius, idx, d2, cnt);
    covariances(xyz, n, stride, k, idx, cnt, eps, min_nbr, cov6);
    return SLAM_OK;
}
void kgo_plane_covariance(const double *C6, double eps, double *out6) { plane_covariance(C6, eps, out6); }
// one pair's terms from zero: h21, g6, cost
void kgo_pair(const double *T12, const float *p, const float *q, const double *Cp, const double *Cq, double *h21, double *g6, double *cost)
{
    std::memset(h21, 0, 21 * sizeof(double)), std::memset(g6, 0, 6 * sizeof(double));
    *cost = 0;
    gicp_pair(T12, p, q, Cp, Cq, h21, g6, cost);
}
int kgo_step(const double *H36, const double *g6, const double *T12, double *N12) { return gicp_step(H36, g6, T12, N12) ? 1 : 0; }

void *kgo_index_create(const float *xyz, int n, int stride, double cell, const double *cov6)
{
    Index *ix = new Index();
    ix->n = n, ix->inv = 1.0 / cell;
    ix->p.resize(3 * (size_t)n);
    ix->cov.assign(cov6, cov6 + 6 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) ix->p[3 * (size_t)i + k] = xyz[(size_t)i * stride + k];
        const float *p = &ix->p[3 * (size_t)i];
        ix->cells[key_of(coord(p[0], ix->inv), coord(p[1], ix->inv), coord(p[2], ix->inv))].push_back(i);
    }
    return ix;
}
void kgo_index_destroy(void *h) { delete static_cast<Index *>(h); }
void kgo_gicp(void *tgt, const float *src, int ns, int stride, const double *src_cov, const float *init, double gate, const slam_kf_gicp_params *P,
              slam_kf_gicp_result *out, int32_t *trace, int trace_cap, double *margin)
{
    gicp(*static_cast<Index *>(tgt), src, ns, stride, src_cov, init, gate, *P, out, trace, trace_cap, margin);
}
// fitness and fitness_pairs of `out` from out->edge.transform; abs_sum (optional): the sum of the terms, for the bound
void kgo_fitness(void *tgt, const float *src, int ns, int stride, double gate, slam_kf_gicp_result *out, double *abs_sum)
{
    const Index &ix = *static_cast<Index *>(tgt);
    const double gate2 = gate * gate;
    double       sum = 0;
    int          n = 0;
    for (int i = 0; i < ns; ++i) {
        float s[3], d2;
        move_f32(out->edge.transform, src + (size_t)i * stride, s);
        const int j = nearest(ix, s, &d2);
        if (!(j >= 0 && (double)d2 < gate2)) continue;
        sum += (double)d2, ++n;
    }
    out->fitness_pairs = n, out->fitness = n ? sum / (double)n : 0.0;
    if (abs_sum) *abs_sum = sum;
}
}
