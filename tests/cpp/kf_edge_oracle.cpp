// kf_edge_oracle.cpp -- scalar restatement of graph_slam's keyframe edge (graph_slam/src/graphSlamTools.cpp), the
// yardstick slam_kf_* is held against:
//   setup_gicp                       :27-39    gate 0.75, 200 iterations, both epsilons 1e-6
//   computeEdgeInformationLUM        :108-214
//   calcEdgeIcp                      :218-364  (the ICP is pcl::IterativeClosestPoint<PointXYZ, PointXYZ>::align)
// PCL, Eigen, FLANN and tf are not available to this project, so the PCL side -- correspondence estimation,
// TransformationEstimationSVD (Eigen::umeyama without scaling), DefaultConvergenceCriteria -- is restated from what
// PCL 1.7 is known to do, as the rules of docs/KF_EDGE.md ("restated, unpinned").  Nothing here is compiled from it.
//
// Two modes.  mode 0 is the contract of the device path: sums, SVD and the total transform in double, every iteration
// moves the ORIGINAL f32 points by the TOTAL transform and rounds once.  mode 1 follows PCL's own order of operations in
// float (the moved cloud is moved again by each step, Matrix4f products, float SVD); the difference between the two
// is what the stated deviation costs, and docs/KF_EDGE.md records it.
//
// Built by tests/kf_edge_oracle.py with g++ -O2 -ffp-contract=off (the reference is x86-64 without FMA).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

#include "kf_oracle_common.hpp"
#include "slam_mi355x.h"

namespace {

// ---------------------------------------------------------------- Umeyama without scaling
// One-sided Jacobi SVD of a 3 x 3 matrix: A = U diag(s) V', s descending.  Columns of U for vanishing singular values
// are completed to a right-handed frame.  Returns the rank (singular values above 3 eps of the largest).
template <typename S>
int svd3(const S A[9], S U[9], S s[3], S V[9])
{
    const S eps = std::numeric_limits<S>::epsilon();
    S a[9];
    for (int i = 0; i < 9; ++i) a[i] = A[i], V[i] = (i % 4 == 0) ? S(1) : S(0);
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                S al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) {
                    al += a[3 * i + p] * a[3 * i + p];
                    be += a[3 * i + q] * a[3 * i + q];
                    ga += a[3 * i + p] * a[3 * i + q];
                }
                if (ga == S(0) || std::fabs(ga) <= eps * std::sqrt(al * be)) continue;
                rotated = true;
                const S zeta = (be - al) / (S(2) * ga);
                const S t = (zeta >= S(0) ? S(1) : S(-1)) / (std::fabs(zeta) + std::sqrt(S(1) + zeta * zeta));
                const S c = S(1) / std::sqrt(S(1) + t * t), sn = c * t;
                for (int i = 0; i < 3; ++i) {
                    const S ap = a[3 * i + p], aq = a[3 * i + q];
                    a[3 * i + p] = c * ap - sn * aq;
                    a[3 * i + q] = sn * ap + c * aq;
                    const S vp = V[3 * i + p], vq = V[3 * i + q];
                    V[3 * i + p] = c * vp - sn * vq;
                    V[3 * i + q] = sn * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < 3; ++j) s[j] = std::sqrt(a[j] * a[j] + a[3 + j] * a[3 + j] + a[6 + j] * a[6 + j]);
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i) // selection sort, descending, stable
        for (int j = i + 1; j < 3; ++j)
            if (s[ord[j]] > s[ord[i]]) std::swap(ord[i], ord[j]);
    S ss[3], vv[9], uu[9];
    for (int j = 0; j < 3; ++j) {
        ss[j] = s[ord[j]];
        for (int i = 0; i < 3; ++i) vv[3 * i + j] = V[3 * i + ord[j]], uu[3 * i + j] = a[3 * i + ord[j]];
    }
    int rank = 0;
    for (int j = 0; j < 3; ++j)
        if (ss[j] > S(0) && ss[j] > S(3) * eps * ss[0]) ++rank;
    for (int j = 0; j < rank; ++j)
        for (int i = 0; i < 3; ++i) uu[3 * i + j] /= ss[j];
    if (rank == 0) {
        for (int i = 0; i < 9; ++i) uu[i] = (i % 4 == 0) ? S(1) : S(0);
    } else {
        if (rank == 1) { // any unit vector orthogonal to u0: u0 x e_k, e_k the axis u0 leans on least
            int k = 0;
            for (int i = 1; i < 3; ++i)
                if (std::fabs(uu[3 * i]) < std::fabs(uu[3 * k])) k = i;
            S e[3] = {0, 0, 0};
            e[k] = 1;
            S w[3] = {uu[3] * e[2] - uu[6] * e[1], uu[6] * e[0] - uu[0] * e[2], uu[0] * e[1] - uu[3] * e[0]};
            const S nw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            for (int i = 0; i < 3; ++i) uu[3 * i + 1] = w[i] / nw;
        }
        if (rank <= 2) { // u2 = u0 x u1
            uu[2] = uu[3] * uu[7] - uu[6] * uu[4];
            uu[5] = uu[6] * uu[1] - uu[0] * uu[7];
            uu[8] = uu[0] * uu[4] - uu[3] * uu[1];
        }
    }
    for (int i = 0; i < 9; ++i) U[i] = uu[i], V[i] = vv[i];
    for (int j = 0; j < 3; ++j) s[j] = ss[j];
    return rank;
}

template <typename S>
S det3(const S m[9])
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// p -> q: centroids, H = sum (q - qm)(p - pm)' / n, R = U diag(1, 1, +-1) V', t = qm - R pm.  Full rank: the sign is that of
// det H; rank 2 (a planar pair set): that of det U det V (Umeyama 1991, eq. 39 ff.); below that the same rule, so that R is
// a proper rotation whatever the pairs.  p, q: 3 floats per pair.
template <typename S>
int solve(const float *p, const float *q, int n, S R[9], S t[3])
{
    S pm[3] = {0, 0, 0}, qm[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) pm[k] += (S)p[3 * i + k], qm[k] += (S)q[3 * i + k];
    for (int k = 0; k < 3; ++k) pm[k] /= (S)n, qm[k] /= (S)n;
    S H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) H[3 * r + c] += ((S)q[3 * i + r] - qm[r]) * ((S)p[3 * i + c] - pm[c]);
    for (int k = 0; k < 9; ++k) H[k] /= (S)n;
    S U[9], s[3], V[9];
    const int rank = svd3(H, U, s, V);
    S sign;
    if (rank == 3)
        sign = det3(H) < S(0) ? S(-1) : S(1);
    else
        sign = det3(U) * det3(V) > S(0) ? S(1) : S(-1);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + sign * U[3 * r + 2] * V[3 * c + 2];
    for (int r = 0; r < 3; ++r) t[r] = qm[r] - ((R[3 * r] * pm[0] + R[3 * r + 1] * pm[1]) + R[3 * r + 2] * pm[2]);
    return rank;
}

// ---------------------------------------------------------------- the ICP loop
// DefaultConvergenceCriteria::hasConverged after a step (R, t), in the order of docs/KF_EDGE.md; 0 = go on
int stop_rule(int iterations, const double R[9], const double t[3], double mse, double *mse_prev, const slam_kf_params &P, Margin *mg)
{
    if (iterations >= P.max_iterations) return SLAM_KF_ITERATIONS;
    const double cosa = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    mg->see(1.0 - cosa, P.transformation_epsilon);
    if (cosa >= 1.0 - P.transformation_epsilon) {
        mg->see(tt, P.transformation_epsilon);
        if (tt <= P.transformation_epsilon) return SLAM_KF_TRANSFORM;
    }
    const double d = std::fabs(mse - *mse_prev);
    mg->see(d, 1e-12);
    if (d < 1e-12) return SLAM_KF_ABS_MSE;
    mg->see(d / *mse_prev, P.fitness_epsilon);
    if (d / *mse_prev < P.fitness_epsilon) return SLAM_KF_REL_MSE;
    *mse_prev = mse;
    return 0;
}

void icp(const Index &tgt, const float *src, int ns, int stride, const float init[16], const slam_kf_params &P, int mode,
         slam_kf_edge_result *out, int32_t *trace, int trace_cap, double *margin)
{
    const double gate2 = P.gate * P.gate;
    double T[16]; // mode 0: the total transform
    float  Tf[16];
    for (int i = 0; i < 16; ++i) T[i] = init[i], Tf[i] = init[i];
    std::vector<float> cur(3 * (size_t)ns), pp, qq;
    if (mode == 1)
        for (int i = 0; i < ns; ++i) move_f32(Tf, src + (size_t)i * stride, &cur[3 * (size_t)i]);
    int    iterations = 0, state = 0, converged = 0, pairs = 0;
    double mse = 0, mse_prev = DBL_MAX;
    Margin mg;
    for (int i = 0; i < trace_cap; ++i) trace[i] = -1;
    for (;;) {
        if (mode == 0)
            for (int i = 0; i < ns; ++i) {
                const float *p = src + (size_t)i * stride;
                for (int r = 0; r < 3; ++r)
                    cur[3 * (size_t)i + r] = (float)(((T[4 * r] * (double)p[0] + T[4 * r + 1] * (double)p[1]) + T[4 * r + 2] * (double)p[2]) + T[4 * r + 3]);
            }
        pp.clear(), qq.clear();
        double sum = 0;
        for (int i = 0; i < ns; ++i) {
            float     d2;
            const int j = nearest(tgt, &cur[3 * (size_t)i], &d2);
            if (j < 0 || !((double)d2 <= gate2)) continue; // PCL skips on > (a NaN distance is dropped here)
            for (int k = 0; k < 3; ++k) pp.push_back(cur[3 * (size_t)i + k]), qq.push_back(tgt.p[3 * (size_t)j + k]);
            sum += (double)d2;
        }
        pairs = (int)(pp.size() / 3);
        mse = pairs ? sum / (double)pairs : 0.0;
        if (iterations < trace_cap) trace[iterations] = pairs;
        if (pairs < 3) {
            state = SLAM_KF_NO_CORRESPONDENCES;
            converged = 0;
            break;
        }
        double R[9], t[3];
        if (mode == 0) {
            solve<double>(pp.data(), qq.data(), pairs, R, t);
            double N[16];
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) N[4 * r + c] = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
                N[4 * r + 3] = ((R[3 * r] * T[3] + R[3 * r + 1] * T[7]) + R[3 * r + 2] * T[11]) + t[r];
            }
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) T[4 * r + c] = N[4 * r + c];
        } else {
            float Rf[9], tf[3], St[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, N[16];
            solve<float>(pp.data(), qq.data(), pairs, Rf, tf);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) St[4 * r + c] = Rf[3 * r + c], R[3 * r + c] = Rf[3 * r + c];
                St[4 * r + 3] = tf[r], t[r] = tf[r];
            }
            std::vector<float> nxt(cur.size());
            for (int i = 0; i < ns; ++i) move_f32(St, &cur[3 * (size_t)i], &nxt[3 * (size_t)i]);
            cur.swap(nxt);
            for (int r = 0; r < 4; ++r) // final_transformation_ = transformation_ * final_transformation_
                for (int c = 0; c < 4; ++c) N[4 * r + c] = ((St[4 * r] * Tf[c] + St[4 * r + 1] * Tf[4 + c]) + St[4 * r + 2] * Tf[8 + c]) + St[4 * r + 3] * Tf[12 + c];
            std::memcpy(Tf, N, sizeof N);
        }
        ++iterations;
        state = stop_rule(iterations, R, t, mse, &mse_prev, P, &mg);
        if (state) {
            converged = 1;
            break;
        }
    }
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < 16; ++i) {
        out->transform64[i] = mode == 0 ? T[i] : (double)Tf[i];
        out->transform[i] = mode == 0 ? (float)T[i] : Tf[i];
    }
    out->iterations = iterations, out->state = state, out->converged = converged, out->pairs = pairs, out->mse = mse;
    if (margin) *margin = mg.m;
}

// ---------------------------------------------------------------- computeEdgeInformationLUM, :108-214
// Eigen's inverse of a fixed 6 x 6 goes through PartialPivLU; so does this.  A vanishing pivot divides by zero and the
// non-finite entries travel on to ss, where :203 catches them.
void inverse6(const double A[36], double X[36])
{
    double a[36];
    int    piv[6];
    std::memcpy(a, A, sizeof a);
    for (int i = 0; i < 6; ++i) piv[i] = i;
    for (int k = 0; k < 6; ++k) {
        int m = k;
        for (int i = k + 1; i < 6; ++i)
            if (std::fabs(a[6 * i + k]) > std::fabs(a[6 * m + k])) m = i;
        if (m != k) {
            for (int c = 0; c < 6; ++c) std::swap(a[6 * k + c], a[6 * m + c]);
            std::swap(piv[k], piv[m]);
        }
        for (int i = k + 1; i < 6; ++i) {
            a[6 * i + k] /= a[6 * k + k];
            for (int c = k + 1; c < 6; ++c) a[6 * i + c] -= a[6 * i + k] * a[6 * k + c];
        }
    }
    for (int col = 0; col < 6; ++col) {
        double y[6];
        for (int i = 0; i < 6; ++i) {
            y[i] = piv[i] == col ? 1.0 : 0.0;
            for (int c = 0; c < i; ++c) y[i] -= a[6 * i + c] * y[c];
        }
        for (int i = 5; i >= 0; --i) {
            for (int c = i + 1; c < 6; ++c) y[i] -= a[6 * i + c] * y[c];
            y[i] /= a[6 * i + i];
        }
        for (int i = 0; i < 6; ++i) X[6 * i + col] = y[i];
    }
}

struct LumOut {
    double info[36], MM[36], MZ[6];
    int    num_corr, singular;
    float  ss;
};

void lum(const Index &tgt, const float *src, int ns, int stride, const float T[16], double gate, LumOut *o, float *aver_out, float *diff_out)
{
    std::vector<float> aver, diff;
    const double       gate2 = gate * gate;
    for (int i = 0; i < ns; ++i) {
        float s[3], d2;
        move_f32(T, src + (size_t)i * stride, s); // :301 pcl::transformPointCloud(*to_cld, *temp, transformation)
        const int j = nearest(tgt, s, &d2);
        if (j < 0 || !((double)d2 < gate2)) continue; // :132, strict
        for (int k = 0; k < 3; ++k) {
            const float t = tgt.p[3 * (size_t)j + k];
            aver.push_back(0.5f * (s[k] + t)); // :138-139
            diff.push_back(s[k] - t);
        }
    }
    const int n = (int)(aver.size() / 3);
    if (aver_out) std::memcpy(aver_out, aver.data(), aver.size() * sizeof(float));
    if (diff_out) std::memcpy(diff_out, diff.data(), diff.size() * sizeof(float));
    double MM[36], MZ[6];
    std::memset(MM, 0, sizeof MM), std::memset(MZ, 0, sizeof MZ);
#define M(r, c) MM[6 * (r) + (c)]
    for (int ci = 0; ci < n; ++ci) { // :153-176, the float products as the reference's Vector3f gives them
        const float *a = &aver[3 * (size_t)ci], *d = &diff[3 * (size_t)ci];
        M(0, 4) -= a[1];
        M(0, 5) += a[2];
        M(1, 3) -= a[2];
        M(1, 4) += a[0];
        M(2, 3) += a[1];
        M(2, 5) -= a[0];
        M(3, 4) -= a[0] * a[2];
        M(3, 5) -= a[0] * a[1];
        M(4, 5) -= a[1] * a[2];
        M(3, 3) += a[1] * a[1] + a[2] * a[2];
        M(4, 4) += a[0] * a[0] + a[1] * a[1];
        M(5, 5) += a[0] * a[0] + a[2] * a[2];
        MZ[0] += d[0];
        MZ[1] += d[1];
        MZ[2] += d[2];
        MZ[3] += a[1] * d[2] - a[2] * d[1];
        MZ[4] += a[0] * d[1] - a[1] * d[0];
        MZ[5] += a[2] * d[0] - a[0] * d[2];
    }
    M(0, 0) = M(1, 1) = M(2, 2) = static_cast<float>(n); // :179-188
    M(4, 0) = M(0, 4);
    M(5, 0) = M(0, 5);
    M(3, 1) = M(1, 3);
    M(4, 1) = M(1, 4);
    M(3, 2) = M(2, 3);
    M(5, 2) = M(2, 5);
    M(4, 3) = M(3, 4);
    M(5, 3) = M(3, 5);
    M(5, 4) = M(4, 5);
#undef M
    double inv[36], D[6];
    inverse6(MM, inv);
    for (int r = 0; r < 6; ++r) { // :191
        D[r] = 0;
        for (int c = 0; c < 6; ++c) D[r] += inv[6 * r + c] * MZ[c];
    }
    float ss = 0.0f;
    for (int ci = 0; ci < n; ++ci) { // :194-200, signs and index pairs as written there
        const float *a = &aver[3 * (size_t)ci], *d = &diff[3 * (size_t)ci];
        const double e0 = (double)d[0] - ((D[0] + (double)a[2] * D[5]) - (double)a[1] * D[4]);
        const double e1 = (double)d[1] - ((D[1] + (double)a[0] * D[4]) - (double)a[2] * D[3]);
        const double e2 = (double)d[2] - ((D[2] + (double)a[1] * D[3]) - (double)a[0] * D[5]);
        ss += static_cast<float>((e0 * e0 + e1 * e1) + e2 * e2);
    }
    std::memcpy(o->MM, MM, sizeof MM), std::memcpy(o->MZ, MZ, sizeof MZ);
    o->num_corr = n, o->ss = ss;
    if (ss < 0.0000000000001 || !std::isfinite(ss)) { // :203-208
        o->singular = 1;
        for (int i = 0; i < 36; ++i) o->info[i] = (i % 7 == 0) ? 1.0 : 0.0;
        return;
    }
    o->singular = 0;
    const float w = 1.0f / ss; // :211 MM * (1.0f / ss)
    for (int i = 0; i < 36; ++i) o->info[i] = MM[i] * (double)w;
}

} // namespace

extern "C" {

// cell: the lattice edge as the store makes it (slam_kf_keyframe_info does not return it: cell_size or gate, times 1 + 2^-16)
void *kfo_index_create(const float *xyz, int n, int stride, double cell)
{
    Index *ix = new Index();
    ix->n = n, ix->inv = 1.0 / cell;
    ix->p.resize(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) ix->p[3 * (size_t)i + k] = xyz[(size_t)i * stride + k];
        const float *p = &ix->p[3 * (size_t)i];
        ix->cells[key_of(coord(p[0], ix->inv), coord(p[1], ix->inv), coord(p[2], ix->inv))].push_back(i);
    }
    return ix;
}
void kfo_index_destroy(void *h) { delete static_cast<Index *>(h); }
void kfo_index_stats(void *h, int *cells, int *max_cell)
{
    const Index *ix = static_cast<Index *>(h);
    *cells = (int)ix->cells.size(), *max_cell = 0;
    for (const auto &kv : ix->cells) *max_cell = std::max(*max_cell, (int)kv.second.size());
}
void kfo_nearest(void *h, const float *q, int n, int stride, double gate, int strict, int32_t *idx, float *d2)
{
    const Index *ix = static_cast<Index *>(h);
    const double g2 = gate * gate;
    for (int i = 0; i < n; ++i) {
        float     d;
        const int j = nearest(*ix, q + (size_t)i * stride, &d);
        const bool keep = j >= 0 && (strict ? (double)d < g2 : (double)d <= g2);
        idx[i] = keep ? j : -1, d2[i] = keep ? d : 0.0f;
    }
}
int kfo_solve(const float *p, const float *q, int n, int use_float, double *R, double *t)
{
    if (!use_float) return solve<double>(p, q, n, R, t);
    float Rf[9], tf[3];
    const int rank = solve<float>(p, q, n, Rf, tf);
    for (int i = 0; i < 9; ++i) R[i] = Rf[i];
    for (int i = 0; i < 3; ++i) t[i] = tf[i];
    return rank;
}
void kfo_icp(void *tgt, const float *src, int ns, int stride, const float *init, const slam_kf_params *P, int mode,
             slam_kf_edge_result *out, int32_t *trace, int trace_cap, double *margin)
{
    icp(*static_cast<Index *>(tgt), src, ns, stride, init, *P, mode, out, trace, trace_cap, margin);
}
// fills the LUM fields of `out` from out->transform; MM_MZ (optional): 36 + 6 doubles; aver / diff (optional): 3 * ns floats
void kfo_lum(void *tgt, const float *src, int ns, int stride, double gate, slam_kf_edge_result *out, double *MM_MZ, float *aver, float *diff)
{
    LumOut o;
    lum(*static_cast<Index *>(tgt), src, ns, stride, out->transform, gate, &o, aver, diff);
    std::memcpy(out->information, o.info, sizeof o.info);
    out->num_corr = o.num_corr, out->singular = o.singular, out->ss = o.ss;
    if (MM_MZ) std::memcpy(MM_MZ, o.MM, sizeof o.MM), std::memcpy(MM_MZ + 36, o.MZ, sizeof o.MZ);
}
void kfo_inverse6(const double *A, double *X) { inverse6(A, X); }
}
