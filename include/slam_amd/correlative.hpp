// slam_amd/correlative.hpp -- header-only C++ adapter of the correlative scan matcher (slam_csm_*, docs/CSM.md) in the
// shape of slam_amd::Icp (icp.hpp): the constructor takes the model arrays Icp's takes, match() takes the scene arrays and
// R, t in/out that Icp::fit takes.  The reference has no such class; a caller that has lost its pose writes
//
//     slam_amd::CorrelativeMatcher csm(M_GA, M_NGA, nGA, nNGA);
//     slam_amd::IcpPointToPoint    icp(M_GA, M_NGA, nGA, nNGA, 2);
//     csm.match(T_GA, T_NGA, tGA, tNGA, R, t);          // the best pose of the window around (R, t)
//     icp.fit(T_GA, T_NGA, tGA, tNGA, R, t, indist, 0); // ... refined
//
// Conventions of icp.hpp: a failed construction logs and leaves an unusable object; match() is synchronous and leaves R, t
// alone where it cannot answer (fewer than 5 scene points).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "slam_amd/icp.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

// The posterior of a match (slam_csm_posterior, docs/CSM.md section 6) with what a consumer asks of it.  Index 0 is x, 1 is
// y, 2 is theta; matrices are 3 x 3 row-major.
struct Posterior {
    slam_csm_posterior p = {};
    double             u[3] = {0.0, 0.0, 0.0}; // resolution, resolution, theta_step
    int                score = 0, n_points = 0; // of the match

    // floor: u_i^2 / 12 on the diagonal -- the matcher cannot know a pose better than one cell
    void covariance(double out[9], bool floor = true) const
    {
        const double *c = p.cov;
        const double  m[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
        for (int i = 0; i < 9; ++i) out[i] = m[i];
        if (floor)
            for (int i = 0; i < 3; ++i) {
                const double uu = u[i] * u[i];
                out[4 * i] = out[4 * i] + uu / 12.0;
            }
    }
    // the inverse of the floored covariance by the symmetric adjugate; false: the determinant is not positive and finite
    bool information(double out[9]) const
    {
        double m[9];
        covariance(m, true);
        const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[8];
        const double de = d * f, ee = e * e, ce = c * e, bf = b * f, be = b * e, cd = c * d;
        const double af = a * f, cc = c * c, bc = b * c, ae = a * e, ad = a * d, bb = b * b;
        const double A = de - ee, B = ce - bf, C = be - cd, D = af - cc, E = bc - ae, F = ad - bb;
        const double aA = a * A, bB = b * B, cC = c * C;
        const double s = aA + bB, det = s + cC;
        if (!(det > 0.0 && std::isfinite(det))) return false;
        out[0] = A / det, out[1] = B / det, out[2] = C / det;
        out[3] = B / det, out[4] = D / det, out[5] = E / det;
        out[6] = C / det, out[7] = E / det, out[8] = F / det;
        return true;
    }
    // a second, separate pose scores within max_deficit_per_point * n_points of the winner
    bool ambiguous(int max_deficit_per_point) const
    {
        return p.valid && p.second_score >= 0 && score - p.second_score <= max_deficit_per_point * n_points;
    }
};

class CorrelativeMatcher {
public:
    CorrelativeMatcher(double *M_GA, double *M_NGA, const int32_t M_GA_num, const int32_t M_NGA_num, const slam_csm_params *params = nullptr)
    {
        if (slam_csm_create(M_GA, M_GA_num, M_NGA, M_NGA_num, params, &h_) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            h_ = nullptr;
        }
    }
    ~CorrelativeMatcher() { slam_csm_destroy(h_); }
    CorrelativeMatcher(const CorrelativeMatcher &) = delete;
    CorrelativeMatcher &operator=(const CorrelativeMatcher &) = delete;

    // the search window: +- half_x, half_y cells of the lattice, +- half_theta steps of theta_step radians
    bool setWindow(int32_t half_x, int32_t half_y, int32_t half_theta, double theta_step)
    {
        return h_ && slam_csm_set_window(h_, half_x, half_y, half_theta, theta_step) == SLAM_OK;
    }
    // the same in metres and radians, on the lattice and the angular step in force
    bool setWindowMetres(double x, double y, double theta)
    {
        slam_csm_params p;
        if (!h_ || slam_csm_info(h_, &p, nullptr, nullptr, nullptr, nullptr) != SLAM_OK) return false;
        return setWindow((int32_t)(x / p.resolution + 0.5), (int32_t)(y / p.resolution + 0.5), (int32_t)(theta / p.theta_step + 0.5), p.theta_step);
    }
    void setExhaustive(bool on) { if (h_) slam_csm_set_exhaustive(h_, on ? 1 : 0); }

    // R (2 x 2) and t (2 x 1) in/out; returns the score's share of the most the scan could score, or -1 (R, t untouched)
    double match(double *T_GA, double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, Matrix &R, Matrix &t)
    {
        if (!h_) return -1.0;
        double Rr[4] = {R.val[0][0], R.val[0][1], R.val[1][0], R.val[1][1]};
        double tt[2] = {t.val[0][0], t.val[1][0]};
        if (slam_csm_match(h_, T_GA, T_GA_num, T_NGA, T_NGA_num, Rr, tt, &last_) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            return -1.0;
        }
        R.val[0][0] = Rr[0];
        R.val[0][1] = Rr[1];
        R.val[1][0] = Rr[2];
        R.val[1][1] = Rr[3];
        t.val[0][0] = tt[0];
        t.val[1][0] = tt[1];
        return last_.max_score > 0 ? (double)last_.score / (double)last_.max_score : 0.0;
    }
    // the posterior parameters (nullptr: the defaults); matchPosterior needs it first
    bool setPosterior(const slam_csm_post_params *params = nullptr)
    {
        slam_csm_post_params p;
        slam_csm_default_post_params(&p);
        if (params) p = *params;
        return h_ && slam_csm_set_post_params(h_, &p) == SLAM_OK;
    }
    bool setPosterior(const slam_csm_post_params &params) { return setPosterior(&params); }
    // match() with the posterior of its answer
    double matchPosterior(double *T_GA, double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, Matrix &R, Matrix &t, Posterior &post)
    {
        slam_csm_params P;
        if (!h_ || slam_csm_info(h_, &P, nullptr, nullptr, nullptr, nullptr) != SLAM_OK) return -1.0;
        double Rr[4] = {R.val[0][0], R.val[0][1], R.val[1][0], R.val[1][1]};
        double tt[2] = {t.val[0][0], t.val[1][0]};
        if (slam_csm_match_post(h_, T_GA, T_GA_num, T_NGA, T_NGA_num, Rr, tt, &last_, &post.p) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            return -1.0;
        }
        post.u[0] = post.u[1] = P.resolution, post.u[2] = P.theta_step;
        post.score = last_.score, post.n_points = last_.n_points;
        R.val[0][0] = Rr[0];
        R.val[0][1] = Rr[1];
        R.val[1][0] = Rr[2];
        R.val[1][1] = Rr[3];
        t.val[0][0] = tt[0];
        t.val[1][0] = tt[1];
        return last_.max_score > 0 ? (double)last_.score / (double)last_.max_score : 0.0;
    }
    const slam_csm_result &result() const { return last_; } // of the last match()
    bool                   valid() const { return h_ != nullptr; }

private:
    slam_csm_t     *h_ = nullptr;
    slam_csm_result last_ = {0, 0, 0, -1, 0, 0, 0};
};

} // namespace slam_amd
