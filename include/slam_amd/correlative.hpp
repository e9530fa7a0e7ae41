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
#include <cstdint>
#include <cstdio>

#include "slam_amd/icp.hpp"
#include "slam_mi355x.h"

namespace slam_amd {

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
    const slam_csm_result &result() const { return last_; } // of the last match()
    bool                   valid() const { return h_ != nullptr; }

private:
    slam_csm_t     *h_ = nullptr;
    slam_csm_result last_ = {0, 0, 0, -1, 0, 0, 0};
};

} // namespace slam_amd
