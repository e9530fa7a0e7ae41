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
//
// fromPlane / fromPlaneDev make a matcher whose table is a byte plane (docs/GRID_MATCH.md): a likelihood field computed from an
// occupancy grid, a saved map.  slam_amd::GridMatcher (below) puts grid, field and such a matcher together.
// slam_amd::ParticleFilter (at the end) keeps a belief between scans over a GridMatcher (docs/PARTICLE_FILTER.md).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "slam_amd/buffer.hpp"
#include "slam_amd/icp.hpp"
#include "slam_amd/mls.hpp"
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
    // slam_csm_create_from_plane[_dev]: the table is the w x h byte plane itself, element (0, 0) at lattice cell (origin_x, origin_y)
    static CorrelativeMatcher fromPlane(const uint8_t *plane, int w, int h, int origin_x, int origin_y, const slam_csm_params *params = nullptr)
    {
        return CorrelativeMatcher(plane, w, h, origin_x, origin_y, false, params);
    }
    static CorrelativeMatcher fromPlaneDev(const uint8_t *d_plane, int w, int h, int origin_x, int origin_y, const slam_csm_params *params = nullptr)
    {
        return CorrelativeMatcher(d_plane, w, h, origin_x, origin_y, true, params);
    }
    CorrelativeMatcher(const uint8_t *plane, int w, int h, int origin_x, int origin_y, bool on_device, const slam_csm_params *params = nullptr)
    {
        const int rc = on_device ? slam_csm_create_from_plane_dev(plane, w, h, origin_x, origin_y, params, &h_)
                                 : slam_csm_create_from_plane(plane, w, h, origin_x, origin_y, params, &h_);
        if (rc != SLAM_OK) {
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
    // slam_csm_set_plane_dev: another device plane of the same size at any origin, a copy and the slide enqueued on `stream`;
    // false (logged) on a matcher made from a model
    bool setPlane(const uint8_t *d_plane, int origin_x, int origin_y, slam_stream_t stream = nullptr)
    {
        if (!h_) return false;
        if (slam_csm_set_plane_dev(h_, d_plane, origin_x, origin_y, stream) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            return false;
        }
        return true;
    }
    // slam_csm_score_poses: poses = n_poses x (cos, sin, tx, ty); score and counted are sized here.  false (logged): refused
    bool scorePoses(const double *T_GA, const double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, const double *poses, int32_t n_poses,
                    std::vector<int32_t> &score, std::vector<int32_t> &counted)
    {
        if (!h_ || T_GA_num < 0 || T_NGA_num < 0 || n_poses < 0) return false;
        std::vector<double> pts;
        pts.reserve(2 * ((size_t)T_GA_num + T_NGA_num));
        pts.insert(pts.end(), T_GA, T_GA + 2 * (size_t)T_GA_num);
        pts.insert(pts.end(), T_NGA, T_NGA + 2 * (size_t)T_NGA_num);
        score.assign((size_t)n_poses, 0);
        counted.assign((size_t)n_poses, 0);
        if (slam_csm_score_poses(h_, pts.data(), T_GA_num + T_NGA_num, T_GA_num, poses, n_poses, score.data(), counted.data()) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            return false;
        }
        return true;
    }

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
    slam_csm_t            *handle() const { return h_; }

private:
    slam_csm_t     *h_ = nullptr;
    slam_csm_result last_ = {0, 0, 0, -1, 0, 0, 0};
};

// GridMatcher localises a scan in an occupancy grid itself (docs/GRID_MATCH.md): the twin of slam_amd.api.GridMatcher over
// slam_amd::MLS (mls.hpp), slam_amd::DistanceField and a plane-built CorrelativeMatcher.
//
//     slam_amd::MLS         mls(500, 500, 0.1, true);            // ... the mapper fills it
//     slam_amd::GridMatcher gm(mls, 0.2);                        // sigma 0.2 m; R = ceil(3 sigma / res - 1e-9) cells
//     gm.update();                                               // grid -> likelihood field -> the matcher's table; waits for nothing
//     gm.match(T_GA, T_NGA, tGA, tNGA, R, t);                    // the best pose of the window around (R, t), map frame
//     gm.relocalize(T_GA, T_NGA, tGA, tNGA, 0.05, R, t);         // no prior: the whole grid, all angles
//
// The field is created with slam_grid_likelihood_table and unknown_keep_from = 0, so that unknown cells keep their likelihood
// byte; the matcher is created at the grid's resolution and its plane element (0, 0) is lattice cell (-size_x / 2, -size_y / 2),
// the grid's own cell_coord.  The window's frame is centred on the grid's pose when the grid rolls (slam_grid_get_pose) and on
// (0, 0) when it does not: the adapter subtracts that centre from a start translation and adds it to the answer, one double
// operation each; the C-ABI underneath stays in the window's frame.  The matcher keeps its cell rule (floor, double), the grid's
// is (int) truncation on float points: inside the window they agree.  A failure logs and leaves ok() == false.
class GridMatcher {
public:
    // params: the matcher's (window, block; resolution is the grid's, sigma and kernel_cells are the field's business)
    GridMatcher(MLS &grid, double sigma, int max_cells = 0, const slam_csm_params *params = nullptr) : grid_(grid)
    {
        double res = 0.0;
        if (!grid.handle() || slam_grid_info(grid.handle(), &sx_, &sy_, &res, nullptr, nullptr) != SLAM_OK) {
            std::fprintf(stderr, "GridMatcher: the grid is not usable\n");
            return;
        }
        const double cells = std::ceil(3.0 * sigma / res - 1e-9);
        const int    R = max_cells > 0 ? max_cells : (cells >= 1.0 && cells <= 254.0 ? (int)cells : 0);
        std::vector<uint8_t> table(R > 0 ? (size_t)R * R + 2 : 1);
        if (slam_grid_likelihood_table(res, sigma, R, table.data(), (int)table.size()) != SLAM_OK) {
            std::fprintf(stderr, "%s\n", slam_last_error());
            return;
        }
        slam_gdist_params gp;
        slam_gdist_default_params(&gp);
        gp.max_cells = R, gp.unknown_keep_from = 0;
        std::unique_ptr<DistanceField> field(new DistanceField(sx_, sy_, &gp));
        // a plane to make the matcher from: the empty grid's; update() brings the grid's own
        const std::vector<int8_t> empty((size_t)sx_ * sy_, (int8_t)0);
        uint8_t                  *d_cost = nullptr;
        if (!field->ok() || !field->setTable(table) || !field->compute(empty.data()) ||
            slam_gdist_planes_dev(field->handle(), nullptr, &d_cost) != SLAM_OK || !d_cost)
            return;
        slam_csm_params p;
        slam_csm_default_params(&p);
        if (params) p = *params;
        p.resolution = res;
        std::unique_ptr<CorrelativeMatcher> matcher(new CorrelativeMatcher(d_cost, sx_, sy_, -(sx_ / 2), -(sy_ / 2), true, &p));
        if (!matcher->valid()) return;
        field_ = std::move(field), matcher_ = std::move(matcher);
        max_cells_ = R, d_cost_ = d_cost;
        readCentre();
    }
    GridMatcher(const GridMatcher &) = delete;
    GridMatcher &operator=(const GridMatcher &) = delete;

    bool ok() const { return matcher_ && field_; }
    int  maxCells() const { return max_cells_; }
    // slam_grid_distance_field, then slam_csm_set_plane_dev, on `stream`; waits for nothing
    bool update(slam_stream_t stream = nullptr)
    {
        if (!ok()) return false;
        if (!field_->computeFromGrid(grid_.handle(), stream) || !matcher_->setPlane(d_cost_, -(sx_ / 2), -(sy_ / 2), stream)) return false;
        readCentre();
        return true;
    }
    // CorrelativeMatcher::match with R, t in the map frame
    double match(double *T_GA, double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, Matrix &R, Matrix &t)
    {
        if (!ok()) return -1.0;
        Matrix       tw = toWindow(t);
        const double share = matcher_->match(T_GA, T_NGA, T_GA_num, T_NGA_num, R, tw);
        if (share >= 0.0) toMap(tw, t);
        return share;
    }
    bool   setPosterior(const slam_csm_post_params *params = nullptr) { return ok() && matcher_->setPosterior(params); }
    double matchPosterior(double *T_GA, double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, Matrix &R, Matrix &t, Posterior &post)
    {
        if (!ok()) return -1.0;
        Matrix       tw = toWindow(t);
        const double share = matcher_->matchPosterior(T_GA, T_NGA, T_GA_num, T_NGA_num, R, tw, post);
        if (share >= 0.0) toMap(tw, t);
        return share;
    }
    // poses = n_poses x (cos, sin, tx, ty) in the map frame
    bool scorePoses(const double *T_GA, const double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, const double *poses, int32_t n_poses,
                    std::vector<int32_t> &score, std::vector<int32_t> &counted)
    {
        if (!ok() || n_poses < 0) return false;
        std::vector<double> w(poses, poses + 4 * (size_t)n_poses);
        for (int32_t i = 0; i < n_poses; ++i) w[4 * (size_t)i + 2] = w[4 * (size_t)i + 2] - cx_, w[4 * (size_t)i + 3] = w[4 * (size_t)i + 3] - cy_;
        return matcher_->scorePoses(T_GA, T_NGA, T_GA_num, T_NGA_num, w.data(), n_poses, score, counted);
    }
    // No prior: the window covers the whole grid and all angles and starts from the window's centre; R, t are outputs
    double relocalize(double *T_GA, double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num, double theta_step, Matrix &R, Matrix &t)
    {
        if (!ok() || !matcher_->setWindow(sx_ / 2, sy_ / 2, (int32_t)std::ceil(M_PI / theta_step), theta_step)) return -1.0;
        Matrix R0 = Matrix::eye(2), t0(2, 1);
        t0.val[0][0] = cx_, t0.val[1][0] = cy_;
        const double share = match(T_GA, T_NGA, T_GA_num, T_NGA_num, R0, t0);
        if (share >= 0.0) R = R0, t = t0;
        return share;
    }
    const slam_csm_result &result() const { return matcher_->result(); }
    CorrelativeMatcher    &matcher() { return *matcher_; }
    DistanceField         &field() { return *field_; }
    void                   centre(double &x, double &y) const { x = cx_, y = cy_; }

private:
    void readCentre()
    {
        cx_ = cy_ = 0.0;
        if (grid_.rolling()) slam_grid_get_pose(grid_.handle(), &cx_, &cy_);
    }
    Matrix toWindow(const Matrix &t) const
    {
        Matrix w(2, 1);
        w.val[0][0] = t.val[0][0] - cx_, w.val[1][0] = t.val[1][0] - cy_;
        return w;
    }
    void toMap(const Matrix &w, Matrix &t) const { t.val[0][0] = w.val[0][0] + cx_, t.val[1][0] = w.val[1][0] + cy_; }

    MLS                                &grid_;
    std::unique_ptr<DistanceField>      field_;
    std::unique_ptr<CorrelativeMatcher> matcher_;
    uint8_t                            *d_cost_ = nullptr;
    int                                 sx_ = 0, sy_ = 0, max_cells_ = 0;
    double                              cx_ = 0.0, cy_ = 0.0;
};

// ParticleFilter keeps a belief between scans over a GridMatcher (docs/PARTICLE_FILTER.md): the twin of
// slam_amd.api.ParticleFilter over slam_pf_*.  Its update scores the particles against the grid's likelihood plane with the
// matcher's own scorer and passes the centre of a rolling window, which GridMatcher::update keeps.
//
//     slam_amd::GridMatcher    gm(mls, 0.2);
//     slam_amd::ParticleFilter pf(gm, 4096);                     // 4 096 particles, the other parameters at their defaults
//     pf.initGaussian(x, y, k, 0.1, 0.1, 8.0);                   // around a start pose; k in heading steps of 2 pi / n_angles
//     ... per scan:  gm.update();  pf.predict(motion);  pf.update(T_GA, T_NGA, tGA, tNGA);  pf.state(s);   // s.x, s.y, s.theta
//
// A failure logs the library's error and answers false; a failed construction leaves ok() == false.
struct PfParams : slam_pf_params { // at the library's defaults
    PfParams() { slam_pf_default_params(this); }
};
using PfMotion = slam_pf_motion;
using PfState = slam_pf_state;

class ParticleFilter {
public:
    ParticleFilter(GridMatcher &gm, int n_particles, const PfParams *params = nullptr) : gm_(gm)
    {
        if (params) p_ = *params;
        p_.n_particles = n_particles;
        if (!gm.ok()) {
            std::fprintf(stderr, "ParticleFilter: the grid matcher is not usable\n");
            return;
        }
        if (slam_pf_create(&p_, &h_) != SLAM_OK) {
            detail::warn("ParticleFilter");
            h_ = nullptr;
        }
    }
    ~ParticleFilter() { slam_pf_destroy(h_); }
    ParticleFilter(const ParticleFilter &) = delete;
    ParticleFilter &operator=(const ParticleFilter &) = delete;

    bool                  ok() const { return h_ != nullptr; }
    slam_pf_t            *handle() const { return h_; }
    const PfParams        &params() const { return p_; }
    int                   size() const { return p_.n_particles; }

    // the host-made tables (no device is touched); each vector is sized here
    static bool angleTable(int n_angles, std::vector<double> &cs)
    {
        cs.assign(n_angles > 0 && n_angles <= (1 << 16) ? 2 * (size_t)n_angles : 1, 0.0);
        return done(slam_pf_angle_table(n_angles, cs.data(), (int)cs.size()));
    }
    static bool gaussTable(int bits, std::vector<double> &G)
    {
        G.assign(bits >= 0 && bits <= 16 ? (size_t)1 << bits : 1, 0.0);
        return done(slam_pf_gauss_table(bits, G.data(), (int)G.size()));
    }
    static bool weightTable(double scale, int shift, int L, std::vector<uint32_t> &wtab)
    {
        wtab.assign(L > 0 && L <= (1 << 16) ? (size_t)L : 1, 0u);
        return done(slam_pf_weight_table(scale, shift, L, wtab.data()));
    }
    // other tables of the right lengths; an empty vector leaves that table as it is
    bool setTables(const std::vector<double> &cs, const std::vector<double> &G, const std::vector<uint32_t> &wtab)
    {
        return h_ && done(slam_pf_set_tables(h_, cs.empty() ? nullptr : cs.data(), (int)cs.size(), G.empty() ? nullptr : G.data(), (int)G.size(),
                                             wtab.empty() ? nullptr : wtab.data(), (int)wtab.size()));
    }
    bool setParticles(const std::vector<double> &x, const std::vector<double> &y, const std::vector<int32_t> &k)
    {
        if (!h_ || x.size() != y.size() || x.size() != k.size()) return false;
        return done(slam_pf_set_particles(h_, x.data(), y.data(), k.data(), (int)x.size()));
    }
    bool particles(std::vector<double> &x, std::vector<double> &y, std::vector<int32_t> &k)
    {
        if (!h_) return false;
        x.assign((size_t)size(), 0.0), y.assign((size_t)size(), 0.0), k.assign((size_t)size(), 0);
        return done(slam_pf_read_particles(h_, x.data(), y.data(), k.data()));
    }
    bool weights(std::vector<int64_t> &acc, std::vector<uint32_t> &w)
    {
        if (!h_) return false;
        acc.assign((size_t)size(), 0), w.assign((size_t)size(), 0u);
        return done(slam_pf_read_weights(h_, acc.data(), w.data()));
    }
    bool initGaussian(double x, double y, int k, double sx, double sy, double sk) { return h_ && done(slam_pf_init_gaussian(h_, x, y, k, sx, sy, sk)); }
    // the motion model: host form (an invalid motion is refused, logged) and device form (the motion is read on the device)
    bool predict(const PfMotion &m) { return h_ && done(slam_pf_predict(h_, &m)); }
    bool predictDev(const PfMotion *d_motion, slam_stream_t stream = nullptr) { return h_ && done(slam_pf_predict_dev(h_, d_motion, stream)); }
    // the measurement step against the grid's plane as GridMatcher::update left it; the rolling centre is the matcher's
    bool update(const double *T_GA, const double *T_NGA, const int32_t T_GA_num, const int32_t T_NGA_num)
    {
        if (!h_ || !gm_.ok() || T_GA_num < 0 || T_NGA_num < 0) return false;
        std::vector<double> pts;
        pts.reserve(2 * ((size_t)T_GA_num + T_NGA_num));
        pts.insert(pts.end(), T_GA, T_GA + 2 * (size_t)T_GA_num);
        pts.insert(pts.end(), T_NGA, T_NGA + 2 * (size_t)T_NGA_num);
        double cx, cy;
        gm_.centre(cx, cy);
        return done(slam_pf_update(h_, gm_.matcher().handle(), pts.data(), T_GA_num + T_NGA_num, T_GA_num, cx, cy));
    }
    // d_pts: n points on the device, the first n_ga of class GA; enqueued on `stream`, waits for nothing
    bool updateDev(const double *d_pts, int n, int n_ga, slam_stream_t stream = nullptr)
    {
        if (!h_ || !gm_.ok()) return false;
        double cx, cy;
        gm_.centre(cx, cy);
        return done(slam_pf_update_dev(h_, gm_.matcher().handle(), d_pts, n, n_ga, cx, cy, stream));
    }
    // the resampling rule alone: src[j] = min { i : C_i n > j W + (r mod W) } over w.size() <= size() weights
    bool resampleIndices(const std::vector<uint32_t> &w, uint64_t r, std::vector<int32_t> &src)
    {
        if (!h_ || w.empty()) return false;
        detail::DeviceBuffer d_w, d_src;
        src.assign(w.size(), 0);
        if (!d_w.alloc(sizeof(uint32_t) * w.size()) || !d_src.alloc(sizeof(int32_t) * w.size())) return done(SLAM_E_NOMEM);
        return done(slam_memcpy_h2d(d_w.p, w.data(), d_w.cap, nullptr)) &&
               done(slam_pf_resample_indices_dev(h_, d_w.as<uint32_t>(), (int)w.size(), r, d_src.as<int32_t>(), nullptr)) &&
               done(slam_memcpy_d2h(src.data(), d_src.p, d_src.cap, nullptr));
    }
    // the counter, the last update's sums and flags, and the estimate (x, y, theta); waits
    bool state(PfState &s) { return h_ && done(slam_pf_read_state(h_, &s)); }

private:
    static bool done(int rc)
    {
        if (rc != SLAM_OK) detail::warn("ParticleFilter");
        return rc == SLAM_OK;
    }

    GridMatcher   &gm_;
    PfParams       p_;
    slam_pf_t     *h_ = nullptr;
};

} // namespace slam_amd
