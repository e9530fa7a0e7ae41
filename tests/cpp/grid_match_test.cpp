// What a caller of slam_amd::GridMatcher does (include/slam_amd/correlative.hpp): fill an MLS occupancy grid, update, match a
// scan from a start pose, score a pose set, relocalize from no prior; then CorrelativeMatcher::fromPlane over the field's plane
// read back, and the failure paths.  Inputs from plain binary files, results as integers and hexadecimal doubles on stdout;
// tests/test_gpu_grid_match_adapter.py compares them with the Python path bit for bit.
//   grid_match_test <dir> <size> <resolution> <sigma> <centre_x> <centre_y> <half_xy> <half_theta> <theta_step> <relocalize_step>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/correlative.hpp"

template <class T>
static std::vector<T> read_all(const std::string &path)
{
    std::vector<T> v;
    FILE          *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) std::exit(2);
    std::fclose(f);
    return v;
}

static void print_pose(const char *name, const slam_amd::Matrix &R, const slam_amd::Matrix &t, const slam_csm_result &r, double share)
{
    std::printf("%s %a %a %a %a %a %a %d %d %d %d %d %d %a\n", name, R.val[0][0], R.val[0][1], R.val[1][0], R.val[1][1], t.val[0][0], t.val[1][0], r.k,
                r.a, r.b, r.score, r.max_score, r.n_points, share);
}

int main(int argc, char **argv)
{
    if (argc < 11) return 2;
    const std::string dir = argv[1];
    const int         size = std::atoi(argv[2]), half_xy = std::atoi(argv[7]), half_theta = std::atoi(argv[8]);
    const double      res = std::atof(argv[3]), sigma = std::atof(argv[4]), cx = std::atof(argv[5]), cy = std::atof(argv[6]);
    const double      step = std::atof(argv[9]), reloc_step = std::atof(argv[10]);
    auto obs = read_all<float>(dir + "/obstacles.f32"); // x y per point, already relative to the window's centre
    auto t_ga = read_all<double>(dir + "/t_ga.f64"), t_nga = read_all<double>(dir + "/t_nga.f64");
    auto init = read_all<double>(dir + "/init.f64");    // R00 R01 R10 R11 t0 t1, map frame
    auto poses = read_all<double>(dir + "/poses.f64");  // cos sin tx ty per pose, map frame
    const int32_t n_ga = (int32_t)t_ga.size() / 2, n_nga = (int32_t)t_nga.size() / 2, n_poses = (int32_t)poses.size() / 4;

    using namespace slam_amd;
    MLS mls(size, size, res, true);
    mls.setMinClusterPoints(0);
    mls.setPose(cx, cy);
    mls.addToOccupancy(obs.data(), (int)obs.size() / 2, nullptr, 0, 2);

    slam_csm_params p;
    slam_csm_default_params(&p);
    p.half_x = p.half_y = half_xy, p.half_theta = half_theta, p.theta_step = step;
    GridMatcher gm(mls, sigma, 0, &p);
    if (!gm.ok() || !gm.update()) return 3;
    double gx = 0, gy = 0;
    gm.centre(gx, gy);
    std::printf("setup %d %a %a\n", gm.maxCells(), gx, gy);

    Matrix       R(2, 2, init.data()), t(2, 1, init.data() + 4);
    const double share = gm.match(t_ga.data(), t_nga.data(), n_ga, n_nga, R, t);
    print_pose("match", R, t, gm.result(), share);

    Posterior post;
    Matrix    Rp(2, 2, init.data()), tp(2, 1, init.data() + 4);
    const bool   set = gm.setPosterior();
    const double share_p = gm.matchPosterior(t_ga.data(), t_nga.data(), n_ga, n_nga, Rp, tp, post);
    print_pose("post", Rp, tp, gm.result(), share_p);
    std::printf("posterior %d %d %d %d %lld %a %a %a\n", (int)set, post.p.valid, post.p.n_within, post.p.margin, (long long)post.p.m0, post.p.cov[0],
                post.p.cov[3], post.p.cov[5]);

    std::vector<int32_t> score, counted;
    const bool           scored = gm.scorePoses(t_ga.data(), t_nga.data(), n_ga, n_nga, poses.data(), n_poses, score, counted);
    std::printf("scores %d", (int)scored);
    for (int32_t i = 0; i < n_poses; ++i) std::printf(" %d %d", score[(size_t)i], counted[(size_t)i]);
    std::printf("\n");

    // the same plane read back and handed to CorrelativeMatcher::fromPlane: the window's frame, so the centre is the caller's
    std::vector<uint8_t> cost;
    if (!gm.field().read(nullptr, &cost)) return 4;
    p.resolution = res;
    CorrelativeMatcher direct = CorrelativeMatcher::fromPlane(cost.data(), size, size, -(size / 2), -(size / 2), &p);
    Matrix             Rd(2, 2, init.data()), td(2, 1);
    td.val[0][0] = init[4] - gx, td.val[1][0] = init[5] - gy;
    const double share_d = direct.match(t_ga.data(), t_nga.data(), n_ga, n_nga, Rd, td);
    td.val[0][0] = td.val[0][0] + gx, td.val[1][0] = td.val[1][0] + gy;
    print_pose("direct", Rd, td, direct.result(), share_d);

    Matrix       Rr(2, 2), tr(2, 1);
    const double share_r = gm.relocalize(t_ga.data(), t_nga.data(), n_ga, n_nga, reloc_step, Rr, tr);
    print_pose("relocalize", Rr, tr, gm.result(), share_r);

    // failure paths: each logs and leaves an unusable object or answers false, and nothing above is disturbed
    std::vector<double> model = {0.0, 0.0, 0.1, 0.1, 0.2, 0.0, 0.3, 0.1, 0.0, 0.3};
    CorrelativeMatcher  from_model(model.data(), nullptr, 5, 0);
    const bool          refused_model = from_model.valid() && !from_model.setPlane(cost.data(), 0, 0);
    CorrelativeMatcher  empty = CorrelativeMatcher::fromPlane(cost.data(), 0, size, 0, 0);
    CorrelativeMatcher  far = CorrelativeMatcher::fromPlane(cost.data(), size, size, 1 << 30, 0);
    MLS                 none(0, 0, res, true);
    GridMatcher         over_none(none, sigma);
    GridMatcher         bad_sigma(mls, -1.0);
    GridMatcher         too_wide(mls, 1000.0 * res); // 3000 cells of kernel
    Matrix              R4 = Matrix::eye(2), t4(2, 1);
    const double        four = gm.match(t_ga.data(), t_nga.data(), 2, 2, R4, t4);
    std::vector<int32_t> s0, c0;
    const bool           no_poses = gm.scorePoses(t_ga.data(), t_nga.data(), n_ga, n_nga, poses.data(), 0, s0, c0) && s0.empty();
    std::printf("edges %d %d %d %d %d %d %d %d %d\n", (int)refused_model, (int)!empty.valid(), (int)!far.valid(), (int)!over_none.ok(),
                (int)!bad_sigma.ok(), (int)!too_wide.ok(), (int)(four == -1.0 && R4.val[0][0] == 1.0 && t4.val[0][0] == 0.0), (int)no_poses,
                (int)(gm.ok() && direct.valid()));
    return 0;
}
