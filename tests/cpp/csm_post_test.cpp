// slam_amd::CorrelativeMatcher::matchPosterior and slam_amd::Posterior (include/slam_amd/correlative.hpp) on one scene:
// inputs from plain binary files (as tests/cpp/csm_test.cpp), the window on the command line; the pose, the posterior's
// integers and its doubles, the floored covariance, the information matrix and ambiguous(1) on stdout, doubles in
// hexadecimal.  tests/test_gpu_csm_post_adapter.py compares them with the Python path bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "slam_amd/correlative.hpp"

static std::vector<double> read_all(const std::string &path)
{
    std::vector<double> v;
    FILE               *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(double));
    if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) std::exit(2);
    std::fclose(f);
    return v;
}

static void row(const char *name, const double *v, int n)
{
    std::printf("%s", name);
    for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    const std::string dir = argv[1];
    auto m_ga = read_all(dir + "/m_ga.f64"), m_nga = read_all(dir + "/m_nga.f64");
    auto t_ga = read_all(dir + "/t_ga.f64"), t_nga = read_all(dir + "/t_nga.f64");
    auto init = read_all(dir + "/init.f64"); // R00 R01 R10 R11 t0 t1

    using namespace slam_amd;
    Matrix R(2, 2, init.data()), t(2, 1, init.data() + 4);
    CorrelativeMatcher csm(m_ga.data(), m_nga.data(), (int32_t)m_ga.size() / 2, (int32_t)m_nga.size() / 2);
    if (!csm.valid()) return 3;
    if (!csm.setWindow(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atof(argv[5]))) return 4;
    Posterior post;
    // before setPosterior the call is refused and leaves R, t alone
    const double early = csm.matchPosterior(t_ga.data(), t_nga.data(), (int32_t)t_ga.size() / 2, (int32_t)t_nga.size() / 2, R, t, post);
    slam_csm_post_params pp;
    slam_csm_default_post_params(&pp);
    const bool   set = csm.setPosterior(pp);
    const double share = csm.matchPosterior(t_ga.data(), t_nga.data(), (int32_t)t_ga.size() / 2, (int32_t)t_nga.size() / 2, R, t, post);
    const slam_csm_result    &r = csm.result();
    const slam_csm_posterior &p = post.p;
    std::printf("candidate %a %a %a %a %a %a\n", R.val[0][0], R.val[0][1], R.val[1][0], R.val[1][1], t.val[0][0], t.val[1][0]);
    std::printf("result %d %d %d %d %d %d %a\n", r.k, r.a, r.b, r.score, r.max_score, r.n_points, share);
    std::printf("ints %d %d %d %d %d %d %d %d\n", p.valid, p.n_within, p.margin, p.blocks_evaluated, p.second_score, p.second_k, p.second_a, p.second_b);
    std::printf("sums %" PRId64, p.m0);
    for (int i = 0; i < 3; ++i) std::printf(" %" PRId64, p.m1[i]);
    for (int i = 0; i < 6; ++i) std::printf(" %" PRId64, p.m2[i]);
    std::printf("\n");
    row("mean", p.mean, 3);
    row("cov", p.cov, 6);
    double c[9], c0[9], info[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    post.covariance(c);
    post.covariance(c0, false);
    const bool inv = post.information(info);
    row("covariance", c, 9);
    row("unfloored", c0, 9);
    row("information", info, 9);
    std::printf("flags %d %d %d %d %d\n", (int)(early == -1.0), (int)set, (int)inv, (int)post.ambiguous(1), (int)post.ambiguous(0));
    return 0;
}
