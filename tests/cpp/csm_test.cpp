// The call pair a ccicp2d caller makes once it has lost its pose: slam_amd::CorrelativeMatcher::match, then
// slam_amd::IcpPointToPoint::fit from the candidate (include/slam_amd/correlative.hpp, icp.hpp).  Inputs from plain binary
// files, the two poses and the matcher's result as hexadecimal doubles on stdout; tests/test_gpu_csm_adapter.py compares
// them with the Python path bit for bit.
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

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int         max_iter = std::atoi(argv[2]);
    auto m_ga = read_all(dir + "/m_ga.f64"), m_nga = read_all(dir + "/m_nga.f64");
    auto t_ga = read_all(dir + "/t_ga.f64"), t_nga = read_all(dir + "/t_nga.f64");
    auto init = read_all(dir + "/init.f64"); // R00 R01 R10 R11 t0 t1

    using namespace slam_amd;
    Matrix R(2, 2, init.data()), t(2, 1, init.data() + 4);
    CorrelativeMatcher csm(m_ga.data(), m_nga.data(), (int32_t)m_ga.size() / 2, (int32_t)m_nga.size() / 2);
    IcpPointToPoint    icp(m_ga.data(), m_nga.data(), (int32_t)m_ga.size() / 2, (int32_t)m_nga.size() / 2, 2);
    if (!csm.valid() || !icp.valid()) return 3;
    icp.setMaxIterations(max_iter);
    const double share = csm.match(t_ga.data(), t_nga.data(), (int32_t)t_ga.size() / 2, (int32_t)t_nga.size() / 2, R, t);
    const slam_csm_result &r = csm.result();
    std::printf("candidate %a %a %a %a %a %a\n", R.val[0][0], R.val[0][1], R.val[1][0], R.val[1][1], t.val[0][0], t.val[1][0]);
    std::printf("result %d %d %d %d %d %d %a\n", r.k, r.a, r.b, r.score, r.max_score, r.n_points, share);
    icp.fit(t_ga.data(), t_nga.data(), (int32_t)t_ga.size() / 2, (int32_t)t_nga.size() / 2, R, t, 5, 0);
    std::printf("fit %a %a %a %a %a %a\n", R.val[0][0], R.val[0][1], R.val[1][0], R.val[1][1], t.val[0][0], t.val[1][0]);

    // a scan of four points: logged, R and t untouched
    Matrix R2 = Matrix::eye(2), t2(2, 1);
    const double none = csm.match(t_ga.data(), t_nga.data(), 0, 4, R2, t2);
    // a narrower window in metres: +- 0.5 m, +- 0.1 rad -> 5 cells, 10 steps
    const bool set = csm.setWindowMetres(0.5, 0.5, 0.1);
    std::printf("edges %d %d %d\n", none == -1.0 && R2.val[0][0] == 1.0 && R2.val[0][1] == 0.0 && t2.val[0][0] == 0.0, (int)set, (int)csm.valid());
    return 0;
}
