// What a caller of slam_amd::ParticleFilter does (include/slam_amd/correlative.hpp): fill an MLS occupancy grid, update a
// GridMatcher, start a filter around a pose, then predict and update over a few scans, reading particles, weights and state after
// every step; the resampling rule alone; and the failure paths.  Inputs from plain binary files, results as integers and hexadecimal
// doubles on stdout; tests/test_gpu_pf_adapter.py compares them with the Python path bit for bit.
//   pf_test <dir> <size> <resolution> <sigma> <centre_x> <centre_y> <n_particles> <seed> <steps>
#include <cinttypes>
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

// FNV-1a over the bytes of an array: a row stays short and any changed bit changes it
template <class T>
static uint64_t digest(const std::vector<T> &v)
{
    uint64_t             h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

static void print_step(const char *name, slam_amd::ParticleFilter &pf, bool ok)
{
    std::vector<double>   x, y;
    std::vector<int32_t>  k;
    std::vector<int64_t>  acc;
    std::vector<uint32_t> w;
    slam_amd::PfState     s;
    ok = pf.particles(x, y, k) && pf.weights(acc, w) && pf.state(s) && ok;
    std::printf("%s %d %u %d %d %d %d %d %" PRId64 " %" PRId64 " %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64
                " %a %a %a %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n",
                name, (int)ok, (uint32_t)s.t, (int)s.n, (int)s.resampled, (int)s.degenerate, (int)s.best, (int)s.refused, s.n_resamples, s.A_max,
                (uint64_t)s.W, (uint64_t)s.S2, s.MX, s.MY, s.MC, s.MS, s.x, s.y, s.theta, digest(x), digest(y), digest(k), digest(acc), digest(w));
}

int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const std::string dir = argv[1];
    const int         size = std::atoi(argv[2]), n_particles = std::atoi(argv[7]), steps = std::atoi(argv[9]);
    const double      res = std::atof(argv[3]), sigma = std::atof(argv[4]), cx = std::atof(argv[5]), cy = std::atof(argv[6]);
    const uint64_t    seed = std::strtoull(argv[8], nullptr, 10);
    auto obs = read_all<float>(dir + "/obstacles.f32"); // x y per point, already relative to the window's centre
    auto start = read_all<double>(dir + "/start.f64");  // x y k sx sy sk of init_gaussian, map frame
    auto motions = read_all<double>(dir + "/motions.f64"); // dx dy sx sy sk dk per step
    auto weights = read_all<uint32_t>(dir + "/weights.u32");

    using namespace slam_amd;
    MLS mls(size, size, res, true);
    mls.setMinClusterPoints(0);
    mls.setPose(cx, cy);
    mls.addToOccupancy(obs.data(), (int)obs.size() / 2, nullptr, 0, 2);
    GridMatcher gm(mls, sigma);
    if (!gm.ok() || !gm.update()) return 3;
    double gx = 0, gy = 0;
    gm.centre(gx, gy);

    PfParams p;
    p.seed = seed;
    ParticleFilter pf(gm, n_particles, &p);
    if (!pf.ok()) return 4;
    std::printf("setup %d %a %a %d\n", gm.maxCells(), gx, gy, pf.size());

    std::vector<double>   cs, G;
    std::vector<uint32_t> wtab;
    const bool tables = ParticleFilter::angleTable(p.n_angles, cs) && ParticleFilter::gaussTable(p.gauss_bits, G) &&
                        ParticleFilter::weightTable(p.weight_scale, p.weight_shift, p.weight_len, wtab) && pf.setTables(cs, G, wtab);
    std::printf("tables %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", (int)tables, digest(cs), digest(G), digest(wtab));

    print_step("init", pf, pf.initGaussian(start[0], start[1], (int)start[2], start[3], start[4], start[5]));
    for (int i = 0; i < steps; ++i) {
        const double        *m = &motions[6 * (size_t)i];
        const PfMotion        motion = {m[0], m[1], m[2], m[3], m[4], (int32_t)m[5], 0};
        auto                 t_ga = read_all<double>(dir + "/t_ga_" + std::to_string(i) + ".f64");
        auto                 t_nga = read_all<double>(dir + "/t_nga_" + std::to_string(i) + ".f64");
        const bool           ok = pf.predict(motion) && pf.update(t_ga.data(), t_nga.data(), (int32_t)t_ga.size() / 2, (int32_t)t_nga.size() / 2);
        print_step(("step" + std::to_string(i)).c_str(), pf, ok);
    }
    // particles handed in, and the device forms on the null stream
    std::vector<double>  x, y;
    std::vector<int32_t> k;
    bool                 moved = pf.particles(x, y, k);
    for (size_t i = 0; i < x.size(); ++i) x[i] = x[i] + 0.5, k[i] = (k[i] + 7) % p.n_angles;
    print_step("set", pf, moved && pf.setParticles(x, y, k));

    std::vector<int32_t> src;
    const bool           sampled = pf.resampleIndices(weights, 12345, src);
    std::printf("resample %d %zu %016" PRIx64 "\n", (int)sampled, src.size(), digest(src));

    // failure paths: each logs and answers false or leaves an unusable object, and nothing above is disturbed
    MLS                  none(0, 0, res, true);
    GridMatcher          over_none(none, sigma);
    ParticleFilter       orphan(over_none, 16);
    ParticleFilter       too_many(gm, (1 << 18) + 1);
    p.n_angles = 100;
    ParticleFilter       odd_angles(gm, 16, &p);
    const PfMotion       bad = {0.0, 0.0, -1.0, 0.0, 0.0, 0, 0};
    const bool           refused = !pf.predict(bad);
    std::vector<int32_t> short_k(3, 0);
    const bool           short_set = !pf.setParticles(std::vector<double>(3, 0.0), std::vector<double>(3, 0.0), short_k);
    k[0] = p.n_angles + 4096;
    const bool           bad_heading = !pf.setParticles(x, y, k);
    std::vector<uint32_t> high(wtab);
    high[1] = 65537u;
    const bool bad_table = !pf.setTables({}, {}, high);
    const bool no_weights = !pf.resampleIndices({}, 0, src);
    PfState s;
    std::printf("edges %d %d %d %d %d %d %d %d %d\n", (int)!orphan.ok(), (int)!too_many.ok(), (int)!odd_angles.ok(), (int)refused, (int)short_set,
                (int)bad_heading, (int)bad_table, (int)no_weights, (int)(pf.ok() && pf.state(s) && s.t == (uint32_t)steps));
    return 0;
}
