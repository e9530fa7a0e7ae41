// nav_field_test.cpp -- slam_amd::NavField and slam_amd::MLS::enablePlanner / planPath (include/slam_amd/mls.hpp), the C++ twin of
// tests/test_gpu_grid_nav.py, which builds and runs it and compares every file with the Python binding's answers bit for bit.
//   argv[1]: directory with
//     plane.u8, goals.i32, plane.f64 (size_x, size_y, orth_w, diag_w, neutral, lethal_from, unknown_step, start_x, start_y)
//     obs0.f32, gnd0.f32, obs1.f32, gnd1.f32 (x, y, z, 0 per point) and params.f64 (size_x, size_y, resolution, pose1_x, pose1_y,
//     inscribed, inflation, scaling, max_cells, from_x, from_y, to_x, to_y)
//   writes  a_pot.u32, a_path.i32, a_state.i64 (the seven, then the path's status) -- the field alone on the host plane
//           b_cost.u8, b_pot.u32, b_cells.i32, b_points.f64, b_meta.f64 (status, cells of the start, cells of the goal, 2 x 2
//           outside answers) -- the map's planner
#include <cstdio>
#include <string>
#include <vector>

#include "slam_amd/mls.hpp"

template <class T>
static std::vector<T> load(const std::string &path)
{
    std::vector<T> v;
    FILE          *f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

template <class T>
static bool save(const std::string &path, const std::vector<T> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    // ---- the field alone
    {
        const auto pp = load<double>(d + "plane.f64");
        const auto plane = load<uint8_t>(d + "plane.u8");
        const auto goals = load<int32_t>(d + "goals.i32");
        if (pp.size() != 9 || plane.size() != (size_t)pp[0] * (size_t)pp[1] || goals.empty()) return 2;
        slam_amd::NavField bad(0, 5);
        if (bad.ok() || bad.compute(plane.data(), goals)) return 10; // refused, and unusable afterwards
        slam_amd::NavField nf((int)pp[0], (int)pp[1], (int)pp[2], (int)pp[3]);
        if (!nf.ok() || !nf.setSteps((int)pp[4], (int)pp[5], (int)pp[6])) return 11;
        if (nf.setTable(std::vector<uint32_t>(255, 1u))) return 12; // a table of the wrong length
        if (!nf.compute(plane.data(), goals)) return 13;
        std::vector<uint32_t> pot;
        std::vector<int32_t>  cells;
        int                   status = -1;
        slam_gnav_state       st;
        if (!(nf.read(&pot) && nf.path((int)pp[7], (int)pp[8], &cells, &status) && nf.state(st))) return 14;
        const std::vector<int64_t> state = {st.rounds,          st.converged,     st.goals_used,       st.goals_skipped,
                                            st.tiles_processed, st.last_path_len, st.last_path_status, status};
        if (!(save(d + "a_pot.u32", pot) && save(d + "a_path.i32", cells) && save(d + "a_state.i64", state))) return 15;
    }
    // ---- the map's planner
    const auto prm = load<double>(d + "params.f64");
    if (prm.size() != 13) return 2;
    const std::vector<float> obs[2] = {load<float>(d + "obs0.f32"), load<float>(d + "obs1.f32")};
    const std::vector<float> gnd[2] = {load<float>(d + "gnd0.f32"), load<float>(d + "gnd1.f32")};
    const double             pose[2][2] = {{0.0, 0.0}, {prm[3], prm[4]}};
    slam_amd::MLS            m((int)prm[0], (int)prm[1], prm[2], true);
    m.setMinClusterPoints(0);
    if (m.enablePlanner()) return 20;                                       // needs enableCostmap first
    if (m.planPath(prm[9], prm[10], prm[11], prm[12]).status != SLAM_GNAV_PATH_NOT_CONVERGED) return 21; // nothing before enablePlanner
    if (!m.enableCostmap(prm[5], prm[6], prm[7], (int)prm[8])) return 22;
    if (m.enablePlanner(slam_amd::NavParams(0, 17))) return 23;             // a weight out of range: refused
    if (!m.enablePlanner()) return 24;
    for (int k = 0; k < 2; ++k)
        m.addToMap(obs[k].data(), (int)(obs[k].size() / 4), gnd[k].data(), (int)(gnd[k].size() / 4), pose[k][0], pose[k][1], 4);
    const slam_amd::NavPath p = m.planPath(prm[9], prm[10], prm[11], prm[12]);
    std::vector<uint32_t>   pot;
    if (!m.planner()->read(&pot)) return 25;
    int sx = -1, sy = -1, gx = -1, gy = -1;
    if (!m.worldToCell(prm[9], prm[10], &sx, &sy) || !m.worldToCell(prm[11], prm[12], &gx, &gy)) return 26;
    const double              far = 1e6;
    const slam_amd::NavPath   out_from = m.planPath(far, 0.0, prm[11], prm[12]), out_to = m.planPath(prm[9], prm[10], 0.0, -far);
    const std::vector<double> meta = {(double)p.status,      (double)sx, (double)sy, (double)gx, (double)gy, (double)out_from.status,
                                      (double)out_from.cells.size(), (double)out_to.status, (double)out_to.cells.size()};
    if (!(save(d + "b_cost.u8", m.getCostmap().cost) && save(d + "b_pot.u32", pot) && save(d + "b_cells.i32", p.cells) &&
          save(d + "b_points.f64", p.points) && save(d + "b_meta.f64", meta)))
        return 27;
    return 0;
}
