// Every function of include/slam_amd/pose.hpp on poses from a binary file, for tests/test_pose_math.py to hold against the
// Python restatements bit for bit.  Needs no library: g++ -O2 -ffp-contract=off pose_math_test.cpp.
//   pose_math_test <in> <out>
// <in>: records of 14 doubles, two poses a and b as x y z qx qy qz qw.  <out>: 50 doubles per record --
//   tf_matrix(a) 9 | eigen_matrix(a) 9 | eigen_quaternion(tf_matrix(a)) 4 | tf_quaternion(tf_matrix(a)) 4 |
//   relative_f32(a, b) 16, widened | tf_yaw(a) 1 | euler_ypr(a) yaw pitch roll | quat_from_rpy(a.x, a.y, a.z) 4
#include <cstdio>
#include <vector>

#include "slam_amd/pose.hpp"

using namespace slam_amd;

static Pose pose_at(const double *v)
{
    Pose p;
    p.x = v[0], p.y = v[1], p.z = v[2], p.qx = v[3], p.qy = v[4], p.qz = v[5], p.qw = v[6];
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double              rec[14];
    while (std::fread(rec, sizeof rec, 1, f) == 1) in.insert(in.end(), rec, rec + 14);
    std::fclose(f);
    std::vector<double> out;
    for (size_t i = 0; i < in.size(); i += 14) {
        const Pose a = pose_at(&in[i]), b = pose_at(&in[i + 7]);
        double     o[50], *w = o;
        detail::tf_matrix(a, w);
        detail::eigen_matrix(a, w + 9);
        Pose q;
        detail::eigen_quaternion(w, &q);
        w[18] = q.qx, w[19] = q.qy, w[20] = q.qz, w[21] = q.qw;
        detail::tf_quaternion(w, &q);
        w[22] = q.qx, w[23] = q.qy, w[24] = q.qz, w[25] = q.qw;
        float rel[16];
        detail::relative_f32(a, b, rel);
        for (int k = 0; k < 16; ++k) w[26 + k] = (double)rel[k];
        w[42] = detail::tf_yaw(a);
        detail::euler_ypr(a, w[43], w[44], w[45]);
        detail::quat_from_rpy(a.x, a.y, a.z, q);
        w[46] = q.qx, w[47] = q.qy, w[48] = q.qz, w[49] = q.qw;
        out.insert(out.end(), o, o + 50);
    }
    f = std::fopen(argv[2], "wb");
    if (!f || (out.size() && std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size())) return 2;
    std::fclose(f);
    return 0;
}
