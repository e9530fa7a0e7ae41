// slam_amd/pose.hpp -- the pose type of the adapters and every rotation convention they use, each exactly once.
//
// Pure host arithmetic: no device call, no library behind it.  Two libraries' conventions meet in the reference, tf's and
// Eigen's, and they do not give the same bits (tf divides by |q|^2, Eigen does not), so each function below is named after
// the library whose operations, in whose order, it restates:
//
//   tf_matrix         tf::Matrix3x3::setRotation      what tf::getYaw, getEulerYPR and MLS's pose transform go through
//   eigen_matrix      Eigen::Quaterniond::toRotationMatrix, unnormalised: the rotation of tf::poseMsgToEigen
//   eigen_quaternion  Eigen::Quaterniond(Matrix3d)    tf::poseEigenToMsg
//   tf_quaternion     tf::Matrix3x3::getRotation
//   tf_yaw, euler_ypr tf::getYaw, tf::Matrix3x3::getEulerYPR(.., 1)
//   quat_from_rpy     tf::createQuaternionFromRPY
//   relative_f32      (Mfrom^-1 Mto).cast<float>() of two poseMsgToEigen transforms
//
// Matrices are row-major double[9].  tf_matrix and eigen_matrix agree for unit quaternions up to rounding and differ for
// every other length: they stay two functions.
#pragma once
#include <cmath>

namespace slam_amd {

struct Pose { // geometry_msgs::Pose
    double x = 0, y = 0, z = 0;
    double qx = 0, qy = 0, qz = 0, qw = 1;
};

namespace detail {

// tf::Matrix3x3::setRotation (behind tf::Matrix3x3(q): icpTools.cpp:208, scan_registration.cpp:134, graphSlamTools.cpp:268;
// behind tf::getYaw: icpTools.cpp:174, graphSlamTools.cpp:335, graph_slam.cpp:363; the pose transform of mls.cpp:46 and
// graph_slam.cpp:272).  The all-zero quaternion, which tf rejects by assertion, gives the identity here (s = 0), so its
// yaw, pitch and roll are 0; every other quaternion gets tf's operations in tf's order.
inline void tf_matrix(const Pose &q, double m[9])
{
    const double d = q.qx * q.qx + q.qy * q.qy + q.qz * q.qz + q.qw * q.qw, s = d > 0 ? 2.0 / d : 0.0;
    const double xs = q.qx * s, ys = q.qy * s, zs = q.qz * s, wx = q.qw * xs, wy = q.qw * ys, wz = q.qw * zs, xx = q.qx * xs,
                 xy = q.qx * ys, xz = q.qx * zs, yy = q.qy * ys, yz = q.qy * zs, zz = q.qz * zs;
    m[0] = 1.0 - (yy + zz), m[1] = xy - wz, m[2] = xz + wy;
    m[3] = xy + wz, m[4] = 1.0 - (xx + zz), m[5] = yz - wx;
    m[6] = xz - wy, m[7] = yz + wx, m[8] = 1.0 - (xx + yy);
}

// Eigen::Quaterniond(w, x, y, z).toRotationMatrix(), the rotation of tf::poseMsgToEigen (graphSlamTools.cpp:242-243): no
// division by |q|^2, so a quaternion that is not of unit length gives a scaled matrix, as Eigen does
inline void eigen_matrix(const Pose &q, double m[9])
{
    const double tx = 2.0 * q.qx, ty = 2.0 * q.qy, tz = 2.0 * q.qz;
    const double twx = tx * q.qw, twy = ty * q.qw, twz = tz * q.qw, txx = tx * q.qx, txy = ty * q.qx, txz = tz * q.qx, tyy = ty * q.qy,
                 tyz = tz * q.qy, tzz = tz * q.qz;
    m[0] = 1.0 - (tyy + tzz), m[1] = txy - twz, m[2] = txz + twy;
    m[3] = txy + twz, m[4] = 1.0 - (txx + tzz), m[5] = tyz - twx;
    m[6] = txz - twy, m[7] = tyz + twx, m[8] = 1.0 - (txx + tyy);
}

// (Mfrom^-1 Mto).cast<float>(), graphSlamTools.cpp:258, row-major 4 x 4
inline void relative_f32(const Pose &from, const Pose &to, float out[16])
{
    double Rf[9], Rt[9];
    eigen_matrix(from, Rf);
    eigen_matrix(to, Rt);
    const double d[3] = {to.x - from.x, to.y - from.y, to.z - from.z};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (float)((Rf[r] * Rt[c] + Rf[3 + r] * Rt[3 + c]) + Rf[6 + r] * Rt[6 + c]);
        out[4 * r + 3] = (float)((Rf[r] * d[0] + Rf[3 + r] * d[1]) + Rf[6 + r] * d[2]);
    }
    out[12] = out[13] = out[14] = 0.0f, out[15] = 1.0f;
}

// Eigen::Quaterniond(Matrix3d) (tf::poseEigenToMsg, which also makes w >= 0: graphSlamTools.cpp:259-260)
inline void eigen_quaternion(const double m[9], Pose *p)
{
    double q[4]; // x y z w
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t, q[1] = (m[2] - m[6]) * t, q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
    if (q[3] < 0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
    p->qx = q[0], p->qy = q[1], p->qz = q[2], p->qw = q[3];
}

// tf::Matrix3x3::getRotation (graphSlamTools.cpp:318-331)
inline void tf_quaternion(const double m[9], Pose *p)
{
    const double trace = m[0] + m[4] + m[8];
    double       temp[4];
    if (trace > 0.0) {
        double s = std::sqrt(trace + 1.0);
        temp[3] = s * 0.5;
        s = 0.5 / s;
        temp[0] = (m[7] - m[5]) * s, temp[1] = (m[2] - m[6]) * s, temp[2] = (m[3] - m[1]) * s;
    } else {
        const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double    s = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        temp[i] = s * 0.5;
        s = 0.5 / s;
        temp[3] = (m[3 * k + j] - m[3 * j + k]) * s;
        temp[j] = (m[3 * j + i] + m[3 * i + j]) * s;
        temp[k] = (m[3 * k + i] + m[3 * i + k]) * s;
    }
    p->qx = temp[0], p->qy = temp[1], p->qz = temp[2], p->qw = temp[3];
}

// tf::getYaw (graphSlamTools.cpp:335, graph_slam.cpp:363,374): Matrix3x3(q).getRPY's yaw -- setRotation, then
// getEulerYPR's first solution
inline double tf_yaw(const Pose &q)
{
    double m[9];
    tf_matrix(q, m);
    if (std::fabs(m[6]) >= 1.0) return 0.0;
    const double pitch = -std::asin(m[6]), cp = std::cos(pitch);
    return std::atan2(m[3] / cp, m[0] / cp);
}

// tf::Matrix3x3(q).getEulerYPR(yaw, pitch, roll, 1) (icpTools.cpp:208, scan_registration.cpp:134)
inline void euler_ypr(const Pose &p, double &yaw, double &pitch, double &roll)
{
    double m[9];
    tf_matrix(p, m);
    if (std::fabs(m[6]) >= 1) { // gimbal lock branch of tf
        yaw = 0;
        const double delta = std::atan2(m[1], m[2]);
        if (m[6] < 0) {
            pitch = M_PI / 2.0;
            roll = delta;
        } else {
            pitch = -M_PI / 2.0;
            roll = delta;
        }
    } else {
        pitch = -std::asin(m[6]);
        roll = std::atan2(m[7] / std::cos(pitch), m[8] / std::cos(pitch));
        yaw = std::atan2(m[3] / std::cos(pitch), m[0] / std::cos(pitch));
    }
}

// tf::createQuaternionFromRPY (icpTools.cpp:205-212)
inline void quat_from_rpy(double roll, double pitch, double yaw, Pose &p)
{
    const double hy = yaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
    const double cy = std::cos(hy), sy = std::sin(hy), cp = std::cos(hp), sp = std::sin(hp), cr = std::cos(hr),
                 sr = std::sin(hr);
    p.qx = sr * cp * cy - cr * sp * sy;
    p.qy = cr * sp * cy + sr * cp * sy;
    p.qz = cr * cp * sy - sr * sp * cy;
    p.qw = cr * cp * cy + sr * sp * sy;
}

} // namespace detail
} // namespace slam_amd
