"""include/slam_amd/pose.hpp against its restatements, bit for bit: tests/cpp/pose_math_test.cpp (g++ -O2 -ffp-contract=off,
no library) runs every function of the header on the poses below.  What is made of + - * / and sqrt only -- the two
matrices, the two quaternion extractions, relative_f32 -- is held to tests/kf_edge_oracle.py; the trigonometric ones
(tf_yaw, euler_ypr, quat_from_rpy) to restatements over Python's math module, which calls the C library the program links."""
import math
import os
import subprocess

import numpy as np
import pytest

import kf_edge_oracle as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = math.sqrt(0.5)

# name -> quaternion (x, y, z, w)
NAMED = {
    "identity": (0.0, 0.0, 0.0, 1.0),
    "about x": (math.sin(0.35), 0.0, 0.0, math.cos(0.35)),
    "about y": (0.0, math.sin(-0.6), 0.0, math.cos(-0.6)),
    "about z": (0.0, 0.0, math.sin(1.1), math.cos(1.1)),
    "general": (0.18, -0.37, 0.55, 0.73),
    "scaled 0.5": (0.5 * 0.18, 0.5 * -0.37, 0.5 * 0.55, 0.5 * 0.73),
    "scaled 3": (3 * 0.18, 3 * -0.37, 3 * 0.55, 3 * 0.73),
    "w < 0": (0.1, 0.2, 0.3, -0.9),
    "w < 0, trace <= 0": (1.0, 0.02, 0.01, -0.05),
    "trace > 0": (0.1, -0.1, 0.2, 0.95),
    "m00 largest": (1.0, 0.02, 0.01, 0.0),      # half a turn about (nearly) x: trace <= 0, i = 0
    "m11 largest": (0.02, 1.0, 0.01, 0.0),
    "m22 largest": (0.01, 0.02, 1.0, 0.0),
    "pitch +pi/2": (0.0, 1.0, 0.0, 1.0),        # d = 2, s = 1: m20 = -1 exactly, the gimbal branch
    "pitch -pi/2": (0.0, -1.0, 0.0, 1.0),
    "zero": (0.0, 0.0, 0.0, 0.0),
}
SCALED = ("scaled 0.5", "scaled 3")


def poses():
    """Records (a, b) of two poses x y z qx qy qz qw.  a's x y z double as the roll, pitch, yaw quat_from_rpy gets."""
    rs = np.random.RandomState(20261019)
    rec, names = [], []
    for name, q in NAMED.items():
        rec.append([0.3, -0.2, 1.7] + list(q) + [1.5, -2.5, 0.25, 0.05, -0.02, 0.3, 0.95])
        names.append(name)
    for i in range(300):
        qa, qb = rs.randn(4), rs.randn(4)
        if i % 3:                                   # two in three of unit length (to rounding), the others as drawn
            qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
        rec.append(list(rs.uniform(-math.pi, math.pi, 3)) + list(qa) + list(rs.uniform(-50, 50, 3)) + list(qb))
        names.append("random %d" % i)
    return np.array(rec, np.float64), names


def py_tf_yaw(q):
    m = K.tf_matrix(q)
    if abs(m[6]) >= 1.0:
        return 0.0
    cp = math.cos(-math.asin(m[6]))
    return math.atan2(m[3] / cp, m[0] / cp)


def py_euler_ypr(q):
    """tf::Matrix3x3::getEulerYPR(yaw, pitch, roll, 1) as detail::euler_ypr states it"""
    m = K.tf_matrix(q)
    if abs(m[6]) >= 1:
        return 0.0, (math.pi / 2.0 if m[6] < 0 else -math.pi / 2.0), math.atan2(m[1], m[2])
    pitch = -math.asin(m[6])
    return math.atan2(m[3] / math.cos(pitch), m[0] / math.cos(pitch)), pitch, math.atan2(m[7] / math.cos(pitch), m[8] / math.cos(pitch))


def py_quat_from_rpy(roll, pitch, yaw):
    hy, hp, hr = yaw * 0.5, pitch * 0.5, roll * 0.5
    cy, sy, cp, sp, cr, sr = math.cos(hy), math.sin(hy), math.cos(hp), math.sin(hp), math.cos(hr), math.sin(hr)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def bits(v):
    return np.asarray([float(x) for x in v], np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_math")
    exe = str(d / "pose_math_test")
    # -fno-builtin-sin/-cos: at -O2 g++ turns sin(x) and cos(x) of one x (quat_from_rpy's half angles) into one sincos(x), and
    # glibc's sincos is not its cos to the last place (cos(1.1054393948489673): ...f63p-2, sincos: ...f64p-2).  With the two
    # calls kept apart the program calls what Python's math calls, and the comparison stays bit for bit.
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-builtin-sin", "-fno-builtin-cos", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_math_test.cpp"), "-o", exe])
    rec, names = poses()
    rec.tofile(str(d / "in.f64"))
    subprocess.check_call([exe, str(d / "in.f64"), str(d / "out.f64")])
    out = np.fromfile(str(d / "out.f64"), np.float64).reshape(len(rec), 50)
    assert not np.isnan(out).any()
    return rec, names, out


def test_matrices_quaternions_and_relative_bit_for_bit(run):
    rec, names, out = run
    for r, name, o in zip(rec, names, out):
        a, b = r[:7], r[7:]
        tfm = K.tf_matrix(a[3:])
        assert np.array_equal(bits(o[0:9]), bits(tfm)), name
        assert np.array_equal(bits(o[9:18]), bits(K.quat_to_matrix(a[3:]))), name
        assert np.array_equal(bits(o[18:22]), bits(K.eigen_quaternion(tfm))), name
        assert np.array_equal(bits(o[22:26]), bits(K.tf_quaternion(tfm))), name
        assert np.array_equal(o[26:42].astype(np.float32).view(np.uint32), K.relative_f32(a, b).reshape(16).view(np.uint32)), name
        assert np.array_equal(o[26:42].astype(np.float32).astype(np.float64), o[26:42]), name      # (they were floats)


def test_trigonometric_functions_bit_for_bit(run):
    rec, names, out = run
    for r, name, o in zip(rec, names, out):
        q = r[3:7]
        assert np.array_equal(bits(o[42:43]), bits([py_tf_yaw(q)])), name
        assert np.array_equal(bits(o[43:46]), bits(py_euler_ypr(q))), name
        assert np.array_equal(bits(o[46:50]), bits(py_quat_from_rpy(r[0], r[1], r[2]))), name
        assert o[42] == o[43], name                              # tf::getYaw is getEulerYPR's yaw


def test_every_branch_is_fed(run):
    rec, names, out = run
    by = dict(zip(names, out))
    pick = {}
    for name in ("trace > 0", "m00 largest", "m11 largest", "m22 largest"):
        m = by[name][0:9]
        pick[name] = "trace" if m[0] + m[4] + m[8] > 0.0 else int(np.argmax([m[0], m[4], m[8]]))
    assert pick == {"trace > 0": "trace", "m00 largest": 0, "m11 largest": 1, "m22 largest": 2}
    assert by["pitch +pi/2"][6] == -1.0 and by["pitch -pi/2"][6] == 1.0
    assert tuple(by["pitch +pi/2"][43:45]) == (0.0, math.pi / 2.0) and tuple(by["pitch -pi/2"][43:45]) == (0.0, -math.pi / 2.0)
    # Eigen's extraction (poseEigenToMsg) makes w >= 0; tf's keeps the sign the off-diagonal elements give it
    assert by["w < 0"][21] > 0 and by["w < 0"][25] > 0
    assert by["w < 0, trace <= 0"][21] > 0 > by["w < 0, trace <= 0"][25]


def test_tf_and_eigen_matrices_are_two_functions(run):
    """For a quaternion that is not of unit length tf divides by |q|^2 and Eigen does not: the answers differ, and not by rounding."""
    rec, names, out = run
    by = dict(zip(names, out))
    for name in SCALED:
        assert np.abs(by[name][0:9] - by[name][9:18]).max() > 0.1, name
    assert np.abs(by["general"][0:9] - by["general"][9:18]).max() < 1e-2      # (0.9987 of unit length)


def test_zero_quaternion_gives_identity_and_zero_yaw(run):
    rec, names, out = run
    o = dict(zip(names, out))["zero"]
    assert list(o[0:9]) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert o[42] == 0.0 and list(o[43:46]) == [0.0, 0.0, 0.0]
