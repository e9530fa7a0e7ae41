"""slam_amd::PoseGraphOptimizer (include/slam_amd/pose_graph.hpp) in graph_slam's back-end loop (graph_slam.cpp:479-560):
tests/cpp/pose_graph_test.cpp sends eight keyframes through KeyframeGraph (the node and its edges), PoseGraphOptimizer
(addVertex, addEdge, optimizeGraph) and MLSMap (the map replayed with the optimised poses).  slam_amd.api.PoseGraph fed the
same edges gives the same bits at every keyframe, the restatement (tests/cpp/pgo_oracle.cpp) the same poses within the
project's pose bound, and the map replayed from here is the map the program built."""
import os
import subprocess

import numpy as np
import pytest

import mls_map_oracle as MO
import pgo_cases as K
import pgo_oracle as O
from slam_amd import api, build, synth
from test_gpu_mls_map_adapter import quat_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYFRAMES = list(range(8))
# what curPose is off the truth by when keyframe k arrives (x, y, yaw): odometry that drifts
DRIFT = [(0, 0, 0), (0.1, -0.05, 0.01), (0.2, -0.1, 0.02), (0.25, -0.2, 0.02), (0.35, -0.2, 0.03), (0.4, -0.3, 0.03), (0.5, -0.3, 0.04),
         (0.55, -0.4, 0.04)]
RUN_SECONDS = 120
MIN_CLUSTER_POINTS = 2      # of the map replay: the clouds are 16 rings of 512, a cell rarely collects graph_slam's 10


def clouds_and_poses():
    clouds, poses = [], []
    x0, y0, _ = synth.true_pose(KEYFRAMES[0], 50)
    for k, (ex, ey, eth) in zip(KEYFRAMES, DRIFT):
        xyz, (x, y, th) = synth.make_cloud3d(k, n_loop=50, rings=16, n_az=512)
        clouds.append(xyz)
        poses.append([x - x0 + ex, y - y0 + ey, 0.0, 0.0, 0.0, np.sin(0.5 * (th + eth)), np.cos(0.5 * (th + eth))])
    return clouds, np.array(poses, np.float64)


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "pose_graph_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_graph_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_pose_graph_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def test_pose_offset_is_the_arithmetic_as_written():
    """graph_slam.cpp:356-384: y takes + vpx sin (not a rotation), and a wrapped yaw difference is negated"""
    pre = [1.0, 2.0, 0.1, 0, 0, np.sin(0.2), np.cos(0.2)]
    post = [1.5, 1.0, 0.3, 0, 0, np.sin(0.35), np.cos(0.35)]
    cur = [4.0, 3.0, 0.0, 0, 0, np.sin(0.25), np.cos(0.25)]
    off = api.PoseGraph.pose_offset(pre, post, cur)
    vn, vpx, vpy = 0.3, 3.0, 1.0
    assert off[:3] == pytest.approx([(vpx * np.cos(vn) + vpy * np.sin(vn) + 0.5) - vpx, (vpy * np.cos(vn) + vpx * np.sin(vn) - 1.0) - vpy, 0.2],
                                    abs=1e-12)
    assert 2 * np.arctan2(off[5], off[6]) == pytest.approx(0.3 + 0.1, abs=1e-12)
    # yaw from -3.0 to 3.0 rad: the difference 6.0 > pi is wrapped to -(6 - 2 pi) = 0.2832 where a rotation would say -0.2832
    pre, post = [0, 0, 0, 0, 0, np.sin(-1.5), np.cos(-1.5)], [0, 0, 0, 0, 0, np.sin(1.5), np.cos(1.5)]
    off = api.PoseGraph.pose_offset(pre, post, pre)
    assert 2 * np.arctan2(off[5], off[6]) == pytest.approx(2 * np.pi - 6.0, abs=1e-12)


@pytest.mark.gpu
def test_the_loop_in_cpp_in_python_and_in_the_restatement(tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    clouds, poses = clouds_and_poses()
    poses.tofile(os.path.join(d, "poses.f64"))
    for i, c in enumerate(clouds):
        np.ascontiguousarray(c, np.float32).tofile(os.path.join(d, "kf%d.f32" % i))
    out = os.path.join(d, "out")
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, out, str(len(clouds)), str(MIN_CLUSTER_POINTS)], timeout=RUN_SECONDS, stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    edges = np.fromfile(out + ".edges", np.float64).reshape(-1, 45)
    steps = np.fromfile(out + ".steps", np.float64)
    assert len(edges) >= len(clouds) - 1

    g, ora = api.PoseGraph(), O.OracleGraph()
    nodes = [g.init_optimizer(poses[0])]
    ora.add_vertex(0, nodes[0], True)
    at, used = 0, 0
    for k in range(1, len(clouds)):
        head, offset = steps[at:at + 7], steps[at + 7:at + 14]
        cpp_nodes = steps[at + 14:at + 14 + 7 * (k + 1)].reshape(k + 1, 7)
        at += 14 + 7 * (k + 1)
        nodes.append(poses[k])
        g.add_vertex(k, poses[k], False)
        ora.add_vertex(k, poses[k], False)
        for e in edges[used:int(head[0])]:
            assert int(e[1]) == k and 0 <= int(e[0]) < k
            g.add_edge(int(e[0]), int(e[1]), e[2:9], e[9:])
            ora.add_edge(int(e[0]), int(e[1]), e[2:9], e[9:])
        used = int(head[0])
        est, off, res = g.optimize_graph(nodes, poses[k])
        want = ora.optimize(10)
        dm, dr = K.pose_errors(est, ora.read_vertices())
        print("keyframe %d: %d edges, chi2 %.6g -> %.6g (restatement %.6g), %d trials, against the restatement %.3g m %.3g rad"
              % (k, used, res.chi2_initial, res.chi2_final, want.chi2_final, res.n_trials, dm.max(), dr.max()))
        # the C++ run and this one made the same C-ABI calls: the same bits
        assert est.tobytes() == cpp_nodes.tobytes(), k
        assert [res.iterations, res.stop_reason, res.n_trials, res.half_bandwidth] == [int(v) for v in head[1:5]]
        assert (res.chi2_initial, res.chi2_final) == (head[5], head[6])
        assert off.tobytes() == offset.tobytes(), (k, off, offset)
        assert dm.max() <= K.POSE_TOL_M and dr.max() <= K.POSE_TOL_RAD
        assert res.chi2_final <= res.chi2_initial
        nodes = list(est)
    assert at == len(steps) and used == len(edges)

    # regenerateGlobalMap from here with the optimised poses: the map the program ended with
    m = api.MlsMap(1000, 1000, 0.5)
    m.clear()
    m.set_params(min_cluster_points=MIN_CLUSTER_POINTS)
    for c, p in zip(clouds, nodes):
        m.add_cloud(MO.transform(c, quat_matrix(p[3:]), np.array(p[:3])), p[:2])
    drv = m.read_drivability()
    print("map: %d cells known, %d of them drivable" % ((drv >= 0).sum(), (drv == 0).sum()))
    assert np.array_equal(np.fromfile(out + ".drivability", np.int8), drv) and (drv >= 0).sum() > 100
    m.close(), g.close()
