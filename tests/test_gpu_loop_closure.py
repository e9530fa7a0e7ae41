"""Loop closure by appearance, end to end (tests/cpp/loop_closure_test.cpp over include/slam_amd/graph_edges.hpp and
pose_graph.hpp).  Two laps of the synthetic 48-pose loop: keyframes 0 .. 47 are lap one, 48 .. 95 the same poses again from
other noise seeds, 0.52 to 0.78 m from one keyframe to the next.  The pose estimates of lap two drift: keyframe 48 + i is off
the truth by (i + 1) / 48 of (3 m along x, 0.1 rad), 3 m and 0.1 rad at the end, where x points out of the loop.
docs/SCAN_CONTEXT.md section 4 has what a run on the MI355X gave."""
import os
import subprocess

import numpy as np
import pytest

import sc_cases as K
from slam_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAP = 48
DRIFT = (3.0, 0.0, 0.1)          # x, y (3 m) and yaw at the end of lap two, growing linearly over it
RUN_SECONDS = 120
NEAR = 1.5                       # a loop edge counts when the two keyframes are truly this close
ALLOWANCE = 0.25                 # half the 0.5 m voxel leaf, the resolution of the clouds the registration sees
# KeyframeGraph::SC_MAX_DISTANCE for this run: a mean height difference of 2 bins (4 cm) a cell, 20 x 64 cells -- the same
# place seen again through other noise, not a neighbour 0.5 m on.  The room looks alike from across, turned by half a turn
# (docs/SCAN_CONTEXT.md section 4); ICP agrees with that start and its gate accepts it, so the candidates need a limit.
SC_MAX_DISTANCE = 20 * 64 * 2
# (GSLAM_KNN, registration): the reference's pose-based edges (3 nearest by pose and the predecessor, point-to-point ICP); the
# edge to the predecessor alone; the same with Generalized ICP as the solver of every edge
VARIANTS = {"reference": (3, 0), "predecessor": (0, 0), "predecessor_gicp": (0, 1)}


def inputs():
    """(clouds, drifting poses [96, 7], truth [96, 3]) in the frame of keyframe 0's position"""
    ks = list(range(LAP)) + list(range(LAP))
    x0, y0, _ = synth.true_pose(0, LAP)
    clouds, poses, truth = [], [], []
    for n, k in enumerate(ks):
        xyz, (x, y, th) = synth.make_cloud3d(k, LAP, rings=32, n_az=512, **({} if n < LAP else {"seed_base": 20000}))
        f = 0.0 if n < LAP else (n - LAP + 1) / float(LAP)
        clouds.append(xyz)
        truth.append([x - x0, y - y0, th])
        ex, ey, eth = x - x0 + f * DRIFT[0], y - y0 + f * DRIFT[1], th + f * DRIFT[2]
        poses.append([ex, ey, 0.0, 0.0, 0.0, np.sin(0.5 * eth), np.cos(0.5 * eth)])
    return clouds, np.array(poses), np.array(truth)


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "loop_closure_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loop_closure_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_loop_closure_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header's new members are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def edge_error(row, truth):
    """how far the edge's measurement is from the true relative pose of its keyframes: (m, rad)"""
    f, t = truth[int(row[1])], truth[int(row[2])]
    c, s = np.cos(f[2]), np.sin(f[2])
    dx, dy = t[0] - f[0], t[1] - f[1]
    want = (c * dx + s * dy, -s * dx + c * dy, t[2] - f[2])
    yaw = 2.0 * np.arctan2(row[15], row[16])
    dth = (yaw - want[2] + np.pi) % (2.0 * np.pi) - np.pi
    return float(np.hypot(row[10] - want[0], row[11] - want[1])), abs(float(dth))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The program's three runs (VARIANTS), each under its own time limit (a fault ends it and the tests with it).
    -> {variant: (edges, poses after optimisation [2, 96, 7], the drifting estimates, the truth)}"""
    d = str(tmp_path_factory.mktemp("loop_closure"))
    exe = compile_test(d)
    clouds, poses, truth = inputs()
    poses.tofile(os.path.join(d, "poses.f64"))
    truth.tofile(os.path.join(d, "truth.f64"))
    for i, c in enumerate(clouds):
        np.ascontiguousarray(c, np.float32).tofile(os.path.join(d, "kf%d.f32" % i))
    got = {}
    for name, (knn, gicp) in VARIANTS.items():
        out = os.path.join(d, "out_" + name)
        r = subprocess.run([exe, d, out, str(2 * LAP), str(LAP), str(K.PLACE_MAX_RANGE), str(SC_MAX_DISTANCE), str(knn), str(gicp)], timeout=RUN_SECONDS,
                           stderr=subprocess.PIPE, text=True)
        print("%s\n%s" % (name, r.stderr))
        assert r.returncode == 0, r.stderr
        edges = np.fromfile(out + ".edges", np.float64).reshape(-1, 19)
        est = np.fromfile(out + ".poses", np.float64).reshape(2, 2 * LAP, 7)
        for e in edges:
            if e[1] < LAP <= e[2] and name == "reference":
                print("kind %d  %2d -> %2d  accepted %d  pairs %5d  true distance %.2f m  error %.3f m %.4f rad  descriptor distance %d"
                      % ((e[0], e[1], e[2], e[3], e[4], true_distance(e, truth)) + edge_error(e, truth) + (e[18],)))
        got[name] = (edges, est, poses, truth)
    return got


def true_distance(e, truth):
    return float(np.hypot(*(truth[int(e[1]), :2] - truth[int(e[2]), :2])))


@pytest.mark.gpu
def test_pose_based_edges_alone_find_no_edge_between_the_laps(run):
    """addEdgesForNewNode alone yields no accepted edge between the laps at the end of lap two: with 3 m of drift the keyframes
    nearest to the last one by estimated pose are its own predecessors (1.1, 1.8 and 2.4 m against 2.9 m to the nearest of lap
    one), so no edge to lap one is even tried.  Earlier in the lap, where the drifting estimate passes over lap one, edges
    between the laps are tried and accepted (calcEdgeIcp's gate is 10 m and 0.2 rad); those are printed with their errors."""
    edges, _, _, truth = run["reference"]
    cross = [e for e in edges if e[0] == 0 and e[1] < LAP <= e[2]]
    end = [e for e in cross if e[2] == 2 * LAP - 1]
    wrong = [e for e in cross if e[3] and edge_error(e, truth)[0] > 1.0]
    print("pose-based: %d edges between the laps tried, %d accepted, %d of those more than 1 m from the true relative pose (the worst "
          "%.2f m); for the last keyframe %d tried, %d accepted"
          % (len(cross), sum(e[3] for e in cross), len(wrong), max([edge_error(e, truth)[0] for e in wrong] or [0.0]), len(end),
             sum(e[3] for e in end)))
    assert any(e[0] == 0 and e[2] == 2 * LAP - 1 for e in edges)      # it did get its pose-based edges
    assert not any(e[3] for e in end)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_two_laps_with_drift_are_closed_by_appearance(run, name):
    """In every variant: each keyframe of lap two gets an accepted loop edge to a keyframe of lap one truly within NEAR, and the
    optimised graph is no worse than with ground-truth pairs and yaw plus ALLOWANCE.  What the variants show beside that (MI355X,
    maximum position error of lap two, 3.000 m as estimated; loop edges / ground-truth edges): reference 2.809 / 2.901 m -- the
    pose-based edges between the laps, 49 of 119 of them false closures, sit in both graphs; predecessor 4.823 / 4.926 m -- a
    consistent graph (chi2 2.8) of edges that point-to-point ICP makes 0.2 to 0.4 m too short on these clouds;
    predecessor_gicp 0.022 / 0.021 m."""
    edges, est, poses, truth = run[name]
    # by appearance: every keyframe of lap two gets an accepted edge to a keyframe of lap one that is truly within NEAR
    loop = [e for e in edges if e[0] == 1]
    for k in range(LAP, 2 * LAP):
        assert any(e[3] and e[2] == k and e[1] < LAP and true_distance(e, truth) <= NEAR for e in loop), k
    worst = max(edge_error(e, truth)[0] for e in loop if e[3])
    print("loop edges: %d tried, %d accepted, the worst %.3f m from the true relative pose; ground-truth edges: the worst %.3f m"
          % (len(loop), sum(e[3] for e in loop), worst, max(edge_error(e, truth)[0] for e in edges if e[0] == 2 and e[3])))
    # after optimisation: no worse than the same graph closed with ground-truth pairs and yaw, plus ALLOWANCE
    err = [float(np.hypot(*(est[g, LAP:, :2] - truth[LAP:, :2]).T).max()) for g in range(2)]
    before = float(np.hypot(*(poses[LAP:, :2] - truth[LAP:, :2]).T).max())
    print("%s: " % name, end="")
    print("maximum position error of lap two: %.3f m as estimated, %.3f m with loop edges, %.3f m with ground-truth edges" % (before, err[0], err[1]))
    assert err[0] <= err[1] + ALLOWANCE
