"""slam_amd::GridMatcher and CorrelativeMatcher::fromPlane / setPlane / scorePoses (include/slam_amd/correlative.hpp):
tests/cpp/grid_match_test.cpp fills an MLS grid with the synthetic room, updates, matches, scores a pose set, relocalizes and
walks the failure paths; every number must be the Python path's (slam_amd.api.GridMatcher) bit for bit -- both go
through the same C-ABI entry points -- on a fixed grid and on one whose window has rolled."""
import os
import subprocess

import numpy as np
import pytest

import csm_oracle as CO
from slam_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = 96
SIZE, RES, SIGMA, HALF_XY, HALF_THETA, STEP, RELOC_STEP = 128, 0.5, 0.5, 6, 4, 0.05, 0.05
RUN_SECONDS = 120


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "grid_match_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "grid_match_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_grid_match_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter headers are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


def row_pose(words):
    """(R, t bytes, the six integers, the score's share) of a printed pose row"""
    return (np.array([float.fromhex(w) for w in words[:6]]).tobytes(), [int(v) for v in words[6:12]], float.fromhex(words[12]))


def python_pose(R, t, res):
    share = res.score / res.max_score if res.max_score > 0 else 0.0
    return (np.concatenate([np.reshape(R, 4), t]).tobytes(), [res.k, res.a, res.b, res.score, res.max_score, res.n_points], share)


@pytest.mark.gpu
@pytest.mark.parametrize("centre", ((0.0, 0.0), (7 * RES + 0.2, -5 * RES - 0.1)))
def test_the_cpp_twin_equals_the_python_path(tmp_path, centre):
    d = str(tmp_path)
    exe = compile_test(d)
    # the Python path first: it also says where the window's centre is, which the obstacle cloud is relative to
    g = api.Grid(SIZE, SIZE, RES)
    g.set_min_cluster_points(0)
    g.set_pose(*centre)
    c = np.asarray(g.get_pose(), np.float64)
    m_ga, m_nga = CO.synth_map()
    obs = (np.concatenate([m_ga, m_nga]) - c).astype(np.float32)
    g.add_scan_inorder(obs, np.zeros((0, 2), np.float32))
    gm = api.GridMatcher(g, SIGMA, half_x=HALF_XY, half_y=HALF_XY, half_theta=HALF_THETA, theta_step=STEP)
    gm.update()
    t_ga, t_nga, pose = synth.make_scan(SCAN, 256)
    R0, t0 = synth.pose_to_Rt(pose[0] + 1.3, pose[1] - 0.9, pose[2] + 0.08)
    th = pose[2] + np.linspace(-0.3, 0.3, 9)
    poses = api.CorrelativeMatcher.poses(th, np.full(9, pose[0]), np.full(9, pose[1]))
    poses[4, 2] = np.nan
    for name, a, dt in (("obstacles.f32", obs, np.float32), ("t_ga.f64", t_ga, np.float64), ("t_nga.f64", t_nga, np.float64),
                        ("init.f64", np.concatenate([R0.reshape(4), t0]), np.float64), ("poses.f64", poses, np.float64)):
        np.ascontiguousarray(a, dt).tofile(os.path.join(d, name))

    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(SIZE), repr(RES), repr(SIGMA), repr(centre[0]), repr(centre[1]), str(HALF_XY), str(HALF_THETA), repr(STEP),
                        repr(RELOC_STEP)], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    rows = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}

    assert int(rows["setup"][0]) == gm.max_cells == 3
    assert (float.fromhex(rows["setup"][1]), float.fromhex(rows["setup"][2])) == gm.centre == tuple(c)
    R, t, res = gm.match(t_ga, t_nga, R0, t0)
    assert row_pose(rows["match"]) == python_pose(R, t, res)
    assert abs(t[0] - pose[0]) <= RES and abs(t[1] - pose[1]) <= RES                 # map frame, rolled or not
    gm.matcher.set_post_params()
    Rp, tp, resp, post = gm.match_post(t_ga, t_nga, R0, t0)
    assert row_pose(rows["post"]) == python_pose(Rp, tp, resp) == python_pose(R, t, res)
    w = rows["posterior"]
    assert [int(v) for v in w[:5]] == [1, post.valid, post.n_within, post.margin, post.m0]
    assert [float.fromhex(v) for v in w[5:]] == [post.cov[0], post.cov[3], post.cov[5]]
    s, n = gm.score_poses(t_ga, t_nga, poses)
    assert [int(v) for v in rows["scores"]] == [1] + [int(v) for pair in zip(s, n) for v in pair]
    assert n[4] == 0 and s[4] == 0 and s.max() > 0
    assert row_pose(rows["direct"]) == python_pose(R, t, res)                        # fromPlane over the plane read back
    Rr, tr, resr = gm.relocalize(t_ga, t_nga, RELOC_STEP)
    assert row_pose(rows["relocalize"]) == python_pose(Rr, tr, resr)
    assert abs(tr[0] - pose[0]) <= RES and abs(tr[1] - pose[1]) <= RES
    assert rows["edges"] == ["1"] * 9
    for word in ("slam_csm_set_plane_dev", "slam_csm_create_from_plane", "slam_grid_likelihood_table", "GridMatcher: the grid is not usable"):
        assert word in r.stderr, word                                                # every failure is logged
    gm.close()
